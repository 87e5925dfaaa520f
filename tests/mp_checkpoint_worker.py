"""worker of the two-rank checkpoint test (tests/test_hip_checkpoint.py): N processes share cuda:0 and exchange through
gloo (host-staged), like tests/mp_snapshot_worker.py; TGV 32^3 on y slabs, RK3, fused driver.
  run     6 steps with checkpoint_freq = 3: `<prefix>_000003.r<rank>.npz`, `<prefix>_000006.r<rank>.npz`
  resume  a fresh case restored from `<prefix>_000003.r<rank>.npz`, run to step 6
Either mode leaves its final u, v, w in `<prefix>.final.<mode>.<rank>.npz`."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    mode, prefix = sys.argv[1], sys.argv[2]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    from x3d2_amd import make_tgv
    from x3d2_amd.checkpoint import CheckpointConfig, Checkpoints, restore
    from x3d2_amd.parallel import Comm
    case = make_tgv(32, nproc_dir=(1, size, 1), rank=rank, comm=Comm(), fused=True, time_intg="RK3")
    if mode == "run":
        case.checkpoints = Checkpoints(case.solver, CheckpointConfig(checkpoint_freq=3, checkpoint_prefix=prefix), case)
    else:
        assert restore(case, "%s_000003.r%d.npz" % (prefix, rank)) == 3
    case.run(n_iters=6)
    s = case.solver
    u, v, w = (s.backend.get_field_data(f) for f in (s.u, s.v, s.w))
    np.savez("%s.final.%s.%d.npz" % (prefix, mode, rank), u=u, v=v, w=w)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
