"""worker of the multi-rank particle tests (tests/test_hip_particles_mp.py): N processes share cuda:0 and exchange through gloo
(host-staged), like tests/mp_les_worker.py.  argv: scenario, layout "1,Py,Pz", output prefix, a JSON list of cases.  Every rank
saves `<out>.<rank>.npz`; what the scenarios do is in test_hip_particles_mp.py (fixed_run, edge_run, overflow_run, real_run).
X3D_SINGLE_PREC=1 in the environment selects the FP32 flavour of the library, as in tests/particles_sp_worker.py."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    scenario, layout, out, cases = sys.argv[1], tuple(int(x) for x in sys.argv[2].split(",")), sys.argv[3], json.loads(sys.argv[4])
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    assert int(np.prod(layout)) == size
    import test_hip_particles_mp as t
    from x3d2_amd import _lib
    from x3d2_amd.parallel import Comm
    assert _lib.SINGLE == (os.environ.get("X3D_SINGLE_PREC") == "1")
    comm = Comm()
    res = {"dtype": np.array(str(np.dtype(_lib.NP_REAL)))}
    run = {"fixed": t.fixed_run, "edges": t.edge_run, "overflow": t.overflow_run, "real": t.real_run, "restart": t.restart_run}[scenario]
    for i, case in enumerate(cases):
        for k, v in run(layout, rank, comm, out=out, **case).items():
            res["c%d_%s" % (i, k)] = v
        dist.barrier()
    np.savez(out + ".%d.npz" % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
