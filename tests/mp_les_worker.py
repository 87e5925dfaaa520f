"""worker of the two-rank LES test (tests/test_hip_les.py): N processes share cuda:0 and exchange through gloo (host-staged),
like tests/mp_loads_worker.py.  Every rank adds the subgrid term of its part of the same global noisy field to zeroed blocks
and saves its part of the term and the monitor figures it holds (the global ones)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    layout = tuple(int(x) for x in sys.argv[1].split(","))
    out = sys.argv[2]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    assert int(np.prod(layout)) == size
    import test_hip_les as t
    from x3d2_amd.parallel import Comm
    d, mon, lo, nl, _ = t.mp_run(layout, rank, Comm())
    keys = ("nut_mean", "eps_sgs", "nut_max", "diffusion_number")
    np.savez(out + ".%d.npz" % rank, d0=d[0], d1=d[1], d2=d[2], lo=np.array(lo), nl=np.array(nl),
             mon=np.array([mon[k] for k in keys]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
