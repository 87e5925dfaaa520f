"""worker of the two-rank band-forcing test (tests/test_hip_forcing.py): N processes share cuda:0 and exchange through gloo
(host-staged), like tests/mp_scalars_worker.py; z slabs.  Every rank projects its block of the initial field without the sum
over the ranks, runs two forced steps of the isotropic-turbulence case on its slab, and saves its coefficients and fields."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    dims = tuple(int(x) for x in sys.argv[1].split(","))
    out = sys.argv[2]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    import test_hip_forcing as t
    from x3d2_amd.parallel import Comm
    res = t.mp_run(dims, nproc_dir=(1, 1, size), rank=rank, comm=Comm())
    np.savez(out + ".%d.npz" % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
