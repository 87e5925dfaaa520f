"""worker of the two-rank active-scalars test (tests/test_hip_scalars.py): N processes share cuda:0 and exchange through gloo
(host-staged), like tests/mp_stats_worker.py; z slabs.  Every rank runs two steps of the Rayleigh-Benard case on its slab,
takes a profile sample after each (the plane sums are added over the ranks), and saves its fields, the running means and the
monitor's min / max."""
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
    import test_hip_scalars as t
    from x3d2_amd.parallel import Comm
    res = t.rb_two_steps_with_profiles(dims, nproc_dir=(1, 1, size), rank=rank, comm=Comm())
    np.savez(out + ".%d.npz" % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
