"""worker of the two-rank loads and probes test (tests/test_hip_loads.py): N processes share cuda:0 and exchange through
gloo (host-staged), like tests/mp_diagnostics_worker.py.  Every rank masks its part of the same global random fields with
its part of a sphere that straddles the cut and samples the probes it owns, two rows per device table so that a table is
flushed, landed by poll() and summed over the ranks on the way; saves the combined rows."""
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
    import test_hip_loads as t
    from x3d2_amd.parallel import Comm
    loads, probes, has_file = t.box_run(layout, rank, Comm(), out)
    np.savez(out + ".%d.npz" % rank, loads=loads, probes=probes, has_file=has_file)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
