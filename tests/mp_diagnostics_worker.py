"""worker of the two-rank diagnostics test (tests/test_hip_diagnostics.py): N processes share cuda:0 and exchange through
gloo (host-staged), like tests/mp_stats_worker.py; z slabs.  Every rank records n rows from its slab of the same global
random blocks (both ranks own the first and the last y row: the wall flags are on for both), with two rows per device
table so that a table is flushed, landed by poll() and combined over the ranks on the way; saves the combined rows."""
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
    n, out = int(sys.argv[2]), sys.argv[3]
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, size = dist.get_rank(), dist.get_world_size()
    import test_hip_diagnostics as t
    from x3d2_amd.parallel import Comm
    b = t.make_backend(dims, t.WALL, nproc_dir=(1, 1, size), rank=rank, comm=Comm())
    s = t.Fields(b)
    nzl = dims[2] // size
    tables = t.random_tables(dims, 77)
    tables[2] = tables[2][rank * nzl:(rank + 1) * nzl]
    dg = t.diagnostics_of(s, out, tables, flush_every=2, divergence=False)
    assert dg.first_y and dg.last_y
    for it in range(1, n + 1):
        arrays = [np.ascontiguousarray(a[rank * nzl:(rank + 1) * nzl]) for a in t.random_arrays(dims, 300 + it)]
        blocks = t.poisoned_blocks(b, arrays)
        dg.record(it, blocks[0], blocks[1], blocks[2], blocks[3:])
        dg.poll()
        for f in blocks:
            b.allocator.release_block(f)
    dg.finalise()
    np.savez(out + ".%d.npz" % rank, raw=dg.raw_rows(), iteration=dg.rows()["iteration"], has_file=dg.file is not None)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
