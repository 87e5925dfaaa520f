"""worker of the two-rank test of the LES eddy diffusivity (tests/test_hip_les_scalar.py): N processes share cuda:0 and exchange
through gloo (host-staged), like tests/mp_les_worker.py.  Every rank adds the subgrid terms of its part of the same global
noisy fields to zeroed blocks and saves its part of the species' term and the monitor figures it holds (the global ones)."""
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
    import test_hip_les_scalar as ts
    from x3d2_amd.parallel import Comm
    dphi, mon, lo, nl, _ = ts.mp_run(layout, rank, Comm())
    np.savez(out + ".%d.npz" % rank, dphi=dphi, lo=np.array(lo), nl=np.array(nl),
             mon=np.array([mon["eps_phi"][0], mon["diffusion_number_phi"]]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
