"""Explicit large-eddy simulation: a Smagorinsky or WALE eddy viscosity and the subgrid term it adds to the right-hand side,
on the device (csrc/les.hip).  Not in the reference (Xcompact3d has both models; x3d2 has none yet): this project's addition.

    case = make_channel((256, 129, 128), fused=True)
    case.solver.les = Les(case.solver, LesConfig(model="wale", cw=0.5))   # or model="smagorinsky", cs=0.17
    case.run(n_iters=...)
    m = case.solver.les.monitor()   # nut_mean, nut_max, eps_sgs, diffusion_number: one host wait, only when asked

Model, with g_ij = du_i/dx_j and S_ij = 1/2 (g_ij + g_ji):
    filter width   D2 = (h_x[i] h_y[j] h_z[k])^(2/3), h_d = 1 / diagnostics.spacing_tables(mesh)[d]: a stretched y is handled.
                   The host forms a_d = h_d^(2/3) once per Les object; the kernel takes D2 = a_x[i] a_y[j] a_z[k].
    Smagorinsky    nu_t = C_s^2 D2 sqrt(2 S:S)
    WALE           G = g g, Sd_ij = 1/2 (G_ij + G_ji) - 1/3 delta_ij G_kk,
                   nu_t = C_w^2 D2 (Sd:Sd)^(3/2) / ((S:S)^(5/2) + (Sd:Sd)^(5/4)), 0 where the denominator is 0
    stress         tau_ij = 2 nu_t S_ij;  the term is sgs_i = sum_j d/dx_j tau_ij with the der1st operator of each direction
The defaults C_s = 0.17 and C_w = 0.5 are this project's choice (common textbook values), not the reference's.

The conservative form needs 9 + 9 operator applications (the non-conservative one 21), no block beyond the nine gradient
blocks, and conserves momentum exactly on a periodic box.  Its known weakness: der1st applied twice vanishes at the Nyquist
mode, so the model does not damp the 2 Delta wave.

Les.add(du, dv, dw), called by BaseCase.substep right after the case's forcings: flush_grad, the nine gradients
(Solver.velocity_gradients), ONE kernel that turns them into the stress in place and leaves four scalars on the device
(HipBackend.les_stress), nine tds_apply(accumulate=True), the nine blocks released (stream-ordered).  No call waits for the
host.  Several ranks: tds_apply and spacing_tables are decomposition-aware, the term needs nothing more; monitor() combines
its row in two collectives.  Les has no state: checkpoint and restart need nothing new.

Not served, each an X3dError with nothing launched: transported species (eddy diffusivity for scalars is not built, and
molecular-only scalars next to an LES velocity would be silently inconsistent); a Neumann boundary (the stress components'
parities would need der1st_sym choices that are not built; periodic and Dirichlet are served -- for Dirichlet der1st and
der1st_sym coincide); an unknown model; a negative constant."""
import numpy as np
import torch

from .common import BC_NEUMANN, DIR_X, DIR_Y, DIR_Z, VERT, X3dError
from .diagnostics import spacing_tables

MODELS = ("smagorinsky", "wale")
NSLOT = 4  # sum nu_t, sum 2 nu_t S:S, max nu_t, max nu_t (ih_x^2 + ih_y^2 + ih_z^2)
# the block of the nine (compute_vorticity's order) that holds tau_ij after the kernel; nu_t is in block 3, blocks 6 and 7
# keep their gradients
TAU_BLOCK = ((0, 1, 2), (1, 4, 5), (2, 5, 8))
NUT_BLOCK = 3


class LesConfig:
    """the model ("smagorinsky" or "wale") and its constant: cs (default 0.17) or cw (default 0.5)"""

    def __init__(self, model="smagorinsky", cs=0.17, cw=0.5):
        self.model = str(model).lower()
        if self.model not in MODELS:
            raise X3dError("LesConfig: unknown model %r (one of %s)" % (model, ", ".join(MODELS)))
        self.cs, self.cw = float(cs), float(cw)
        if not self.cs >= 0.0 or not self.cw >= 0.0:
            raise X3dError("LesConfig: a model constant must not be negative")

    @property
    def constant(self):
        return self.cs if self.model == "smagorinsky" else self.cw

    @property
    def c2(self):
        """the square the kernel multiplies by"""
        return self.constant * self.constant


def width_tables(mesh):
    """this rank's three tables a_d = h_d^(2/3), h_d = 1 / spacing_tables(mesh)[d] (float64, one value per local vertex):
    a_x[i] a_y[j] a_z[k] is the filter width squared"""
    return [np.ascontiguousarray((1.0 / ih) ** (2.0 / 3.0)) for ih in spacing_tables(mesh)]


def check_served(solver):
    if int(getattr(solver, "nspecies", 0)) > 0:
        raise X3dError("Les: transported species are not served (eddy diffusivity for scalars is not built)")
    if np.any(np.asarray(solver.mesh.BCs_global) == BC_NEUMANN):
        raise X3dError("Les: a Neumann boundary is not served (periodic and Dirichlet are)")


class Les:
    """Les(solver, cfg), attached as `solver.les = Les(solver, cfg)`"""

    def __init__(self, solver, cfg=None):
        self.cfg = cfg = cfg or LesConfig()
        check_served(solver)
        self.solver = solver
        b, m = solver.backend, solver.mesh
        self.n_vert = float(np.prod(m.get_global_dims(VERT)))
        self.a_host, self.ih_host = width_tables(m), spacing_tables(m)
        self.a = [torch.from_numpy(t).to(b.device) for t in self.a_host]
        self.ih = [torch.from_numpy(t).to(b.device) for t in self.ih_host]
        self.row = torch.zeros(NSLOT, dtype=torch.float64, device=b.device)  # of the last add()

    def stress(self, grads, row=None):
        """the nine gradient blocks -> stress and eddy viscosity in place (TAU_BLOCK, NUT_BLOCK), the four scalars -> row (a
        device float64 tensor of 4 values; default: this object's); no host wait"""
        row = self.row if row is None else row
        if row.dtype != torch.float64 or not row.is_cuda or row.numel() < NSLOT:
            raise X3dError("Les.stress: row is a device float64 tensor of 4 values")
        self.solver.backend.les_stress(grads, self.cfg.model, self.cfg.c2, self.a, self.ih, row.data_ptr())
        return row

    def add(self, du, dv, dw):
        """d_i += sum_j d/dx_j tau_ij of the solver's velocity; no host wait"""
        s = self.solver
        b = s.backend
        s.flush_grad()  # a velocity correction left pending is not in u, v, w yet
        grads = s.velocity_gradients()
        self.stress(grads)
        for i, d in enumerate((du, dv, dw)):
            for j, (dirps, direction) in enumerate(((s.xdirps, DIR_X), (s.ydirps, DIR_Y), (s.zdirps, DIR_Z))):
                b.tds_apply(d, grads[TAU_BLOCK[i][j]], dirps.der1st, direction, accumulate=True)
        for g in grads:  # (stream-ordered: whoever takes them next writes behind the operators)
            b.allocator.release_block(g)

    def monitor(self):
        """{nut_mean, nut_max, eps_sgs, diffusion_number} of the last add(), over all ranks: ONE host wait (and, on
        several ranks, two collectives: every rank calls it).  eps_sgs = <2 nu_t S:S>, the subgrid dissipation;
        diffusion_number = dt max nu_t (1/h_x^2 + 1/h_y^2 + 1/h_z^2), the explicit diffusion number of the term."""
        s = self.solver
        raw = self.row.cpu().numpy().copy()
        comm = s.backend.comm
        if comm.size > 1:
            sums, maxs = torch.from_numpy(raw[:2].copy()), torch.from_numpy(raw[2:].copy())
            comm.allreduce_tensor(sums, "sum")
            comm.allreduce_tensor(maxs, "max")
            raw[:2], raw[2:] = sums.numpy(), maxs.numpy()
        return {"nut_mean": float(raw[0]) / self.n_vert, "nut_max": float(raw[2]), "eps_sgs": float(raw[1]) / self.n_vert,
                "diffusion_number": float(s.dt) * float(raw[3])}
