"""Explicit large-eddy simulation: a Smagorinsky or WALE eddy viscosity and the subgrid term it adds to the right-hand side,
on the device (csrc/les.hip).  Not in the reference (Xcompact3d has both models; x3d2 has none yet): this project's addition.

    case = make_channel((256, 129, 128), fused=True)
    case.solver.les = Les(case.solver, LesConfig(model="wale", cw=0.5))   # or model="smagorinsky", cs=0.17
    case.run(n_iters=...)
    m = case.solver.les.monitor()   # nut_mean, nut_max, eps_sgs, diffusion_number: one host wait, only when asked
    # with transported species: LesConfig(model="wale", prt=0.85) adds their eddy diffusivity (below)

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

Species: LesConfig(prt=...) gives every transported species the eddy diffusivity kappa_t = nu_t / Pr_t (prt: one number for
all species or a list with one per species; 0.85 is a common choice for heat in air-like fluids) and the subgrid flux in
conservative form,
    q_j = kappa_t dphi_s/dx_j        dphi_s += sum_j d/dx_j q_j        with the der1st operator of each direction.
Les.add(du, dv, dw, dphi, phi) does this after the nine momentum accumulations, with nu_t still in block 3: species in groups
of at most two, their six gradients written with tds_apply into six of the blocks the momentum divergence has consumed (0, 1,
2, 4, 5, 8), ONE launch per group (HipBackend.les_scalar_flux: q_j in place, sum kappa_t |grad phi_s|^2 into Les.row_phi on the
device), three tds_apply(accumulate=True) per species.  No tenth block, no host wait.  monitor() then also gives eps_phi =
[<kappa_t |grad phi_s|^2>] and diffusion_number_phi = diffusion_number / min(prt).  Without species arguments the calls are
exactly those above.  Scalars (x3d2_amd/scalars.py) accepts a Les with serves_species and no other model.  Still no state.

Not served, each an X3dError with nothing launched: transported species without prt (molecular-only scalars next to an LES
velocity would be silently inconsistent); a prt that is not positive and finite; a prt list whose length is not the solver's
number of species (refused by check_served, which Les.__init__ calls: the config does not know the solver); a Neumann
boundary (the stress components' parities would need der1st_sym choices that are not built; periodic and Dirichlet are
served -- for Dirichlet der1st and der1st_sym coincide); an unknown model; a negative constant.

Not built: the dynamic procedure; wall damping for Smagorinsky; the subgrid flux in Scalars' flux profiles and nu_vol (they
hold the resolved flux only; nu_lo / nu_hi at a wall are unaffected where nu_t vanishes there, as WALE's does)."""
import math

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
# the blocks that take the gradients of a group of two species once the momentum divergence has consumed the stress: x, y, z
# of the first, then of the second (blocks 6 and 7 stay spare)
PHI_BLOCK = (0, 1, 2, 4, 5, 8)


def _prt_value(x):
    """a turbulent Prandtl (Schmidt) number: a positive finite number, nothing else"""
    if isinstance(x, (str, bytes, bool)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise X3dError("LesConfig: prt is a positive finite number, a list of them (one per species) or None (got %r)" % (x,))
    x = float(x)
    if not (math.isfinite(x) and x > 0.0):
        raise X3dError("LesConfig: a turbulent Prandtl number must be finite and positive (got %r)" % x)
    return x


class LesConfig:
    """the model ("smagorinsky" or "wale") and its constant: cs (default 0.17) or cw (default 0.5); prt: the turbulent Prandtl
    (Schmidt) number of the transported species -- None (default: a solver with species is refused), one positive finite
    number for every species, or a list with one per species.  The list's length is checked where the solver is known:
    check_served, which Les.__init__ calls."""

    def __init__(self, model="smagorinsky", cs=0.17, cw=0.5, prt=None):
        self.model = str(model).lower()
        if self.model not in MODELS:
            raise X3dError("LesConfig: unknown model %r (one of %s)" % (model, ", ".join(MODELS)))
        self.cs, self.cw = float(cs), float(cw)
        if not self.cs >= 0.0 or not self.cw >= 0.0:
            raise X3dError("LesConfig: a model constant must not be negative")
        if prt is None:
            self.prt = None
        elif isinstance(prt, (list, tuple)):
            if not prt:
                raise X3dError("LesConfig: prt is an empty list")
            self.prt = [_prt_value(x) for x in prt]
        else:
            self.prt = _prt_value(prt)

    def prt_of(self, nspecies):
        """[Pr_t] * nspecies, or None when prt was not given"""
        if self.prt is None:
            return None
        return list(self.prt) if isinstance(self.prt, list) else [self.prt] * int(nspecies)

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


def check_served(solver, cfg=None):
    """X3dError for what Les does not serve; cfg = None: as for a LesConfig without prt"""
    ns = int(getattr(solver, "nspecies", 0))
    prt = None if cfg is None else cfg.prt
    if ns > 0 and prt is None:
        raise X3dError("Les: transported species are not served without a turbulent Prandtl number (LesConfig(prt=...): "
                       "molecular-only scalars next to an LES velocity would be silently inconsistent)")
    if isinstance(prt, list) and len(prt) != ns:
        raise X3dError("Les: prt has %d entries, the solver %d species" % (len(prt), ns))
    if np.any(np.asarray(solver.mesh.BCs_global) == BC_NEUMANN):
        raise X3dError("Les: a Neumann boundary is not served (periodic and Dirichlet are)")


class Les:
    """Les(solver, cfg), attached as `solver.les = Les(solver, cfg)`"""

    def __init__(self, solver, cfg=None):
        self.cfg = cfg = cfg or LesConfig()
        check_served(solver, cfg)
        self.solver = solver
        b, m = solver.backend, solver.mesh
        self.n_vert = float(np.prod(m.get_global_dims(VERT)))
        self.a_host, self.ih_host = width_tables(m), spacing_tables(m)
        self.a = [torch.from_numpy(t).to(b.device) for t in self.a_host]
        self.ih = [torch.from_numpy(t).to(b.device) for t in self.ih_host]
        ns = int(getattr(solver, "nspecies", 0))
        self.prt = cfg.prt_of(ns) if ns > 0 else None
        self.inv_prt = [1.0 / p for p in self.prt] if self.prt else []
        # of the last add(): the model's four scalars, then sum kappa_t |grad phi_s|^2 per served species -- one tensor, so
        # that monitor() reads both with one copy
        self._rows = torch.zeros(NSLOT + len(self.inv_prt), dtype=torch.float64, device=b.device)
        self.row, self.row_phi = self._rows[:NSLOT], self._rows[NSLOT:]

    @property
    def serves_species(self):
        """does add() take the species?  (prt was given and the solver transports some)"""
        return bool(self.inv_prt)

    def stress(self, grads, row=None):
        """the nine gradient blocks -> stress and eddy viscosity in place (TAU_BLOCK, NUT_BLOCK), the four scalars -> row (a
        device float64 tensor of 4 values; default: this object's); no host wait"""
        row = self.row if row is None else row
        if row.dtype != torch.float64 or not row.is_cuda or row.numel() < NSLOT:
            raise X3dError("Les.stress: row is a device float64 tensor of 4 values")
        self.solver.backend.les_stress(grads, self.cfg.model, self.cfg.c2, self.a, self.ih, row.data_ptr())
        return row

    def add(self, du, dv, dw, dphi=None, phi=None):
        """d_i += sum_j d/dx_j tau_ij of the solver's velocity and, with dphi and phi (the species' derivatives and values,
        one each per species of the solver), dphi_s += sum_j d/dx_j (nu_t / Pr_t,s dphi_s/dx_j); no host wait"""
        s = self.solver
        b = s.backend
        species = dphi is not None or phi is not None
        if species:
            if not self.serves_species:
                raise X3dError("Les.add: species are served only with LesConfig(prt=...) on a solver that transports some")
            if dphi is None or phi is None or len(dphi) != len(self.inv_prt) or len(phi) != len(self.inv_prt):
                raise X3dError("Les.add: one derivative and one value block per species expected")
        dirs = ((s.xdirps, DIR_X), (s.ydirps, DIR_Y), (s.zdirps, DIR_Z))
        s.flush_grad()  # a velocity correction left pending is not in u, v, w yet
        grads = s.velocity_gradients()
        self.stress(grads)
        for i, d in enumerate((du, dv, dw)):
            for j, (dirps, direction) in enumerate(dirs):
                b.tds_apply(d, grads[TAU_BLOCK[i][j]], dirps.der1st, direction, accumulate=True)
        if species:
            # the momentum divergence has consumed the stress: its blocks take the species' gradients, two species at a
            # time, next to nu_t, which is still in block 3
            for s0 in range(0, len(self.inv_prt), 2):
                n = min(2, len(self.inv_prt) - s0)
                gb = [grads[m] for m in PHI_BLOCK[:3 * n]]
                for q in range(n):
                    for j, (dirps, direction) in enumerate(dirs):
                        b.tds_apply(gb[3 * q + j], phi[s0 + q], dirps.der1st, direction)
                b.les_scalar_flux(grads[NUT_BLOCK], gb, self.inv_prt[s0:s0 + n], self.row_phi.data_ptr() + 8 * s0)
                for q in range(n):
                    for j, (dirps, direction) in enumerate(dirs):
                        b.tds_apply(dphi[s0 + q], gb[3 * q + j], dirps.der1st, direction, accumulate=True)
        for g in grads:  # (stream-ordered: whoever takes them next writes behind the operators)
            b.allocator.release_block(g)

    def monitor(self):
        """{nut_mean, nut_max, eps_sgs, diffusion_number} of the last add(), over all ranks: ONE host wait (and, on
        several ranks, two collectives: every rank calls it).  eps_sgs = <2 nu_t S:S>, the subgrid dissipation;
        diffusion_number = dt max nu_t (1/h_x^2 + 1/h_y^2 + 1/h_z^2), the explicit diffusion number of the term.  With species
        served also eps_phi = [<nu_t / Pr_t,s |grad phi_s|^2>], the subgrid dissipation of each species' variance (its sums
        travel in the sum collective), and diffusion_number_phi = diffusion_number / min(Pr_t)."""
        s = self.solver
        raw = self._rows.cpu().numpy().copy()
        comm = s.backend.comm
        if comm.size > 1:
            sums = torch.from_numpy(np.concatenate([raw[:2], raw[NSLOT:]]))
            maxs = torch.from_numpy(raw[2:NSLOT].copy())
            comm.allreduce_tensor(sums, "sum")
            comm.allreduce_tensor(maxs, "max")
            raw[:2], raw[2:NSLOT], raw[NSLOT:] = sums.numpy()[:2], maxs.numpy(), sums.numpy()[2:]
        out = {"nut_mean": float(raw[0]) / self.n_vert, "nut_max": float(raw[2]), "eps_sgs": float(raw[1]) / self.n_vert,
               "diffusion_number": float(s.dt) * float(raw[3])}
        if self.serves_species:
            out["eps_phi"] = [float(x) / self.n_vert for x in raw[NSLOT:]]
            out["diffusion_number_phi"] = out["diffusion_number"] / min(self.prt)
        return out
