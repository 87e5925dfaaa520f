"""x3d2_amd: MI355X-native backend for x3d2's per-timestep hot path.

The compute path is libx3d2_hip.so (hand-written HIP for gfx950 behind the C
ABI of include/x3d2_hip.h); the modules here mirror the reference's host-side
operator interface (base_backend_t, tdsops_t, poisson_fft_t, solver_t, ...)."""
from .common import *  # noqa: F401,F403
from .mesh import Mesh  # noqa: F401
from .tdsops import Dirps, Tdsops  # noqa: F401


def make_tgv(n, nproc_dir=(1, 1, 1), rank=0, Re=1600.0, dt=1e-3, time_intg="RK3", poisson="FFT", comm=None,
             device=None, fused=False, n_species=0, pr_species=None, lazy=None, lowmem_transeq=False, L=None):
    """TGV set-up of examples/TGV/input.x3d on an n^3 (or (nx,ny,nz)) grid; L: domain lengths (default 2 pi each)."""
    from .backend import HipBackend
    from .case import TGVCase
    from .solver import Solver, SolverConfig
    dims = (n, n, n) if isinstance(n, int) else tuple(n)
    twopi = 6.283185307179586
    mesh = Mesh(dims, nproc_dir, (twopi,) * 3 if L is None else tuple(L), ("periodic",) * 2, ("periodic",) * 2,
                ("periodic",) * 2, nrank=rank)
    backend = HipBackend(mesh, device=device, comm=comm, lazy=lazy)
    solver = Solver(backend, mesh, SolverConfig(Re=Re, dt=dt, time_intg=time_intg, poisson_solver_type=poisson,
                                                 fused=fused, n_species=n_species, pr_species=pr_species,
                                                 lowmem_transeq=lowmem_transeq))
    return TGVCase(solver)


def make_hit(n, L=None, Re=1600.0, dt=1e-3, time_intg="RK3", k0=4.0, ke0=0.5, seed=0, forcing=None, fused=True,
             nproc_dir=(1, 1, 1), rank=0, comm=None, poisson="FFT", device=None, lazy=None):
    """homogeneous isotropic turbulence on an n^3 (or (nx, ny, nz)) three-periodic box L (default 2 pi each): an initial field
    with E(k) ~ k^4 exp(-2 (k / k0)^2) and kinetic energy ke0 from default_rng(seed) (case.hit_initial_field), and, with
    forcing = a forcing.ForcingConfig, the band forcing attached as solver.forcing.  y and z may be cut, x never.  Not in the
    reference."""
    from .backend import HipBackend
    from .case import HITCase, HITConfig
    from .solver import Solver, SolverConfig
    dims = (n, n, n) if isinstance(n, int) else tuple(n)
    twopi = 6.283185307179586
    cfg = HITConfig(k0=k0, ke0=ke0, seed=seed)
    if forcing is not None:
        from .forcing import Forcing, ForcingConfig
        if not isinstance(forcing, ForcingConfig):
            raise X3dError("make_hit: forcing is a ForcingConfig or None")
        if int(tuple(nproc_dir)[0]) > 1:
            raise X3dError("make_hit: x is never cut (nproc_dir[0] = %d)" % int(tuple(nproc_dir)[0]))
    mesh = Mesh(dims, tuple(nproc_dir), (twopi,) * 3 if L is None else tuple(L), ("periodic",) * 2, ("periodic",) * 2,
                ("periodic",) * 2, nrank=rank)
    backend = HipBackend(mesh, device=device, comm=comm, lazy=lazy)
    solver = Solver(backend, mesh, SolverConfig(Re=Re, dt=dt, time_intg=time_intg, poisson_solver_type=poisson, fused=fused))
    if forcing is not None:
        solver.forcing = Forcing(solver, forcing)  # (refuses before the case generates its field)
    return HITCase(solver, cfg)


def make_channel(dims=(128, 65, 64), L=(4.0, 2.0, 2.0), stretching="top-bottom", beta=0.259065151, Re=4200.0,
                 dt=5e-3, time_intg="RK3", poisson="FFT", fused=False, device=None, comm=None, nproc_dir=(1, 1, 1),
                 rank=0, lazy=None, lowmem_transeq=False, n_species=0, pr_species=None, **channel_kw):
    """channel set-up of examples/channel/input.x3d: periodic x/z, no-slip y walls (Dirichlet),
    y stretched towards the walls; channel_kw -> ChannelConfig (rotation, omega_rot, n_rotate, noise).
    dims, L: the GLOBAL grid; nproc_dir = (1, 1, N): z slabs (the wall-normal direction stays whole on every rank:
    poisson_fft.HipSlabPoissonFFT010)"""
    from .backend import HipBackend
    from .case import ChannelCase, ChannelConfig
    from .solver import Solver, SolverConfig
    st = ("uniform", stretching, "uniform")
    mesh = Mesh(tuple(dims), tuple(nproc_dir), tuple(L), ("periodic",) * 2, ("dirichlet",) * 2, ("periodic",) * 2,
                st, (1.0, beta, 1.0), nrank=rank)
    backend = HipBackend(mesh, device=device, comm=comm, lazy=lazy)
    solver = Solver(backend, mesh, SolverConfig(Re=Re, dt=dt, time_intg=time_intg, poisson_solver_type=poisson,
                                                 fused=fused, lowmem_transeq=lowmem_transeq, n_species=n_species,
                                                 pr_species=pr_species))
    return ChannelCase(solver, ChannelConfig(**channel_kw))


def make_rayleigh_benard(dims=(128, 65, 128), L=(4.0, 1.0, 4.0), Ra=1e6, Pr=1.0, stretching="uniform", beta=0.259065151,
                         dt=2e-3, time_intg="RK3", poisson="FFT", fused=False, device=None, comm=None, nproc_dir=(1, 1, 1),
                         rank=0, noise=1e-3, seed=None, les=None, **scalars_kw):
    """Rayleigh-Benard convection on the channel's mesh and Poisson path (periodic x / z, no-slip y walls, z slabs allowed) in
    free-fall units: Re = sqrt(Ra / Pr), one species (the temperature, pr_species = [Pr]) held at 1 below and 0 above, buoyancy
    ri = 1 along up = (0, 1, 0), the fluid at rest on the conduction profile plus a seeded perturbation of amplitude `noise`
    (case.RayleighBenardCase).  case.scalars is the attached scalars.Scalars with profile_dir = 2; scalars_kw -> its
    ScalarsConfig (initstat, istatfreq, istatout, prefix).  les: a les.LesConfig, or None (no model) -- les.Les is attached
    as solver.les before the scalars, with the eddy diffusivity nu_t / Pr_t for the temperature; a config without prt gets
    prt = 0.85, which is this project's choice (a common value for air-like fluids), not the reference's.  Not in the
    reference."""
    import math
    from .backend import HipBackend
    from .case import RayleighBenardCase, RayleighBenardConfig
    from .solver import Solver, SolverConfig
    if not (Ra > 0.0 and Pr > 0.0 and math.isfinite(Ra) and math.isfinite(Pr)):
        raise X3dError("make_rayleigh_benard: Ra and Pr are positive and finite")
    mesh = Mesh(tuple(dims), tuple(nproc_dir), tuple(L), ("periodic",) * 2, ("dirichlet",) * 2, ("periodic",) * 2,
                ("uniform", stretching, "uniform"), (1.0, beta, 1.0), nrank=rank)
    backend = HipBackend(mesh, device=device, comm=comm)
    solver = Solver(backend, mesh, SolverConfig(Re=math.sqrt(Ra / Pr), dt=dt, time_intg=time_intg, poisson_solver_type=poisson,
                                                 fused=fused, n_species=1, pr_species=[Pr]))
    if les is not None:
        from .les import Les, LesConfig
        if not isinstance(les, LesConfig):
            raise X3dError("make_rayleigh_benard: les is a LesConfig or None")
        if les.prt is None:
            les = LesConfig(model=les.model, cs=les.cs, cw=les.cw, prt=0.85)
        solver.les = Les(solver, les)  # (before the case attaches Scalars, which asks the model whether it serves species)
    return RayleighBenardCase(solver, RayleighBenardConfig(noise=noise, seed=seed, **scalars_kw))


def make_cylinder(dims=(257, 128, 32), L=(20.0, 12.0, 6.0), Re=300.0, dt=0.0075, time_intg="AB3", poisson="FFT",
                  fused=False, device=None, lazy=None, centre=None, radius=0.5, ep1=None, **cylinder_kw):
    """cylinder set-up of examples/cylinder/input.x3d: Dirichlet ends in x (inflow / convective outflow), periodic
    y and z, AB3, immersed boundary on; cylinder_kw -> CylinderConfig (init_noise, inlet_noise, seed).  One rank.

    The reference reads its body from a file written by an outside tool.  The default here is this project's own choice:
    a circular cylinder of diameter 1 (radius 0.5) along z through (L_x / 4, L_y / 2).  centre / radius change it,
    ep1 (numpy [nz, ny, nx]) replaces it by any mask."""
    from .backend import HipBackend
    from .case import CylinderCase, CylinderConfig
    from .ibm import Ibm, cylinder_mask
    from .solver import Solver, SolverConfig
    mesh = Mesh(tuple(dims), (1, 1, 1), tuple(L), ("dirichlet",) * 2, ("periodic",) * 2, ("periodic",) * 2)
    backend = HipBackend(mesh, device=device, lazy=lazy)
    solver = Solver(backend, mesh, SolverConfig(Re=Re, dt=dt, time_intg=time_intg, poisson_solver_type=poisson,
                                                 fused=fused, ibm_on=True))
    own_body = ep1 is None
    if own_body:
        ep1 = cylinder_mask(mesh, (L[0] / 4.0, L[1] / 2.0) if centre is None else centre, radius, axis=2)
    solver.ibm = Ibm(solver, ep1)
    if own_body:
        solver.ibm.area_ref = 2.0 * float(radius) * float(L[2])  # D * L_z: the frontal area the loads' coefficients refer to
    return CylinderCase(solver, CylinderConfig(**cylinder_kw))
