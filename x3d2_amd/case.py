"""Flow cases: mirror of base_case_t%run (/root/reference/src/case/base_case.f90:181-353),
the TGV case (src/case/tgv.f90), the channel (src/case/channel.f90), the cylinder (src/case/cylinder.f90) and the
monitoring series
(src/postprocess/monitoring.f90:46-90)."""
import time

import numpy as np

from .common import BC_DIRICHLET, CELL, DIR_X, DIR_Z, VERT, Y_FACE, X3dError


class Monitoring:
    """enstrophy = 1/(2N) sum |curl u|^2 ; max / mean |div u|"""

    def __init__(self, solver):
        self.solver = solver
        self.rows = []

    def write_step(self, t, u, v, w):
        s = self.solver
        s.flush_grad()  # a velocity correction left pending by step(more=True) is completed first
        b, al = s.backend, s.backend.allocator
        du, dv, dw = (al.get_block(DIR_X, VERT) for _ in range(3))
        s.curl(du, dv, dw, u, v, w)
        enstrophy = 0.5 * (b.scalar_product(du, du) + b.scalar_product(dv, dv)
                           + b.scalar_product(dw, dw)) / s.ngrid
        for f in (du, dv, dw):
            al.release_block(f)
        div_u = al.get_block(DIR_Z)
        s.divergence_v2p(div_u, u, v, w)
        div_u_max, div_u_mean = b.field_max_mean(div_u)
        al.release_block(div_u)
        row = (t, enstrophy, div_u_max, div_u_mean)
        self.rows.append(row)
        return row

    def kinetic_energy(self):
        """1/(2N) sum (u^2+v^2+w^2): not written by the reference, asked for by the north star"""
        s = self.solver
        s.flush_grad()
        b = s.backend
        return 0.5 * (b.scalar_product(s.u, s.u) + b.scalar_product(s.v, s.v)
                      + b.scalar_product(s.w, s.w)) / s.ngrid


class BaseCase:
    def __init__(self, solver):
        self.solver = solver
        self.monitoring = Monitoring(solver)
        self.stats = None  # optional stats.Stats(solver, cfg): run() then samples and writes it (io_manager, base_case.f90:319-329)
        self.spectra = None  # optional spectra.Spectra(solver, cfg): run() then samples and writes it (not in the reference)
        self.snapshots = None  # optional snapshot.Snapshots(solver, cfg): run() then writes it (handle_io_step, :307-329)
        # optional checkpoint.Checkpoints(solver, cfg, case): run() then writes it (handle_io_step); restarted is set by
        # checkpoint.restore (io_mgr%is_restart, :212)
        self.checkpoints = None
        # optional diagnostics.Diagnostics(solver, cfg, append=self.restarted): run() then samples, polls and finalises it
        self.diagnostics = None
        self.budgets = None  # optional budgets.Budgets(solver, cfg): run() then samples and writes it (not in the reference)
        # optional loads.Loads(solver, cfg, append=self.restarted): Ibm.body then takes the force on the body along; run()
        # polls and finalises it.  It reads no completed state: not one of `attached` below
        self.loads = None
        # optional probes.Probes(solver, cfg, append=self.restarted): run() then samples, polls and finalises it
        self.probes = None
        # optional particles.Particles(solver, cfg): run() then advances it at every step, writes, polls and finalises it (not in
        # the reference)
        self.particles = None
        self.restarted = False
        self.step_times = []
        self.initial_conditions()

    # hooks, src/case/base_case.f90:42-46
    def initial_conditions(self):
        raise NotImplementedError

    def define_BC(self):
        pass

    def forcings(self, du, dv, dw, it):
        pass

    def apply_BC(self, u, v, w):
        pass

    def deferred_walls(self):
        """three fields whose y faces are ALL that apply_BC would stamp on u, v, w (then the fused driver does it
        inside the kernels that form the new velocity), or None: apply_BC has to run as it is"""
        return None

    def forcings_idle(self, it):
        """True: forcings() does not touch the derivatives in iteration `it` whenever Solver.transeq_fused leaves the last
        accumulation of transeq pending (the fused driver may then fold it and the RK stage together)"""
        return type(self).forcings is BaseCase.forcings

    def correction_deferrable(self):
        """True: between a sub-step's pressure correction and the next sub-step's transeq_x no hook of this case reads
        the velocity in a way that needs the correction applied -- it may then wait for that kernel
        (Solver.transeq_fused).  The base hooks read nothing; a case that overrides define_BC / apply_BC says so itself."""
        return type(self).define_BC is BaseCase.define_BC and type(self).apply_BC is BaseCase.apply_BC

    def mean_target_of_next_BC(self):
        """the target of the field_mean_shift(u, target) this case's define_BC will ask for at the start of the next
        sub-step, or None"""
        return None

    def postprocess(self, it, t):
        return self.monitoring.write_step(t, self.solver.u, self.solver.v, self.solver.w)

    def checkpoint_state(self):
        """checkpoint_state_t (src/io/checkpoint_state.f90): what a restarted run needs of the case beyond the solver's
        fields, as a dict of scalars; written under `case_<key>` by checkpoint.Checkpoints"""
        return {}

    def load_checkpoint_state(self, state):
        pass

    def substep(self, it, last=True):
        """body of the sub_iter loop, base_case.f90:261-289"""
        s = self.solver
        al = s.backend.allocator
        curr = [s.u, s.v, s.w] + list(s.species)  # base_case.f90:236-241
        self.define_BC()
        deriv = [al.get_block(DIR_X) for _ in range(s.nvars)]
        # nothing reads the new velocity between the stage and the pressure correction when the case has no
        # BC hook: its update may then be formed inside the pressure correction's first kernels
        # (a case whose BC hook only stamps wall values hands them over instead: deferred_walls)
        walls = self.deferred_walls() if s.fused and not s.sw.no_defer_walls else None
        defer_upd = (s.fused and (type(self).apply_BC is BaseCase.apply_BC or walls is not None)
                     and not s.sw.no_defer and s.time_integrator.sname.upper().startswith("RK"))
        ibm = s.ibm
        if ibm is not None:
            # ibm%body masks the COMPLETED velocity with the BCs already stamped (base_case.f90:281-285): the new velocity
            # cannot be formed inside the pressure correction's first kernels then -- the explicit order
            walls, defer_upd = None, False
        les = s.les
        sca = s.scalars
        frc = s.forcing
        fb = s.particle_feedback
        if s.fused and les is None and frc is None and fb is None and self.forcings_idle(it) and (sca is None or not sca.coupled):
            # nothing touches the derivatives between transeq and the RK / AB stage: the last accumulation of
            # transeq may be folded into the stage's linear combination (Solver.transeq_fused)
            pending = s.transeq(deriv, curr, defer=True)
            if type(self).forcings is not BaseCase.forcings:
                self.forcings(deriv[0], deriv[1], deriv[2], it)  # (idle, see forcings_idle -- or nothing is pending)
            s.time_integrator.step(curr, deriv, s.dt, pending=pending, defer_update=defer_upd)
        else:
            s.transeq(deriv, curr)
            self.forcings(deriv[0], deriv[1], deriv[2], it)
            if frc is not None:
                # the band forcing reads the velocity transeq has completed and needs the derivatives stored, like the subgrid term;
                # its coefficients are those of THIS sub-step's velocity (forcing.Forcing: no state)
                frc.add(deriv[0], deriv[1], deriv[2], s.u, s.v, s.w)
            if fb is not None:
                # the drag reaction of two-way coupled particles: the records of the last update, the same in every sub-step of
                # the step (particles.Feedback); eight sparse passes over the stored derivatives
                fb.add(deriv[0], deriv[1], deriv[2])
            if les is not None:
                # the subgrid term reads the velocity transeq has completed (pending correction, bulk shift) and needs the
                # derivatives stored: never the deferred branch above
                if getattr(les, "serves_species", False):  # (eddy diffusivity: the species' subgrid flux with it)
                    les.add(deriv[0], deriv[1], deriv[2], deriv[3:], curr[3:])
                else:
                    les.add(deriv[0], deriv[1], deriv[2])
            if sca is not None:
                # buoyancy and the imposed-gradient term need the derivatives stored, like the subgrid term
                sca.add(deriv, curr)
            if s.fused:
                s.time_integrator.step(curr, deriv, s.dt, defer_update=defer_upd)
            else:
                s.time_integrator.step(curr, deriv, s.dt)
        if not defer_upd:
            for f in deriv:
                al.release_block(f)
            deriv = []
        if defer_upd and walls is not None:
            s.pending_walls = walls  # apply_BC happens inside the pressure correction's first kernels
        else:
            self.apply_BC(s.u, s.v, s.w)
        if sca is not None:
            sca.apply_bc()  # (species are never part of a deferred update: the stage has written them)
        if ibm is not None:
            ibm.body(s.u, s.v, s.w)
        # not the last sub-step of the step and no hook looks at the velocity before the next transeq: its
        # pressure-gradient correction can wait for that kernel (Solver.transeq_fused)
        defer_grad = not last and s.fused and self.correction_deferrable()
        if defer_grad:
            # (a case whose next define_BC wants the volume integral of u says so: the kernel that forms the new u takes it
            #  along, Solver.pressure_correction_fused / take_mean_shift)
            s.mean_request = self.mean_target_of_next_BC()
            s.pressure_correction(s.u, s.v, s.w, defer_grad=True)
        else:
            s.pressure_correction(s.u, s.v, s.w)
        for f in deriv:  # (kept until the deferred updates that read them were done)
            al.release_block(f)

    def step(self, it, more=False, want_pressure=False):
        """one time step.  more=True: another step follows at once and nothing looks at the fields in between, so
        the last sub-step's velocity correction may also wait for the next transeq_x kernel; whoever reads the
        velocity next without going through step() must call solver.flush_grad() first (run() does).
        want_pressure: a snapshot or a budgets sample of this step is due and solver.keep_pressure is set -- the fused driver then keeps
        the pressure of the step's last sub-step (Solver.pressure_correction_fused)."""
        s = self.solver
        ns = s.time_integrator.nstage
        for i in range(ns):
            if s.keep_pressure:  # (fused driver: only the last sub-step of a snapshot step keeps its pressure)
                s.pressure_wanted = bool(want_pressure) and i == ns - 1
            self.substep(it, last=(i == ns - 1 and not more))

    def run(self, n_iters=None, verbose=False):
        s = self.solver
        n_iters = s.n_iters if n_iters is None else n_iters
        if self.restarted and n_iters <= s.current_iter:  # base_case.f90:218-221
            raise X3dError("Restart requires n_iters greater than the restart iteration.")
        self.postprocess(s.current_iter, s.current_iter * s.dt)
        start = s.current_iter + 1
        for it in range(start, n_iters + 1):
            t0 = time.perf_counter()
            diag, snap, ckpt, bud = self.diagnostics, self.snapshots, self.checkpoints, self.budgets
            # a statistics, spectra or budgets sample, a row of the diagnostics series, a snapshot
            # (snapshot_manager.f90:125-126) and a checkpoint (checkpoint_manager.f90, handle_checkpoint_step) read the
            # velocity like an output step does
            loads, probes, parts, sca = self.loads, self.probes, self.particles, s.scalars
            attached = [a for a in (self.stats, self.spectra, diag, bud, probes, parts, snap, ckpt, sca) if a is not None]
            read = (s.n_output > 0 and it % s.n_output == 0) or any(a.reads_state(it) for a in attached)
            snap_due = snap is not None and snap.reads_state(it)
            budgets_due = bud is not None and bud.pressure_due(it)  # (a budgets sample with pressure=True reads it too)
            self.step(it, more=(it < n_iters and not read), want_pressure=(snap_due or budgets_due) and s.keep_pressure)
            s.current_iter = it
            if self.stats is not None:
                self.stats.update(it)  # update_stats, base_case.f90:319
            if sca is not None:
                sca.update(it)  # one pass over u, v, w and the species, the recurrence; no host wait
            if self.spectra is not None:
                self.spectra.update(it)  # the transforms and the reductions; no host wait
            if diag is not None:
                diag.update(it)  # nine gradients, one reduction into the device table; no host wait
            if bud is not None:
                bud.update(it)  # nine gradients, the vertex pressure, one reduction, the recurrence; no host wait
            if probes is not None:
                probes.update(it)  # one gather into the device table; no host wait
            if parts is not None:
                parts.update(it)  # one launch: advance, boundaries, sample (and the sort when it is due); no host wait
            if s.n_output > 0 and it % s.n_output == 0:
                row = self.postprocess(it, it * s.dt)
                if verbose and s.mesh.is_root():
                    print("time = %g iteration = %d enstrophy: %.13e div u max mean: %.3e %.3e"
                          % (row[0], it, row[1], row[2], row[3]))
            if self.stats is not None:
                self.stats.write(it)  # handle_io_step, base_case.f90:328
            if sca is not None:
                sca.write(it)
            if self.spectra is not None:
                self.spectra.write(it)
            if bud is not None:
                bud.write(it)
            if snap is not None:
                snap.write(it)  # packs and starts the copy; no host wait
                snap.poll()     # files of the snapshots whose copies have landed
            if parts is not None:
                parts.write(it)  # packs and starts the copy; no host wait
                parts.poll()
            if diag is not None:
                diag.poll()     # rows of the tables whose copies have landed
            if loads is not None:
                loads.poll()
            if probes is not None:
                probes.poll()
            if ckpt is not None:
                if ckpt.cfg.due(it):
                    for series in (diag, loads, probes):
                        if series is not None:
                            series.flush()  # the series on disk reaches the checkpoint it may be continued from
                ckpt.write(it)  # one pack launch, one asynchronous copy; no host wait
                ckpt.poll()     # the file of a checkpoint whose copy has landed
            s.backend.sync()
            self.step_times.append(time.perf_counter() - t0)
        s.flush_grad()
        if self.snapshots is not None:
            self.snapshots.finalise()
        if self.checkpoints is not None:
            self.checkpoints.finalise()
        if self.diagnostics is not None:
            self.diagnostics.finalise()
        if self.loads is not None:
            self.loads.finalise()
        if self.probes is not None:
            self.probes.finalise()
        if self.particles is not None:
            self.particles.finalise()
        return self.monitoring.rows


class TGVCase(BaseCase):
    """src/case/tgv.f90:40-72"""

    def initial_conditions(self):
        s = self.solver
        m = s.mesh
        x = m.vert_coords[0][None, None, :]
        y = m.vert_coords[1][None, :, None]
        z = m.vert_coords[2][:, None, None]
        for f in (s.u, s.v, s.w):
            f.set_data_loc(VERT)
        s.backend.set_field_data(s.u, np.sin(x) * np.cos(y) * np.cos(z))
        s.backend.set_field_data(s.v, -np.cos(x) * np.sin(y) * np.cos(z))
        s.w.fill(0.0)


class HITConfig:
    """k0: the peak of the initial spectrum E(k) ~ k^4 exp(-2 (k / k0)^2); ke0: the initial kinetic energy 1/2 <u.u>; seed: of
    numpy's default_rng"""

    def __init__(self, k0=4.0, ke0=0.5, seed=0):
        self.k0, self.ke0, self.seed = float(k0), float(ke0), int(seed)
        if not (self.k0 > 0.0 and self.ke0 > 0.0 and np.isfinite(self.k0) and np.isfinite(self.ke0)):
            raise X3dError("HITConfig: k0 and ke0 are positive and finite")
        if self.seed < 0:
            raise X3dError("HITConfig: the seed must not be negative")


def hit_initial_field(n, L, k0=4.0, ke0=0.5, seed=0):
    """u, v, w [nz, ny, nx] on the GLOBAL three-periodic vertex grid n = (nx, ny, nz) of the box L, in float64 on the host: three
    white-noise fields (default_rng(seed).standard_normal((nz, ny, nx)) for u, then v, then w), their rfftn times
    |k| exp(-(|k| / k0)^2) (E(k) ~ k^4 exp(-2 (k / k0)^2), peak at k0), the Nyquist planes and the mean zeroed, the solenoidal
    projection with the spectral k, the irfftn, and one scale factor so that 1/2 <u.u> = ke0"""
    nx, ny, nz = (int(v) for v in n)
    rng = np.random.default_rng(int(seed))
    axes = (0, 1, 2)
    hat = [np.fft.rfftn(rng.standard_normal((nz, ny, nx)), axes=axes) for _ in range(3)]
    kz = (2.0 * np.pi / float(L[2])) * (np.fft.fftfreq(nz) * nz)[:, None, None]
    ky = (2.0 * np.pi / float(L[1])) * (np.fft.fftfreq(ny) * ny)[None, :, None]
    kx = (2.0 * np.pi / float(L[0])) * np.arange(nx // 2 + 1, dtype=np.float64)[None, None, :]
    kk = kx * kx + ky * ky + kz * kz
    k = np.sqrt(kk)
    shape = k * np.exp(-(k / float(k0)) ** 2)
    keep = np.ones(kk.shape)
    keep[0, 0, 0] = 0.0
    if nz % 2 == 0:
        keep[nz // 2, :, :] = 0.0
    if ny % 2 == 0:
        keep[:, ny // 2, :] = 0.0
    if nx % 2 == 0:
        keep[:, :, nx // 2] = 0.0
    hat = [h * shape * keep for h in hat]
    kk_safe = np.where(kk > 0.0, kk, 1.0)
    div = (kx * hat[0] + ky * hat[1] + kz * hat[2]) / kk_safe
    hat = [hat[0] - kx * div, hat[1] - ky * div, hat[2] - kz * div]
    f = [np.fft.irfftn(h, s=(nz, ny, nx), axes=axes) for h in hat]
    ke = 0.5 * float(np.mean(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]))
    if not ke > 0.0:
        raise X3dError("hit_initial_field: the field is empty (k0 = %r on %r points)" % (k0, (nx, ny, nz)))
    a = np.sqrt(float(ke0) / ke)
    return [np.ascontiguousarray(a * x) for x in f]


class HITCase(BaseCase):
    """Homogeneous isotropic turbulence in a three-periodic box; not in the reference.  The initial field has a prescribed
    spectrum (hit_initial_field, generated on the host from the GLOBAL grid, so that every rank slices the same field); with a
    forcing.Forcing attached as solver.forcing (make_hit does it) the large scales are held and the flow becomes stationary."""

    def __init__(self, solver, hit_cfg=None):
        self.hit_cfg = hit_cfg or HITConfig()
        super().__init__(solver)

    def initial_conditions(self):
        s, m, c = self.solver, self.solver.mesh, self.hit_cfg
        if not all(m.periodic_BC) or any(m.stretched):
            raise X3dError("HITCase: a three-periodic uniform box")
        nx, ny, nz = (int(v) for v in m.get_dims(VERT))
        ox, oy, oz = (int(o) for o in m.n_offset)
        fields = hit_initial_field(m.get_global_dims(VERT), m.L, c.k0, c.ke0, c.seed)
        for f, a in zip((s.u, s.v, s.w), fields):
            f.set_data_loc(VERT)
            s.backend.set_field_data(f, np.ascontiguousarray(a[oz:oz + nz, oy:oy + ny, ox:ox + nx]))

    def checkpoint_state(self):
        # (for the record only: the fields are in the checkpoint)
        c = self.hit_cfg
        return {"seed": np.uint64(c.seed), "k0": np.float64(c.k0), "ke0": np.float64(c.ke0)}

    def load_checkpoint_state(self, state):
        c = self.hit_cfg
        c.seed, c.k0, c.ke0 = int(state["seed"]), float(state["k0"]), float(state["ke0"])


class ChannelConfig:
    """channel_config_t, src/config.f90:46-54, 207-249 (namelist channel_nml)"""

    def __init__(self, init_noise=(0.0, 0.0, 0.0), inlet_noise=(0.0, 0.0, 0.0), rotation=False, omega_rot=0.0,
                 n_rotate=0, seed=None):
        self.init_noise, self.inlet_noise = tuple(init_noise), tuple(inlet_noise)
        self.rotation, self.omega_rot, self.n_rotate = bool(rotation), float(omega_rot), int(n_rotate)
        self.seed = seed  # the reference draws unseeded random_number; a seed makes runs repeatable


class ChannelCase(BaseCase):
    """src/case/channel.f90: bulk velocity held at 2/3 by a shift of u, optional rotation forcing
    for the first n_rotate iterations, no-slip y walls stamped after each sub-step.

    The reference rebuilds the wall values on the host and uploads three full DIR_C blocks per
    sub-step (:97-130); here the three wall fields live on the device, are zero-filled once when
    inlet_noise = 0 (the example's setting) and only rewritten when noise is asked for."""

    def __init__(self, solver, channel_cfg=None):
        self.channel_cfg = channel_cfg or ChannelConfig()
        self.rng = np.random.default_rng(self.channel_cfg.seed)  # initial condition (host, once)
        seed = self.channel_cfg.seed
        self.noise_seed = int(seed) if seed is not None else int(np.random.SeedSequence().entropy) & (2 ** 63 - 1)
        self.noise_draws = 0
        self.bc_start_y = None
        super().__init__(solver)

    def initial_conditions(self):  # :139-189
        s, m = self.solver, self.solver.mesh
        nx, ny, nz = m.get_dims(VERT)
        y = m.vert_coords[1][None, :, None] - m.L[1] / 2.0
        um = np.exp(-0.2 * y * y)
        noise = [self.channel_cfg.inlet_noise[2]] * 3  # :154 takes inlet_noise(3) for all three
        shape = (nz, ny, nx)
        fields = []
        for c, base in enumerate((1.0 - y * y, 0.0, 0.0)):
            r = self.rng.random(shape) if noise[c] != 0.0 else 0.5
            f = base + noise[c] * um * (2 * r - 1.0) * np.ones(shape)
            f[:, 0, :] = 0.0
            f[:, -1, :] = 0.0
            fields.append(f)
        for f, a in zip((s.u, s.v, s.w), fields):
            f.set_data_loc(VERT)
            s.backend.set_field_data(f, a)

    def define_BC(self):  # :53-137
        s, b = self.solver, self.solver.backend
        # ub -> 2/3, no host round trip on one rank; fused driver: the shift itself is left to transeq_x's kernel
        sh = None
        if s.fused and not s.sw.no_rot_fused:
            # (round 6: the integral may have been taken by the kernel that formed this u, mean_target_of_next_BC)
            sh = s.take_mean_shift(s.u, 2.0 / 3.0) or b.field_mean_shift(s.u, 2.0 / 3.0)
        if sh is not None:
            s.shift_request = sh
        else:
            b.field_shift_to_mean(s.u, 2.0 / 3.0)
        noise = self.channel_cfg.inlet_noise
        first = self.bc_start_y is None
        if first:
            self.bc_start_y = [b.allocator.get_block(DIR_X, VERT) for _ in range(3)]
            for f in self.bc_start_y:
                f.set_data_loc(VERT)
                f.fill(0.0)
        if any(n != 0.0 for n in noise):
            # the reference draws six random_number planes on the host and uploads three full blocks per
            # sub-step (:97-130); here the wall planes are generated in place (x3d_wall_noise).  `draw` numbers
            # the draws so that a run is repeatable for a given seed (the reference's is not: unseeded)
            for c, (f, n) in enumerate(zip(self.bc_start_y, noise)):
                b.wall_noise(f, n, self.noise_seed, 3 * self.noise_draws + c)
            self.noise_draws += 1

    def checkpoint_state(self):
        return {"noise_seed": np.uint64(self.noise_seed), "noise_draws": np.int64(self.noise_draws)}

    def load_checkpoint_state(self, state):
        self.noise_seed, self.noise_draws = int(state["noise_seed"]), int(state["noise_draws"])

    def substep(self, it, last=True):
        c, s = self.channel_cfg, self.solver
        # fused driver: the rotation forcing is offered to transeq_x's kernel (Solver.transeq_fused); forcings()
        # below applies it with the reference's two vecadd's when that kernel did not take it
        s.rot_request = c.omega_rot if (s.fused and c.rotation and it < c.n_rotate) else 0.0
        super().substep(it, last)

    def forcings(self, du, dv, dw, it):  # :191-207
        c, s = self.channel_cfg, self.solver
        if s.rot_applied:
            s.rot_applied = False
            return
        if c.rotation and it < c.n_rotate:
            s.backend.vecadd(-c.omega_rot, s.v, 1.0, du)
            s.backend.vecadd(c.omega_rot, s.u, 1.0, dv)

    def deferred_walls(self):
        return self.bc_start_y

    def mean_target_of_next_BC(self):
        return 2.0 / 3.0 if not self.solver.sw.no_mean_in_lincomb else None

    def correction_deferrable(self):
        # define_BC reads the volume integral of u only, and the pending correction does not change it: dp/dx is a
        # periodic compact x derivative (stagder_p2v: A d = B p with circulant A, B and zero row sums of B), so every x
        # pencil of it sums to zero up to rounding; apply_BC's walls are stamped BEFORE the correction (as in the
        # reference: apply_BC ; pressure_correction) by the kernels that form the new velocity (deferred_walls).
        # One rank only: field_mean_shift hands the shift over as a device scalar (X3D_NO_ROT_FUSED=1: host path).
        # Offered where the x kernel takes the correction along: 1024-row x pencils (csrc/xwide.hip, k_xwide_transeq3_upd).
        s = self.solver
        return (s.fused and s.backend.comm.size == 1 and int(s.mesh.get_dims(VERT)[0]) == 1024
                and not s.sw.no_rot_fused and not s.sw.no_channel_defer_grad
                and type(self).define_BC is ChannelCase.define_BC and type(self).apply_BC is ChannelCase.apply_BC)

    def forcings_idle(self, it):
        # no rotation in this iteration, or transeq_x's kernel applies it (rot_request, substep above) -- and where that
        # kernel does not, Solver.transeq_fused leaves nothing pending and forcings() below acts as in the reference
        # (a subclass with its own forcings() must see complete derivatives: ADVICE round 5)
        return type(self).forcings is ChannelCase.forcings

    def apply_BC(self, u, v, w):  # :214-231
        b = self.solver.backend
        for f, st in zip((u, v, w), self.bc_start_y):
            b.field_set_face_from_field(f, st, 0.0, Y_FACE)


class RayleighBenardConfig:
    """noise: amplitude of the seeded perturbation of the conduction profile; seed: of numpy's default_rng (None: drawn once
    and carried by the checkpoints); scalars_kw -> ScalarsConfig (initstat, istatfreq, istatout, prefix)"""

    def __init__(self, noise=1e-3, seed=None, **scalars_kw):
        self.noise = float(noise)
        self.seed = int(seed) if seed is not None else int(np.random.SeedSequence().entropy) & (2 ** 63 - 1)
        self.scalars_kw = dict(scalars_kw)


class RayleighBenardCase(BaseCase):
    """Rayleigh-Benard convection between two no-slip walls in y, periodic in x and z; not in the reference.  Free-fall
    units: the solver's Re is sqrt(Ra / Pr), its one species the temperature with pr_species = [Pr], held at 1 on the lower
    and 0 on the upper wall, and buoyancy ri = 1 along up = (0, 1, 0) (scalars.Scalars, attached by this case as
    solver.scalars with profile_dir = 2).  The fluid starts at rest on the conduction profile plus a seeded perturbation:
        phi = 1 - y / H + noise sin(pi y / H) (2 r - 1),   r from default_rng(seed) on the GLOBAL grid, so that ranks agree
    The velocity is held at zero on the walls the way the channel holds it (three zero wall fields, deferred_walls)."""

    def __init__(self, solver, rb_cfg=None):
        self.rb_cfg = rb_cfg or RayleighBenardConfig()
        self.bc_start_y = None
        super().__init__(solver)

    @property
    def scalars(self):
        return self.solver.scalars

    def initial_conditions(self):
        from .scalars import Scalars, ScalarsConfig
        s, m, c = self.solver, self.solver.mesh, self.rb_cfg
        if s.nspecies != 1:
            raise X3dError("RayleighBenardCase: the solver transports one species, the temperature")
        for f in (s.u, s.v, s.w):
            f.set_data_loc(VERT)
            f.fill(0.0)
        gx, gy, gz = (int(n) for n in m.get_global_dims(VERT))
        nx, ny, nz = m.get_dims(VERT)
        ox, oy, oz = (int(o) for o in m.n_offset)
        H = float(m.L[1])
        y = np.asarray(m.vert_coords[1])[None, :, None]
        phi = (1.0 - y / H) * np.ones((nz, ny, nx))
        if c.noise != 0.0:
            r = np.random.default_rng(c.seed).random((gz, gy, gx))[oz:oz + nz, oy:oy + ny, ox:ox + nx]
            phi = phi + c.noise * np.sin(np.pi * y / H) * (2.0 * r - 1.0)
        self.bc_start_y = [s.backend.allocator.get_block(DIR_X, VERT) for _ in range(3)]
        for f in self.bc_start_y:
            f.fill(0.0)
        s.scalars = Scalars(s, ScalarsConfig(ri=[1.0], ref=[0.0], up=(0, 1, 0), wall=[{"y": (1.0, 0.0)}], init=[phi],
                                             profile_dir=2, **c.scalars_kw))

    def checkpoint_state(self):
        return {"seed": np.uint64(self.rb_cfg.seed)}

    def load_checkpoint_state(self, state):
        self.rb_cfg.seed = int(state["seed"])

    def deferred_walls(self):
        return self.bc_start_y

    def apply_BC(self, u, v, w):
        b = self.solver.backend
        for f, st in zip((u, v, w), self.bc_start_y):
            b.field_set_face_from_field(f, st, 0.0, Y_FACE)


class CylinderConfig:
    """cylinder_config_t, src/config.f90:56-61, 251-286 (namelist cylinder_nml)"""

    def __init__(self, init_noise=(0.0, 0.0, 0.0), inlet_noise=(0.0, 0.0, 0.0), seed=None):
        self.init_noise, self.inlet_noise = tuple(float(n) for n in init_noise), tuple(float(n) for n in inlet_noise)
        self.seed = seed  # the reference draws unseeded random_number; a seed makes runs repeatable


class CylinderCase(BaseCase):
    """src/case/cylinder.f90: uniform inflow u = 1 at x = 0, convective outflow at x = L_x, the body through the
    solver's immersed boundary (solver.ibm).

    The reference takes three slice reductions through the host, rebuilds the inlet profile there and uploads three
    full blocks per sub-step (:129-134, 192-218), then stamps the faces with three launches (:231-242).  Here the two
    outflow parameters stay on the device (x3d_outflow_params), the inlet fields are filled once when inlet_noise = 0
    (the example's setting) and regenerated in place otherwise (x3d_inlet_noise), and apply_BC is one launch that
    reads the parameters where they are (x3d_cylinder_apply_bc).  No call of a sub-step waits for the host.

    One rank: the non-periodic Poisson solve is not built for a decomposed mesh."""

    def __init__(self, solver, cylinder_cfg=None):
        self.cylinder_cfg = cylinder_cfg or CylinderConfig()
        seed = self.cylinder_cfg.seed
        self.rng = np.random.default_rng(seed)  # initial condition (host, once)
        self.noise_seed = int(seed) if seed is not None else int(np.random.SeedSequence().entropy) & (2 ** 63 - 1)
        self.noise_draws = 0
        self.bc_start_x = None   # bc_start_u_x / v_x / w_x: the inlet fields
        self.params = None       # device address of {out_vel, flow_rate_diff}
        self.out_vel = self.flow_rate_diff = 0.0
        self.outflow_rows = []   # (t, out_vel, flow_rate_diff) next to monitoring.rows
        if solver.backend.comm.size > 1:
            raise X3dError("CylinderCase: one rank only")
        super().__init__(solver)

    def initial_conditions(self):  # :56-102
        s, m = self.solver, self.solver.mesh
        nx, ny, nz = m.get_dims(VERT)
        x = m.vert_coords[0][None, None, :] - m.L[0] / 2.0
        um = np.exp(-0.2 * x * x)
        shape = (nz, ny, nx)
        noise = self.cylinder_cfg.init_noise
        for f, base, n in zip((s.u, s.v, s.w), (1.0, 0.0, 0.0), noise):
            r = self.rng.random(shape) if n != 0.0 else 0.5
            f.set_data_loc(VERT)
            s.backend.set_field_data(f, base + n * um * (2 * r - 1.0) * np.ones(shape))

    def define_BC(self):  # :159-219
        s, b = self.solver, self.solver.backend
        # Two quirks of the reference are kept.  (1) define_BC runs BEFORE this sub-step's integrator stage, so gdt is
        # the previous stage's -- and 0.0 on the very first sub-step (time_integrator.f90 initialises it so): out_vel is
        # then 0 and the first outflow stamp only adds flow_rate_diff.  (2) flow_rate_diff divides by THIS rank's
        # ny * nz (:124-126), not the global plane.
        self.params = b.outflow_params(s.u, s.time_integrator.gdt, float(s.mesh.d[0]))
        noise = self.cylinder_cfg.inlet_noise
        first = self.bc_start_x is None
        if first:
            self.bc_start_x = [b.allocator.get_block(DIR_X, VERT) for _ in range(3)]
            for f, base in zip(self.bc_start_x, (1.0, 0.0, 0.0)):
                f.set_data_loc(VERT)
                f.fill(base)  # (only the plane x = 1 is ever read)
        if any(n != 0.0 for n in noise):
            half_L = float(s.mesh.L[0]) / 2.0
            um = float(np.exp(-0.2 * half_L * half_L))  # :169-170, folded into the amplitude
            for c, (f, base, n) in enumerate(zip(self.bc_start_x, (1.0, 0.0, 0.0), noise)):
                b.inlet_noise(f, base, n * um, self.noise_seed, 3 * self.noise_draws + c)
            self.noise_draws += 1

    def checkpoint_state(self):
        # (out_vel / flow_rate_diff: the row postprocess writes before the restarted run's first define_BC)
        return {"noise_seed": np.uint64(self.noise_seed), "noise_draws": np.int64(self.noise_draws),
                "out_vel": np.float64(self.out_vel), "flow_rate_diff": np.float64(self.flow_rate_diff)}

    def load_checkpoint_state(self, state):
        self.noise_seed, self.noise_draws = int(state["noise_seed"]), int(state["noise_draws"])
        self.out_vel, self.flow_rate_diff = float(state["out_vel"]), float(state["flow_rate_diff"])

    def apply_BC(self, u, v, w):  # :226-243
        fu, fv, fw = self.bc_start_x
        self.solver.backend.cylinder_apply_bc(u, v, w, fu, fv, fw, self.params)

    def postprocess(self, it, t):  # :258-274
        if self.params is not None:
            self.out_vel, self.flow_rate_diff = self.solver.backend.outflow_params_get()
        self.outflow_rows.append((t, self.out_vel, self.flow_rate_diff))
        return super().postprocess(it, t)
