"""The reference's cylinder step composed from the oracle's pieces (a test helper, not product code).

base_case.f90:261-289 with case/cylinder.f90's hooks and module/ibm.f90's body:
  define_BC (compute_outflow_params) ; transeq ; time_integrator%step ; apply_BC (X_FACE stamp) ; ibm%body ;
  pressure_correction
The oracle supplies transeq, the integrator, the pressure correction and the monitoring; what it lacks -- the three plane
reductions, field_set_face_from_field(X_FACE) (src/backend/omp/backend.f90:978-1003) and the mask product -- is plain
numpy here.  test_ibm_host.py pins the composition: with a mask of ones and the BC steps off it IS orc.Solver.step."""
import numpy as np

from oracle import x3d_oracle as orc


def smooth_perturbation(mesh, seed=7):
    """three smooth fields [nz, ny, nx] with seeded amplitudes of a few per cent: zero at both x ends, periodic in y, z"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.02, 0.05, size=3)
    ph = rng.uniform(0.0, 2.0 * np.pi, size=3)
    X = np.pi * np.asarray(mesh.vert_coords[0])[None, None, :] / mesh.L[0]
    Y = 2 * np.pi * np.asarray(mesh.vert_coords[1])[None, :, None] / mesh.L[1]
    Z = 2 * np.pi * np.asarray(mesh.vert_coords[2])[:, None, None] / mesh.L[2]
    return (a[0] * np.sin(X) ** 2 * np.cos(Y + ph[0]) * np.cos(Z), a[1] * np.sin(2 * X) ** 2 * np.sin(Y + ph[1]) * np.cos(Z),
            a[2] * np.sin(X) ** 2 * np.cos(Y) * np.sin(Z + ph[2]))


class CylinderRef:
    def __init__(self, dims, L, Re=300.0, dt=0.0075, time_intg="AB3", ep1=None, bc=True, bc_x=("dirichlet", "dirichlet")):
        self.mesh = orc.Mesh(list(dims), [1, 1, 1], list(L), list(bc_x), ["periodic"] * 2, ["periodic"] * 2)
        self.o = orc.Solver(self.mesh, Re=Re, dt=dt, time_intg=time_intg, poisson="FFT")
        self.bc = bool(bc)
        self.gdt = 0.0  # time_integrator%gdt: 0 until the first stage has run (time_integrator.f90:125-126)
        self.out_vel = self.flow_rate_diff = 0.0
        self.inlet = (1.0, 0.0, 0.0)  # define_BC_cylinder with inlet_noise = 0
        o, b = self.o, self.o.backend
        for f in (o.u, o.v, o.w):
            f.data_loc = orc.VERT
        self.ep1 = None if ep1 is None else np.array(ep1, dtype=np.float64)
        self.ep1_field = None
        if ep1 is not None:
            # src/module/ibm.f90:126-132: a block of ones (padding included) with ep1 on the vertices
            nz, ny, nx = self.ep1.shape
            c = b.get_block(orc.DIR_C, orc.VERT)
            c.data[...] = 1.0
            c.data[:nz, :ny, :nx] = self.ep1
            self.ep1_field = b.get_block(orc.DIR_X, orc.VERT)
            b.reorder(self.ep1_field, c, orc.RDR[(orc.DIR_C, orc.DIR_X)])

    def set_velocity(self, u, v, w):
        o = self.o
        for f, a in zip((o.u, o.v, o.w), (u, v, w)):
            o.backend.set_field_data(f, np.asarray(a, dtype=np.float64))

    def velocity(self):
        o = self.o
        return tuple(o.backend.get_field_data(f) for f in (o.u, o.v, o.w))

    def _stage_gdt(self):
        """what time_integrator%step will leave in gdt (:182, :246)"""
        ti = self.o.time_integrator
        if ti.method == "AB":
            return self.o.dt
        return ti.RK_B[ti.order][ti.istage - 1] * self.o.dt

    def outflow_params(self):
        """compute_outflow_params, src/case/cylinder.f90:109-147"""
        u = self.o.backend.get_field_data(self.o.u)
        nz, ny, nx = u.shape
        ny_nz = float(ny * nz)
        out_vel = float(u[:, :, nx - 2].max()) * self.gdt / float(self.mesh.d[0])
        return out_vel, float(u[:, :, 0].sum()) / ny_nz - float(u[:, :, nx - 1].sum()) / ny_nz

    def step(self):
        o, b = self.o, self.o.backend
        curr = [o.u, o.v, o.w]
        for _ in range(o.time_integrator.nstage):
            if self.bc:  # define_BC: the parameters see the gdt of the PREVIOUS stage
                self.out_vel, self.flow_rate_diff = self.outflow_params()
            deriv = [b.get_block(orc.DIR_X) for _ in range(3)]
            o.transeq(deriv, curr)
            self.gdt = self._stage_gdt()
            o.time_integrator.step(curr, deriv, o.dt)
            if self.bc:  # apply_BC: field_set_face_from_field(X_FACE, flow_rate_diff=)
                for f, start in zip(curr, self.inlet):
                    a = b.get_field_data(f)
                    a[:, :, 0] = start
                    fd, fd1 = a[:, :, -1].copy(), a[:, :, -2]
                    a[:, :, -1] = fd - self.out_vel * (fd - fd1) + self.flow_rate_diff
                    b.set_field_data(f, a)
            if self.ep1_field is not None:  # ibm%body
                for f in curr:
                    b.vecmult(f, self.ep1_field)
            o.pressure_correction(o.u, o.v, o.w)

    def monitor(self):
        return self.o.monitor()
