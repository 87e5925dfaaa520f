// Point probes: the velocity at a few hundred fixed vertices, gathered into a row of a device table.
//
// Not in the reference: this project's own addition, like the diagnostics series whose table -> pinned copy -> file path it
// shares.  A probe sits ON a vertex (the host snaps every point to its nearest one), so a sample is the field's own value
// widened to double: one launch, one thread per (owned probe, field), no interpolation, no host.
#include "common.h"

#include <algorithm>

struct x3d_probe {
    x3d_backend *b;
    int n_owned, n_total;
    int imax, jmax, kmax;  // the largest local index per direction over the owned probes (-1 without any)
    int4 *pts;             // device [n_owned]: (i, j, k, slot), 0-based local vertex indices
};

extern "C" int x3d_probe_create(x3d_backend *b, const int *ijk_local, int n_owned, const int *slot_of, int n_total,
                                x3d_probe **out)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && out && (n_owned == 0 || (ijk_local && slot_of)), "x3d_probe_create: null argument");
    X3D_REQUIRE(n_total >= 1 && n_total <= X3D_PROBE_MAX, "x3d_probe_create: %d probes, 1 to %d can be held", n_total,
                X3D_PROBE_MAX);
    X3D_REQUIRE(n_owned >= 0 && n_owned <= n_total, "x3d_probe_create: %d of %d probes owned", n_owned, n_total);
    std::vector<int4> pts((size_t)n_owned);
    std::vector<char> taken((size_t)n_total, 0);
    int imax = -1, jmax = -1, kmax = -1;
    for (int q = 0; q < n_owned; q++) {
        const int i = ijk_local[3 * q], j = ijk_local[3 * q + 1], k = ijk_local[3 * q + 2], s = slot_of[q];
        X3D_REQUIRE(i >= 0 && i < b->nx && j >= 0 && j < b->ny && k >= 0 && k < b->nz,
                    "x3d_probe_create: probe %d at (%d,%d,%d) is outside this rank's vertices (%d,%d,%d)", q, i, j, k, b->nx,
                    b->ny, b->nz);
        X3D_REQUIRE(s >= 0 && s < n_total, "x3d_probe_create: probe %d has slot %d of %d", q, s, n_total);
        X3D_REQUIRE(!taken[s], "x3d_probe_create: slot %d has two owners", s);
        taken[s] = 1;
        pts[q] = make_int4(i, j, k, s);
        imax = std::max(imax, i); jmax = std::max(jmax, j); kmax = std::max(kmax, k);
    }
    x3d_probe *p = new x3d_probe();
    p->b = b;
    p->n_owned = n_owned; p->n_total = n_total;
    p->imax = imax; p->jmax = jmax; p->kmax = kmax;
    p->pts = nullptr;
    if (n_owned > 0) {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->pts), sizeof(int4) * pts.size());
        // (the host vector dies with this call: a synchronous copy)
        if (e == hipSuccess) e = hipMemcpy(p->pts, pts.data(), sizeof(int4) * pts.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (p->pts) hipFree(p->pts);
            delete p;
            x3d_set_error("x3d_probe_create: %s", hipGetErrorString(e));
            return 1;
        }
    }
    *out = p;
    return 0;
}

extern "C" int x3d_probe_destroy(x3d_probe *p)
{
    X3D_RANGE(__func__);
    if (!p) return 0;
    if (p->pts) hipFree(p->pts);
    delete p;
    return 0;
}

struct Probe3 {
    const real_t *f[3];
};

__global__ void __launch_bounds__(256) k_probe_sample(Probe3 F, const int4 *__restrict__ pts, int n_owned, long nxp, long nyp,
                                                      double *__restrict__ row)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 3 * n_owned) return;
    const int q = t / 3, c = t - 3 * q;
    const int4 e = pts[q];
    row[3 * e.w + c] = (double)F.f[c][nxp * (e.y + nyp * (long)e.z) + e.x];
}

extern "C" int x3d_probe_sample(x3d_backend *b, const x3d_probe *p, const real_t *u, const real_t *v, const real_t *w,
                                const int dims[3], double *row_dev)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && p && u && v && w && dims && row_dev, "x3d_probe_sample: null argument");
    X3D_REQUIRE(p->b == b, "x3d_probe_sample: the probes belong to another backend");
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_probe_sample: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    X3D_REQUIRE(p->imax < dims[0] && p->jmax < dims[1] && p->kmax < dims[2],
                "x3d_probe_sample: a probe lies outside dims (%d,%d,%d)", dims[0], dims[1], dims[2]);
    if (p->n_owned == 0) return 0;  // this rank's slots stay at the zero the row was cleared to
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    Probe3 F;
    F.f[0] = u; F.f[1] = v; F.f[2] = w;
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_probe_sample, dim3((unsigned)((3 * p->n_owned + 255) / 256)), dim3(256), 0, b->stream, F,
                       (const int4 *)p->pts, p->n_owned, (long)b->nxp, (long)b->nyp, row_dev);
    X3D_HIP(hipGetLastError());
    return 0;
}
