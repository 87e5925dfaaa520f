// Active scalars: what makes a transported species act on the flow and what a scalar between two walls needs.  Not in the
// reference (x3d2 transports species but never sets, bounds or couples one): this project's own addition.
//
//    d_i     +=  up_i sum_s ri_s (phi_s - ref_s)              Boussinesq buoyancy               (x3d_scalars_couple)
//    dphi_s  +=  -(G_s,x u + G_s,y v + G_s,z w)                imposed mean scalar gradient      (x3d_scalars_couple)
//    phi_s    =  value on a face                               Dirichlet wall value              (x3d_scalars_apply_bc)
//    sum phi, phi phi, u phi, v phi, w phi per plane; min, max phi                               (x3d_scalars_profile_sums)
//
// Every factor is widened to double before any product, in both flavours, as k_les_stress does; each output is rounded once
// to the real kind.  All three kernels walk whole x rows: a work item is one 16-byte vector per stream and thread, 256
// threads side by side along x in one (j, k) row, a scalar tail where the row ends inside a vector, `long` offsets on the
// padded pitches.  Row padding is never read into a result and never written.  No atomics anywhere.
#include "common.h"

#define SCA_G X3D_SCALARS_GROUP
#define SCA_NMOM X3D_SCALARS_NMOM
#define SCA_V (16 / X3D_RB)  // points per 16-byte access: 2 (FP64), 4 (FP32)
#define SCA_MAXWG 2048       // eight workgroups per CU, the rest by a grid stride: the BLAS-1 kernels' geometry
typedef real_t sca_vec __attribute__((ext_vector_type(SCA_V)));

// the vector of a row at `off` (16-byte aligned: the pitch is a multiple of 16 elements); n = points of it inside the row
__device__ __forceinline__ void sca_load(const real_t *f, long off, int n, real_t (&v)[SCA_V])
{
    if (n >= SCA_V) {
        const sca_vec x = __builtin_nontemporal_load(reinterpret_cast<const sca_vec *>(f + off));
#pragma unroll
        for (int q = 0; q < SCA_V; q++) v[q] = x[q];
    } else {
#pragma unroll
        for (int q = 0; q < SCA_V; q++) v[q] = q < n ? __builtin_nontemporal_load(f + off + q) : (real_t)0;
    }
}

__device__ __forceinline__ void sca_store(real_t *f, long off, int n, const real_t (&v)[SCA_V])
{
    if (n >= SCA_V) {
        sca_vec x;
#pragma unroll
        for (int q = 0; q < SCA_V; q++) x[q] = v[q];
        __builtin_nontemporal_store(x, reinterpret_cast<sca_vec *>(f + off));
    } else {
#pragma unroll
        for (int q = 0; q < SCA_V; q++)
            if (q < n) f[off + q] = v[q];
    }
}

// ---------------------------------------------------------------- kernel 1: the coupling terms
struct ScaCouple {
    real_t *d[3];            // momentum derivatives (touched where bit i of mom is set)
    real_t *dphi[SCA_G];     // species derivatives (touched where bit s of gmask is set)
    const real_t *vel[3];    // loaded only if gmask != 0
    const real_t *phi[SCA_G];  // loaded where bit s of bmask is set
    double up[3], ri[SCA_G], ref[SCA_G], g[SCA_G][3];
    int mom, bmask, gmask;   // run-time masks of the general form
    int nx, ny, nchunk;
    long nitem, nxp, nyp;
};

// NS: species of this group.  AXIS 0, 1, 2: the common case compiled out -- up along that one axis, every species of the
// group buoyant, no imposed gradient: phi_s read, d[AXIS] read and written, nothing else touched (24 B/DoF in FP64 at
// NS = 1).  AXIS = -1: the general form, whose masks are the same in every lane (scalar branches per item, none per point).
template <int NS, int AXIS>
__global__ void __launch_bounds__(256) k_scalars_couple(ScaCouple A)
{
    for (long t = blockIdx.x; t < A.nitem; t += gridDim.x) {
        const long row = t / A.nchunk;
        const int ch = (int)(t - row * A.nchunk);
        const int j = (int)(row % A.ny);
        const long k = row / A.ny;
        const int i0 = (ch * 256 + (int)threadIdx.x) * SCA_V;
        const long off = A.nxp * (j + A.nyp * k) + i0;
        const int n = A.nx - i0;
        if (n <= 0) continue;
        if (AXIS >= 0) {
            real_t p[NS][SCA_V], d[SCA_V];
#pragma unroll
            for (int s = 0; s < NS; s++) sca_load(A.phi[s], off, n, p[s]);
            sca_load(A.d[AXIS], off, n, d);
#pragma unroll
            for (int q = 0; q < SCA_V; q++) {
                double bs = 0.0;
#pragma unroll
                for (int s = 0; s < NS; s++) bs += A.ri[s] * ((double)p[s][q] - A.ref[s]);
                d[q] = (real_t)((double)d[q] + A.up[AXIS] * bs);
            }
            sca_store(A.d[AXIS], off, n, d);
        } else {
            real_t p[NS][SCA_V];
            double bs[SCA_V];
#pragma unroll
            for (int q = 0; q < SCA_V; q++) bs[q] = 0.0;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (A.bmask >> s & 1) {
                    sca_load(A.phi[s], off, n, p[s]);
#pragma unroll
                    for (int q = 0; q < SCA_V; q++) bs[q] += A.ri[s] * ((double)p[s][q] - A.ref[s]);
                }
            }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                if (A.mom >> i & 1) {
                    real_t d[SCA_V];
                    sca_load(A.d[i], off, n, d);
#pragma unroll
                    for (int q = 0; q < SCA_V; q++) d[q] = (real_t)((double)d[q] + A.up[i] * bs[q]);
                    sca_store(A.d[i], off, n, d);
                }
            }
            if (A.gmask) {
                real_t u[3][SCA_V];
#pragma unroll
                for (int i = 0; i < 3; i++) sca_load(A.vel[i], off, n, u[i]);
#pragma unroll
                for (int s = 0; s < NS; s++) {
                    if (A.gmask >> s & 1) {
                        real_t d[SCA_V];
                        sca_load(A.dphi[s], off, n, d);
#pragma unroll
                        for (int q = 0; q < SCA_V; q++) {
                            const double adv = (A.g[s][0] * (double)u[0][q] + A.g[s][1] * (double)u[1][q]) + A.g[s][2] * (double)u[2][q];
                            d[q] = (real_t)((double)d[q] - adv);
                        }
                        sca_store(A.dphi[s], off, n, d);
                    }
                }
            }
        }
    }
}

template <int NS>
static void sca_launch_couple(x3d_backend *b, const ScaCouple &A, int axis, int grid)
{
    switch (axis) {
    case 0: hipLaunchKernelGGL((k_scalars_couple<NS, 0>), dim3(grid), dim3(256), 0, b->stream, A); break;
    case 1: hipLaunchKernelGGL((k_scalars_couple<NS, 1>), dim3(grid), dim3(256), 0, b->stream, A); break;
    case 2: hipLaunchKernelGGL((k_scalars_couple<NS, 2>), dim3(grid), dim3(256), 0, b->stream, A); break;
    default: hipLaunchKernelGGL((k_scalars_couple<NS, -1>), dim3(grid), dim3(256), 0, b->stream, A); break;
    }
}

// More than one group: the buoyancy of ALL species in one launch, so that every momentum derivative is still rounded once.  The
// species are a run-time loop over a table in the kernel arguments (scalar loads; the sum needs no per-species registers).
#define SCA_WIDE 64
struct ScaWide {
    real_t *d[3];
    const real_t *phi[SCA_WIDE];
    double up[3], ri[SCA_WIDE], ref[SCA_WIDE];
    int n, mom;
    int nx, ny, nchunk;
    long nitem, nxp, nyp;
};

__global__ void __launch_bounds__(256) k_scalars_buoyancy_wide(ScaWide A)
{
    for (long t = blockIdx.x; t < A.nitem; t += gridDim.x) {
        const long row = t / A.nchunk;
        const int ch = (int)(t - row * A.nchunk);
        const int j = (int)(row % A.ny);
        const long k = row / A.ny;
        const int i0 = (ch * 256 + (int)threadIdx.x) * SCA_V;
        const long off = A.nxp * (j + A.nyp * k) + i0;
        const int n = A.nx - i0;
        if (n <= 0) continue;
        double bs[SCA_V];
#pragma unroll
        for (int q = 0; q < SCA_V; q++) bs[q] = 0.0;
        for (int s = 0; s < A.n; s++) {
            real_t p[SCA_V];
            sca_load(A.phi[s], off, n, p);
#pragma unroll
            for (int q = 0; q < SCA_V; q++) bs[q] += A.ri[s] * ((double)p[q] - A.ref[s]);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            if (A.mom >> i & 1) {
                real_t d[SCA_V];
                sca_load(A.d[i], off, n, d);
#pragma unroll
                for (int q = 0; q < SCA_V; q++) d[q] = (real_t)((double)d[q] + A.up[i] * bs[q]);
                sca_store(A.d[i], off, n, d);
            }
        }
    }
}

static inline bool sca_finite(double x) { return x == x && x <= 1.79e308 && x >= -1.79e308; }

static inline bool sca_dims_ok(const x3d_backend *b, const int dims[3])
{
    return dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp;
}

extern "C" int x3d_scalars_couple(x3d_backend *b, x3d_real *const d[3], x3d_real *const *dphi, const x3d_real *const vel[3],
                                  const x3d_real *const *phi, const int dims[3], const x3d_scalars_params *params)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && d && dphi && vel && phi && dims && params, "x3d_scalars_couple: null argument");
    const int ns = params->ns;
    X3D_REQUIRE(ns >= 1, "x3d_scalars_couple: ns must be at least 1 (got %d)", ns);
    X3D_REQUIRE(params->ri && params->ref, "x3d_scalars_couple: null coefficient table");
    X3D_REQUIRE(sca_dims_ok(b, dims), "x3d_scalars_couple: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    for (int i = 0; i < 3; i++) {
        X3D_REQUIRE(d[i] && vel[i], "x3d_scalars_couple: momentum block %d is null", i);
        X3D_REQUIRE(sca_finite(params->up[i]), "x3d_scalars_couple: up[%d] is not finite", i);
    }
    for (int s = 0; s < ns; s++) {
        X3D_REQUIRE(dphi[s] && phi[s], "x3d_scalars_couple: species block %d is null", s);
        X3D_REQUIRE(sca_finite(params->ri[s]) && sca_finite(params->ref[s]), "x3d_scalars_couple: ri or ref of species %d is not finite", s);
        for (int i = 0; i < 3; i++)
            X3D_REQUIRE(!params->grad || sca_finite(params->grad[3 * s + i]), "x3d_scalars_couple: grad[%d][%d] is not finite", s, i);
    }
    // outputs: d[0..2], dphi[0..ns-1]; inputs: vel[0..2], phi[0..ns-1].  No output is an input or another output.
    for (int a = 0; a < 3 + ns; a++) {
        const real_t *oa = a < 3 ? d[a] : dphi[a - 3];
        for (int c = 0; c < a; c++)
            X3D_REQUIRE(oa != (c < 3 ? d[c] : dphi[c - 3]), "x3d_scalars_couple: outputs %d and %d are the same block", c, a);
        for (int c = 0; c < 3 + ns; c++)
            X3D_REQUIRE(oa != (c < 3 ? vel[c] : phi[c - 3]), "x3d_scalars_couple: output %d is input %d", a, c);
    }
    int upmask = 0;
    for (int i = 0; i < 3; i++) upmask |= (params->up[i] != 0.0) << i;
    const int nchunk = (dims[0] + 256 * SCA_V - 1) / (256 * SCA_V);
    const long nitem = (long)dims[1] * dims[2] * nchunk;
    const int grid = (int)(nitem < SCA_MAXWG ? nitem : SCA_MAXWG);
    auto has_grad = [&](int s) {
        return params->grad && (params->grad[3 * s] != 0.0 || params->grad[3 * s + 1] != 0.0 || params->grad[3 * s + 2] != 0.0);
    };
    int nact = 0, nbuoy = 0;
    for (int s = 0; s < ns; s++) {
        const bool buoy = upmask && params->ri[s] != 0.0;
        nbuoy += buoy;
        nact += buoy || has_grad(s);
    }
    // more active species than one group holds: the buoyancy of all of them first, SCA_WIDE per launch (one launch, and one
    // rounding of each momentum derivative, up to that many); the groups below are then left the imposed-gradient terms
    const bool wide = nact > SCA_G && nbuoy > 0;
    for (int s = 0; wide && s < ns;) {
        ScaWide W = {};
        for (; s < ns && W.n < SCA_WIDE; s++) {
            if (params->ri[s] == 0.0) continue;
            const real_t *in = phi[s];
            X3D_LAZY_IN(b, in);
            W.phi[W.n] = in;
            W.ri[W.n] = params->ri[s];
            W.ref[W.n] = params->ref[s];
            W.n++;
        }
        if (W.n == 0) break;
        W.mom = upmask;
        for (int i = 0; i < 3; i++) {
            real_t *out = d[i];
            if (upmask >> i & 1) X3D_LAZY_OUT(b, out, false);
            W.d[i] = out;
            W.up[i] = params->up[i];
        }
        W.nx = dims[0];
        W.ny = dims[1];
        W.nchunk = nchunk;
        W.nitem = nitem;
        W.nxp = b->nxp;
        W.nyp = b->nyp;
        X3D_LAZY_EAGER(b);
        ProfScope ps(b, X3D_K_BLAS1);
        hipLaunchKernelGGL(k_scalars_buoyancy_wide, dim3(grid), dim3(256), 0, b->stream, W);
        X3D_HIP(hipGetLastError());
    }
    // the species that have something to do, in order, in groups of SCA_G
    int s = 0;
    while (s < ns) {
        ScaCouple A = {};
        int n = 0;
        for (; s < ns && n < SCA_G; s++) {
            const bool buoy = !wide && upmask && params->ri[s] != 0.0;
            const bool adv = has_grad(s);
            if (!buoy && !adv) continue;
            const real_t *in = phi[s];
            real_t *out = dphi[s];
            if (buoy) X3D_LAZY_IN(b, in);
            if (adv) X3D_LAZY_OUT(b, out, false);
            A.phi[n] = in;
            A.dphi[n] = out;
            A.ri[n] = buoy ? params->ri[s] : 0.0;
            A.ref[n] = params->ref[s];
            for (int i = 0; i < 3; i++) A.g[n][i] = adv ? params->grad[3 * s + i] : 0.0;
            A.bmask |= (int)buoy << n;
            A.gmask |= (int)adv << n;
            n++;
        }
        if (n == 0) break;
        A.mom = A.bmask ? upmask : 0;
        for (int i = 0; i < 3; i++) {
            real_t *out = d[i];
            const real_t *in = vel[i];
            if (A.mom >> i & 1) X3D_LAZY_OUT(b, out, false);
            if (A.gmask) X3D_LAZY_IN(b, in);
            A.d[i] = out;
            A.vel[i] = in;
            A.up[i] = params->up[i];
        }
        A.nx = dims[0];
        A.ny = dims[1];
        A.nchunk = nchunk;
        A.nitem = nitem;
        A.nxp = b->nxp;
        A.nyp = b->nyp;
        const int axis = (A.gmask == 0 && A.bmask == (1 << n) - 1 && (upmask == 1 || upmask == 2 || upmask == 4))
                             ? (upmask == 1 ? 0 : upmask == 2 ? 1 : 2) : -1;
        X3D_LAZY_EAGER(b);
        ProfScope ps(b, X3D_K_BLAS1);
        switch (n) {
        case 1: sca_launch_couple<1>(b, A, axis, grid); break;
        case 2: sca_launch_couple<2>(b, A, axis, grid); break;
        case 3: sca_launch_couple<3>(b, A, axis, grid); break;
        case 4: sca_launch_couple<4>(b, A, axis, grid); break;
        case 5: sca_launch_couple<5>(b, A, axis, grid); break;
        case 6: sca_launch_couple<6>(b, A, axis, grid); break;
        case 7: sca_launch_couple<7>(b, A, axis, grid); break;
        default: sca_launch_couple<8>(b, A, axis, grid); break;
        }
        X3D_HIP(hipGetLastError());
    }
    return 0;
}

// ---------------------------------------------------------------- kernel 2: Dirichlet wall values
struct ScaFaces {
    real_t *phi[SCA_G];
    real_t val[SCA_G][6];
    int mask[SCA_G];  // bit 2 d + side: stamp that face (requested and owned)
    int nx, ny, nz;
    long nxp, nyp;
};

// blockIdx.y = species of the group, blockIdx.z = direction d; a thread owns one point (a, c) of the two planes of d.  A
// point that a stamped face of a LATER direction also holds is left to that face's thread: x < y < z, no race.
__global__ void __launch_bounds__(256) k_scalars_faces(ScaFaces A)
{
    const int s = blockIdx.y, d = blockIdx.z;
    const int m = A.mask[s];
    if (!(m >> (2 * d) & 3)) return;
    const int na = d == 0 ? A.ny : A.nx, nc = d == 2 ? A.ny : A.nz;  // the two directions of the plane, the faster first
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)na * nc) return;
    const int a = (int)(t % na), c = (int)(t / na);
    const int i = d == 0 ? 0 : a, j = d == 0 ? a : (d == 1 ? 0 : c), k = d == 2 ? 0 : c;  // (0 along d: the first plane)
    bool later = false;  // on a stamped face of a later direction
    if (d < 1) later = later || ((m >> 2 & 1) && j == 0) || ((m >> 3 & 1) && j == A.ny - 1);
    if (d < 2) later = later || ((m >> 4 & 1) && k == 0) || ((m >> 5 & 1) && k == A.nz - 1);
    if (later) return;
    const long first = i + A.nxp * (j + A.nyp * (long)k);
    const long last = first + (d == 0 ? (long)(A.nx - 1) : d == 1 ? A.nxp * (A.ny - 1) : A.nxp * A.nyp * (A.nz - 1));
    real_t *f = A.phi[s];
    // (one plane thick in d: the last plane is also the first -- the high side, stamped second, holds then)
    if (m >> (2 * d) & 1) f[first] = A.val[s][2 * d];
    if (m >> (2 * d + 1) & 1) f[last] = A.val[s][2 * d + 1];
}

extern "C" int x3d_scalars_apply_bc(x3d_backend *b, x3d_real *const *phi, int ns, const int dims[3], const int *mask,
                                    const double *value, int own_mask)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && phi && dims && mask && value, "x3d_scalars_apply_bc: null argument");
    X3D_REQUIRE(ns >= 1, "x3d_scalars_apply_bc: ns must be at least 1 (got %d)", ns);
    X3D_REQUIRE(sca_dims_ok(b, dims), "x3d_scalars_apply_bc: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    X3D_REQUIRE(own_mask >= 0 && own_mask < 64, "x3d_scalars_apply_bc: own_mask (%d) has six bits", own_mask);
    for (int s = 0; s < ns; s++) {
        X3D_REQUIRE(phi[s], "x3d_scalars_apply_bc: species block %d is null", s);
        X3D_REQUIRE(mask[s] >= 0 && mask[s] < 64, "x3d_scalars_apply_bc: mask[%d] (%d) has six bits", s, mask[s]);
        for (int c = 0; c < s; c++) X3D_REQUIRE(phi[s] != phi[c], "x3d_scalars_apply_bc: species %d and %d are the same block", c, s);
        for (int f = 0; f < 6; f++)
            X3D_REQUIRE(!(mask[s] >> f & 1) || sca_finite(value[6 * s + f]), "x3d_scalars_apply_bc: value of face %d of species %d is not finite", f, s);
    }
    long npl = (long)dims[0] * dims[1];
    if ((long)dims[0] * dims[2] > npl) npl = (long)dims[0] * dims[2];
    if ((long)dims[1] * dims[2] > npl) npl = (long)dims[1] * dims[2];
    int s = 0;
    while (s < ns) {
        ScaFaces A = {};
        int n = 0;
        for (; s < ns && n < SCA_G; s++) {
            const int m = mask[s] & own_mask;
            if (!m) continue;
            real_t *out = phi[s];
            X3D_LAZY_OUT(b, out, false);
            A.phi[n] = out;
            A.mask[n] = m;
            for (int f = 0; f < 6; f++) A.val[n][f] = (m >> f & 1) ? (real_t)value[6 * s + f] : (real_t)0;
            n++;
        }
        if (n == 0) break;
        A.nx = dims[0];
        A.ny = dims[1];
        A.nz = dims[2];
        A.nxp = b->nxp;
        A.nyp = b->nyp;
        X3D_LAZY_EAGER(b);
        ProfScope ps(b, X3D_K_BLAS1);
        hipLaunchKernelGGL(k_scalars_faces, dim3((unsigned)((npl + 255) / 256), (unsigned)n, 3), dim3(256), 0, b->stream, A);
        X3D_HIP(hipGetLastError());
    }
    return 0;
}

// ---------------------------------------------------------------- kernel 3: plane sums, min and max
// Scheme and summation order of k_budget_rows (budget.hip): blockIdx.y = kept index q, blockIdx.x = part; a part takes the
// rows part, part + nparts, ... of q; a thread adds its items in the order it meets them, the points of a vector one after
// the other; a wave adds its lanes by the shuffle tree 32, 16, .. 1; the four waves are added in wave order through LDS; a
// second small launch adds the parts in part order.  part[(q * nparts + part) * (7 NS) + 7 s + m], m = 5: min, 6: max.
#define SCA_NSLOT (SCA_NMOM + 2)

struct ScaProf {
    const real_t *vel[3];
    const real_t *phi[SCA_G];
    int nx, nrows, nchunk;
    long qstride, rstride;
};

template <int NS>
__global__ void __launch_bounds__(256) k_scalars_rows(ScaProf A, double *__restrict__ part)
{
    __shared__ double sm[4][NS * SCA_NSLOT];
    const int nparts = gridDim.x;
    double sum[NS][SCA_NMOM], lo[NS], hi[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) {
#pragma unroll
        for (int m = 0; m < SCA_NMOM; m++) sum[s][m] = 0.0;
        lo[s] = __builtin_inf();
        hi[s] = -__builtin_inf();
    }
    const long base = (long)blockIdx.y * A.qstride;
    for (int r = blockIdx.x; r < A.nrows; r += nparts) {
        for (int ch = 0; ch < A.nchunk; ch++) {
            const int i0 = (ch * 256 + (int)threadIdx.x) * SCA_V;
            const int n = A.nx - i0;
            if (n <= 0) continue;
            const long off = base + (long)r * A.rstride + i0;
            real_t u[3][SCA_V];
#pragma unroll
            for (int i = 0; i < 3; i++) sca_load(A.vel[i], off, n, u[i]);
#pragma unroll
            for (int s = 0; s < NS; s++) {
                real_t p[SCA_V];
                sca_load(A.phi[s], off, n, p);
#pragma unroll
                for (int q = 0; q < SCA_V; q++) {
                    if (q < n) {
                        const double x = (double)p[q];
                        sum[s][0] += x;
                        sum[s][1] += x * x;
                        sum[s][2] += (double)u[0][q] * x;
                        sum[s][3] += (double)u[1][q] * x;
                        sum[s][4] += (double)u[2][q] * x;
                        lo[s] = fmin(lo[s], x);
                        hi[s] = fmax(hi[s], x);
                    }
                }
            }
        }
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < NS; s++) {
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int m = 0; m < SCA_NMOM; m++) sum[s][m] += __shfl_down(sum[s][m], o);
            lo[s] = fmin(lo[s], __shfl_down(lo[s], o));
            hi[s] = fmax(hi[s], __shfl_down(hi[s], o));
        }
        if (ln == 0) {
#pragma unroll
            for (int m = 0; m < SCA_NMOM; m++) sm[wv][SCA_NSLOT * s + m] = sum[s][m];
            sm[wv][SCA_NSLOT * s + 5] = lo[s];
            sm[wv][SCA_NSLOT * s + 6] = hi[s];
        }
    }
    __syncthreads();
    if (threadIdx.x < NS * SCA_NSLOT) {
        const int e = threadIdx.x, m = e % SCA_NSLOT;
        const double a0 = sm[0][e], a1 = sm[1][e], a2 = sm[2][e], a3 = sm[3][e];
        const double r = m < SCA_NMOM ? ((a0 + a1) + a2) + a3 : m == 5 ? fmin(fmin(a0, a1), fmin(a2, a3)) : fmax(fmax(a0, a1), fmax(a2, a3));
        part[((long)blockIdx.y * nparts + blockIdx.x) * (NS * SCA_NSLOT) + e] = r;
    }
}

// stage 2: sums[s][m][q] = part[q][0][s][m] + part[q][1][s][m] + ... in part order, rounded once
__global__ void __launch_bounds__(256) k_scalars_finish(const double *__restrict__ part, int ns, int nkeep, int nparts,
                                                        real_t *__restrict__ sums)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)ns * SCA_NMOM * nkeep) return;
    const int q = (int)(t % nkeep);
    const int sm = (int)(t / nkeep);  // s * 5 + m
    const int s = sm / SCA_NMOM, m = sm - s * SCA_NMOM;
    double r = 0.0;
    for (int p = 0; p < nparts; p++) r += part[((long)q * nparts + p) * (ns * SCA_NSLOT) + SCA_NSLOT * s + m];
    sums[t] = (real_t)r;
}

// ... and minmax[s][2]: workgroup e = 2 s + which over all (q, part) partials (min and max do not depend on the order)
__global__ void __launch_bounds__(256) k_scalars_minmax(const double *__restrict__ part, int ns, long nqp, real_t *__restrict__ minmax)
{
    __shared__ double sm[4];
    const int s = blockIdx.x >> 1, which = blockIdx.x & 1;
    double r = which ? -__builtin_inf() : __builtin_inf();
    for (long p = threadIdx.x; p < nqp; p += 256) {
        const double x = part[p * (ns * SCA_NSLOT) + SCA_NSLOT * s + 5 + which];
        r = which ? fmax(r, x) : fmin(r, x);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double x = __shfl_down(r, o);
        r = which ? fmax(r, x) : fmin(r, x);
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        r = which ? fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3])) : fmin(fmin(sm[0], sm[1]), fmin(sm[2], sm[3]));
        minmax[2 * s + which] = (real_t)r;
    }
}

extern "C" int x3d_scalars_profile_sums(x3d_backend *b, const x3d_real *u, const x3d_real *v, const x3d_real *w,
                                        const x3d_real *const *phi, int ns, const int dims[3], int dir_keep, x3d_real *sums,
                                        x3d_real *minmax)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && u && v && w && phi && dims && sums && minmax, "x3d_scalars_profile_sums: null argument");
    X3D_REQUIRE(ns >= 1, "x3d_scalars_profile_sums: ns must be at least 1 (got %d)", ns);
    for (int s = 0; s < ns; s++) X3D_REQUIRE(phi[s], "x3d_scalars_profile_sums: species block %d is null", s);
    X3D_REQUIRE(dir_keep != X3D_DIR_X, "x3d_scalars_profile_sums: dir_keep = 1 is not built (2 or 3)");
    X3D_REQUIRE(dir_keep == X3D_DIR_Y || dir_keep == X3D_DIR_Z, "x3d_scalars_profile_sums: dir_keep must be 2 or 3 (got %d)", dir_keep);
    X3D_REQUIRE(sca_dims_ok(b, dims), "x3d_scalars_profile_sums: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    const long nxp = b->nxp, nyp = b->nyp;
    const int nkeep = dims[dir_keep - 1];
    const int nrows = dir_keep == X3D_DIR_Y ? dims[2] : dims[1];
    // parts per kept index as x3d_stats_profile_sums': enough workgroups to fill the chip (about 4096), never more than rows
    long nparts = (4096 + nkeep - 1) / nkeep;
    if (nparts > nrows) nparts = nrows;
    const long need = (long)nkeep * nparts * SCA_NSLOT * (ns < SCA_G ? ns : SCA_G);
    if (need > b->stats_cap) {  // (the statistics' partial buffer, grown on demand; same stream, so ordered)
        if (b->stats_part) X3D_HIP(hipFree(b->stats_part));
        b->stats_part = nullptr;
        b->stats_cap = 0;
        X3D_HIP(hipMalloc(reinterpret_cast<void **>(&b->stats_part), sizeof(double) * (size_t)need));
        b->stats_cap = need;
    }
    const real_t *vel[3] = {u, v, w};
    for (int i = 0; i < 3; i++) X3D_LAZY_IN(b, vel[i]);
    for (int s0 = 0; s0 < ns; s0 += SCA_G) {
        const int n = ns - s0 < SCA_G ? ns - s0 : SCA_G;
        ScaProf A = {};
        for (int i = 0; i < 3; i++) A.vel[i] = vel[i];
        for (int s = 0; s < n; s++) {
            const real_t *in = phi[s0 + s];
            X3D_LAZY_IN(b, in);
            A.phi[s] = in;
        }
        A.nx = dims[0];
        A.nrows = nrows;
        A.nchunk = (dims[0] + 256 * SCA_V - 1) / (256 * SCA_V);
        A.qstride = dir_keep == X3D_DIR_Y ? nxp : nxp * nyp;
        A.rstride = dir_keep == X3D_DIR_Y ? nxp * nyp : nxp;
        X3D_LAZY_EAGER(b);
        ProfScope ps(b, X3D_K_REDUCE);
        const dim3 grid((unsigned)nparts, (unsigned)nkeep);
        double *part = b->stats_part;
        switch (n) {
        case 1: hipLaunchKernelGGL(k_scalars_rows<1>, grid, dim3(256), 0, b->stream, A, part); break;
        case 2: hipLaunchKernelGGL(k_scalars_rows<2>, grid, dim3(256), 0, b->stream, A, part); break;
        case 3: hipLaunchKernelGGL(k_scalars_rows<3>, grid, dim3(256), 0, b->stream, A, part); break;
        case 4: hipLaunchKernelGGL(k_scalars_rows<4>, grid, dim3(256), 0, b->stream, A, part); break;
        case 5: hipLaunchKernelGGL(k_scalars_rows<5>, grid, dim3(256), 0, b->stream, A, part); break;
        case 6: hipLaunchKernelGGL(k_scalars_rows<6>, grid, dim3(256), 0, b->stream, A, part); break;
        case 7: hipLaunchKernelGGL(k_scalars_rows<7>, grid, dim3(256), 0, b->stream, A, part); break;
        default: hipLaunchKernelGGL(k_scalars_rows<8>, grid, dim3(256), 0, b->stream, A, part); break;
        }
        const long nsum = (long)n * SCA_NMOM * nkeep;
        hipLaunchKernelGGL(k_scalars_finish, dim3((unsigned)((nsum + 255) / 256)), dim3(256), 0, b->stream, (const double *)part, n,
                           nkeep, (int)nparts, sums + (long)s0 * SCA_NMOM * nkeep);
        hipLaunchKernelGGL(k_scalars_minmax, dim3((unsigned)(2 * n)), dim3(256), 0, b->stream, (const double *)part, n,
                           (long)nkeep * nparts, minmax + 2 * s0);
        X3D_HIP(hipGetLastError());
    }
    return 0;
}
