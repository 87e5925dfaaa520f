// Explicit LES: the eddy viscosity (Smagorinsky or WALE) and the subgrid stress tau_ij = 2 nu_t S_ij from the nine velocity
// gradients, in ONE pass that overwrites seven of the nine gradient blocks, plus four scalars of the model left on the
// device.  Not in the reference (Xcompact3d has both models; x3d2 has none yet): this project's own addition.
//
// With g_ij = grads[3 i + j] and S_ij = 1/2 (g_ij + g_ji):
//    Smagorinsky   nu_t = c2 D2 sqrt(2 S:S)
//    WALE          G = g g,  Sd_ij = 1/2 (G_ij + G_ji) - 1/3 delta_ij G_kk,
//                  nu_t = c2 D2 (Sd:Sd)^(3/2) / ((S:S)^(5/2) + (Sd:Sd)^(5/4)),  0 where the denominator is 0
// D2 = a_x[i] a_y[j] a_z[k] (the host's tables h^(2/3): no cbrt or pow here); the powers are products and sqrt only.
// Every factor is widened to double before any product, in both flavours (WALE's fifth powers underflow on 4-byte reals
// otherwise); each output is rounded once to the real kind.
//
// In place: tau_11 -> grads[0], tau_12 -> grads[1], tau_13 -> grads[2], nu_t -> grads[3], tau_22 -> grads[4],
// tau_23 -> grads[5], tau_33 -> grads[8]; grads[6] and grads[7] keep what they hold.  A thread loads the nine values of its
// points before it stores any of them, and the next item's loads are issued before the current item's stores: the pointers
// alias by design and carry no __restrict__.  72 B read + 56 B written per point in FP64.
//
// Row (4 doubles in both flavours): 0 sum nu_t, 1 sum 2 nu_t S:S, 2 max nu_t, 3 max nu_t (ih_x^2 + ih_y^2 + ih_z^2).
// Mapping and summation order are x3d_diag_reduce's (diagnostics.hip): a work item is one 16-byte vector per block and
// thread, 256 threads side by side along x in one (j, k) row; item t = row * nchunk + chunk goes to workgroup t mod G,
// G = min(items, 512).  A thread adds its items in the order it meets them, a wave adds its lanes by the shuffle tree
// 32, 16, .. 1, the four waves are added in wave order, the G partials in index order by a second small launch.  No atomics.
//
// Species (x3d_les_scalar_flux, at the end of this file): the eddy diffusivity kappa = nu_t / Pr_t and the flux q_j = kappa
// dphi/dx_j of one or two species, in place on their gradient blocks, from the nu_t block the stress kernel leaves behind, and
// sum kappa |grad phi|^2 per species.  It takes the stress kernel's item map, loads and partial sums (les_place, les_ld_blocks,
// les_sum_partials), which left k_les_stress's machine code as it was.
#include "common.h"

#define LES_NSLOT 4
#define LES_MAXWG 512  // two workgroups per CU: all resident at once in both flavours (a late workgroup would own its share alone)
#define LES_V (16 / X3D_RB)  // points per 16-byte access: 2 (FP64), 4 (FP32)
typedef real_t les_vec __attribute__((ext_vector_type(LES_V)));

struct LesArgs {
    real_t *f[9];  // (no __restrict__: inputs and outputs are the same blocks)
    const double *a_x, *a_y, *a_z, *ih_x, *ih_y, *ih_z;
    double c2;
    int nx, ny, nchunk;
    long nitem, nxp, nyp;
};

struct LesItem {
    real_t g[9][LES_V];
    double d2[LES_V], q[LES_V];  // filter width squared; ih_x^2 + ih_y^2 + ih_z^2
    long off;
    int n;  // points of this vector inside the row: <= 0 none, >= LES_V all
};

// where item t = row * nchunk + chunk puts this thread: the offset of its vector in a block, the points of it inside the row
// (<= 0 none, >= LES_V all) and its indices.  Shared by the stress and the scalar-flux kernels.
struct LesPlace {
    long off, k;
    int n, i0, j;
};
__device__ __forceinline__ LesPlace les_place(int nx, int ny, int nchunk, long nxp, long nyp, long t)
{
    LesPlace p;
    const long row = t / nchunk;
    const int ch = (int)(t - row * nchunk);
    p.j = (int)(row % ny);
    p.k = row / ny;
    p.i0 = (ch * 256 + (int)threadIdx.x) * LES_V;
    p.off = nxp * (p.j + nyp * p.k) + p.i0;  // (nxp is a multiple of 16 elements: 16-byte aligned)
    p.n = nx - p.i0;
    return p;
}

// the vectors of NB blocks at one place, non-temporal: one 16-byte load per block, or point by point in the row's tail;
// points beyond the row read as zero and the row padding is not touched
template <int NB>
__device__ __forceinline__ void les_ld_blocks(real_t *const (&f)[NB], long off, int n, real_t (&g)[NB][LES_V])
{
    if (n >= LES_V) {
#pragma unroll
        for (int m = 0; m < NB; m++) {
            const les_vec x = __builtin_nontemporal_load(reinterpret_cast<const les_vec *>(f[m] + off));
#pragma unroll
            for (int q = 0; q < LES_V; q++) g[m][q] = x[q];
        }
    } else {
#pragma unroll
        for (int m = 0; m < NB; m++)
#pragma unroll
            for (int q = 0; q < LES_V; q++) g[m][q] = q < n ? __builtin_nontemporal_load(f[m] + off + q) : (real_t)0;
    }
}

// the vector of item t that belongs to this thread; points beyond nx read as zero gradients on a zero width
__device__ __forceinline__ void les_load(const LesArgs &A, long t, LesItem &it)
{
    const LesPlace p = les_place(A.nx, A.ny, A.nchunk, A.nxp, A.nyp, t);
    const int j = p.j, i0 = p.i0;
    const long k = p.k;
    it.off = p.off;
    it.n = p.n;
    les_ld_blocks<9>(A.f, it.off, it.n, it.g);
    const double ay = A.a_y[j], az = A.a_z[k], hy = A.ih_y[j], hz = A.ih_z[k];
    const double hyz = hy * hy + hz * hz;
#pragma unroll
    for (int q = 0; q < LES_V; q++) {
        const double ax = q < it.n ? A.a_x[i0 + q] : 0.0;
        const double hx = q < it.n ? A.ih_x[i0 + q] : 0.0;
        it.d2[q] = ax * ay * az;
        it.q[q] = hx * hx + hyz;
    }
}

// nu_t and the stress of the item's points into it.g (slots as stored), the four scalars into s / mx
template <int MODEL>
__device__ __forceinline__ void les_point(const LesArgs &A, LesItem &it, double (&s)[2], double (&mx)[2])
{
#pragma unroll
    for (int q = 0; q < LES_V; q++) {
        const double g11 = it.g[0][q], g12 = it.g[1][q], g13 = it.g[2][q], g21 = it.g[3][q], g22 = it.g[4][q],
                     g23 = it.g[5][q], g31 = it.g[6][q], g32 = it.g[7][q], g33 = it.g[8][q];
        const double s12 = 0.5 * (g12 + g21), s13 = 0.5 * (g13 + g31), s23 = 0.5 * (g23 + g32);
        const double ss = g11 * g11 + g22 * g22 + g33 * g33 + 2.0 * (s12 * s12 + s13 * s13 + s23 * s23);
        const double cd = A.c2 * it.d2[q];
        double nut;
        if (MODEL == 0) {
            nut = cd * sqrt(2.0 * ss);
        } else {
            const double G11 = g11 * g11 + g12 * g21 + g13 * g31, G22 = g21 * g12 + g22 * g22 + g23 * g32,
                         G33 = g31 * g13 + g32 * g23 + g33 * g33;
            const double G12 = g11 * g12 + g12 * g22 + g13 * g32, G21 = g21 * g11 + g22 * g21 + g23 * g31;
            const double G13 = g11 * g13 + g12 * g23 + g13 * g33, G31 = g31 * g11 + g32 * g21 + g33 * g31;
            const double G23 = g21 * g13 + g22 * g23 + g23 * g33, G32 = g31 * g12 + g32 * g22 + g33 * g32;
            const double tr = (G11 + G22 + G33) * (1.0 / 3.0);
            const double d11 = G11 - tr, d22 = G22 - tr, d33 = G33 - tr;
            const double d12 = 0.5 * (G12 + G21), d13 = 0.5 * (G13 + G31), d23 = 0.5 * (G23 + G32);
            const double dd = d11 * d11 + d22 * d22 + d33 * d33 + 2.0 * (d12 * d12 + d13 * d13 + d23 * d23);
            const double rd = sqrt(dd);
            const double den = ss * ss * sqrt(ss) + dd * sqrt(rd);
            nut = den > 0.0 ? cd * (dd * rd) / den : 0.0;
        }
        const double t2 = 2.0 * nut;
        s[0] += nut;
        s[1] += t2 * ss;
        mx[0] = fmax(mx[0], nut);
        mx[1] = fmax(mx[1], nut * it.q[q]);
        it.g[0][q] = (real_t)(t2 * g11);
        it.g[1][q] = (real_t)(t2 * s12);
        it.g[2][q] = (real_t)(t2 * s13);
        it.g[3][q] = (real_t)nut;
        it.g[4][q] = (real_t)(t2 * g22);
        it.g[5][q] = (real_t)(t2 * s23);
        it.g[8][q] = (real_t)(t2 * g33);
    }
}

__device__ __forceinline__ void les_store(const LesArgs &A, const LesItem &it)
{
    const int out[7] = {0, 1, 2, 3, 4, 5, 8};
    if (it.n >= LES_V) {
#pragma unroll
        for (int m = 0; m < 7; m++) {
            les_vec x;
#pragma unroll
            for (int q = 0; q < LES_V; q++) x[q] = it.g[out[m]][q];
            *reinterpret_cast<les_vec *>(A.f[out[m]] + it.off) = x;
        }
    } else {
#pragma unroll
        for (int m = 0; m < 7; m++)
#pragma unroll
            for (int q = 0; q < LES_V; q++)
                if (q < it.n) A.f[out[m]][it.off + q] = it.g[out[m]][q];
    }
}

// stage 1: the stress in place and part[workgroup][4]
template <int MODEL>
__global__ void __launch_bounds__(256) k_les_stress(LesArgs A, double *part)
{
    __shared__ double sm[4][LES_NSLOT];
    double s[2] = {0.0, 0.0}, mx[2] = {0.0, 0.0};
    const long G = gridDim.x;
    long t = blockIdx.x;  // (G <= nitem: every workgroup has a first item)
    LesItem cur;
    les_load(A, t, cur);
    for (t += G; t < A.nitem; t += G) {
        LesItem nxt;
        les_load(A, t, nxt);
        les_point<MODEL>(A, cur, s, mx);
        les_store(A, cur);
        cur = nxt;
    }
    les_point<MODEL>(A, cur, s, mx);
    les_store(A, cur);
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int m = 0; m < 2; m++) {
            s[m] += __shfl_down(s[m], o);
            mx[m] = fmax(mx[m], __shfl_down(mx[m], o));
        }
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0) {
        sm[wv][0] = s[0];
        sm[wv][1] = s[1];
        sm[wv][2] = mx[0];
        sm[wv][3] = mx[1];
    }
    __syncthreads();
    if (threadIdx.x < LES_NSLOT) {
        const int slot = threadIdx.x;
        const double r = slot < 2 ? ((sm[0][slot] + sm[1][slot]) + sm[2][slot]) + sm[3][slot]
                                  : fmax(fmax(sm[0][slot], sm[1][slot]), fmax(sm[2][slot], sm[3][slot]));
        part[(long)blockIdx.x * LES_NSLOT + slot] = r;
    }
}

// partials part[p * STRIDE + slot], p < nparts, added in index order with a compensated sum: one fixed order, the same bits for
// the same partials
template <int STRIDE>
__device__ __forceinline__ double les_sum_partials(const double *__restrict__ part, int nparts, int slot)
{
    double r = 0.0, c = 0.0;
#pragma unroll 4
    for (int p = 0; p < nparts; p++) {
        const double x = part[(long)p * STRIDE + slot];
        const double t = r + x;
        c += fabs(r) >= fabs(x) ? (r - t) + x : (x - t) + r;
        r = t;
    }
    r += c;
    return r;
}

// stage 2: the partials in index order (the sums compensated, as k_diag_finish's: one fixed order, the same bits for the
// same partials)
__global__ void __launch_bounds__(64) k_les_finish(const double *__restrict__ part, int nparts, double *__restrict__ row)
{
    const int slot = threadIdx.x;
    if (slot >= LES_NSLOT) return;
    double r = 0.0;
    if (slot < 2) {
        r = les_sum_partials<LES_NSLOT>(part, nparts, slot);
    } else {
#pragma unroll 8
        for (int p = 0; p < nparts; p++) r = fmax(r, part[(long)p * LES_NSLOT + slot]);
    }
    row[slot] = r;
}

extern "C" int x3d_les_stress(x3d_backend *b, x3d_real *const grads[9], const int dims[3], const x3d_les_params *params,
                              double *row_dev)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && grads && dims && params && row_dev, "x3d_les_stress: null argument");
    X3D_REQUIRE(params->a_x && params->a_y && params->a_z, "x3d_les_stress: null width table");
    X3D_REQUIRE(params->ih_x && params->ih_y && params->ih_z, "x3d_les_stress: null spacing table");
    real_t *g[9];
    for (int m = 0; m < 9; m++) {
        X3D_REQUIRE(grads[m], "x3d_les_stress: gradient block %d is null", m);
        for (int q = 0; q < m; q++)
            X3D_REQUIRE(grads[m] != grads[q], "x3d_les_stress: gradient blocks %d and %d are the same block", q, m);
        g[m] = grads[m];
    }
    X3D_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, "x3d_les_stress: dims (%d,%d,%d) must be positive", dims[0], dims[1],
                dims[2]);
    X3D_REQUIRE(dims[0] <= b->nxp && dims[1] <= b->nyp && dims[2] <= b->nzp, "x3d_les_stress: dims (%d,%d,%d) outside the block",
                dims[0], dims[1], dims[2]);
    X3D_REQUIRE(params->model == X3D_LES_SMAGORINSKY || params->model == X3D_LES_WALE, "x3d_les_stress: unknown model %d",
                params->model);
    X3D_REQUIRE(params->c2 >= 0.0 && params->c2 <= 1.79e308, "x3d_les_stress: the squared constant (%g) must be finite and not negative", params->c2);
    LesArgs A;
    A.nx = dims[0];
    A.ny = dims[1];
    A.nchunk = (dims[0] + 256 * LES_V - 1) / (256 * LES_V);
    A.nitem = (long)dims[1] * dims[2] * A.nchunk;
    A.nxp = b->nxp;
    A.nyp = b->nyp;
    const int grid = (int)(A.nitem < LES_MAXWG ? A.nitem : LES_MAXWG);
    // the partials live in the backend's reduction buffer, read as doubles
    const long cap = (long)(sizeof(real_t) * 2 * (size_t)b->red_cap / sizeof(double));
    X3D_REQUIRE((long)grid * LES_NSLOT <= cap, "x3d_les_stress: %d x %d partials, the reduction buffer holds %ld", grid, LES_NSLOT,
                cap);
    for (int m = 0; m < 9; m++) {
        if (m == 6 || m == 7) {
            const real_t *in = g[m];
            X3D_LAZY_IN(b, in);
            g[m] = const_cast<real_t *>(in);
        } else {
            X3D_LAZY_OUT(b, g[m], false);
        }
    }
    X3D_LAZY_EAGER(b);
    for (int m = 0; m < 9; m++) A.f[m] = g[m];
    A.a_x = params->a_x;
    A.a_y = params->a_y;
    A.a_z = params->a_z;
    A.ih_x = params->ih_x;
    A.ih_y = params->ih_y;
    A.ih_z = params->ih_z;
    A.c2 = params->c2;
    double *part = reinterpret_cast<double *>(b->red_buf);
    ProfScope ps(b, X3D_K_BLAS1);
    if (params->model == X3D_LES_SMAGORINSKY)
        hipLaunchKernelGGL(k_les_stress<0>, dim3(grid), dim3(256), 0, b->stream, A, part);
    else
        hipLaunchKernelGGL(k_les_stress<1>, dim3(grid), dim3(256), 0, b->stream, A, part);
    hipLaunchKernelGGL(k_les_finish, dim3(1), dim3(64), 0, b->stream, (const double *)part, grid, row_dev);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---- the species' subgrid flux: eddy diffusivity kappa = nu_t / Pr_t and q_j = kappa dphi/dx_j, in place on the gradient blocks
// of one or two species, from the nu_t block x3d_les_stress leaves behind (read once for both species).  Per point and
// species, every factor widened to double before any product, in both flavours:
//    kappa = nu_t inv_prt[s];   q_j = kappa g_j, each rounded once to the real kind;   row[s] += kappa ((g_x^2 + g_y^2) + g_z^2)
// Mapping, tail handling and summation order are k_les_stress's (above): the same work items on the same workgroups, the
// next item's loads issued before the current item's stores, the shuffle tree, the four waves in wave order, the partials in
// the backend's reduction buffer added in index order by a second small launch.  No atomics: two launches on the same
// blocks give the same bits.  1 + 3 ns blocks read and 3 ns written: 56 B per point (ns = 1) and 104 B (ns = 2) in FP64.
template <int NS>
struct LesFluxArgs {
    real_t *f[1 + 3 * NS];  // nu_t (only read), then g_x, g_y, g_z of each species (overwritten by q_x, q_y, q_z)
    double ipr[NS];         // 1 / Pr_t of each species
    int nx, ny, nchunk;
    long nitem, nxp, nyp;
};

template <int NS>
struct LesFluxItem {
    real_t g[1 + 3 * NS][LES_V];
    long off;
    int n;
};

template <int NS>
__device__ __forceinline__ void les_flux_load(const LesFluxArgs<NS> &A, long t, LesFluxItem<NS> &it)
{
    const LesPlace p = les_place(A.nx, A.ny, A.nchunk, A.nxp, A.nyp, t);
    it.off = p.off;
    it.n = p.n;
    les_ld_blocks<1 + 3 * NS>(A.f, it.off, it.n, it.g);
}

// the fluxes of the item's points into it.g[1 ..], kappa |grad phi|^2 into s (points beyond the row hold zeros and add zero)
template <int NS>
__device__ __forceinline__ void les_flux_point(const LesFluxArgs<NS> &A, LesFluxItem<NS> &it, double (&s)[NS])
{
#pragma unroll
    for (int q = 0; q < LES_V; q++) {
        const double nut = it.g[0][q];
#pragma unroll
        for (int sp = 0; sp < NS; sp++) {
            const double kap = nut * A.ipr[sp];
            const double gx = it.g[1 + 3 * sp][q], gy = it.g[2 + 3 * sp][q], gz = it.g[3 + 3 * sp][q];
            s[sp] += kap * ((gx * gx + gy * gy) + gz * gz);
            it.g[1 + 3 * sp][q] = (real_t)(kap * gx);
            it.g[2 + 3 * sp][q] = (real_t)(kap * gy);
            it.g[3 + 3 * sp][q] = (real_t)(kap * gz);
        }
    }
}

template <int NS>
__device__ __forceinline__ void les_flux_store(const LesFluxArgs<NS> &A, const LesFluxItem<NS> &it)
{
    if (it.n >= LES_V) {
#pragma unroll
        for (int m = 1; m < 1 + 3 * NS; m++) {
            les_vec x;
#pragma unroll
            for (int q = 0; q < LES_V; q++) x[q] = it.g[m][q];
            *reinterpret_cast<les_vec *>(A.f[m] + it.off) = x;
        }
    } else {
#pragma unroll
        for (int m = 1; m < 1 + 3 * NS; m++)
#pragma unroll
            for (int q = 0; q < LES_V; q++)
                if (q < it.n) A.f[m][it.off + q] = it.g[m][q];
    }
}

// stage 1: the fluxes in place and part[workgroup][NS]
template <int NS>
__global__ void __launch_bounds__(256) k_les_scalar_flux(LesFluxArgs<NS> A, double *part)
{
    __shared__ double sm[4][NS];
    double s[NS];
#pragma unroll
    for (int m = 0; m < NS; m++) s[m] = 0.0;
    const long G = gridDim.x;
    long t = blockIdx.x;  // (G <= nitem: every workgroup has a first item)
    LesFluxItem<NS> cur;
    les_flux_load<NS>(A, t, cur);
    for (t += G; t < A.nitem; t += G) {
        LesFluxItem<NS> nxt;
        les_flux_load<NS>(A, t, nxt);
        les_flux_point<NS>(A, cur, s);
        les_flux_store<NS>(A, cur);
        cur = nxt;
    }
    les_flux_point<NS>(A, cur, s);
    les_flux_store<NS>(A, cur);
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int m = 0; m < NS; m++) s[m] += __shfl_down(s[m], o);
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0) {
#pragma unroll
        for (int m = 0; m < NS; m++) sm[wv][m] = s[m];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const int slot = threadIdx.x;
        part[(long)blockIdx.x * NS + slot] = ((sm[0][slot] + sm[1][slot]) + sm[2][slot]) + sm[3][slot];
    }
}

// stage 2: row[s] = the partials of species s in index order, compensated as k_les_finish's sums
template <int NS>
__global__ void __launch_bounds__(64) k_les_flux_finish(const double *__restrict__ part, int nparts, double *__restrict__ row)
{
    const int slot = threadIdx.x;
    if (slot >= NS) return;
    row[slot] = les_sum_partials<NS>(part, nparts, slot);
}

template <int NS>
static void les_flux_launch(x3d_backend *b, const real_t *nut, real_t *const g[], const double *inv_prt, const int dims[3],
                            int grid, double *row_dev)
{
    LesFluxArgs<NS> A;
    A.f[0] = const_cast<real_t *>(nut);
    for (int m = 0; m < 3 * NS; m++) A.f[1 + m] = g[m];
    for (int s = 0; s < NS; s++) A.ipr[s] = inv_prt[s];
    A.nx = dims[0];
    A.ny = dims[1];
    A.nchunk = (dims[0] + 256 * LES_V - 1) / (256 * LES_V);
    A.nitem = (long)dims[1] * dims[2] * A.nchunk;
    A.nxp = b->nxp;
    A.nyp = b->nyp;
    double *part = reinterpret_cast<double *>(b->red_buf);
    hipLaunchKernelGGL(k_les_scalar_flux<NS>, dim3(grid), dim3(256), 0, b->stream, A, part);
    hipLaunchKernelGGL(k_les_flux_finish<NS>, dim3(1), dim3(64), 0, b->stream, (const double *)part, grid, row_dev);
}

extern "C" int x3d_les_scalar_flux(x3d_backend *b, const x3d_real *nut, x3d_real *const gphi[], int ns, const int dims[3],
                                   const double *inv_prt, double *row_dev)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && nut && gphi && dims && inv_prt && row_dev, "x3d_les_scalar_flux: null argument");
    X3D_REQUIRE(ns >= 1 && ns <= 2, "x3d_les_scalar_flux: %d species in one call (1 or 2)", ns);
    real_t *g[6];
    for (int m = 0; m < 3 * ns; m++) {
        X3D_REQUIRE(gphi[m], "x3d_les_scalar_flux: gradient block %d is null", m);
        X3D_REQUIRE(gphi[m] != nut, "x3d_les_scalar_flux: gradient block %d and nu_t are the same block", m);
        for (int q = 0; q < m; q++)
            X3D_REQUIRE(gphi[m] != gphi[q], "x3d_les_scalar_flux: gradient blocks %d and %d are the same block", q, m);
        g[m] = gphi[m];
    }
    X3D_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, "x3d_les_scalar_flux: dims (%d,%d,%d) must be positive", dims[0],
                dims[1], dims[2]);
    X3D_REQUIRE(dims[0] <= b->nxp && dims[1] <= b->nyp && dims[2] <= b->nzp,
                "x3d_les_scalar_flux: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    for (int s = 0; s < ns; s++)
        X3D_REQUIRE(inv_prt[s] > 0.0 && inv_prt[s] <= 1.79e308,
                    "x3d_les_scalar_flux: 1 / Pr_t of species %d (%g) must be finite and positive", s, inv_prt[s]);
    const int nchunk = (dims[0] + 256 * LES_V - 1) / (256 * LES_V);
    const long nitem = (long)dims[1] * dims[2] * nchunk;
    const int grid = (int)(nitem < LES_MAXWG ? nitem : LES_MAXWG);
    // the partials live in the backend's reduction buffer, read as doubles
    const long cap = (long)(sizeof(real_t) * 2 * (size_t)b->red_cap / sizeof(double));
    X3D_REQUIRE((long)grid * ns <= cap, "x3d_les_scalar_flux: %d x %d partials, the reduction buffer holds %ld", grid, ns, cap);
    X3D_LAZY_IN(b, nut);
    for (int m = 0; m < 3 * ns; m++) X3D_LAZY_OUT(b, g[m], false);
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_BLAS1);
    if (ns == 1)
        les_flux_launch<1>(b, nut, g, inv_prt, dims, grid, row_dev);
    else
        les_flux_launch<2>(b, nut, g, inv_prt, dims, grid, row_dev);
    X3D_HIP(hipGetLastError());
    return 0;
}
