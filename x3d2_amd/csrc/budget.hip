// Reynolds-stress budget profiles: the plane sums of 41 raw moments of u, v, w, the vertex pressure and the nine velocity
// gradients along y or z, from ONE pass over the thirteen blocks (104 B/DoF in FP64), left on the device.  The host path it
// replaces pulls thirteen full blocks per sample through pageable memory.  The write-time algebra (x3d2_amd/budgets.py)
// forms central moments as differences of these raw ones, so every factor is widened to double before any product and
// every accumulator, partial and sum is FP64 in both flavours of the library.
//
// Moment order (d = dir_keep - 1, g_ij = grads[3 i + j], p = p_scale * f->p, pairs = uu, vv, ww, uv, uw, vw):
//    0..2   u, v, w               3  p                    4..9   u_i u_j          10  p p          11..13  p u, p v, p w
//    14..19 u_i u_j u_d           20..28  g_ij            29..34 sum_k g_ik g_jk  35..40  p (g_ij + g_ji)
//
// Summation order (what makes the bits of `sums` a function of the fields, dims and dir_keep alone), as k_prof_rows'
// (stats.hip): blockIdx.y = kept index q, blockIdx.x = part; a part takes the rows part, part + nparts, ... of q; lanes run
// along x, one 16-byte vector per stream and thread, 256 threads side by side.  A thread adds its items in the order it
// meets them, the points of a vector one after the other; a wave adds its lanes by the shuffle tree 32, 16, .. 1; the four
// waves are added in wave order through LDS; a second small launch adds the parts in part order.  No atomics.
#include "common.h"

#define BUD_NMOM X3D_NBUDGET
#define BUD_NF 13                // streams: u, v, w, nine gradients, p (last: the instantiation without p never touches it)
#define BUD_V (16 / X3D_RB)      // points per 16-byte load: 2 (FP64), 4 (FP32)
typedef real_t bud_vec __attribute__((ext_vector_type(BUD_V)));

struct BudIn {
    const real_t *f[BUD_NF];  // u, v, w, g_00 .. g_22, p
    int nx, nrows, nchunk, d;
    long qstride, rstride;
    double p_scale;
};

template <bool HAS_P>
struct BudItem {
    real_t v[HAS_P ? BUD_NF : BUD_NF - 1][BUD_V];
};

// the vectors of item n of this part that belong to this thread: row part + (n / nchunk) * nparts, chunk n % nchunk.  Points
// beyond nx read as zero and then add +0.0 to every sum.
template <bool HAS_P>
__device__ __forceinline__ void bud_load(const BudIn &A, long base, int nparts, int n, BudItem<HAS_P> &it)
{
    constexpr int NF = HAS_P ? BUD_NF : BUD_NF - 1;
    const int k = n / A.nchunk, ch = n - k * A.nchunk;
    const int i0 = (ch * 256 + (int)threadIdx.x) * BUD_V;
    const long off = base + (long)k * nparts * A.rstride + i0;  // (strides are multiples of the pitch: 16-byte aligned)
    const int left = A.nx - i0;
    if (left >= BUD_V) {
#pragma unroll
        for (int m = 0; m < NF; m++) {
            const bud_vec x = __builtin_nontemporal_load(reinterpret_cast<const bud_vec *>(A.f[m] + off));
#pragma unroll
            for (int q = 0; q < BUD_V; q++) it.v[m][q] = x[q];
        }
    } else {
#pragma unroll
        for (int m = 0; m < NF; m++)
#pragma unroll
            for (int q = 0; q < BUD_V; q++) it.v[m][q] = q < left ? __builtin_nontemporal_load(A.f[m] + off + q) : (real_t)0;
    }
}

// one point after the other: 41 accumulators stay live, a point's thirteen doubles do not outlive it
template <bool HAS_P>
__device__ __forceinline__ void bud_add(const BudIn &A, const BudItem<HAS_P> &it, double (&s)[BUD_NMOM])
{
#pragma unroll
    for (int q = 0; q < BUD_V; q++) {
        double u[3], g[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++) u[i] = (double)it.v[i][q];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) g[i][j] = (double)it.v[3 + 3 * i + j][q];
        const double ud = A.d == 1 ? u[1] : u[2];
        constexpr int PI[6] = {0, 1, 2, 0, 0, 1}, PJ[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int i = 0; i < 3; i++) s[i] += u[i];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int i = PI[k], j = PJ[k];
            const double uu = u[i] * u[j];
            s[4 + k] += uu;
            s[14 + k] += uu * ud;
            s[29 + k] += (g[i][0] * g[j][0] + g[i][1] * g[j][1]) + g[i][2] * g[j][2];
        }
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) s[20 + 3 * i + j] += g[i][j];
        if constexpr (HAS_P) {
            const double p = A.p_scale * (double)it.v[BUD_NF - 1][q];
            s[3] += p;
            s[10] += p * p;
#pragma unroll
            for (int i = 0; i < 3; i++) s[11 + i] += p * u[i];
#pragma unroll
            for (int k = 0; k < 6; k++) s[35 + k] += p * (g[PI[k]][PJ[k]] + g[PJ[k]][PI[k]]);
        }
    }
}

// stage 1: part[(q * nparts + part) * 41 + m].  The next item's loads are issued before the current item is added up.
template <bool HAS_P>
__global__ void __launch_bounds__(256) k_budget_rows(BudIn A, double *__restrict__ part)
{
    __shared__ double sm[4][BUD_NMOM];
    const int nparts = gridDim.x;
    double s[BUD_NMOM];
#pragma unroll
    for (int m = 0; m < BUD_NMOM; m++) s[m] = 0.0;
    // (nparts <= nrows: every part has a first row)
    const int nitem = ((A.nrows - (int)blockIdx.x + nparts - 1) / nparts) * A.nchunk;
    const long base = (long)blockIdx.y * A.qstride + (long)blockIdx.x * A.rstride;
    BudItem<HAS_P> cur;
    bud_load<HAS_P>(A, base, nparts, 0, cur);
    for (int n = 1; n < nitem; n++) {
        BudItem<HAS_P> nxt;
        bud_load<HAS_P>(A, base, nparts, n, nxt);
        bud_add<HAS_P>(A, cur, s);
        cur = nxt;
    }
    bud_add<HAS_P>(A, cur, s);
#pragma unroll
    for (int m = 0; m < BUD_NMOM; m++)
        for (int o = 32; o > 0; o >>= 1) s[m] += __shfl_down(s[m], o);
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0)
#pragma unroll
        for (int m = 0; m < BUD_NMOM; m++) sm[wv][m] = s[m];
    __syncthreads();
    if (threadIdx.x < BUD_NMOM) {
        const int m = threadIdx.x;
        part[((long)blockIdx.y * nparts + blockIdx.x) * BUD_NMOM + m] = ((sm[0][m] + sm[1][m]) + sm[2][m]) + sm[3][m];
    }
}

// stage 2: sums[m][q] = part[q][0][m] + part[q][1][m] + ... in part order
__global__ void __launch_bounds__(256) k_budget_finish(const double *__restrict__ part, int nkeep, int nparts,
                                                       double *__restrict__ sums)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)nkeep * BUD_NMOM) return;
    const int m = (int)(t % BUD_NMOM);
    const long q = t / BUD_NMOM;
    double s = 0.0;
    for (int p = 0; p < nparts; p++) s += part[(q * nparts + p) * BUD_NMOM + m];
    sums[(long)m * nkeep + q] = s;
}

extern "C" int x3d_budget_profile_sums(x3d_backend *b, const x3d_budget_fields *f, const int dims[3], int dir_keep,
                                       double p_scale, double *sums)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && f && dims && sums, "x3d_budget_profile_sums: null argument");
    X3D_REQUIRE(f->u && f->v && f->w, "x3d_budget_profile_sums: null argument (u, v or w)");
    const real_t *in[BUD_NF] = {f->u, f->v, f->w};
    for (int m = 0; m < 9; m++) {
        X3D_REQUIRE(f->grads[m], "x3d_budget_profile_sums: gradient block %d is null", m);
        in[3 + m] = f->grads[m];
    }
    in[BUD_NF - 1] = f->p;
    X3D_REQUIRE(dir_keep != X3D_DIR_X, "x3d_budget_profile_sums: dir_keep = 1 is not built (2 or 3)");
    X3D_REQUIRE(dir_keep == X3D_DIR_Y || dir_keep == X3D_DIR_Z, "x3d_budget_profile_sums: dir_keep must be 2 or 3 (got %d)",
                dir_keep);
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_budget_profile_sums: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    const bool has_p = f->p != nullptr;
    const int nf = has_p ? BUD_NF : BUD_NF - 1;
    for (int m = 0; m < nf; m++) X3D_LAZY_IN(b, in[m]);
    X3D_LAZY_EAGER(b);
    const long nxp = b->nxp, nyp = b->nyp;
    const int nkeep = dims[dir_keep - 1];
    BudIn A;
    for (int m = 0; m < BUD_NF; m++) A.f[m] = in[m];
    A.nx = dims[0];
    A.nchunk = (dims[0] + 256 * BUD_V - 1) / (256 * BUD_V);
    A.d = dir_keep - 1;
    A.p_scale = p_scale;
    if (dir_keep == X3D_DIR_Y) {
        A.nrows = dims[2];
        A.qstride = nxp;
        A.rstride = nxp * nyp;
    } else {
        A.nrows = dims[1];
        A.qstride = nxp * nyp;
        A.rstride = nxp;
    }
    // parts per kept index as x3d_stats_profile_sums': enough workgroups to fill the chip (about 4096), never more than rows
    long nparts = (4096 + nkeep - 1) / nkeep;
    if (nparts > A.nrows) nparts = A.nrows;
    const long need = (long)nkeep * nparts * BUD_NMOM;
    if (need > b->stats_cap) {  // (the statistics' partial buffer, grown on demand; same stream, so ordered)
        if (b->stats_part) X3D_HIP(hipFree(b->stats_part));
        b->stats_part = nullptr;
        b->stats_cap = 0;
        X3D_HIP(hipMalloc(reinterpret_cast<void **>(&b->stats_part), sizeof(double) * (size_t)need));
        b->stats_cap = need;
    }
    ProfScope ps(b, X3D_K_REDUCE);
    const dim3 grid((unsigned)nparts, (unsigned)nkeep);
    if (has_p)
        hipLaunchKernelGGL(k_budget_rows<true>, grid, dim3(256), 0, b->stream, A, b->stats_part);
    else
        hipLaunchKernelGGL(k_budget_rows<false>, grid, dim3(256), 0, b->stream, A, b->stats_part);
    hipLaunchKernelGGL(k_budget_finish, dim3((unsigned)(((long)nkeep * BUD_NMOM + 255) / 256)), dim3(256), 0, b->stream,
                       (const double *)b->stats_part, nkeep, (int)nparts, sums);
    X3D_HIP(hipGetLastError());
    return 0;
}

// prof += (sums * scale - prof) * inc on n doubles (accumulate_mean on the plane means)
__global__ void __launch_bounds__(256) k_budget_accumulate(double *__restrict__ prof, const double *__restrict__ sums, long n,
                                                           double scale, double inc)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double p = prof[t];
    prof[t] = p + (sums[t] * scale - p) * inc;
}

extern "C" int x3d_budget_profile_accumulate(x3d_backend *b, double *prof, const double *sums, long n, double scale,
                                             double inc)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && prof && sums, "x3d_budget_profile_accumulate: null argument");
    X3D_REQUIRE(n > 0, "x3d_budget_profile_accumulate: n must be positive (got %ld)", n);
    X3D_REQUIRE(prof != sums, "x3d_budget_profile_accumulate: prof and sums are the same buffer");
    X3D_LAZY_FLUSH(b);  // (small device buffers, not blocks: nothing to translate, but ordered behind what was recorded)
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_BLAS1);
    hipLaunchKernelGGL(k_budget_accumulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, prof, sums, n, scale,
                       inc);
    X3D_HIP(hipGetLastError());
    return 0;
}
