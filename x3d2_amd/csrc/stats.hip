// Flow statistics on the device: running means of u, v, w and their six products, the write-time fluctuations, and
// profiles over the homogeneous directions.  The reference's stats_manager_t (src/io/stats.f90) copies three blocks
// to the host per sample and makes nine array passes there (:139-159); here a sample is one kernel that reads u, v, w
// and read-modify-writes the nine accumulators (168 B/DoF in FP64), or -- profiles -- one read of u, v, w (24 B/DoF)
// and a few KB of sums.
#include "common.h"

// Moment order everywhere (src/io/stats.f90:151-159): u, v, w, uu, vv, ww, uv, uw, vw
#define X3D_NMOM 9

// ---------------------------------------------------------------- 3-D accumulators
// The access pattern of the measured copy ceiling (profiles/r04_copy_ceiling.txt): 16-byte non-temporal loads and
// stores, one contiguous chunk of STAT_CHUNK 16-byte elements per workgroup and stream (32 KiB in FP64), as many
// workgroups as there are chunks -- not the grid-stride loop of the BLAS-1 kernels.
#define STAT_CHUNK 2048

struct Mean9 { real2_t *m[X3D_NMOM]; };

// accumulate_mean (src/io/stats.f90:61-70): mean = mean + (val - mean) * stat_inc
__device__ __forceinline__ real2_t acc_mean(real2_t m, real_t vx, real_t vy, real_t inc)
{
    m.x = m.x + (vx - m.x) * inc;
    m.y = m.y + (vy - m.y) * inc;
    return m;
}

__global__ void __launch_bounds__(256) k_stats_uvw(const real2_t *__restrict__ u, const real2_t *__restrict__ v,
                                                   const real2_t *__restrict__ w, Mean9 M, size_t n2, real_t inc)
{
    const size_t base = (size_t)blockIdx.x * STAT_CHUNK;
#pragma unroll 2
    for (int it = 0; it < STAT_CHUNK / 256; it++) {
        const size_t i = base + (size_t)it * 256 + threadIdx.x;
        if (i >= n2) break;
        const real2_t a = ldg_stream(u + i), b = ldg_stream(v + i), c = ldg_stream(w + i);
        real2_t m[X3D_NMOM];
#pragma unroll
        for (int k = 0; k < X3D_NMOM; k++) m[k] = ldg_stream(M.m[k] + i);
        m[0] = acc_mean(m[0], a.x, a.y, inc);
        m[1] = acc_mean(m[1], b.x, b.y, inc);
        m[2] = acc_mean(m[2], c.x, c.y, inc);
        m[3] = acc_mean(m[3], a.x * a.x, a.y * a.y, inc);
        m[4] = acc_mean(m[4], b.x * b.x, b.y * b.y, inc);
        m[5] = acc_mean(m[5], c.x * c.x, c.y * c.y, inc);
        m[6] = acc_mean(m[6], a.x * b.x, a.y * b.y, inc);
        m[7] = acc_mean(m[7], a.x * c.x, a.y * c.y, inc);
        m[8] = acc_mean(m[8], b.x * c.x, b.y * c.y, inc);
#pragma unroll
        for (int k = 0; k < X3D_NMOM; k++) stg_stream(M.m[k] + i, m[k]);
    }
}

template <bool SECOND>
__global__ void __launch_bounds__(256) k_stats_scalar(const real2_t *__restrict__ phi, real2_t *__restrict__ m1,
                                                      real2_t *__restrict__ m2, size_t n2, real_t inc)
{
    const size_t base = (size_t)blockIdx.x * STAT_CHUNK;
#pragma unroll 4
    for (int it = 0; it < STAT_CHUNK / 256; it++) {
        const size_t i = base + (size_t)it * 256 + threadIdx.x;
        if (i >= n2) break;
        const real2_t a = ldg_stream(phi + i);
        stg_stream(m1 + i, acc_mean(ldg_stream(m1 + i), a.x, a.y, inc));
        if (SECOND) stg_stream(m2 + i, acc_mean(ldg_stream(m2 + i), a.x * a.x, a.y * a.y, inc));
    }
}

// write-time fluctuations (src/io/stats.f90:232-237)
struct Out6 { real2_t *o[6]; };
struct CMean9 { const real2_t *m[X3D_NMOM]; };

__device__ __forceinline__ real_t rms_of(real_t sq, real_t mean)
{
    const real_t d = sq - mean * mean;
    return sqrt(d > (real_t)0 ? d : (real_t)0);
}

__global__ void __launch_bounds__(256) k_stats_derive(Out6 O, CMean9 M, size_t n2)
{
    const size_t base = (size_t)blockIdx.x * STAT_CHUNK;
    for (int it = 0; it < STAT_CHUNK / 256; it++) {
        const size_t i = base + (size_t)it * 256 + threadIdx.x;
        if (i >= n2) break;
        real2_t m[X3D_NMOM];
#pragma unroll
        for (int k = 0; k < X3D_NMOM; k++) m[k] = ldg_stream(M.m[k] + i);
        stg_stream(O.o[0] + i, make_real2(rms_of(m[3].x, m[0].x), rms_of(m[3].y, m[0].y)));
        stg_stream(O.o[1] + i, make_real2(rms_of(m[4].x, m[1].x), rms_of(m[4].y, m[1].y)));
        stg_stream(O.o[2] + i, make_real2(rms_of(m[5].x, m[2].x), rms_of(m[5].y, m[2].y)));
        stg_stream(O.o[3] + i, make_real2(m[6].x - m[0].x * m[1].x, m[6].y - m[0].y * m[1].y));
        stg_stream(O.o[4] + i, make_real2(m[7].x - m[0].x * m[2].x, m[7].y - m[0].y * m[2].y));
        stg_stream(O.o[5] + i, make_real2(m[8].x - m[1].x * m[2].x, m[8].y - m[1].y * m[2].y));
    }
}

static inline unsigned stat_grid(size_t n2) { return (unsigned)((n2 + STAT_CHUNK - 1) / STAT_CHUNK); }

extern "C" int x3d_stats_update_uvw(x3d_backend *b, const real_t *u, const real_t *v, const real_t *w,
                                    real_t *const mean[9], real_t stat_inc)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && u && v && w && mean, "x3d_stats_update_uvw: null argument");
    const real_t *in[3] = {u, v, w};
    real_t *acc[X3D_NMOM];
    for (int k = 0; k < X3D_NMOM; k++) {
        X3D_REQUIRE(mean[k], "x3d_stats_update_uvw: accumulator %d is null", k);
        for (int q = 0; q < 3; q++)
            X3D_REQUIRE(mean[k] != in[q], "x3d_stats_update_uvw: accumulator %d is one of u, v, w", k);
        for (int q = 0; q < k; q++)
            X3D_REQUIRE(mean[k] != mean[q], "x3d_stats_update_uvw: accumulators %d and %d are the same block", q, k);
        acc[k] = mean[k];
    }
    for (int q = 0; q < 3; q++) X3D_LAZY_IN(b, in[q]);
    for (int k = 0; k < X3D_NMOM; k++) X3D_LAZY_OUT(b, acc[k], false);
    X3D_LAZY_EAGER(b);
    Mean9 M;
    for (int k = 0; k < X3D_NMOM; k++) M.m[k] = (real2_t *)acc[k];
    ProfScope ps(b, X3D_K_BLAS1);
    const size_t n2 = b->nblock / 2;
    hipLaunchKernelGGL(k_stats_uvw, dim3(stat_grid(n2)), dim3(256), 0, b->stream, (const real2_t *)in[0],
                       (const real2_t *)in[1], (const real2_t *)in[2], M, n2, stat_inc);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_stats_update_scalar(x3d_backend *b, const real_t *phi, real_t *mean_phi, real_t *mean_phiphi,
                                       real_t stat_inc)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && phi && mean_phi, "x3d_stats_update_scalar: null argument");
    X3D_REQUIRE(mean_phi != phi && mean_phiphi != phi && mean_phi != mean_phiphi,
                "x3d_stats_update_scalar: the accumulators must be distinct from each other and from phi");
    X3D_LAZY_IN(b, phi);
    X3D_LAZY_OUT(b, mean_phi, false);
    if (mean_phiphi) X3D_LAZY_OUT(b, mean_phiphi, false);
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_BLAS1);
    const size_t n2 = b->nblock / 2;
    if (mean_phiphi)
        hipLaunchKernelGGL(k_stats_scalar<true>, dim3(stat_grid(n2)), dim3(256), 0, b->stream, (const real2_t *)phi,
                           (real2_t *)mean_phi, (real2_t *)mean_phiphi, n2, stat_inc);
    else
        hipLaunchKernelGGL(k_stats_scalar<false>, dim3(stat_grid(n2)), dim3(256), 0, b->stream, (const real2_t *)phi,
                           (real2_t *)mean_phi, (real2_t *)nullptr, n2, stat_inc);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_stats_derive(x3d_backend *b, real_t *const out[6], const real_t *const mean[9])
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && out && mean, "x3d_stats_derive: null argument");
    const real_t *in[X3D_NMOM];
    real_t *o[6];
    for (int k = 0; k < X3D_NMOM; k++) {
        X3D_REQUIRE(mean[k], "x3d_stats_derive: accumulator %d is null", k);
        in[k] = mean[k];
    }
    for (int k = 0; k < 6; k++) {
        X3D_REQUIRE(out[k], "x3d_stats_derive: output %d is null", k);
        for (int q = 0; q < X3D_NMOM; q++)
            X3D_REQUIRE(out[k] != mean[q], "x3d_stats_derive: output %d is one of the accumulators", k);
        for (int q = 0; q < k; q++)
            X3D_REQUIRE(out[k] != out[q], "x3d_stats_derive: outputs %d and %d are the same block", q, k);
        o[k] = out[k];
    }
    for (int k = 0; k < X3D_NMOM; k++) X3D_LAZY_IN(b, in[k]);
    for (int k = 0; k < 6; k++) X3D_LAZY_OUT(b, o[k], true);
    X3D_LAZY_EAGER(b);
    Out6 O;
    CMean9 M;
    for (int k = 0; k < 6; k++) O.o[k] = (real2_t *)o[k];
    for (int k = 0; k < X3D_NMOM; k++) M.m[k] = (const real2_t *)in[k];
    ProfScope ps(b, X3D_K_BLAS1);
    const size_t n2 = b->nblock / 2;
    hipLaunchKernelGGL(k_stats_derive, dim3(stat_grid(n2)), dim3(256), 0, b->stream, O, M, n2);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- profiles
// Two stages, deterministic like the other reductions (backend.hip, "reductions"): stage 1 leaves, per kept index and
// part, nine partial sums formed in an order that depends on the launch geometry only; stage 2 adds the parts of a
// kept index in part order.  No atomics.  Partials are FP64 in both flavours; one rounding, at the store to `sums`.
__device__ __forceinline__ void mom_add(double (&s)[X3D_NMOM], double a, double b, double c)
{
    s[0] += a; s[1] += b; s[2] += c;
    s[3] += a * a; s[4] += b * b; s[5] += c * c;
    s[6] += a * b; s[7] += a * c; s[8] += b * c;
}

// kept direction y or z: the points of kept index q are `nrows` x rows of nx points.  blockIdx.y = q, blockIdx.x = part:
// rows part, part + nparts, ...; lanes run along x, two points each.  part[(q * nparts + part) * 9 + m]
__global__ void __launch_bounds__(256) k_prof_rows(const real_t *__restrict__ u, const real_t *__restrict__ v,
                                                   const real_t *__restrict__ w, int nx, int nrows, long qstride,
                                                   long rstride, double *__restrict__ part)
{
    __shared__ double sm[4][X3D_NMOM];
    const int nparts = gridDim.x;
    double s[X3D_NMOM];
#pragma unroll
    for (int m = 0; m < X3D_NMOM; m++) s[m] = 0.0;
    for (int r = blockIdx.x; r < nrows; r += nparts) {
        const long off = (long)blockIdx.y * qstride + (long)r * rstride;  // (a multiple of the pitch: 16-byte aligned)
        for (int i = 2 * threadIdx.x; i < nx; i += 512) {
            if (i + 1 < nx) {
                const real2_t a = ldg_stream((const real2_t *)(u + off + i)), bb = ldg_stream((const real2_t *)(v + off + i)),
                              c = ldg_stream((const real2_t *)(w + off + i));
                mom_add(s, a.x, bb.x, c.x);
                mom_add(s, a.y, bb.y, c.y);
            } else {
                mom_add(s, u[off + i], v[off + i], w[off + i]);
            }
        }
    }
#pragma unroll
    for (int m = 0; m < X3D_NMOM; m++)
        for (int o = 32; o > 0; o >>= 1) s[m] += __shfl_down(s[m], o);
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0)
#pragma unroll
        for (int m = 0; m < X3D_NMOM; m++) sm[wv][m] = s[m];
    __syncthreads();
    if (threadIdx.x < X3D_NMOM) {
        const int m = threadIdx.x;
        part[((long)blockIdx.y * nparts + blockIdx.x) * X3D_NMOM + m] = (sm[0][m] + sm[1][m]) + (sm[2][m] + sm[3][m]);
    }
}

// kept direction x: lane l of every wave owns x index 64 * blockIdx.x + l; the four waves of a workgroup take the rows
// (y, z) 4 * part + wave, then + 4 * nparts, ...; the waves' sums are added in wave order.
__global__ void __launch_bounds__(256) k_prof_x(const real_t *__restrict__ u, const real_t *__restrict__ v,
                                                const real_t *__restrict__ w, int nx, int ny, long nrows, long nxp,
                                                long nyp, double *__restrict__ part)
{
    __shared__ double sm[4][X3D_NMOM][64];
    const int nparts = gridDim.y;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int i = 64 * blockIdx.x + ln;
    double s[X3D_NMOM];
#pragma unroll
    for (int m = 0; m < X3D_NMOM; m++) s[m] = 0.0;
    if (i < nx) {
#pragma unroll 4
        for (long r = 4L * blockIdx.y + wv; r < nrows; r += 4L * nparts) {
            const long off = nxp * (r % ny + nyp * (r / ny)) + i;
            mom_add(s, __builtin_nontemporal_load(u + off), __builtin_nontemporal_load(v + off),
                    __builtin_nontemporal_load(w + off));
        }
    }
#pragma unroll
    for (int m = 0; m < X3D_NMOM; m++) sm[wv][m][ln] = s[m];
    __syncthreads();
    if (i < nx)
        for (int m = wv; m < X3D_NMOM; m += 4)
            part[((long)i * nparts + blockIdx.y) * X3D_NMOM + m] = (sm[0][m][ln] + sm[1][m][ln]) + (sm[2][m][ln] + sm[3][m][ln]);
}

// sums[m][q] = part[q][0][m] + part[q][1][m] + ... in part order, rounded once to the real kind
__global__ void __launch_bounds__(256) k_prof_finish(const double *__restrict__ part, int nkeep, int nparts,
                                                     real_t *__restrict__ sums)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)nkeep * X3D_NMOM) return;
    const int m = (int)(t % X3D_NMOM);
    const long q = t / X3D_NMOM;
    double s = 0.0;
    for (int p = 0; p < nparts; p++) s += part[(q * nparts + p) * X3D_NMOM + m];
    sums[(long)m * nkeep + q] = (real_t)s;
}

extern "C" int x3d_stats_profile_sums(x3d_backend *b, const real_t *u, const real_t *v, const real_t *w,
                                      const int dims[3], int dir_keep, real_t *sums)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && u && v && w && dims && sums, "x3d_stats_profile_sums: null argument");
    X3D_REQUIRE(x3d_dir_ok(dir_keep), "x3d_stats_profile_sums: dir_keep must be 1, 2 or 3 (got %d)", dir_keep);
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_stats_profile_sums: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    const int nx = dims[0], ny = dims[1], nz = dims[2];
    const long nxp = b->nxp, nyp = b->nyp;
    const int nkeep = dims[dir_keep - 1];
    // parts per kept index: enough workgroups to fill the chip (about 4096), never more than there are rows
    long nparts;
    if (dir_keep == X3D_DIR_X) {
        const long nseg = (nx + 63) / 64, groups = ((long)ny * nz + 3) / 4;
        nparts = (1024 + nseg - 1) / nseg;
        if (nparts > groups) nparts = groups;
    } else {
        const long nrows = dir_keep == X3D_DIR_Y ? nz : ny;
        nparts = (4096 + nkeep - 1) / nkeep;
        if (nparts > nrows) nparts = nrows;
    }
    const long need = (long)nkeep * nparts * X3D_NMOM;
    if (need > b->stats_cap) {
        if (b->stats_part) X3D_HIP(hipFree(b->stats_part));
        b->stats_part = nullptr;
        b->stats_cap = 0;
        X3D_HIP(hipMalloc(reinterpret_cast<void **>(&b->stats_part), sizeof(double) * (size_t)need));
        b->stats_cap = need;
    }
    ProfScope ps(b, X3D_K_REDUCE);
    if (dir_keep == X3D_DIR_X)
        hipLaunchKernelGGL(k_prof_x, dim3((unsigned)((nx + 63) / 64), (unsigned)nparts), dim3(256), 0, b->stream, u, v, w, nx,
                           ny, (long)ny * nz, nxp, nyp, b->stats_part);
    else if (dir_keep == X3D_DIR_Y)
        hipLaunchKernelGGL(k_prof_rows, dim3((unsigned)nparts, (unsigned)nkeep), dim3(256), 0, b->stream, u, v, w, nx, nz, nxp,
                           nxp * nyp, b->stats_part);
    else
        hipLaunchKernelGGL(k_prof_rows, dim3((unsigned)nparts, (unsigned)nkeep), dim3(256), 0, b->stream, u, v, w, nx, ny,
                           nxp * nyp, nxp, b->stats_part);
    hipLaunchKernelGGL(k_prof_finish, dim3((unsigned)(((long)nkeep * X3D_NMOM + 255) / 256)), dim3(256), 0, b->stream,
                       (const double *)b->stats_part, nkeep, (int)nparts, sums);
    X3D_HIP(hipGetLastError());
    return 0;
}

// prof += (sums * scale - prof) * stat_inc on n values (accumulate_mean on the plane means)
__global__ void __launch_bounds__(256) k_prof_accumulate(real_t *__restrict__ prof, const real_t *__restrict__ sums, long n,
                                                         real_t scale, real_t inc)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const real_t p = prof[t];
    prof[t] = p + (sums[t] * scale - p) * inc;
}

extern "C" int x3d_stats_profile_accumulate(x3d_backend *b, real_t *prof, const real_t *sums, long n, real_t scale,
                                            real_t stat_inc)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && prof && sums && n > 0, "x3d_stats_profile_accumulate: bad argument");
    X3D_REQUIRE(prof != sums, "x3d_stats_profile_accumulate: prof and sums are the same buffer");
    X3D_LAZY_FLUSH(b);  // (small device buffers, not blocks: nothing to translate, but ordered behind what was recorded)
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_BLAS1);
    hipLaunchKernelGGL(k_prof_accumulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, prof, sums, n, scale,
                       stat_inc);
    X3D_HIP(hipGetLastError());
    return 0;
}
