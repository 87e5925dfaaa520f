// Energy spectra on the device (no counterpart in the reference: this project's own addition, like the profile mode of
// the statistics).  Shell mode: the plain DFT that x3d_poisson_fft_forward leaves in the solver's workspace
// C[nz][ny][nxs] is read ONCE and binned by |k| into E(k).  Plane mode: a 2-D transform over (z, x) per y row into a
// workspace of this object, read once into the one-sided 1-D spectra E_x[y][kx] and E_z[y][kz].
//
// Deterministic like the other reductions (stats.hip, "profiles"; checkpoint.hip): no floating-point atomics, neither
// in LDS nor in global memory; every sum is formed in an order that depends on the launch geometry only, and the launch
// geometry on the dims only.  Bins, partial sums and running means are FP64 in both flavours.
#include <cmath>

#include "fft_util.h"
#include "poisson_priv.h"

#define SPEC_MAXBINS 4096
#define SPEC_MAXGROUPS 2048        // workgroups of the shell launch (8 per CU)
#define SPEC_PART_CAP (1L << 20)   // doubles of stage-1 partials at most (8 MB)
#define SPEC_ITEMS_PER_WAVE 8      // a wave walks at least this many row segments where there are that many
#define SPEC_PLANE_Q 4             // kx modes per thread of the plane launch: a workgroup covers 1024 modes

struct x3d_spectra {
    x3d_backend *b;
    int mode;                  // X3D_SPECTRA_SHELL / X3D_SPECTRA_PLANE
    int nx, ny, nz, nslots;
    int nxm, nxs;              // modes per row, row pitch of the spectrum that is read (shell: the Poisson object's)
    double dk;
    int nbins;
    long len;                  // values per slot: nbins, or ny * (nxm + nz / 2 + 1)
    double *tab;               // kx2[nxm] ky2[ny] kz2[nz] wx[nxm], one allocation
    double *kx2, *ky2, *kz2, *wx;
    double *inst, *mean;       // [nslots][len]
    double *part;              // stage-1 partials
    long part_len;
    // shell launch geometry
    int nchunk, groups;
    // plane mode
    hipfftHandle plan;
    bool have_plan;
    real2_t *c;                // [nz][ny][nxs]
    void *work;
    int zc, nzparts, nxc;      // z rows per workgroup, workgroups along z, workgroups along kx
};

// ---------------------------------------------------------------- shell mode
// An item is one wave-wide segment of one spectral row: lanes = 64 consecutive kx of row (kz, ky).  Along a row |k| grows
// with kx, so the lanes of equal bin are contiguous: a segmented suffix sum in a fixed tree (offsets 1, 2, ... 32) leaves
// every segment's sum in its first lane, which adds it to the wave's OWN bin array in LDS with a plain read-add-write
// (the heads of one item have distinct bins).  Wave w of workgroup g walks the items 4 g + w, + 4 G, ... in that order.
// The four arrays are added in wave order; part[g][bin] goes to global memory and k_spec_shell_finish adds the G
// partials in index order.
__global__ void __launch_bounds__(256) k_spec_shell(const real2_t *__restrict__ c, const double *__restrict__ kx2,
                                                    const double *__restrict__ ky2, const double *__restrict__ kz2,
                                                    const double *__restrict__ wx, int nxm, int nxs, int ny, long nrows,
                                                    int nchunk, double dk, double inv_n2, int nbins,
                                                    double *__restrict__ part)
{
    extern __shared__ double sm_bins[];  // [4][nbins]
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    double *mine = sm_bins + (size_t)wv * nbins;
    for (int t = ln; t < nbins; t += 64) mine[t] = 0.0;
    wave_lds_fence();
    const long nitems = nrows * nchunk, stride = 4L * gridDim.x;
    for (long it = 4L * blockIdx.x + wv; it < nitems; it += stride) {  // (uniform over the wave: every lane shuffles)
        const long row = it / nchunk;
        const int i = (int)(it - row * nchunk) * 64 + ln;
        const bool valid = i < nxm;
        int bin = 0x7fffffff;  // (the lanes behind the row's last mode: one trailing segment that is never stored)
        double e = 0.0;
        if (valid) {
            const int j = (int)(row % ny), k = (int)(row / ny);
            const real2_t v = c[row * nxs + i];
            const double re = (double)v.x, im = (double)v.y;
            // the bin: this order of operations, in FP64 (restated on the host by the tests' reference)
            bin = (int)floor(sqrt((kx2[i] + ky2[j]) + kz2[k]) / dk + 0.5);
            bin = bin < nbins ? bin : nbins - 1;  // (cannot happen for a consistent nbins; keeps the LDS index inside)
            e = (0.5 * wx[i]) * (re * re + im * im) * inv_n2;
        }
        const int left = __shfl_up(bin, 1);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double eo = __shfl_down(e, o);
            const int bo = __shfl_down(bin, o);
            if (ln + o < 64 && bo == bin) e += eo;
        }
        if (valid && (ln == 0 || left != bin)) mine[bin] += e;
        wave_lds_fence();  // the next item's heads may name this item's bins
    }
    __syncthreads();
    const double *s0 = sm_bins, *s1 = s0 + nbins, *s2 = s1 + nbins, *s3 = s2 + nbins;
    for (int t = threadIdx.x; t < nbins; t += 256) part[(size_t)blockIdx.x * nbins + t] = (s0[t] + s1[t]) + (s2[t] + s3[t]);
}

// out[t] = part[0][t] + part[1][t] + ... in index order
__global__ void __launch_bounds__(256) k_spec_shell_finish(const double *__restrict__ part, int groups, int nbins,
                                                           double *__restrict__ out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nbins) return;
    double s = 0.0;
    for (int g = 0; g < groups; g++) s += part[(size_t)g * nbins + t];
    out[t] = s;
}

// ---------------------------------------------------------------- plane mode
// c[nz][ny][nxs] = the 2-D DFT over (z, x) of every y row.  Workgroup (j, p, xc): y row j, the z rows p zc .. p zc + zc - 1,
// the kx modes 1024 xc + t + 256 q of thread t.  A thread adds its modes' energies over the z rows in z order (E_x); per z
// row the workgroup's share of the row sum is a fixed-tree wave reduction, left per wave in LDS and added in wave order
// (E_z).  px[j][p][kx] and pz[j][xc][kz] are the partials k_spec_plane_finish adds in index order.
__global__ void __launch_bounds__(256) k_spec_plane(const real2_t *__restrict__ c, const double *__restrict__ wx, int nxm,
                                                    int nxs, int ny, int nz, int zc, double inv_n2,
                                                    double *__restrict__ px, double *__restrict__ pz)
{
    extern __shared__ double sm_z[];  // [4][zc]
    const int j = blockIdx.x, p = blockIdx.y, xc = blockIdx.z;
    const int nzparts = gridDim.y, nxc = gridDim.z;
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int i0 = xc * (256 * SPEC_PLANE_Q) + threadIdx.x;
    double ex[SPEC_PLANE_Q], hw[SPEC_PLANE_Q];
#pragma unroll
    for (int q = 0; q < SPEC_PLANE_Q; q++) {
        const int i = i0 + 256 * q;
        ex[q] = 0.0;
        hw[q] = i < nxm ? 0.5 * wx[i] : 0.0;
    }
    const int k0 = p * zc;
    for (int kk = 0; kk < zc; kk++) {  // (uniform over the workgroup)
        const int k = k0 + kk;
        double row = 0.0;
        if (k < nz) {
            const real2_t *r = c + ((size_t)k * ny + j) * nxs;
#pragma unroll
            for (int q = 0; q < SPEC_PLANE_Q; q++) {
                const int i = i0 + 256 * q;
                if (i < nxm) {
                    const real2_t v = ldg_stream(r + i);
                    const double re = (double)v.x, im = (double)v.y;
                    const double e = hw[q] * (re * re + im * im) * inv_n2;
                    ex[q] += e;
                    row += e;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) row += __shfl_down(row, o);
        if (ln == 0) sm_z[wv * zc + kk] = row;
    }
#pragma unroll
    for (int q = 0; q < SPEC_PLANE_Q; q++) {
        const int i = i0 + 256 * q;
        if (i < nxm) px[((size_t)j * nzparts + p) * nxm + i] = ex[q];
    }
    __syncthreads();
    for (int kk = threadIdx.x; kk < zc; kk += 256) {
        const int k = k0 + kk;
        if (k < nz)
            pz[((size_t)j * nxc + xc) * nz + k] = (sm_z[kk] + sm_z[zc + kk]) + (sm_z[2 * zc + kk] + sm_z[3 * zc + kk]);
    }
}

// out = E_x[ny][nxm] then E_z[ny][nzh]: E_x[j][i] = px[j][0][i] + px[j][1][i] + ...; S[k] = pz[j][0][k] + pz[j][1][k] + ...,
// E_z[j][k] = S[k] + S[nz - k] (in that order) where nz - k is another mode, else S[k]
__global__ void __launch_bounds__(256) k_spec_plane_finish(const double *__restrict__ px, const double *__restrict__ pz,
                                                           int nxm, int ny, int nz, int nzparts, int nxc,
                                                           double *__restrict__ out)
{
    const int nzh = nz / 2 + 1;
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long n_x = (long)ny * nxm, n_z = (long)ny * nzh;
    if (t < n_x) {
        const long j = t / nxm;
        const int i = (int)(t - j * nxm);
        double s = 0.0;
        for (int p = 0; p < nzparts; p++) s += px[((size_t)j * nzparts + p) * nxm + i];
        out[t] = s;
    } else if (t < n_x + n_z) {
        const long u = t - n_x, j = u / nzh;
        const int k = (int)(u - j * nzh);
        double a = 0.0;
        for (int x = 0; x < nxc; x++) a += pz[((size_t)j * nxc + x) * nz + k];
        const int km = nz - k;
        if (k > 0 && km != k) {
            double m = 0.0;
            for (int x = 0; x < nxc; x++) m += pz[((size_t)j * nxc + x) * nz + km];
            a = a + m;
        }
        out[t] = a;
    }
}

// ---------------------------------------------------------------- running mean
// the statistics' recurrence on every slot in one launch: mean += (inst - mean) / count
__global__ void __launch_bounds__(256) k_spec_accumulate(double *__restrict__ mean, const double *__restrict__ inst, long n,
                                                         double count)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double m = mean[t];
    mean[t] = m + (inst[t] - m) / count;
}

// ---------------------------------------------------------------- the object
static void spectra_free(x3d_spectra *s)
{
    if (s->have_plan) hipfftDestroy(s->plan);
    hipFree(s->tab); hipFree(s->inst); hipFree(s->mean); hipFree(s->part); hipFree(s->c); hipFree(s->work);
    delete s;
}

static inline double mode_k2(int m, int n, double L)
{
    const int sm = m <= n / 2 ? m : m - n;  // the signed mode number
    const double k = 2.0 * M_PI * (double)sm / L;
    return k * k;
}

extern "C" int x3d_spectra_create(x3d_backend *b, x3d_spectra **out, int mode, const int dims[3], const int periodic[3],
                                  const double L[3], double dk, int nslots)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && out && dims && periodic && L, "x3d_spectra_create: null argument");
    X3D_REQUIRE(mode == X3D_SPECTRA_SHELL || mode == X3D_SPECTRA_PLANE, "x3d_spectra_create: mode must be 0 (shell) or 1 (plane), got %d",
                mode);
    X3D_REQUIRE(nslots > 0 && nslots <= 64, "x3d_spectra_create: nslots must be 1 .. 64 (got %d)", nslots);
    X3D_REQUIRE(dims[0] == b->nx && dims[1] == b->ny && dims[2] == b->nz,
                "x3d_spectra_create: dims (%d,%d,%d) are not this backend's vertex dims (%d,%d,%d): spectra on a "
                "decomposed mesh are not built", dims[0], dims[1], dims[2], b->nx, b->ny, b->nz);
    X3D_REQUIRE(dims[0] >= 2 && dims[1] >= 1 && dims[2] >= 2, "x3d_spectra_create: dims too small");
    if (mode == X3D_SPECTRA_SHELL)
        X3D_REQUIRE(periodic[0] && periodic[1] && periodic[2],
                    "x3d_spectra_create: shell mode needs all three directions periodic (periodic = %d,%d,%d)", periodic[0],
                    periodic[1], periodic[2]);
    else
        X3D_REQUIRE(periodic[0] && periodic[2], "x3d_spectra_create: plane mode needs x and z periodic (periodic = %d,%d,%d)",
                    periodic[0], periodic[1], periodic[2]);
    X3D_REQUIRE(L[0] > 0.0 && L[1] > 0.0 && L[2] > 0.0, "x3d_spectra_create: box lengths must be positive");
    const int nx = dims[0], ny = dims[1], nz = dims[2], nxm = nx / 2 + 1;
    int nbins = 0;
    if (mode == X3D_SPECTRA_SHELL) {
        if (!(dk > 0.0)) {  // the default: the coarsest of the three mode spacings
            dk = 0.0;
            for (int d = 0; d < 3; d++) dk = fmax(dk, 2.0 * M_PI / L[d]);
        }
        double s2 = 0.0;
        for (int d = 0; d < 3; d++) s2 += (M_PI * dims[d] / L[d]) * (M_PI * dims[d] / L[d]);
        const double nb = floor(sqrt(s2) / dk + 0.5) + 1.0;
        X3D_REQUIRE(nb <= (double)SPEC_MAXBINS, "x3d_spectra_create: dk = %g gives %.0f bins, at most %d are served", dk, nb,
                    SPEC_MAXBINS);
        nbins = (int)nb;
    }
    x3d_spectra *s = new x3d_spectra();
    memset(s, 0, sizeof *s);
    s->b = b; s->mode = mode; s->nx = nx; s->ny = ny; s->nz = nz; s->nslots = nslots;
    s->nxm = nxm; s->dk = dk; s->nbins = nbins;
    s->len = mode == X3D_SPECTRA_SHELL ? nbins : (long)ny * (nxm + nz / 2 + 1);
    auto fail = [&](int rc) { spectra_free(s); return rc; };
    // tables, FP64 on the host
    std::vector<double> h((size_t)2 * nxm + ny + nz);
    double *hkx = h.data(), *hky = hkx + nxm, *hkz = hky + ny, *hw = hkz + nz;
    for (int i = 0; i < nxm; i++) {
        hkx[i] = mode_k2(i, nx, L[0]);
        hw[i] = (i == 0 || (nx % 2 == 0 && i == nx / 2)) ? 1.0 : 2.0;  // Hermitian weight of the half spectrum
    }
    for (int j = 0; j < ny; j++) hky[j] = mode_k2(j, ny, L[1]);
    for (int k = 0; k < nz; k++) hkz[k] = mode_k2(k, nz, L[2]);
#define SPEC_TRY(expr)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            x3d_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return fail(1);                                                                    \
        }                                                                                      \
    } while (0)
    SPEC_TRY(hipMalloc(&s->tab, sizeof(double) * h.size()));
    SPEC_TRY(hipMemcpy(s->tab, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
    s->kx2 = s->tab; s->ky2 = s->kx2 + nxm; s->kz2 = s->ky2 + ny; s->wx = s->kz2 + nz;
    const size_t nacc = (size_t)nslots * s->len;
    SPEC_TRY(hipMalloc(&s->inst, sizeof(double) * nacc));
    SPEC_TRY(hipMalloc(&s->mean, sizeof(double) * nacc));
    SPEC_TRY(hipMemset(s->inst, 0, sizeof(double) * nacc));
    SPEC_TRY(hipMemset(s->mean, 0, sizeof(double) * nacc));
    if (mode == X3D_SPECTRA_SHELL) {
        s->nchunk = (nxm + 63) / 64;
        const long nitems = (long)nz * ny * s->nchunk;
        long g = (nitems + 4L * SPEC_ITEMS_PER_WAVE - 1) / (4L * SPEC_ITEMS_PER_WAVE);
        if (g > SPEC_MAXGROUPS) g = SPEC_MAXGROUPS;
        if (g > SPEC_PART_CAP / nbins) g = SPEC_PART_CAP / nbins;
        s->groups = (int)(g < 1 ? 1 : g);
        s->part_len = (long)s->groups * nbins;
    } else {
        s->nxs = (nxm + 7) / 8 * 8;  // 128-byte rows, as the Poisson solvers' spectra
        s->nxc = (nxm + 256 * SPEC_PLANE_Q - 1) / (256 * SPEC_PLANE_Q);
        // z parts: about 2048 workgroups in all, at least 4 z rows each where there are that many
        long parts = (2048 + (long)ny * s->nxc - 1) / ((long)ny * s->nxc);
        if (parts > nz / 4) parts = nz / 4;
        if (parts < (nz + 4095) / 4096) parts = (nz + 4095) / 4096;  // (4 x zc doubles of LDS: at most 128 KB)
        s->zc = (int)((nz + parts - 1) / parts);
        s->nzparts = (nz + s->zc - 1) / s->zc;
        s->part_len = (long)ny * s->nzparts * nxm + (long)ny * s->nxc * nz;
        const size_t nc = (size_t)nz * ny * s->nxs;
        SPEC_TRY(hipMalloc(&s->c, sizeof(real2_t) * nc));
        SPEC_TRY(hipMemset(s->c, 0, sizeof(real2_t) * nc));
        // 2-D over (z, x) on the pitched block, batched over the y rows (the form of plan_x010_fw, poisson.hip)
        int nn[2] = {nz, nx};
        int re[2] = {b->nzp, b->nyp * b->nxp}, ce[2] = {nz, ny * s->nxs};
        size_t ws = 0;
// (not fft_util.h's X3D_FFT on purpose: a failure here frees what has been allocated so far before it returns)
#define SPEC_TRY_FFT(expr)                                                                     \
    do {                                                                                       \
        hipfftResult r_ = (expr);                                                              \
        if (r_ != HIPFFT_SUCCESS) {                                                            \
            x3d_set_error("%s failed: hipfft error %d (%s:%d)", #expr, (int)r_, __FILE__, __LINE__); \
            return fail(3);                                                                    \
        }                                                                                      \
    } while (0)
        SPEC_TRY_FFT(hipfftCreate(&s->plan));
        s->have_plan = true;
        SPEC_TRY_FFT(hipfftSetAutoAllocation(s->plan, 0));
        SPEC_TRY_FFT(hipfftMakePlanMany(s->plan, 2, nn, re, 1, b->nxp, ce, 1, s->nxs, X3D_FFT_R2C, ny, &ws));
        if (ws) SPEC_TRY(hipMalloc(&s->work, ws));
        SPEC_TRY_FFT(hipfftSetWorkArea(s->plan, s->work));
    }
    SPEC_TRY(hipMalloc(&s->part, sizeof(double) * (size_t)s->part_len));
    SPEC_TRY(hipMemset(s->part, 0, sizeof(double) * (size_t)s->part_len));
    SPEC_TRY(hipDeviceSynchronize());
#undef SPEC_TRY
#undef SPEC_TRY_FFT
    *out = s;
    return 0;
}

extern "C" int x3d_spectra_destroy(x3d_spectra *s)
{
    X3D_RANGE(__func__);
    if (s) spectra_free(s);
    return 0;
}

// out = {mode, nslots, nbins, values per slot, nx / 2 + 1, nz / 2 + 1, ny, workgroups of the reduction}
extern "C" int x3d_spectra_sizes(const x3d_spectra *s, long out[8], double *dk)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(s && out, "x3d_spectra_sizes: null argument");
    out[0] = s->mode; out[1] = s->nslots; out[2] = s->nbins; out[3] = s->len; out[4] = s->nxm; out[5] = s->nz / 2 + 1;
    out[6] = s->ny;
    out[7] = s->mode == X3D_SPECTRA_SHELL ? s->groups : (long)s->ny * s->nzparts * s->nxc;
    if (dk) *dk = s->dk;
    return 0;
}

// the reduction alone, on whatever the spectrum `c` holds (bench_ops.py times it; x3d_spectra_sample runs it behind the transform)
static int spectra_reduce(x3d_spectra *s, const real2_t *c, int nxs, int slot)
{
    x3d_backend *b = s->b;
    double *out = s->inst + (size_t)slot * s->len;
    ProfScope ps(b, X3D_K_REDUCE);
    if (s->mode == X3D_SPECTRA_SHELL) {
        const double n = (double)s->nx * s->ny * s->nz;
        const size_t lds = sizeof(double) * 4 * (size_t)s->nbins;
        if (lds > 64 * 1024) X3D_LDS_OPTIN(b, k_spec_shell);
        hipLaunchKernelGGL(k_spec_shell, dim3((unsigned)s->groups), dim3(256), lds, b->stream, c, (const double *)s->kx2,
                           (const double *)s->ky2, (const double *)s->kz2, (const double *)s->wx, s->nxm, nxs, s->ny,
                           (long)s->nz * s->ny, s->nchunk, s->dk, 1.0 / (n * n), s->nbins, s->part);
        hipLaunchKernelGGL(k_spec_shell_finish, dim3((unsigned)((s->nbins + 255) / 256)), dim3(256), 0, b->stream,
                           (const double *)s->part, s->groups, s->nbins, out);
    } else {
        const double n = (double)s->nx * s->nz;
        double *px = s->part, *pz = s->part + (size_t)s->ny * s->nzparts * s->nxm;
        if (sizeof(double) * 4 * (size_t)s->zc > 64 * 1024) X3D_LDS_OPTIN(b, k_spec_plane);
        hipLaunchKernelGGL(k_spec_plane, dim3((unsigned)s->ny, (unsigned)s->nzparts, (unsigned)s->nxc), dim3(256),
                           sizeof(double) * 4 * (size_t)s->zc, b->stream, c, (const double *)s->wx, s->nxm, nxs, s->ny, s->nz,
                           s->zc, 1.0 / (n * n), px, pz);
        hipLaunchKernelGGL(k_spec_plane_finish, dim3((unsigned)((s->len + 255) / 256)), dim3(256), 0, b->stream,
                           (const double *)px, (const double *)pz, s->nxm, s->ny, s->nz, s->nzparts, s->nxc, out);
    }
    X3D_HIP(hipGetLastError());
    return 0;
}

static int spectra_check_poisson(const x3d_spectra *s, const x3d_poisson *p, const char *who)
{
    X3D_REQUIRE(p, "%s: shell mode needs the FFT Poisson object of an all-periodic mesh (got null)", who);
    X3D_REQUIRE(p->b == s->b && !p->ext_middle, "%s: the Poisson object belongs to another backend or is a proxy", who);
    X3D_REQUIRE(p->nx == s->nx && p->ny == s->ny && p->nz == s->nz,
                "%s: the Poisson object transforms (%d,%d,%d) cells, the spectra were made for (%d,%d,%d) vertices: shell mode "
                "needs all three directions periodic", who, p->nx, p->ny, p->nz, s->nx, s->ny, s->nz);
    X3D_REQUIRE((size_t)s->nz * s->ny * p->nxs <= p->c_elems && p->nxm == s->nxm, "%s: unexpected spectral layout", who);
    return 0;
}

extern "C" int x3d_spectra_sample(x3d_spectra *s, x3d_poisson *p, const x3d_real *field, int slot)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(s && field, "x3d_spectra_sample: null argument");
    X3D_REQUIRE(slot >= 0 && slot < s->nslots, "x3d_spectra_sample: slot %d outside 0 .. %d", slot, s->nslots - 1);
    x3d_backend *b = s->b;
    if (s->mode == X3D_SPECTRA_SHELL)
        if (int rc = spectra_check_poisson(s, p, "x3d_spectra_sample")) return rc;
    X3D_LAZY_FLUSH(b);       // what was recorded runs first ...
    X3D_LAZY_IN(b, field);   // ... and the handle becomes the buffer that holds its data
    X3D_LAZY_EAGER(b);
    if (s->mode == X3D_SPECTRA_SHELL) {
        if (int rc = x3d_poisson_fft_forward(p, field)) return rc;
        return spectra_reduce(s, p->c, p->nxs, slot);
    }
    {
        ProfScope ps(b, X3D_K_FFT, 1);
        X3D_FFT(hipfftSetStream(s->plan, b->stream));
        X3D_FFT(x3d_fftExecR2C(s->plan, (x3d_fft_real *)const_cast<x3d_real *>(field), (x3d_fft_cplx *)s->c));
    }
    return spectra_reduce(s, s->c, s->nxs, slot);
}

extern "C" int x3d_spectra_reduce(x3d_spectra *s, x3d_poisson *p, int slot)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(s, "x3d_spectra_reduce: null argument");
    X3D_REQUIRE(slot >= 0 && slot < s->nslots, "x3d_spectra_reduce: slot %d outside 0 .. %d", slot, s->nslots - 1);
    if (s->mode == X3D_SPECTRA_SHELL)
        if (int rc = spectra_check_poisson(s, p, "x3d_spectra_reduce")) return rc;
    X3D_LAZY_FLUSH(s->b);
    X3D_LAZY_EAGER(s->b);
    if (s->mode == X3D_SPECTRA_SHELL) return spectra_reduce(s, p->c, p->nxs, slot);
    return spectra_reduce(s, s->c, s->nxs, slot);
}

extern "C" int x3d_spectra_accumulate(x3d_spectra *s, long count)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(s, "x3d_spectra_accumulate: null argument");
    X3D_REQUIRE(count >= 1, "x3d_spectra_accumulate: count must be at least 1 (got %ld)", count);
    x3d_backend *b = s->b;
    X3D_LAZY_FLUSH(b);
    X3D_LAZY_EAGER(b);
    const long n = (long)s->nslots * s->len;
    ProfScope ps(b, X3D_K_BLAS1);
    hipLaunchKernelGGL(k_spec_accumulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, s->mean,
                       (const double *)s->inst, n, (double)count);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_spectra_read(x3d_spectra *s, int which, double *host)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(s && host, "x3d_spectra_read: null argument");
    X3D_REQUIRE(which == 0 || which == 1, "x3d_spectra_read: which must be 0 (instantaneous) or 1 (running mean)");
    x3d_backend *b = s->b;
    X3D_LAZY_FLUSH(b);
    X3D_LAZY_EAGER(b);
    X3D_HIP(hipStreamSynchronize(b->stream));
    b->n_sync++;
    X3D_HIP(hipMemcpy(host, which ? s->mean : s->inst, sizeof(double) * (size_t)s->nslots * s->len, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int x3d_spectra_load(x3d_spectra *s, const double *host_mean)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(s && host_mean, "x3d_spectra_load: null argument");
    x3d_backend *b = s->b;
    X3D_LAZY_FLUSH(b);
    X3D_LAZY_EAGER(b);
    X3D_HIP(hipStreamSynchronize(b->stream));  // (a sample in flight may still write the arrays)
    X3D_HIP(hipMemcpy(s->mean, host_mean, sizeof(double) * (size_t)s->nslots * s->len, hipMemcpyHostToDevice));
    return 0;
}
