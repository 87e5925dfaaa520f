// What the spectral Poisson solvers share on the host side (poisson.hip, pfft.hip, sfft.hip, sfft010.hip, sfftz.hip,
// zfirst.hip, y010.hip and fft512.hip itself): the hipFFT error macro, the entry points of the 512-point kernels, the
// tiled transpose, the shared work area of a set of plans, and the layout of the rotation tables.
#pragma once
#include <hipfft/hipfft.h>

#include "common.h"

#define X3D_FFT(expr)                                                                          \
    do {                                                                                       \
        hipfftResult r_ = (expr);                                                              \
        if (r_ != HIPFFT_SUCCESS) {                                                            \
            x3d_set_error("%s failed: hipfft error %d (%s:%d)", #expr, (int)r_, __FILE__,      \
                          __LINE__);                                                           \
            return 3;                                                                          \
        }                                                                                      \
    } while (0)

// ---- the 512-point kernels (fft512.hip, which includes this header: a mismatch does not compile)
int x3d_fft512_init();
const real2_t *x3d_fft512_twiddles();
// axis: 1 = y (ny must be 512), 2 = z (nz must be 512); mode 0 fwd, 1 bwd, 2 fused z pass (waves, ab, nx: mode 2 only)
int x3d_fft512_run(x3d_backend *b, real2_t *c, int nxs, int ny, int nz, int axis, int mode, const real_t *waves,
                   const real_t *ab, int nx);
// xbuf != null (y axis, mode 0 or 1): the far side of the pass is the slab-exchange buffer (see k_fft512)
int x3d_fft512_run_x(x3d_backend *b, real2_t *c, int nxs, int ny, int nz, int axis, int mode, const real_t *waves,
                     const real_t *ab, int nx, real2_t *xbuf, int ys, int ysc);
void x3d_fft512_set_rwT(const real_t *rwT);  // for the next fused z pass
// the fused y pass of the z-first solve: C[nkz][512][px] (x: 512 modes), rwZ = [nkz][512 x][512 y]
int x3d_fft512_run_zh(x3d_backend *b, real2_t *c, long px, int kz0, int nkz, const real_t *rwZ, const real_t *ab, int nx,
                      int ny, int nz);
int x3d_fft512_r2c(x3d_backend *b, real2_t *c, const real_t *f, long nrows, long frow, long crow);
// R: one part of the received array [512 N][W]; waves: that part's [W][512 N]; returns *done = false when the
// sizes are not served (N not 1, 2, 4, 8)
int x3d_fft512_peers(x3d_backend *b, real2_t *R, long W, int npeers, const real_t *waves, const real_t *ab, int nx, int ny,
                     int nz, int nxs, int yoff, bool *done);
// y slabs with the z-first spectrum (sfftz.hip)
int x3d_fft512_peers_yl(x3d_backend *b, real2_t *R, long W, int npeers, const real_t *rw, const real_t *ab, int nx, int ny,
                        int nz, int xs, int xoff, int kz0, int part);

// ---- 32 x 32 tiles through LDS: src [nB][nA] (A contiguous) -> dst [nA][nB] (B contiguous), 512-byte rows both ways
template <class E>
__global__ void __launch_bounds__(256) k_transpose32(E *__restrict__ dst, const E *__restrict__ src, long nA, long nB)
{
    __shared__ E tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long a0 = (long)blockIdx.x * 32, b0 = (long)blockIdx.y * 32;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const long bb = b0 + ty + 8 * r, aa = a0 + tx;
        if (aa < nA && bb < nB) tile[ty + 8 * r][tx] = src[bb * nA + aa];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const long aa = a0 + ty + 8 * r, bb = b0 + tx;
        if (aa < nA && bb < nB) dst[aa * nB + bb] = tile[tx][ty + 8 * r];
    }
}
template <class E>
static int transpose32(hipStream_t st, E *dst, const E *src, long nA, long nB)
{
    hipLaunchKernelGGL(k_transpose32<E>, dim3((unsigned)((nA + 31) / 32), (unsigned)((nB + 31) / 32)), dim3(256), 0, st,
                       dst, src, nA, nB);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---- a solver's plans share ONE work area: create them with auto-allocation off, make them (the caller: every plan
// reports its work size), then allocate the largest size once and set it on the plans that were made
static inline int fft_plans_create(hipfftHandle *const pl[], int n)
{
    for (int i = 0; i < n; i++) {
        X3D_FFT(hipfftCreate(pl[i]));
        X3D_FFT(hipfftSetAutoAllocation(*pl[i], 0));
    }
    return 0;
}
// made: which of the n plans were made (null: all of them); *work_size (optional) = the size allocated
static inline int fft_plans_share_work(hipfftHandle *const pl[], const size_t ws[], const bool made[], int n, void **work,
                                       size_t *work_size = nullptr)
{
    size_t wmax = 0;
    for (int i = 0; i < n; i++) wmax = ws[i] > wmax ? ws[i] : wmax;
    if (wmax) X3D_HIP(hipMalloc(work, wmax));
    if (work_size) *work_size = wmax;
    for (int i = 0; i < n; i++)
        if (!made || made[i]) X3D_FFT(hipfftSetWorkArea(*pl[i], *work));
    return 0;
}
static inline void fft_plans_destroy(hipfftHandle *const pl[], int n, void *work)
{
    for (int i = 0; i < n; i++) hipfftDestroy(*pl[i]);
    hipFree(work);
}

// ---- the six rotation tables of process_spectral_000 / _010 on the device: ONE allocation, ax bx ay by az bz back to
// back; the x tables sit in slots of slot_x >= nx entries (sfft010.hip indexes them by padded mode columns)
struct SpecAB {
    const real_t *ax, *bx, *ay, *by, *az, *bz;
};
static inline size_t spec_ab_elems(int slot_x, int ny, int nz) { return 2 * ((size_t)slot_x + ny + nz); }
static inline SpecAB spec_ab_view(const real_t *dev, int slot_x, int ny, int nz)
{
    SpecAB t;
    t.ax = dev; t.bx = t.ax + slot_x; t.ay = t.bx + slot_x; t.by = t.ay + ny; t.az = t.by + ny; t.bz = t.az + nz;
    return t;
}
// host tables of nx_len, nx_len, ny, ny, nz, nz entries -> dev (spec_ab_elems(slot_x, ny, nz) entries)
static inline int spec_ab_upload(real_t *dev, int slot_x, int ny, int nz, int nx_len, const real_t *ax, const real_t *bx,
                                 const real_t *ay, const real_t *by, const real_t *az, const real_t *bz)
{
    const SpecAB t = spec_ab_view(dev, slot_x, ny, nz);
    const real_t *dst[6] = {t.ax, t.bx, t.ay, t.by, t.az, t.bz}, *src[6] = {ax, bx, ay, by, az, bz};
    const int len[6] = {nx_len, nx_len, ny, ny, nz, nz};
    for (int i = 0; i < 6; i++)
        X3D_HIP(hipMemcpy(const_cast<real_t *>(dst[i]), src[i], sizeof(real_t) * len[i], hipMemcpyHostToDevice));
    return 0;
}
