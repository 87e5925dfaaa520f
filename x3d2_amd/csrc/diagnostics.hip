// Diagnostics series: every scalar of one monitoring row -- kinetic energy, enstrophy, dissipation, wall shear, the maxima
// and the CFL number -- from ONE pass over u, v, w and the nine velocity gradients, left on the device.  The reference's
// monitoring (src/postprocess/monitoring.f90) takes a curl with its reorders, three scalar products and a max / mean, each
// ending in a host wait; here a row is two launches (96 B/DoF in FP64) and no call waits for the host.
//
// Row layout (16 doubles in both flavours of the library; sums and maxima over the rank's interior points):
//    0..2  sum u^2, v^2, w^2                   3  sum |curl u|^2              4  sum S_ij S_ij
//    5, 6  sum of du/dy over the first / last y row (0 where the rank does not own that row)
//    7     sum |f|   (x3d_diag_max_sum)        8..10  max |u|, |v|, |w|      11  max |curl u|^2
//    12    max (|u| ih_x[i] + |v| ih_y[j] + |w| ih_z[k])                     13  max |f|  (x3d_diag_max_sum)      14, 15  0
//
// Summation order (what makes the bits of a row a function of the fields and the shape alone): a work item is one 16-byte
// vector per block and thread, 256 threads side by side along x in one (j, k) row; item t = row * nchunk + chunk goes to
// workgroup t mod G, G = min(items, 256).  A thread adds its items in the order it meets them, a wave adds its lanes by the
// shuffle tree 32, 16, .. 1, the four waves are added in wave order, the G partials in index order.  No atomics.
#include "common.h"

#define DIAG_NSLOT 16
#define DIAG_MAXWG 256
#define DIAG_NRED 12  // reduced per workgroup: seven sums (slots 0..6), five maxima (slots 8..12)
#define DIAG_V (16 / X3D_RB)  // points per 16-byte load: 2 (FP64), 4 (FP32)
typedef real_t diag_vec __attribute__((ext_vector_type(DIAG_V)));

struct DiagIn {
    const real_t *f[12];  // u, v, w, ux, uy, uz, vx, vy, vz, wx, wy, wz
    const double *ih_x, *ih_y, *ih_z;
    int nx, ny, nchunk;
    long nitem, nxp, nyp;
    int first_y, last_y;
};

struct DiagItem {
    real_t v[12][DIAG_V];
    double ihx[DIAG_V], ihy, ihz;
    int wall;  // bit 0: the first y row and the flag is on, bit 1: the last
};

// the vector of item t that belongs to this thread; points beyond nx read as zero and then count for nothing: every
// sum gains 0 and every maximum is one of non-negative values
__device__ __forceinline__ void diag_load(const DiagIn &A, long t, DiagItem &it)
{
    const long row = t / A.nchunk;
    const int ch = (int)(t - row * A.nchunk);
    const int j = (int)(row % A.ny);
    const long k = row / A.ny;
    const int i0 = (ch * 256 + (int)threadIdx.x) * DIAG_V;
    const long off = A.nxp * (j + A.nyp * k) + i0;  // (nxp is a multiple of 16 elements: 16-byte aligned)
    const int n = A.nx - i0;
    if (n >= DIAG_V) {
#pragma unroll
        for (int m = 0; m < 12; m++) {
            const diag_vec x = __builtin_nontemporal_load(reinterpret_cast<const diag_vec *>(A.f[m] + off));
#pragma unroll
            for (int q = 0; q < DIAG_V; q++) it.v[m][q] = x[q];
        }
    } else {
#pragma unroll
        for (int m = 0; m < 12; m++)
#pragma unroll
            for (int q = 0; q < DIAG_V; q++) it.v[m][q] = q < n ? __builtin_nontemporal_load(A.f[m] + off + q) : (real_t)0;
    }
#pragma unroll
    for (int q = 0; q < DIAG_V; q++) it.ihx[q] = q < n ? A.ih_x[i0 + q] : 0.0;
    it.ihy = A.ih_y[j];
    it.ihz = A.ih_z[k];
    it.wall = (j == 0 && A.first_y ? 1 : 0) | (j == A.ny - 1 && A.last_y ? 2 : 0);
}

__device__ __forceinline__ void diag_add(const DiagItem &it, double (&s)[7], double (&mx)[5])
{
#pragma unroll
    for (int q = 0; q < DIAG_V; q++) {
        const double u = it.v[0][q], v = it.v[1][q], w = it.v[2][q];
        const double ux = it.v[3][q], uy = it.v[4][q], uz = it.v[5][q], vx = it.v[6][q], vy = it.v[7][q], vz = it.v[8][q],
                     wx = it.v[9][q], wy = it.v[10][q], wz = it.v[11][q];
        s[0] += u * u;
        s[1] += v * v;
        s[2] += w * w;
        const double ox = wy - vz, oy = uz - wx, oz = vx - uy;
        const double w2 = ox * ox + oy * oy + oz * oz;
        s[3] += w2;
        const double a = uy + vx, b = uz + wx, c = vz + wy;
        s[4] += ux * ux + vy * vy + wz * wz + 0.5 * (a * a + b * b + c * c);
        if (it.wall & 1) s[5] += uy;
        if (it.wall & 2) s[6] += uy;
        const double au = fabs(u), av = fabs(v), aw = fabs(w);
        mx[0] = fmax(mx[0], au);
        mx[1] = fmax(mx[1], av);
        mx[2] = fmax(mx[2], aw);
        mx[3] = fmax(mx[3], w2);
        mx[4] = fmax(mx[4], au * it.ihx[q] + av * it.ihy + aw * it.ihz);
    }
}

// stage 1: part[workgroup][16].  The next item's loads are issued before the current item is added up, so that a CU with
// one workgroup still has loads in flight while it computes.
__global__ void __launch_bounds__(256) k_diag_reduce(DiagIn A, double *__restrict__ part)
{
    __shared__ double sm[4][DIAG_NRED];
    double s[7], mx[5];
#pragma unroll
    for (int m = 0; m < 7; m++) s[m] = 0.0;
#pragma unroll
    for (int m = 0; m < 5; m++) mx[m] = 0.0;
    const long G = gridDim.x;
    long t = blockIdx.x;  // (G <= nitem: every workgroup has a first item)
    DiagItem cur;
    diag_load(A, t, cur);
    for (t += G; t < A.nitem; t += G) {
        DiagItem nxt;
        diag_load(A, t, nxt);
        diag_add(cur, s, mx);
        cur = nxt;
    }
    diag_add(cur, s, mx);
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int m = 0; m < 7; m++) s[m] += __shfl_down(s[m], o);
#pragma unroll
        for (int m = 0; m < 5; m++) mx[m] = fmax(mx[m], __shfl_down(mx[m], o));
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0) {
#pragma unroll
        for (int m = 0; m < 7; m++) sm[wv][m] = s[m];
#pragma unroll
        for (int m = 0; m < 5; m++) sm[wv][7 + m] = mx[m];
    }
    __syncthreads();
    if (threadIdx.x < DIAG_NSLOT) {
        const int slot = threadIdx.x;
        double r = 0.0;
        if (slot < 7) r = ((sm[0][slot] + sm[1][slot]) + sm[2][slot]) + sm[3][slot];
        else if (slot >= 8 && slot <= 12) r = fmax(fmax(sm[0][slot - 1], sm[1][slot - 1]), fmax(sm[2][slot - 1], sm[3][slot - 1]));
        part[(long)blockIdx.x * DIAG_NSLOT + slot] = r;
    }
}

// stage 2: the partials in index order; slots 7 and 13 belong to x3d_diag_max_sum and keep what they hold
__global__ void __launch_bounds__(64) k_diag_finish(const double *__restrict__ part, int nparts, double *__restrict__ row)
{
    const int slot = threadIdx.x;
    if (slot >= DIAG_NSLOT || slot == 7 || slot == 13) return;
    double r = 0.0;
    if (slot < 7) {
        // compensated (Neumaier): up to 256 partials of one sign would otherwise cost sqrt(256) roundings -- more than the
        // whole first stage commits.  Still one fixed order, still the same bits for the same partials.
        double c = 0.0;
#pragma unroll 4
        for (int p = 0; p < nparts; p++) {
            const double x = part[(long)p * DIAG_NSLOT + slot];
            const double t = r + x;
            c += fabs(r) >= fabs(x) ? (r - t) + x : (x - t) + r;
            r = t;
        }
        r += c;
    } else if (slot <= 12) {
#pragma unroll 8
        for (int p = 0; p < nparts; p++) r = fmax(r, part[(long)p * DIAG_NSLOT + slot]);
    }
    row[slot] = r;
}

extern "C" int x3d_diag_reduce(x3d_backend *b, const real_t *u, const real_t *v, const real_t *w, const real_t *const grads[9],
                               const int dims[3], const x3d_diag_params *params, double *row_dev)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && u && v && w && grads && dims && params && row_dev, "x3d_diag_reduce: null argument");
    X3D_REQUIRE(params->ih_x && params->ih_y && params->ih_z, "x3d_diag_reduce: null spacing table");
    const real_t *in[12] = {u, v, w};
    for (int m = 0; m < 9; m++) {
        X3D_REQUIRE(grads[m], "x3d_diag_reduce: gradient block %d is null", m);
        in[3 + m] = grads[m];
    }
    X3D_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, "x3d_diag_reduce: dims (%d,%d,%d) must be positive", dims[0], dims[1],
                dims[2]);
    X3D_REQUIRE(dims[0] <= b->nxp && dims[1] <= b->nyp && dims[2] <= b->nzp, "x3d_diag_reduce: dims (%d,%d,%d) outside the block",
                dims[0], dims[1], dims[2]);
    DiagIn A;
    A.nx = dims[0];
    A.ny = dims[1];
    A.nchunk = (dims[0] + 256 * DIAG_V - 1) / (256 * DIAG_V);
    A.nitem = (long)dims[1] * dims[2] * A.nchunk;
    A.nxp = b->nxp;
    A.nyp = b->nyp;
    const int grid = (int)(A.nitem < DIAG_MAXWG ? A.nitem : DIAG_MAXWG);
    // the partials live in the backend's reduction buffer, read as doubles
    const long cap = (long)(sizeof(real_t) * 2 * (size_t)b->red_cap / sizeof(double));
    X3D_REQUIRE((long)grid * DIAG_NSLOT <= cap, "x3d_diag_reduce: %d x %d partials, the reduction buffer holds %ld", grid,
                DIAG_NSLOT, cap);
    for (int m = 0; m < 12; m++) X3D_LAZY_IN(b, in[m]);
    X3D_LAZY_EAGER(b);
    for (int m = 0; m < 12; m++) A.f[m] = in[m];
    A.ih_x = params->ih_x;
    A.ih_y = params->ih_y;
    A.ih_z = params->ih_z;
    A.first_y = params->first_y != 0;
    A.last_y = params->last_y != 0;
    double *part = reinterpret_cast<double *>(b->red_buf);
    ProfScope ps(b, X3D_K_REDUCE);
    hipLaunchKernelGGL(k_diag_reduce, dim3(grid), dim3(256), 0, b->stream, A, part);
    hipLaunchKernelGGL(k_diag_finish, dim3(1), dim3(64), 0, b->stream, (const double *)part, grid, row_dev);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- max |f| and sum |f| of one block
// Stage 1 is x3d_field_max_sum's own launch (backend.hip); stage 2 does on the device what that entry point does on the host:
// the partial sums added in index order in double and rounded to the real kind, so the two give the same bits.
__global__ void __launch_bounds__(256) k_diag_finish_max_sum(const real_t *__restrict__ part_sum, const real_t *__restrict__ part_max,
                                                             int nparts, double *__restrict__ row)
{
    __shared__ real_t ps[2048], pm[2048];
    for (int p = threadIdx.x; p < nparts; p += 256) {
        ps[p] = part_sum[p];
        pm[p] = part_max[p];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;  // (in double in either flavour, as run_reduce's host loop)
#pragma unroll 8
        for (int p = 0; p < nparts; p++) s += (double)ps[p];
        row[7] = (double)(real_t)s;
    } else if (threadIdx.x == 64) {
        real_t m = 0.0;
#pragma unroll 8
        for (int p = 0; p < nparts; p++) m = fmax(m, pm[p]);
        row[13] = (double)m;
    }
}

extern "C" int x3d_diag_max_sum(x3d_backend *b, const real_t *f, const int dims[3], double *row_dev)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && f && dims && row_dev, "x3d_diag_max_sum: null argument");
    X3D_REQUIRE(dims[0] > 0 && dims[1] > 0 && dims[2] > 0, "x3d_diag_max_sum: dims (%d,%d,%d) must be positive", dims[0], dims[1],
                dims[2]);
    X3D_LAZY_IN(b, f);
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_REDUCE);
    int nparts = 0;
    if (int rc = x3d_reduce_abs_partials_c(b, f, dims, &nparts)) return rc;  // (checks dims and the buffer before it launches)
    hipLaunchKernelGGL(k_diag_finish_max_sum, dim3(1), dim3(256), 0, b->stream, (const real_t *)b->red_buf,
                       (const real_t *)(b->red_buf + b->red_cap), nparts, row_dev);
    X3D_HIP(hipGetLastError());
    return 0;
}
