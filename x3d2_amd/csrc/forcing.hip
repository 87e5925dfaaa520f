// Band forcing of a three-periodic box without a transform.  Not in the reference: this project's own addition.
//
// A forced band holds a few dozen Fourier modes m = (mx, my, mz), 0 <= mx <= Mx, |my| <= My, |mz| <= Mz (the half space of a
// real field; M_d <= 8).  Their coefficients U(m) = sum_x u(x) exp(-i k.x) (the unnormalised DFT, numpy's rfftn) are separable
// sums, and the field of a banded spectrum is a separable synthesis:
//
//   A  x3d_forcing_project   one read of u, v, w.  A workgroup owns FRC_RA lines of one z plane, FRC_PTS points of x and one
//      component; a thread owns two neighbouring x points and adds, line by line, u(i, j, k) exp(-i ky y_j) for my = 0 .. My
//      into registers (the negative my are the conjugates: u is real).  At the end of its lines it multiplies by exp(-i kx x_i), adds its two points,
//      the wave adds its lanes by the shuffle tree 32, 16, .. 1, the four waves are added in wave order: for every component,
//      my >= 0 and mx four reals, T e and conj(T) e.  A second small launch, one wave per coefficient, adds the workgroups of a
//      plane in index order, multiplies by exp(-i kz z_k), gives lane l the planes l, l + 64, .. and adds the lanes by the same
//      tree.  No atomics, one fixed order: two calls on the same fields give the same bits.
//   B  x3d_forcing_coeffs    one workgroup: g = U on the band, optionally made solenoidal, D = sum w Re(g . conj U) / N^2,
//      E_band = 1/2 sum w |U|^2 / N^2, F = c g with c = P / D ("power") or c = A ("linear"), F = 0 where D <= d_min; a row of four
//      doubles {E_band, D, c, c D}.  The sums go through LDS in a fixed tree.
//   C  x3d_forcing_synth     one read-modify-write of the three derivative blocks.  A workgroup owns FRC_RC lines of one z plane:
//      it collapses the z sum for its plane (H, LDS), then the y sum for each of its lines (G, LDS, with w(mx) / N folded in);
//      a thread then adds sum_mx Re(G(mx) exp(i kx x_i)) to its two points of every line: Mx + 1 complex multiply-adds per
//      point and component, in FP64, one rounding at the store.  It returns at once where the row's coefficient is 0.
//
// The twiddles come from three tables the host builds in FP64, tw_d[g][m] = {cos, -sin}(2 pi m g / n_d) for the GLOBAL point index
// g and m = 0 .. M_d: a rank of a decomposed box (y and z may be cut, x never) projects its block with the same tables, and the
// small coefficient array is summed over the ranks between A and B by the host.  Accumulators are FP64 in both flavours.  Row
// padding is never read into a result and keeps its bits.  The launch geometry depends on the dims and the mode box alone.
#include "common.h"

#define FRC_RA 128    // lines of a projection workgroup
#define FRC_RC 32     // lines of a synthesis workgroup
#define FRC_PTS 512   // x points of a workgroup: 256 threads, two each
#define FRC_NB (2 * X3D_FORCING_MMAX + 1)
typedef real_t frc_vec __attribute__((ext_vector_type(2)));

struct FrcGeom {
    int nx, ny, nz, oy, oz;
    long nxp, nyp;
    int Mx, My, Mz;
    int nchunk, njp;  // workgroups along x, groups of lines in a plane
};

static long frc_modes(const int M[3]) { return (long)(M[0] + 1) * (2 * M[1] + 1) * (2 * M[2] + 1); }
static long frc_nq(const int M[3]) { return 3L * (M[1] + 1) * (M[0] + 1) * 4; }

// everything the three entry points refuse about the box and the band; 0 when served
static int frc_check(const x3d_backend *b, const x3d_forcing_params *p, const char *who)
{
    X3D_REQUIRE(b && p, "%s: null argument", who);
    X3D_REQUIRE(p->tw_x && p->tw_y && p->tw_z && p->band && p->kvec, "%s: null table", who);
    for (int d = 0; d < 3; d++) {
        X3D_REQUIRE(p->periodic[d], "%s: direction %d is not periodic", who, d);
        X3D_REQUIRE(p->nlocal[d] > 0 && p->offset[d] >= 0 && p->offset[d] + p->nlocal[d] <= p->nglobal[d],
                    "%s: rows %d .. %d of %d in direction %d", who, p->offset[d], p->offset[d] + p->nlocal[d], p->nglobal[d], d);
        X3D_REQUIRE(p->M[d] >= 0 && p->M[d] <= X3D_FORCING_MMAX, "%s: mode box %d in direction %d (at most %d)", who, p->M[d], d,
                    X3D_FORCING_MMAX);
        X3D_REQUIRE(2 * p->M[d] < p->nglobal[d], "%s: mode box %d reaches the Nyquist mode of %d points in direction %d", who, p->M[d],
                    p->nglobal[d], d);
    }
    X3D_REQUIRE(p->nlocal[0] == p->nglobal[0], "%s: x is never cut (%d of %d points)", who, p->nlocal[0], p->nglobal[0]);
    X3D_REQUIRE(p->nlocal[0] <= b->nxp && p->nlocal[1] <= b->nyp && p->nlocal[2] <= b->nzp, "%s: dims (%d,%d,%d) outside the block", who,
                p->nlocal[0], p->nlocal[1], p->nlocal[2]);
    X3D_REQUIRE(p->nband > 0, "%s: the band is empty", who);
    return 0;
}

static FrcGeom frc_geom(const x3d_backend *b, const x3d_forcing_params *p, int lines)
{
    FrcGeom G;
    G.nx = p->nlocal[0];
    G.ny = p->nlocal[1];
    G.nz = p->nlocal[2];
    G.oy = p->offset[1];
    G.oz = p->offset[2];
    G.nxp = b->nxp;
    G.nyp = b->nyp;
    G.Mx = p->M[0];
    G.My = p->M[1];
    G.Mz = p->M[2];
    G.nchunk = (G.nx + FRC_PTS - 1) / FRC_PTS;
    G.njp = (G.ny + lines - 1) / lines;
    return G;
}

extern "C" int x3d_forcing_sizes(const x3d_forcing_params *p, long sizes[4])
{
    X3D_REQUIRE(p && sizes, "x3d_forcing_sizes: null argument");
    for (int d = 0; d < 3; d++)
        X3D_REQUIRE(p->M[d] >= 0 && p->M[d] <= X3D_FORCING_MMAX && p->nlocal[d] > 0, "x3d_forcing_sizes: mode box or dims out of range");
    const long nchunk = (p->nlocal[0] + FRC_PTS - 1) / FRC_PTS, njp = (p->nlocal[1] + FRC_RA - 1) / FRC_RA;
    sizes[0] = frc_modes(p->M);                             // modes of the box
    sizes[1] = 6 * sizes[0];                                // doubles of a coefficient array [3][modes][re, im]
    sizes[2] = (long)p->nlocal[2] * njp * nchunk * frc_nq(p->M);  // doubles of the projection's partial sums
    sizes[3] = X3D_FORCING_NROW;
    return 0;
}

// the two points of a thread at `off`: n >= 2 both (one 16-byte access in FP64), 1 the first alone, <= 0 none; what lies beyond
// the row reads as zero and is not touched
__device__ __forceinline__ void frc_ld(const real_t *f, long off, int n, double (&a)[2])
{
    if (n >= 2) {
        const frc_vec x = __builtin_nontemporal_load(reinterpret_cast<const frc_vec *>(f + off));
        a[0] = x[0];
        a[1] = x[1];
    } else {
        a[0] = n == 1 ? (double)__builtin_nontemporal_load(f + off) : 0.0;
        a[1] = 0.0;
    }
}

// ---------------------------------------------------------------- A: projection
// blockIdx.y is the component: a workgroup streams ONE block, so that the accumulators of a thread (My + 1 complex numbers for
// each of its two points) leave room for eight lines in flight at seven or eight waves per SIMD
struct FrcIn { const real_t *f[3]; };

template <int MY>
__global__ void __launch_bounds__(256) k_frc_project(FrcGeom G, FrcIn in, const double *__restrict__ twx,
                                                     const double *__restrict__ twy, double *__restrict__ part)
{
    __shared__ double sm[4][(MY + 1) * (X3D_FORCING_MMAX + 1) * 4];
    const long t = blockIdx.x;
    const int c = blockIdx.y;
    const real_t *__restrict__ f = c == 0 ? in.f[0] : (c == 1 ? in.f[1] : in.f[2]);
    const int xc = (int)(t % G.nchunk);
    const int jp = (int)((t / G.nchunk) % G.njp);
    const long k = t / ((long)G.nchunk * G.njp);
    const int i0 = (xc * 256 + (int)threadIdx.x) * 2;
    const int n = G.nx - i0;
    const int j0 = jp * FRC_RA, j1 = j0 + FRC_RA < G.ny ? j0 + FRC_RA : G.ny;
    double T[MY + 1][2][2];  // [my][point][re, im]
#pragma unroll
    for (int m = 0; m <= MY; m++)
#pragma unroll
        for (int p = 0; p < 2; p++) T[m][p][0] = T[m][p][1] = 0.0;
    const long base = G.nxp * G.nyp * k + i0;  // (nxp is a multiple of 16 elements and i0 is even: 16-byte aligned)
#pragma unroll 8
    for (int j = j0; j < j1; j++) {
        double a[2];
        frc_ld(f, base + G.nxp * j, n, a);
        const double *ty = twy + (long)(G.oy + j) * (MY + 1) * 2;  // (uniform over the workgroup)
#pragma unroll
        for (int m = 0; m <= MY; m++) {
            const double cs = ty[2 * m], sn = ty[2 * m + 1];
#pragma unroll
            for (int p = 0; p < 2; p++) {
                T[m][p][0] += a[p] * cs;
                T[m][p][1] += a[p] * sn;
            }
        }
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int nmx = G.Mx + 1;
    for (int mx = 0; mx < nmx; mx++) {
        double e[2][2];
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const bool ok = p < n;
            const double *tx = twx + ((long)(ok ? i0 + p : 0) * nmx + mx) * 2;
            e[p][0] = ok ? tx[0] : 0.0;
            e[p][1] = ok ? tx[1] : 0.0;
        }
#pragma unroll
        for (int m = 0; m <= MY; m++) {
            // T e and conj(T) e, T = a + i b, e = cs + i sn, added over the two points
            double r[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const double ac = T[m][p][0] * e[p][0], bs = T[m][p][1] * e[p][1];
                const double as = T[m][p][0] * e[p][1], bc = T[m][p][1] * e[p][0];
                r[0] += ac - bs;
                r[1] += as + bc;
                r[2] += ac + bs;
                r[3] += as - bc;
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
                for (int o = 32; o > 0; o >>= 1) r[q] += __shfl_down(r[q], o);
            if (ln == 0) {
#pragma unroll
                for (int q = 0; q < 4; q++) sm[wv][(m * nmx + mx) * 4 + q] = r[q];
            }
        }
    }
    __syncthreads();
    const int nq1 = (MY + 1) * nmx * 4;  // (of one component; a workgroup's partial sums are [component][my][mx][4])
    for (int q = threadIdx.x; q < nq1; q += 256) part[(t * 3 + c) * nq1 + q] = (sm[0][q] + sm[1][q]) + (sm[2][q] + sm[3][q]);
}

// one wave per coefficient: uhat[c][mode] = sum_k exp(-i kz z_k) sum over the workgroups of plane k, in index order
__global__ void __launch_bounds__(64) k_frc_project_finish(FrcGeom G, const double *__restrict__ part, const double *__restrict__ twz,
                                                           double *__restrict__ uhat)
{
    const int nb = 2 * G.My + 1, nzb = 2 * G.Mz + 1, nmx = G.Mx + 1;
    const int nm = nmx * nb * nzb;
    const int c = blockIdx.x / nm, mode = blockIdx.x % nm;
    const int a = mode / (nb * nzb), my = (mode / nzb) % nb - G.My, mz = mode % nzb - G.Mz;
    const int amy = my < 0 ? -my : my, amz = mz < 0 ? -mz : mz;
    const long nq = 3L * (G.My + 1) * nmx * 4;
    const long q = ((long)(c * (G.My + 1) + amy) * nmx + a) * 4 + (my < 0 ? 2 : 0);
    const int tp = G.njp * G.nchunk;
    double re = 0.0, im = 0.0;
    for (int k = threadIdx.x; k < G.nz; k += 64) {
        double pr = 0.0, pi = 0.0;
        for (int t = 0; t < tp; t++) {
            const double *p = part + ((long)k * tp + t) * nq + q;
            pr += p[0];
            pi += p[1];
        }
        const double *tz = twz + ((long)(G.oz + k) * (G.Mz + 1) + amz) * 2;
        const double cs = tz[0], sn = mz < 0 ? -tz[1] : tz[1];
        re += pr * cs - pi * sn;
        im += pr * sn + pi * cs;
    }
    for (int o = 32; o > 0; o >>= 1) {
        re += __shfl_down(re, o);
        im += __shfl_down(im, o);
    }
    if (threadIdx.x == 0) {
        uhat[2L * blockIdx.x] = re;
        uhat[2L * blockIdx.x + 1] = im;
    }
}

template <int MY>
static void frc_project_launch(x3d_backend *b, const FrcGeom &G, long ntask, const real_t *u, const real_t *v, const real_t *w,
                               const x3d_forcing_params *p, double *part)
{
    FrcIn in;
    in.f[0] = u;
    in.f[1] = v;
    in.f[2] = w;
    hipLaunchKernelGGL(k_frc_project<MY>, dim3((unsigned)ntask, 3), dim3(256), 0, b->stream, G, in, p->tw_x, p->tw_y, part);
}

extern "C" int x3d_forcing_project(x3d_backend *b, const x3d_forcing_params *prm, const x3d_real *u, const x3d_real *v,
                                   const x3d_real *w, double *part, long part_cap, double *uhat)
{
    X3D_RANGE(__func__);
    if (int rc = frc_check(b, prm, "x3d_forcing_project")) return rc;
    X3D_REQUIRE(u && v && w && part && uhat, "x3d_forcing_project: null argument");
    X3D_REQUIRE(u != v && u != w && v != w, "x3d_forcing_project: two components are the same block");
    const FrcGeom G = frc_geom(b, prm, FRC_RA);
    const long ntask = (long)G.nz * G.njp * G.nchunk;
    X3D_REQUIRE(ntask * frc_nq(prm->M) <= part_cap, "x3d_forcing_project: %ld partial sums, the buffer holds %ld", ntask * frc_nq(prm->M),
                part_cap);
    X3D_REQUIRE(ntask < 0x7fffffffL, "x3d_forcing_project: %ld workgroups", ntask);
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_REDUCE);
    switch (G.My) {
    case 0: frc_project_launch<0>(b, G, ntask, u, v, w, prm, part); break;
    case 1: frc_project_launch<1>(b, G, ntask, u, v, w, prm, part); break;
    case 2: frc_project_launch<2>(b, G, ntask, u, v, w, prm, part); break;
    case 3: frc_project_launch<3>(b, G, ntask, u, v, w, prm, part); break;
    case 4: frc_project_launch<4>(b, G, ntask, u, v, w, prm, part); break;
    case 5: frc_project_launch<5>(b, G, ntask, u, v, w, prm, part); break;
    case 6: frc_project_launch<6>(b, G, ntask, u, v, w, prm, part); break;
    case 7: frc_project_launch<7>(b, G, ntask, u, v, w, prm, part); break;
    default: frc_project_launch<8>(b, G, ntask, u, v, w, prm, part); break;
    }
    hipLaunchKernelGGL(k_frc_project_finish, dim3((unsigned)(3 * frc_modes(prm->M))), dim3(64), 0, b->stream, G, (const double *)part,
                       prm->tw_z, uhat);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- B: coefficients
struct FrcCoef {
    int nm, nplane;  // modes of the box; modes of one mx
    int scheme, solenoidal;
    double value, d_min, inv_n2;
};

// g of mode m: U on the band, minus its part along k when solenoidal; returns whether m is in the band
__device__ __forceinline__ bool frc_g(const FrcCoef &C, const int *band, const double *kvec, const double *uhat, int m,
                                      double (&U)[3][2], double (&g)[3][2])
{
    if (!band[m]) return false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        U[c][0] = g[c][0] = uhat[2L * ((long)c * C.nm + m)];
        U[c][1] = g[c][1] = uhat[2L * ((long)c * C.nm + m) + 1];
    }
    if (C.solenoidal) {
        const double kx = kvec[3 * m], ky = kvec[3 * m + 1], kz = kvec[3 * m + 2];
        const double kk = (kx * kx + ky * ky) + kz * kz;  // (> 0: the mean is never in the band)
        const double pr = ((kx * g[0][0] + ky * g[1][0]) + kz * g[2][0]) / kk, pi = ((kx * g[0][1] + ky * g[1][1]) + kz * g[2][1]) / kk;
        g[0][0] -= kx * pr; g[0][1] -= kx * pi;
        g[1][0] -= ky * pr; g[1][1] -= ky * pi;
        g[2][0] -= kz * pr; g[2][1] -= kz * pi;
    }
    return true;
}

__global__ void __launch_bounds__(256) k_frc_coeffs(FrcCoef C, const int *__restrict__ band, const double *__restrict__ kvec,
                                                    const double *__restrict__ uhat, double *__restrict__ fhat, double *__restrict__ row)
{
    __shared__ double sD[256], sE[256];
    __shared__ double s_coef;
    double D = 0.0, E = 0.0;
    double U[3][2], g[3][2];
    for (int m = threadIdx.x; m < C.nm; m += 256) {
        if (!frc_g(C, band, kvec, uhat, m, U, g)) continue;
        const double wgt = m < C.nplane ? 1.0 : 2.0;  // (mx = 0 comes first)
        double d = 0.0, e = 0.0;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            d += g[c][0] * U[c][0] + g[c][1] * U[c][1];
            e += U[c][0] * U[c][0] + U[c][1] * U[c][1];
        }
        D += wgt * d;
        E += 0.5 * wgt * e;
    }
    sD[threadIdx.x] = D;
    sE[threadIdx.x] = E;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sD[threadIdx.x] += sD[threadIdx.x + s];
            sE[threadIdx.x] += sE[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double Dn = sD[0] * C.inv_n2, En = sE[0] * C.inv_n2;
        const bool ok = Dn > C.d_min;  // (false for a NaN too)
        const double coef = ok ? (C.scheme == X3D_FORCING_POWER ? C.value / Dn : C.value) : 0.0;
        s_coef = coef;
        row[0] = En;
        row[1] = Dn;
        row[2] = coef;
        row[3] = coef * Dn;
    }
    __syncthreads();
    const double coef = s_coef;
    for (int m = threadIdx.x; m < C.nm; m += 256) {
        const bool in = coef != 0.0 && frc_g(C, band, kvec, uhat, m, U, g);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            fhat[2L * ((long)c * C.nm + m)] = in ? coef * g[c][0] : 0.0;
            fhat[2L * ((long)c * C.nm + m) + 1] = in ? coef * g[c][1] : 0.0;
        }
    }
}

extern "C" int x3d_forcing_coeffs(x3d_backend *b, const x3d_forcing_params *prm, const double *uhat, int scheme, double value,
                                  int solenoidal, double d_min, double *fhat, double *row)
{
    X3D_RANGE(__func__);
    if (int rc = frc_check(b, prm, "x3d_forcing_coeffs")) return rc;
    X3D_REQUIRE(uhat && fhat && row, "x3d_forcing_coeffs: null argument");
    X3D_REQUIRE(uhat != fhat, "x3d_forcing_coeffs: uhat and fhat are the same array");
    X3D_REQUIRE(scheme == X3D_FORCING_POWER || scheme == X3D_FORCING_LINEAR, "x3d_forcing_coeffs: unknown scheme %d", scheme);
    X3D_REQUIRE(value >= -1.79e308 && value <= 1.79e308, "x3d_forcing_coeffs: the power or coefficient is not finite");
    X3D_REQUIRE(d_min >= 0.0 && d_min <= 1.79e308, "x3d_forcing_coeffs: d_min (%g) must be finite and not negative", d_min);
    X3D_LAZY_FLUSH(b);  // (small device arrays, not blocks: nothing to translate, but ordered behind what was recorded)
    X3D_LAZY_EAGER(b);
    FrcCoef C;
    C.nm = (int)frc_modes(prm->M);
    C.nplane = (2 * prm->M[1] + 1) * (2 * prm->M[2] + 1);
    C.scheme = scheme;
    C.solenoidal = solenoidal != 0;
    C.value = value;
    C.d_min = d_min;
    const double N = (double)prm->nglobal[0] * prm->nglobal[1] * prm->nglobal[2];
    C.inv_n2 = 1.0 / (N * N);
    ProfScope ps(b, X3D_K_BLAS1);
    hipLaunchKernelGGL(k_frc_coeffs, dim3(1), dim3(256), 0, b->stream, C, prm->band, prm->kvec, uhat, fhat, row);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- C: synthesis
template <int MX>
__global__ void __launch_bounds__(256) k_frc_synth(FrcGeom G, real_t *du, real_t *dv, real_t *dw, const double *__restrict__ twx,
                                                   const double *__restrict__ twy, const double *__restrict__ twz,
                                                   const double *__restrict__ fhat, const double *__restrict__ row, double inv_n)
{
    if (row[X3D_FORCING_ROW_COEF] == 0.0) return;  // (the guard, or a zero coefficient: F is zero and no bit changes)
    __shared__ double sH[3 * (MX + 1) * FRC_NB * 2];  // [component][mx][my][re, im]: the z sum of this plane
    __shared__ double sG[FRC_RC * 3 * (MX + 1) * 2];  // [line][component][mx][re, im]: the y sum of each line, times w(mx) / N
    const long t = blockIdx.x;
    const int xc = (int)(t % G.nchunk);
    const int jp = (int)((t / G.nchunk) % G.njp);
    const long k = t / ((long)G.nchunk * G.njp);
    const int j0 = jp * FRC_RC;
    const int nr = G.ny - j0 < FRC_RC ? G.ny - j0 : FRC_RC;
    const int nb = 2 * G.My + 1, nzb = 2 * G.Mz + 1;
    const long nm = (long)(MX + 1) * nb * nzb;
    for (int o = threadIdx.x; o < 3 * (MX + 1) * nb; o += 256) {
        const int c = o / ((MX + 1) * nb), ab = o % ((MX + 1) * nb);
        double re = 0.0, im = 0.0;
        for (int cz = 0; cz < nzb; cz++) {
            const int mz = cz - G.Mz;
            const double *tz = twz + ((long)(G.oz + k) * (G.Mz + 1) + (mz < 0 ? -mz : mz)) * 2;
            const double cs = tz[0], sn = mz < 0 ? tz[1] : -tz[1];  // exp(+i kz z)
            const double *F = fhat + 2 * (c * nm + (long)ab * nzb + cz);
            re += F[0] * cs - F[1] * sn;
            im += F[0] * sn + F[1] * cs;
        }
        sH[2 * o] = re;
        sH[2 * o + 1] = im;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < nr * 3 * (MX + 1); o += 256) {
        const int r = o / (3 * (MX + 1)), ca = o % (3 * (MX + 1));
        const double wgt = (ca % (MX + 1) == 0 ? 1.0 : 2.0) * inv_n;
        double re = 0.0, im = 0.0;
        for (int bb = 0; bb < nb; bb++) {
            const int my = bb - G.My;
            const double *ty = twy + ((long)(G.oy + j0 + r) * (G.My + 1) + (my < 0 ? -my : my)) * 2;
            const double cs = ty[0], sn = my < 0 ? ty[1] : -ty[1];  // exp(+i ky y)
            const double hr = sH[2 * (ca * nb + bb)], hi = sH[2 * (ca * nb + bb) + 1];
            re += hr * cs - hi * sn;
            im += hr * sn + hi * cs;
        }
        sG[2 * o] = re * wgt;
        sG[2 * o + 1] = im * wgt;
    }
    __syncthreads();
    const int i0 = (xc * 256 + (int)threadIdx.x) * 2;
    const int n = G.nx - i0;
    if (n <= 0) return;  // (after the last barrier)
    double e[2][MX + 1][2];  // exp(+i kx x) of the two points
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int m = 0; m <= MX; m++) {
            const double *tx = twx + ((long)(p < n ? i0 + p : i0) * (MX + 1) + m) * 2;
            e[p][m][0] = tx[0];
            e[p][m][1] = -tx[1];
        }
    real_t *const d[3] = {du, dv, dw};
    const long base = G.nxp * (G.nyp * k + j0) + i0;
#pragma unroll 2
    for (int r = 0; r < nr; r++) {
        const long off = base + G.nxp * r;
        double a[3][2];
#pragma unroll
        for (int c = 0; c < 3; c++) frc_ld(d[c], off, n, a[c]);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double f[2] = {0.0, 0.0};
#pragma unroll
            for (int m = 0; m <= MX; m++) {
                const double gr = sG[2 * ((r * 3 + c) * (MX + 1) + m)], gi = sG[2 * ((r * 3 + c) * (MX + 1) + m) + 1];
#pragma unroll
                for (int p = 0; p < 2; p++) f[p] += gr * e[p][m][0] - gi * e[p][m][1];
            }
            if (n >= 2) {
                frc_vec x;
                x[0] = (real_t)(a[c][0] + f[0]);
                x[1] = (real_t)(a[c][1] + f[1]);
                *reinterpret_cast<frc_vec *>(d[c] + off) = x;
            } else {
                d[c][off] = (real_t)(a[c][0] + f[0]);
            }
        }
    }
}

template <int MX>
static void frc_synth_launch(x3d_backend *b, const FrcGeom &G, long ntask, real_t *du, real_t *dv, real_t *dw,
                             const x3d_forcing_params *p, const double *fhat, const double *row, double inv_n)
{
    hipLaunchKernelGGL(k_frc_synth<MX>, dim3((unsigned)ntask), dim3(256), 0, b->stream, G, du, dv, dw, p->tw_x, p->tw_y, p->tw_z, fhat,
                       row, inv_n);
}

extern "C" int x3d_forcing_synth(x3d_backend *b, const x3d_forcing_params *prm, x3d_real *du, x3d_real *dv, x3d_real *dw,
                                 const double *fhat, const double *row)
{
    X3D_RANGE(__func__);
    if (int rc = frc_check(b, prm, "x3d_forcing_synth")) return rc;
    X3D_REQUIRE(du && dv && dw && fhat && row, "x3d_forcing_synth: null argument");
    X3D_REQUIRE(du != dv && du != dw && dv != dw, "x3d_forcing_synth: two derivative blocks are the same block");
    const FrcGeom G = frc_geom(b, prm, FRC_RC);
    const long ntask = (long)G.nz * G.njp * G.nchunk;
    X3D_REQUIRE(ntask < 0x7fffffffL, "x3d_forcing_synth: %ld workgroups", ntask);
    X3D_LAZY_OUT(b, du, false);
    X3D_LAZY_OUT(b, dv, false);
    X3D_LAZY_OUT(b, dw, false);
    X3D_LAZY_EAGER(b);
    const double inv_n = 1.0 / ((double)prm->nglobal[0] * prm->nglobal[1] * prm->nglobal[2]);
    ProfScope ps(b, X3D_K_BLAS1);
    switch (G.Mx) {
    case 0: frc_synth_launch<0>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    case 1: frc_synth_launch<1>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    case 2: frc_synth_launch<2>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    case 3: frc_synth_launch<3>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    case 4: frc_synth_launch<4>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    case 5: frc_synth_launch<5>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    case 6: frc_synth_launch<6>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    case 7: frc_synth_launch<7>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    default: frc_synth_launch<8>(b, G, ntask, du, dv, dw, prm, fhat, row, inv_n); break;
    }
    X3D_HIP(hipGetLastError());
    return 0;
}
