// Lagrangian particles: tracers and inertial points, interpolated from u, v, w and advanced on the device.
//
// Not in the reference: this project's own addition, like the probes whose entry-point conventions it shares.  The state is
// FP64 structure-of-arrays in both flavours of the library (rows of n doubles: x, v, a, the previous v and, for inertial
// particles, the drag-plus-gravity term F and its predecessor), field values are widened to double before any arithmetic.
// One thread per particle, no atomics, and every index is formed from a position that was tested for finiteness and brought
// into the domain first: a particle whose new position is not finite is marked (status 2) and loads nothing, ever again.
//
// The rule of one direction (the cell, the nodes, the Lagrange weights) is part_stencil below; tests/particles_ref.py restates
// it in numpy.
#include "common.h"

#include <algorithm>
#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>

// rows of the state
enum { P_X = 0, P_V = 3, P_A = 6, P_VO = 9, P_F = 12, P_FO = 15, P_NROW_TRACER = 12, P_NROW_INERTIAL = 18 };

struct PartAxis {
    const double *c;  // device table of the n vertex coordinates, ascending
    int n, periodic, uniform;
    double L, lo, hi;  // the period; first and last vertex
    double inv_h;      // uniform: 1 / spacing
};
struct PartGeom {
    PartAxis ax[3];
    long nxp, nyp;
};

struct x3d_particles {
    x3d_backend *b;
    int n, order, inertial, absorb, nrow, have_v0;
    int primed, has_hist;
    double tau, g[3];
    PartGeom G;
    double *tabs;     // the three coordinate tables, one allocation
    double *d[2];     // [nrow][n] each: the state and the set a sort permutes it into
    int *ints[2];     // [2][n] each: id, status
    int cur;          // the set that holds the state
    unsigned *keys;   // [2][n]: cell keys in, sorted out
    int *perm;        // [2][n]: 0..n-1 in, the permutation out
    void *tmp;        // rocPRIM's temporary storage, sized at creation
    size_t tmp_bytes;
    unsigned end_bit; // bits of the largest key
    unsigned dead_key;
    struct PartMp *mp; // several ranks (below): null on one rank
    struct PartFb *fb; // two-way coupling (at the end of this file): null until enabled
};

// ---------------------------------------------------------------- the rule of one direction
__device__ __forceinline__ double part_wrap(double x, double L)
{
    x = x - L * floor(x / L);
    if (x >= L) x = 0.0;
    if (x < 0.0) x = 0.0;  // (x one rounding below a multiple of L)
    return x;
}

// the largest i with c[i] <= x (0 if there is none); the last cell of a periodic direction runs to L, any other direction's
// last cell is n - 2.  x is finite and inside the domain; the guess is clamped all the same, and every loop is bounded by n
__device__ __forceinline__ int part_cell(const PartAxis &A, double x)
{
    const double *__restrict__ c = A.c;
    const int n = A.n;
    int i;
    if (A.uniform) {
        const double g = fmin(fmax((x - A.lo) * A.inv_h, 0.0), (double)(n - 1));
        i = (int)g;
        while (i > 0 && c[i] > x) i--;
        while (i < n - 1 && c[i + 1] <= x) i++;
    } else {
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (c[mid] <= x) lo = mid; else hi = mid - 1;
        }
        i = lo;
    }
    if (!A.periodic && i > n - 2) i = n - 2;
    return i;
}

template <int ORDER>
__device__ __forceinline__ void part_stencil(const PartAxis &A, double x, int idx[ORDER], double w[ORDER])
{
    const int n = A.n;
    int s = part_cell(A, x) - (ORDER == 4 ? 1 : 0);
    if (!A.periodic) s = min(max(s, 0), n - ORDER);  // one-sided next to a wall
    double xi[ORDER];
#pragma unroll
    for (int a = 0; a < ORDER; a++) {
        int m = s + a;
        double shift = 0.0;
        if (A.periodic) {  // (n >= ORDER: one wrap is enough)
            if (m < 0) { m += n; shift = -A.L; }
            else if (m >= n) { m -= n; shift = A.L; }
        }
        idx[a] = m;
        xi[a] = A.c[m] + shift;
    }
#pragma unroll
    for (int a = 0; a < ORDER; a++) {
        double p = 1.0;
#pragma unroll
        for (int q = 0; q < ORDER; q++)
            if (q != a) p *= (x - xi[q]) / (xi[a] - xi[q]);
        w[a] = p;
    }
}

template <int ORDER>
__device__ __forceinline__ void part_sample(const PartGeom &G, const real_t *__restrict__ u, const real_t *__restrict__ v,
                                            const real_t *__restrict__ w, const double x[3], double out[3])
{
    int ix[ORDER], iy[ORDER], iz[ORDER];
    double wx[ORDER], wy[ORDER], wz[ORDER];
    part_stencil<ORDER>(G.ax[0], x[0], ix, wx);
    part_stencil<ORDER>(G.ax[1], x[1], iy, wy);
    part_stencil<ORDER>(G.ax[2], x[2], iz, wz);
    double su = 0.0, sv = 0.0, sw = 0.0;
#pragma unroll
    for (int k = 0; k < ORDER; k++) {
        double ku = 0.0, kv = 0.0, kw = 0.0;
#pragma unroll
        for (int j = 0; j < ORDER; j++) {
            const long row = G.nxp * ((long)iy[j] + G.nyp * (long)iz[k]);
            double ju = 0.0, jv = 0.0, jw = 0.0;
#pragma unroll
            for (int i = 0; i < ORDER; i++) {
                const long o = row + ix[i];
                ju += wx[i] * (double)u[o];
                jv += wx[i] * (double)v[o];
                jw += wx[i] * (double)w[o];
            }
            ku += wy[j] * ju; kv += wy[j] * jv; kw += wy[j] * jw;
        }
        su += wz[k] * ku; sv += wz[k] * kv; sw += wz[k] * kw;
    }
    out[0] = su; out[1] = sv; out[2] = sw;
}

// ---------------------------------------------------------------- kernels
// a0 = u(x0); tracers: v0 = a0; inertial: v0 as given (or a0), F0 = (a0 - v0) / tau + g.  The history rows start empty (0):
// the first advance weighs them with 0
template <int ORDER, bool INERTIAL>
__global__ void __launch_bounds__(256) k_particles_prime(PartGeom G, const real_t *__restrict__ u, const real_t *__restrict__ v,
                                                         const real_t *__restrict__ w, double *__restrict__ d,
                                                         const int *__restrict__ status, int n, int have_v0, double tau,
                                                         double gx, double gy, double gz)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n || status[t] != 1) return;
    const long N = n;
    // (accepted by the host: finite, and inside every non-periodic direction; a periodic coordinate may lie anywhere)
    double x[3] = {d[(P_X + 0) * N + t], d[(P_X + 1) * N + t], d[(P_X + 2) * N + t]};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const PartAxis &A = G.ax[c];
        x[c] = A.periodic ? part_wrap(x[c], A.L) : fmin(fmax(x[c], A.lo), A.hi);
        d[(P_X + c) * N + t] = x[c];
    }
    double a[3];
    part_sample<ORDER>(G, u, v, w, x, a);
    const double g[3] = {gx, gy, gz};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double vel = (INERTIAL && have_v0) ? d[(P_V + c) * N + t] : a[c];
        d[(P_A + c) * N + t] = a[c];
        d[(P_V + c) * N + t] = vel;
        d[(P_VO + c) * N + t] = 0.0;
        if (INERTIAL) {
            d[(P_F + c) * N + t] = (a[c] - vel) / tau + g[c];
            d[(P_FO + c) * N + t] = 0.0;
        }
    }
}

template <int ORDER, bool INERTIAL>
__global__ void __launch_bounds__(256) k_particles_advance(PartGeom G, const real_t *__restrict__ u, const real_t *__restrict__ v,
                                                           const real_t *__restrict__ w, double *__restrict__ d,
                                                           int *__restrict__ status, int n, double dt, double c1, double c0,
                                                           int absorb, double tau, double gx, double gy, double gz)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n || status[t] != 1) return;  // a dead particle loads nothing
    const long N = n;
    double x[3], vel[3], vn[3], Fc[3];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        vel[c] = d[(P_V + c) * N + t];
        x[c] = d[(P_X + c) * N + t] + dt * (c1 * vel[c] + c0 * d[(P_VO + c) * N + t]);
        finite = finite && isfinite(x[c]);
        if (INERTIAL) {
            Fc[c] = d[(P_F + c) * N + t];
            vn[c] = vel[c] + dt * (c1 * Fc[c] + c0 * d[(P_FO + c) * N + t]);
            finite = finite && isfinite(vn[c]);
        }
    }
    if (!finite) {  // before any index is formed
        status[t] = 2;
        return;
    }
    bool dead = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const PartAxis &A = G.ax[c];
        if (A.periodic) {
            x[c] = part_wrap(x[c], A.L);
        } else if (x[c] < A.lo || x[c] > A.hi) {
            if (absorb) {
                dead = true;
            } else {  // mirror once
                x[c] = (x[c] < A.lo ? 2.0 * A.lo : 2.0 * A.hi) - x[c];
                if (INERTIAL) vn[c] = -vn[c];
            }
            x[c] = fmin(fmax(x[c], A.lo), A.hi);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) d[(P_X + c) * N + t] = x[c];
    if (dead) {  // frozen on the boundary: nothing but its position and status changes
        status[t] = 0;
        return;
    }
    double a[3];
    part_sample<ORDER>(G, u, v, w, x, a);
    const double g[3] = {gx, gy, gz};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d[(P_A + c) * N + t] = a[c];
        d[(P_VO + c) * N + t] = vel[c];
        if (INERTIAL) {
            d[(P_V + c) * N + t] = vn[c];
            d[(P_FO + c) * N + t] = Fc[c];
            d[(P_F + c) * N + t] = (a[c] - vn[c]) / tau + g[c];
        } else {
            d[(P_V + c) * N + t] = a[c];
        }
    }
}

// u, v, w at m points of the caller's: pts [3][m] -> out [3][m].  A point that is not finite gives NaN and loads nothing; a
// periodic coordinate is wrapped, any other is brought into [lo, hi]
template <int ORDER>
__global__ void __launch_bounds__(256) k_particles_interpolate(PartGeom G, const real_t *__restrict__ u,
                                                               const real_t *__restrict__ v, const real_t *__restrict__ w,
                                                               const double *__restrict__ pts, int m, double *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const long M = m;
    double x[3] = {pts[t], pts[M + t], pts[2 * M + t]};
    double a[3] = {NAN, NAN, NAN};
    if (isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2])) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const PartAxis &A = G.ax[c];
            x[c] = A.periodic ? part_wrap(x[c], A.L) : fmin(fmax(x[c], A.lo), A.hi);
        }
        part_sample<ORDER>(G, u, v, w, x, a);
    }
    out[t] = a[0]; out[M + t] = a[1]; out[2 * M + t] = a[2];
}

__global__ void __launch_bounds__(256) k_particles_keys(PartGeom G, const double *__restrict__ d, const int *__restrict__ status,
                                                        int n, unsigned dead_key, unsigned *__restrict__ keys,
                                                        int *__restrict__ perm)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long N = n;
    unsigned key = dead_key;
    if (status[t] == 1) {  // (an alive particle's position is finite and inside: k_particles_advance)
        const unsigned i = (unsigned)part_cell(G.ax[0], d[(P_X + 0) * N + t]);
        const unsigned j = (unsigned)part_cell(G.ax[1], d[(P_X + 1) * N + t]);
        const unsigned k = (unsigned)part_cell(G.ax[2], d[(P_X + 2) * N + t]);
        key = (k * (unsigned)G.ax[1].n + j) * (unsigned)G.ax[0].n + i;
    }
    keys[t] = key;
    perm[t] = t;
}

__global__ void __launch_bounds__(256) k_particles_gather(const double *__restrict__ d, const int *__restrict__ ints,
                                                          const int *__restrict__ perm, int n, int nrow, double *__restrict__ d2,
                                                          int *__restrict__ ints2)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long N = n;
    const int src = perm[t];
    if (src < 0 || src >= n) return;  // (a permutation of 0..n-1; never an address from anything else)
    for (int r = 0; r < nrow; r++) d2[r * N + t] = d[r * N + src];
    ints2[t] = ints[src];
    ints2[N + t] = ints[N + src];
}

// x, v, a (nine rows of n doubles), then id and status (two rows of n ints), densely, in device order
__global__ void __launch_bounds__(256) k_particles_pack(const double *__restrict__ d, const int *__restrict__ ints, int n,
                                                        double *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long N = n;
#pragma unroll
    for (int r = 0; r < 9; r++) out[r * N + t] = d[r * N + t];
    int *oi = reinterpret_cast<int *>(out + 9 * N);
    oi[t] = ints[t];
    oi[N + t] = ints[N + t];
}

// ---------------------------------------------------------------- host side
static void part_mp_free(x3d_particles *p);
static void part_fb_free(x3d_particles *p);

static void part_free(x3d_particles *p)
{
    if (!p) return;
    part_mp_free(p);
    part_fb_free(p);
    if (p->tabs) hipFree(p->tabs);
    for (int s = 0; s < 2; s++) {
        if (p->d[s]) hipFree(p->d[s]);
        if (p->ints[s]) hipFree(p->ints[s]);
    }
    if (p->keys) hipFree(p->keys);
    if (p->perm) hipFree(p->perm);
    if (p->tmp) hipFree(p->tmp);
    delete p;
}

// positions finite and inside (a periodic coordinate anywhere), velocities and the other rows finite; 0 or the row at fault + 1
static int part_check_rows(const x3d_particles *p, const double *rows, int nrow)
{
    const long n = p->n;
    for (int r = 0; r < nrow; r++) {
        const PartAxis *A = r < 3 ? &p->G.ax[r] : nullptr;
        for (long t = 0; t < n; t++) {
            const double v = rows[r * n + t];
            if (!std::isfinite(v)) return r + 1;
            if (A && !A->periodic && (v < A->lo || v > A->hi)) return r + 1;
        }
    }
    return 0;
}

extern "C" int x3d_particles_create(x3d_backend *b, const x3d_particles_params *prm, const double *x0, const double *v0,
                                    x3d_particles **out)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && prm && x0 && out && prm->coords[0] && prm->coords[1] && prm->coords[2], "x3d_particles_create: null argument");
    X3D_REQUIRE(prm->n >= 1 && prm->n <= X3D_PARTICLES_MAX, "x3d_particles_create: %d particles, 1 to %d can be held", prm->n,
                X3D_PARTICLES_MAX);
    X3D_REQUIRE(prm->order == 2 || prm->order == 4, "x3d_particles_create: order %d (2 or 4)", prm->order);
    X3D_REQUIRE(prm->wall == X3D_PARTICLES_REFLECT || prm->wall == X3D_PARTICLES_ABSORB, "x3d_particles_create: unknown wall rule %d",
                prm->wall);
    X3D_REQUIRE(std::isfinite(prm->tau) && prm->tau >= 0.0, "x3d_particles_create: tau must be finite and not negative");
    X3D_REQUIRE(std::isfinite(prm->g[0]) && std::isfinite(prm->g[1]) && std::isfinite(prm->g[2]),
                "x3d_particles_create: gravity is not finite");
    const int dims[3] = {b->nx, b->ny, b->nz};
    X3D_REQUIRE((double)dims[0] * dims[1] * dims[2] < 4294967295.0, "x3d_particles_create: the cell index does not fit 32 bits");
    for (int c = 0; c < 3; c++) {
        const double *t = prm->coords[c];
        X3D_REQUIRE(dims[c] >= prm->order, "x3d_particles_create: direction %d has %d vertices, order %d needs %d", c + 1, dims[c],
                    prm->order, prm->order);
        for (int i = 0; i < dims[c]; i++)
            X3D_REQUIRE(std::isfinite(t[i]) && (i == 0 || t[i] > t[i - 1]), "x3d_particles_create: the coordinates of direction %d do not ascend",
                        c + 1);
        if (prm->periodic[c])
            X3D_REQUIRE(std::isfinite(prm->L[c]) && t[0] >= 0.0 && t[dims[c] - 1] < prm->L[c],
                        "x3d_particles_create: the vertices of periodic direction %d do not lie in [0, L)", c + 1);
    }
    x3d_particles *p = new x3d_particles();
    p->b = b;
    p->n = prm->n; p->order = prm->order; p->inertial = prm->tau > 0.0; p->absorb = prm->wall == X3D_PARTICLES_ABSORB;
    p->nrow = p->inertial ? P_NROW_INERTIAL : P_NROW_TRACER;
    p->have_v0 = p->inertial && v0 != nullptr;
    p->tau = prm->tau;
    for (int c = 0; c < 3; c++) p->g[c] = prm->g[c];
    p->G.nxp = b->nxp; p->G.nyp = b->nyp;
    for (int c = 0; c < 3; c++) {
        PartAxis &A = p->G.ax[c];
        const double *t = prm->coords[c];
        A.n = dims[c]; A.periodic = prm->periodic[c] != 0; A.uniform = prm->uniform[c] != 0;
        A.lo = t[0]; A.hi = t[dims[c] - 1];
        A.L = A.periodic ? prm->L[c] : A.hi - A.lo;
        A.inv_h = A.periodic ? dims[c] / prm->L[c] : (dims[c] - 1) / (A.hi - A.lo);
    }
    const long n = p->n;
    // the host accepts the input before anything is allocated for it
    std::vector<double> rows((size_t)p->nrow * n, 0.0);
    memcpy(rows.data(), x0, sizeof(double) * 3 * n);
    if (p->have_v0) memcpy(rows.data() + P_V * n, v0, sizeof(double) * 3 * n);
    if (int bad = part_check_rows(p, rows.data(), 6)) {
        x3d_set_error(bad <= 3 ? "x3d_particles_create: a position is not finite or outside [first, last vertex] of direction %d"
                               : "x3d_particles_create: component %d of a velocity is not finite", bad <= 3 ? bad : bad - 3);
        delete p;
        return 2;
    }
    std::vector<int> ints((size_t)2 * n);
    for (long t = 0; t < n; t++) { ints[t] = (int)t; ints[n + t] = 1; }
    hipError_t e = hipSuccess;
    const size_t ntab = (size_t)dims[0] + dims[1] + dims[2];
    auto alloc = [&e](void **q, size_t bytes) { if (e == hipSuccess) e = hipMalloc(q, bytes); };
    alloc(reinterpret_cast<void **>(&p->tabs), sizeof(double) * ntab);
    for (int s = 0; s < 2; s++) {
        alloc(reinterpret_cast<void **>(&p->d[s]), sizeof(double) * p->nrow * n);
        alloc(reinterpret_cast<void **>(&p->ints[s]), sizeof(int) * 2 * n);
    }
    alloc(reinterpret_cast<void **>(&p->keys), sizeof(unsigned) * 2 * n);
    alloc(reinterpret_cast<void **>(&p->perm), sizeof(int) * 2 * n);
    p->dead_key = (unsigned)((long)dims[0] * dims[1] * dims[2]);  // the largest key
    p->end_bit = 1;
    while (p->end_bit < 32 && (p->dead_key >> p->end_bit) != 0) p->end_bit++;
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(nullptr, p->tmp_bytes, p->keys, p->keys + n, p->perm, p->perm + n, (unsigned)n, 0u, p->end_bit,
                                      b->stream);
    if (p->tmp_bytes == 0) p->tmp_bytes = 16;
    alloc(&p->tmp, p->tmp_bytes);
    if (e == hipSuccess) {  // (the host vectors die with this call: synchronous copies)
        size_t off = 0;
        for (int c = 0; c < 3 && e == hipSuccess; c++) {
            e = hipMemcpy(p->tabs + off, prm->coords[c], sizeof(double) * dims[c], hipMemcpyHostToDevice);
            p->G.ax[c].c = p->tabs + off;
            off += dims[c];
        }
    }
    if (e == hipSuccess) e = hipMemcpy(p->d[0], rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->ints[0], ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        part_free(p);
        x3d_set_error("x3d_particles_create: %s", hipGetErrorString(e));
        return 1;
    }
    *out = p;
    return 0;
}

extern "C" int x3d_particles_destroy(x3d_particles *p)
{
    X3D_RANGE(__func__);
    part_free(p);
    return 0;
}

#define PART_FIELD_ARGS(name)                                                                                                    \
    X3D_REQUIRE(b && p && u && v && w && dims, name ": null argument");                                                          \
    X3D_REQUIRE(p->b == b, name ": the particles belong to another backend");                                                    \
    X3D_REQUIRE(!p->mp, name ": these particles live on several ranks (x3d_particles_mp_*)");                                    \
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,         \
                name ": dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);                                          \
    X3D_REQUIRE(dims[0] == p->G.ax[0].n && dims[1] == p->G.ax[1].n && dims[2] == p->G.ax[2].n,                                   \
                name ": dims (%d,%d,%d) are not the vertices the particles were created for", dims[0], dims[1], dims[2])

#define PART_LAUNCH(kernel, nthreads, ...)                                                                                       \
    do {                                                                                                                         \
        if (p->order == 4) {                                                                                                     \
            if (p->inertial) hipLaunchKernelGGL((kernel<4, true>), dim3((unsigned)(((nthreads) + 255) / 256)), dim3(256), 0,     \
                                                b->stream, __VA_ARGS__);                                                         \
            else hipLaunchKernelGGL((kernel<4, false>), dim3((unsigned)(((nthreads) + 255) / 256)), dim3(256), 0, b->stream,     \
                                    __VA_ARGS__);                                                                                \
        } else {                                                                                                                 \
            if (p->inertial) hipLaunchKernelGGL((kernel<2, true>), dim3((unsigned)(((nthreads) + 255) / 256)), dim3(256), 0,     \
                                                b->stream, __VA_ARGS__);                                                         \
            else hipLaunchKernelGGL((kernel<2, false>), dim3((unsigned)(((nthreads) + 255) / 256)), dim3(256), 0, b->stream,     \
                                    __VA_ARGS__);                                                                                \
        }                                                                                                                        \
    } while (0)

extern "C" int x3d_particles_prime(x3d_backend *b, x3d_particles *p, const real_t *u, const real_t *v, const real_t *w,
                                   const int dims[3])
{
    X3D_RANGE(__func__);
    PART_FIELD_ARGS("x3d_particles_prime");
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_COPY);
    PART_LAUNCH(k_particles_prime, p->n, p->G, u, v, w, p->d[p->cur], (const int *)(p->ints[p->cur] + p->n), p->n, p->have_v0, p->tau,
                p->g[0], p->g[1], p->g[2]);
    X3D_HIP(hipGetLastError());
    p->primed = 1;
    p->has_hist = 0;
    return 0;
}

extern "C" int x3d_particles_advance(x3d_backend *b, x3d_particles *p, const real_t *u, const real_t *v, const real_t *w,
                                     const int dims[3], double dt)
{
    X3D_RANGE(__func__);
    PART_FIELD_ARGS("x3d_particles_advance");
    X3D_REQUIRE(p->primed, "x3d_particles_advance: the state was neither primed nor loaded");
    X3D_REQUIRE(std::isfinite(dt) && dt > 0.0, "x3d_particles_advance: dt must be finite and positive");
    X3D_REQUIRE(!p->inertial || p->tau >= 2.0 * dt, "x3d_particles_advance: tau < 2 dt");
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    const double c1 = p->has_hist ? 1.5 : 1.0, c0 = p->has_hist ? -0.5 : 0.0;
    ProfScope ps(b, X3D_K_COPY);
    PART_LAUNCH(k_particles_advance, p->n, p->G, u, v, w, p->d[p->cur], p->ints[p->cur] + p->n, p->n, dt, c1, c0, p->absorb, p->tau,
                p->g[0], p->g[1], p->g[2]);
    X3D_HIP(hipGetLastError());
    p->has_hist = 1;
    return 0;
}

extern "C" int x3d_particles_interpolate(x3d_backend *b, const x3d_particles *p, const real_t *u, const real_t *v, const real_t *w,
                                         const int dims[3], const double *pts_dev, int m, double *out_dev)
{
    X3D_RANGE(__func__);
    PART_FIELD_ARGS("x3d_particles_interpolate");
    X3D_REQUIRE(pts_dev && out_dev, "x3d_particles_interpolate: null argument");
    X3D_REQUIRE(m >= 1 && m <= X3D_PARTICLES_MAX, "x3d_particles_interpolate: %d points, 1 to %d can be taken", m, X3D_PARTICLES_MAX);
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_COPY);
    const dim3 grid((unsigned)((m + 255) / 256));
    if (p->order == 4) hipLaunchKernelGGL(k_particles_interpolate<4>, grid, dim3(256), 0, b->stream, p->G, u, v, w, pts_dev, m, out_dev);
    else hipLaunchKernelGGL(k_particles_interpolate<2>, grid, dim3(256), 0, b->stream, p->G, u, v, w, pts_dev, m, out_dev);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_sort(x3d_backend *b, x3d_particles *p)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && p, "x3d_particles_sort: null argument");
    X3D_REQUIRE(p->b == b, "x3d_particles_sort: the particles belong to another backend");
    X3D_REQUIRE(!p->mp, "x3d_particles_sort: these particles live on several ranks (x3d_particles_mp_*)");
    const int n = p->n, cur = p->cur;
    const dim3 grid((unsigned)((n + 255) / 256));
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_particles_keys, grid, dim3(256), 0, b->stream, p->G, (const double *)p->d[cur],
                       (const int *)(p->ints[cur] + n), n, p->dead_key, p->keys, p->perm);
    X3D_HIP(hipGetLastError());
    size_t bytes = p->tmp_bytes;
    X3D_HIP(rocprim::radix_sort_pairs(p->tmp, bytes, p->keys, p->keys + n, p->perm, p->perm + n, (unsigned)n, 0u, p->end_bit,
                                      b->stream));
    hipLaunchKernelGGL(k_particles_gather, grid, dim3(256), 0, b->stream, (const double *)p->d[cur], (const int *)p->ints[cur],
                       (const int *)(p->perm + n), n, p->nrow, p->d[1 - cur], p->ints[1 - cur]);
    X3D_HIP(hipGetLastError());
    p->cur = 1 - cur;
    return 0;
}

extern "C" int x3d_particles_pack(x3d_backend *b, const x3d_particles *p, void *dst_dev, long capacity)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && p && dst_dev, "x3d_particles_pack: null argument");
    X3D_REQUIRE(p->b == b, "x3d_particles_pack: the particles belong to another backend");
    X3D_REQUIRE(!p->mp, "x3d_particles_pack: these particles live on several ranks (x3d_particles_mp_*)");
    X3D_REQUIRE(capacity >= 80L * p->n, "x3d_particles_pack: the buffer holds %ld bytes, %ld are needed", capacity, 80L * p->n);
    X3D_REQUIRE(((size_t)dst_dev & 7) == 0, "x3d_particles_pack: the buffer is not aligned to 8 bytes");
    if (int rc = x3d_snapshot_wait_for_copy_c(b, dst_dev)) return rc;  // (a copy out of this buffer may still be in flight)
    ProfScope ps(b, X3D_K_PACK);
    hipLaunchKernelGGL(k_particles_pack, dim3((unsigned)((p->n + 255) / 256)), dim3(256), 0, b->stream, (const double *)p->d[p->cur],
                       (const int *)p->ints[p->cur], p->n, reinterpret_cast<double *>(dst_dev));
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_download(x3d_backend *b, const x3d_particles *p, double *rows, int *id, int *status, int *has_hist)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && p && rows && id && status && has_hist, "x3d_particles_download: null argument");
    X3D_REQUIRE(p->b == b, "x3d_particles_download: the particles belong to another backend");
    X3D_REQUIRE(!p->mp, "x3d_particles_download: these particles live on several ranks (x3d_particles_mp_*)");
    X3D_HIP(hipStreamSynchronize(b->stream));
    b->n_sync++;
    const long n = p->n;
    X3D_HIP(hipMemcpy(rows, p->d[p->cur], sizeof(double) * p->nrow * n, hipMemcpyDeviceToHost));
    X3D_HIP(hipMemcpy(id, p->ints[p->cur], sizeof(int) * n, hipMemcpyDeviceToHost));
    X3D_HIP(hipMemcpy(status, p->ints[p->cur] + n, sizeof(int) * n, hipMemcpyDeviceToHost));
    *has_hist = p->has_hist;
    return 0;
}

extern "C" int x3d_particles_upload(x3d_backend *b, x3d_particles *p, const double *rows, const int *id, const int *status,
                                    int has_hist)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && p && rows && id && status, "x3d_particles_upload: null argument");
    X3D_REQUIRE(p->b == b, "x3d_particles_upload: the particles belong to another backend");
    X3D_REQUIRE(!p->mp, "x3d_particles_upload: these particles live on several ranks (x3d_particles_mp_*)");
    const long n = p->n;
    std::vector<char> seen((size_t)n, 0);
    for (long t = 0; t < n; t++) {
        X3D_REQUIRE(id[t] >= 0 && id[t] < n && !seen[id[t]], "x3d_particles_upload: the ids are not a permutation of 0..n-1");
        seen[id[t]] = 1;
        X3D_REQUIRE(status[t] >= 0 && status[t] <= 2, "x3d_particles_upload: unknown status %d", status[t]);
    }
    if (int bad = part_check_rows(p, rows, p->nrow)) {
        x3d_set_error("x3d_particles_upload: row %d holds a value that is not finite, or a position outside the domain", bad - 1);
        return 2;
    }
    X3D_HIP(hipStreamSynchronize(b->stream));
    b->n_sync++;
    X3D_HIP(hipMemcpy(p->d[p->cur], rows, sizeof(double) * p->nrow * n, hipMemcpyHostToDevice));
    X3D_HIP(hipMemcpy(p->ints[p->cur], id, sizeof(int) * n, hipMemcpyHostToDevice));
    X3D_HIP(hipMemcpy(p->ints[p->cur] + n, status, sizeof(int) * n, hipMemcpyHostToDevice));
    p->primed = 1;
    p->has_hist = has_hist != 0;
    return 0;
}

// ================================================================ several ranks
// The state of a rank is `capacity` slots per row with the local count in a device word; every launch covers the slots and
// exits on t >= n_local.  The tables stay the GLOBAL ones: the cell, the stencil, the node coordinates and the weights are
// formed by part_cell / part_stencil exactly as on one rank, and only the translation of a global node index into a row of
// the local block or of a ghost frame (pmp_local, pmp_row) is new.  x is never cut.
enum { PMP_GL = 1 };                                           // ghost planes below; above: order 4 has 2, order 2 has 1
enum { PMP_N = 0, PMP_NMID = 1, PMP_FLAGS = 2, PMP_NWORDS = 4 };  // the device words: count, count between the two
                                                               // halves of a migration, sticky flags

struct PartDecomp {
    int off[3], nl[3], np[3], rank[3];  // first global vertex, local vertices, ranks along and position in each direction
    int gh;                             // ghost planes above
    const real_t *fy, *fz;              // frames: fy [3][GL + gh][nz][nx], fz [3][GL + gh][ny + GL + gh][nx]
    long fy_comp, fz_comp;              // the distance between two components of a frame
};

struct PartMp {
    PartDecomp D;
    int capacity, mig, nblk;
    std::vector<double> htab[3];  // the global tables on the host: the ownership rule of create and upload
    real_t *frame[3];             // [1]: fy, [2]: fz
    int *cnt;                     // PMP_NWORDS
    unsigned char *cls;           // [capacity]: 0 stays, 1 to pprev, 2 to pnext
    int *blk;                     // [6][nblk]: per block of 256 slots the three counts, then the three offsets
    int *mg;                      // [4]: leavers to pprev / pnext kept back (overflow); leavers to pprev / pnext
};

// THE ownership rule, host and device, comparisons on the table's doubles only: rank r of a direction owns
// c[r nl] <= x < c[(r + 1) nl]; the last rank owns up to L (periodic; x is wrapped into [0, L)) or up to and including the
// last vertex
__host__ __device__ inline bool pmp_owns(const double *c, int nl, int np, int periodic, double L, double hi, int r, double x)
{
    if (!(x >= c[(long)r * nl])) return false;
    if (r == np - 1) return periodic ? x < L : x <= hi;
    return x < c[(long)(r + 1) * nl];
}

// 0: owned here, 1: by pprev, 2: by pnext, 3: by neither.  (Two ranks around a period: the neighbour is pnext.)
__device__ __forceinline__ int pmp_side(const PartAxis &A, const PartDecomp &D, int c, double x)
{
    const int np = D.np[c], r = D.rank[c], nl = D.nl[c];
    if (pmp_owns(A.c, nl, np, A.periodic, A.L, A.hi, r, x)) return 0;
    int q = r + 1;
    if (q == np) q = A.periodic ? 0 : -1;
    if (q >= 0 && pmp_owns(A.c, nl, np, A.periodic, A.L, A.hi, q, x)) return 2;
    q = r - 1;
    if (q < 0) q = A.periodic ? np - 1 : -1;
    if (q >= 0 && pmp_owns(A.c, nl, np, A.periodic, A.L, A.hi, q, x)) return 1;
    return 3;
}

// global node m of direction c -> local row, -GL .. nl + gh - 1 in a cut direction (clamped: never an address from a
// particle that is not owned here)
__device__ __forceinline__ int pmp_local(const PartDecomp &D, int c, int m, int N)
{
    int l = m - D.off[c];
    if (D.np[c] > 1) {
        if (l < -PMP_GL) l += N;
        else if (l >= D.nl[c] + D.gh) l -= N;
        return min(max(l, -PMP_GL), D.nl[c] + D.gh - 1);
    }
    return min(max(l, 0), D.nl[c] - 1);
}

// the x row (jl, kl) of the three components: the block, or a frame
__device__ __forceinline__ void pmp_row(const PartGeom &G, const PartDecomp &D, const real_t *__restrict__ u,
                                        const real_t *__restrict__ v, const real_t *__restrict__ w, int jl, int kl,
                                        const real_t *&pu, const real_t *&pv, const real_t *&pw)
{
    const int nx = D.nl[0], ny = D.nl[1], nz = D.nl[2], ng = PMP_GL + D.gh;
    if (kl < 0 || kl >= nz) {
        const int g = kl < 0 ? kl + PMP_GL : PMP_GL + kl - nz;
        pu = D.fz + ((long)g * (ny + ng) + (jl + PMP_GL)) * nx;
        pv = pu + D.fz_comp;
        pw = pv + D.fz_comp;
    } else if (jl < 0 || jl >= ny) {
        const int g = jl < 0 ? jl + PMP_GL : PMP_GL + jl - ny;
        pu = D.fy + ((long)g * nz + kl) * nx;
        pv = pu + D.fy_comp;
        pw = pv + D.fy_comp;
    } else {
        const long o = G.nxp * ((long)jl + G.nyp * (long)kl);
        pu = u + o; pv = v + o; pw = w + o;
    }
}

// a[q] of a small array held in registers, q known at run time only: selects between values, never an address
template <int ORDER, typename T>
__device__ __forceinline__ T part_pick(const T (&a)[ORDER], int q)
{
    if constexpr (ORDER == 4) {
        const T a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
        const T lo = (q & 1) ? a1 : a0, hi = (q & 1) ? a3 : a2;
        return (q & 2) ? hi : lo;
    } else {
        const T a0 = a[0], a1 = a[1];
        return (q & 1) ? a1 : a0;
    }
}

template <int ORDER>
__device__ __forceinline__ void part_sample_mp(const PartGeom &G, const PartDecomp &D, const real_t *__restrict__ u,
                                               const real_t *__restrict__ v, const real_t *__restrict__ w, const double x[3],
                                               double out[3])
{
    int ix[ORDER], iy[ORDER], iz[ORDER];
    double wx[ORDER], wy[ORDER], wz[ORDER];
    part_stencil<ORDER>(G.ax[0], x[0], ix, wx);
    part_stencil<ORDER>(G.ax[1], x[1], iy, wy);
    part_stencil<ORDER>(G.ax[2], x[2], iz, wz);
#pragma unroll
    for (int a = 0; a < ORDER; a++) {
        ix[a] = min(max(ix[a], 0), D.nl[0] - 1);
        iy[a] = pmp_local(D, 1, iy[a], G.ax[1].n);
        iz[a] = pmp_local(D, 2, iz[a], G.ax[2].n);
    }
    bool inside = true;
#pragma unroll
    for (int a = 0; a < ORDER; a++) inside = inside && iy[a] >= 0 && iy[a] < D.nl[1] && iz[a] >= 0 && iz[a] < D.nl[2];
    double su = 0.0, sv = 0.0, sw = 0.0;
    if (inside) {  // most particles: every row lies in the block, the loops of part_sample
#pragma unroll
        for (int k = 0; k < ORDER; k++) {
            double ku = 0.0, kv = 0.0, kw = 0.0;
#pragma unroll
            for (int j = 0; j < ORDER; j++) {
                const long row = G.nxp * ((long)iy[j] + G.nyp * (long)iz[k]);
                double ju = 0.0, jv = 0.0, jw = 0.0;
#pragma unroll
                for (int i = 0; i < ORDER; i++) {
                    const long o = row + ix[i];
                    ju += wx[i] * (double)u[o];
                    jv += wx[i] * (double)v[o];
                    jw += wx[i] * (double)w[o];
                }
                ku += wy[j] * ju; kv += wy[j] * jv; kw += wy[j] * jw;
            }
            su += wz[k] * ku; sv += wz[k] * kv; sw += wz[k] * kw;
        }
    } else {  // next to a cut face: the same sums in the same order, one row at a time (rolled: the three pointers of sixteen
              // rows held at once cost more registers than the whole fast path)
#pragma unroll 1
        for (int k = 0; k < ORDER; k++) {
            const int kl = part_pick<ORDER>(iz, k);
            const double wk = part_pick<ORDER>(wz, k);
            double ku = 0.0, kv = 0.0, kw = 0.0;
#pragma unroll 1
            for (int j = 0; j < ORDER; j++) {
                const double wj = part_pick<ORDER>(wy, j);
                const real_t *pu, *pv, *pw;
                pmp_row(G, D, u, v, w, part_pick<ORDER>(iy, j), kl, pu, pv, pw);
                double ju = 0.0, jv = 0.0, jw = 0.0;
#pragma unroll
                for (int i = 0; i < ORDER; i++) {
                    ju += wx[i] * (double)pu[ix[i]];
                    jv += wx[i] * (double)pv[ix[i]];
                    jw += wx[i] * (double)pw[ix[i]];
                }
                ku += wj * ju; kv += wj * jv; kw += wj * jw;
            }
            su += wk * ku; sv += wk * kv; sw += wk * kw;
        }
    }
    out[0] = su; out[1] = sv; out[2] = sw;
}

// ---------------------------------------------------------------- ghost planes
// the face planes of u, v, w of direction dir (1: y, 2: z) that the neighbours' stencils reach: the lowest gh planes to pprev
// (ss [3][gh][nr][nx]), the highest GL to pnext (se [3][GL][nr][nx]).  y: nr = nz rows of the block; z: nr = ny + GL + gh rows,
// the y ghosts (frame fy, exchanged before) included, so that the edges of a pencil arrive without diagonal messages
__global__ void __launch_bounds__(256) k_pmp_ghost_pack(PartGeom G, PartDecomp D, int dir, const real_t *__restrict__ u,
                                                        const real_t *__restrict__ v, const real_t *__restrict__ w,
                                                        real_t *__restrict__ ss, real_t *__restrict__ se)
{
    const int nx = D.nl[0], ny = D.nl[1], nz = D.nl[2], gh = D.gh, ng = PMP_GL + gh;
    const int nr = dir == 1 ? nz : ny + ng;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= 3L * ng * nr * nx) return;
    const int i = (int)(t % nx), r = (int)((t / nx) % nr), g = (int)((t / ((long)nx * nr)) % ng), c = (int)(t / ((long)nx * nr * ng));
    const int plane = g < gh ? g : D.nl[dir] - PMP_GL + (g - gh);
    const real_t *f = c == 0 ? u : c == 1 ? v : w;
    real_t val;
    if (dir == 1) {
        val = f[i + G.nxp * ((long)plane + G.nyp * (long)r)];
    } else {
        const int jl = r - PMP_GL;
        if (jl >= 0 && jl < ny) val = f[i + G.nxp * ((long)jl + G.nyp * (long)plane)];
        else if (D.np[1] > 1) val = D.fy[c * D.fy_comp + ((long)(jl < 0 ? jl + PMP_GL : PMP_GL + jl - ny) * nz + plane) * nx + i];
        else val = (real_t)0;  // (y is whole here: these rows are never read)
    }
    if (g < gh) ss[((long)(c * gh + g) * nr + r) * nx + i] = val;
    else se[((long)(c * PMP_GL + (g - gh)) * nr + r) * nx + i] = val;
}

// what arrived from pprev (rs [3][GL][nr][nx]) and from pnext (re [3][gh][nr][nx]) -> frame [3][GL + gh][nr][nx]
__global__ void __launch_bounds__(256) k_pmp_ghost_unpack(real_t *__restrict__ frame, const real_t *__restrict__ rs,
                                                          const real_t *__restrict__ re, int gh, int nr, int nx)
{
    const int ng = PMP_GL + gh;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, plane = (long)nr * nx;
    if (t >= 3L * ng * plane) return;
    const long o = t % plane;
    const int g = (int)((t / plane) % ng), c = (int)(t / (plane * ng));
    frame[t] = g < PMP_GL ? rs[(long)(c * PMP_GL + g) * plane + o] : re[(long)(c * gh + (g - PMP_GL)) * plane + o];
}

// ---------------------------------------------------------------- prime, move, sample
template <int ORDER, bool INERTIAL>
__global__ void __launch_bounds__(256) k_pmp_prime(PartGeom G, PartDecomp D, const real_t *__restrict__ u, const real_t *__restrict__ v,
                                                   const real_t *__restrict__ w, double *__restrict__ d,
                                                   const int *__restrict__ status, const int *__restrict__ cnt, int cap, int have_v0,
                                                   double tau, double gx, double gy, double gz)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= min(cnt[PMP_N], cap) || status[t] != 1) return;
    const long N = cap;
    double x[3] = {d[(P_X + 0) * N + t], d[(P_X + 1) * N + t], d[(P_X + 2) * N + t]};
#pragma unroll
    for (int c = 0; c < 3; c++) {  // (create has wrapped and accepted them: nothing changes here)
        const PartAxis &A = G.ax[c];
        x[c] = A.periodic ? part_wrap(x[c], A.L) : fmin(fmax(x[c], A.lo), A.hi);
        d[(P_X + c) * N + t] = x[c];
    }
    double a[3];
    part_sample_mp<ORDER>(G, D, u, v, w, x, a);
    const double g[3] = {gx, gy, gz};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double vel = (INERTIAL && have_v0) ? d[(P_V + c) * N + t] : a[c];
        d[(P_A + c) * N + t] = a[c];
        d[(P_V + c) * N + t] = vel;
        d[(P_VO + c) * N + t] = 0.0;
        if (INERTIAL) {
            d[(P_F + c) * N + t] = (a[c] - vel) / tau + g[c];
            d[(P_FO + c) * N + t] = 0.0;
        }
    }
}

// the first half of k_particles_advance, the same expressions: the new position (and velocity), the finiteness test before
// any index, wrap and wall rule, and the part of the history rotation that does not need the new fluid velocity
template <bool INERTIAL>
__global__ void __launch_bounds__(256) k_pmp_move(PartGeom G, double *__restrict__ d, int *__restrict__ status,
                                                  const int *__restrict__ cnt, int cap, double dt, double c1, double c0, int absorb)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= min(cnt[PMP_N], cap) || status[t] != 1) return;
    const long N = cap;
    double x[3], vel[3], vn[3], Fc[3];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        vel[c] = d[(P_V + c) * N + t];
        x[c] = d[(P_X + c) * N + t] + dt * (c1 * vel[c] + c0 * d[(P_VO + c) * N + t]);
        finite = finite && isfinite(x[c]);
        if (INERTIAL) {
            Fc[c] = d[(P_F + c) * N + t];
            vn[c] = vel[c] + dt * (c1 * Fc[c] + c0 * d[(P_FO + c) * N + t]);
            finite = finite && isfinite(vn[c]);
        }
    }
    if (!finite) {  // before any index is formed; it stays on this rank for good
        status[t] = 2;
        return;
    }
    bool dead = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const PartAxis &A = G.ax[c];
        if (A.periodic) {
            x[c] = part_wrap(x[c], A.L);
        } else if (x[c] < A.lo || x[c] > A.hi) {
            if (absorb) {
                dead = true;
            } else {  // mirror once
                x[c] = (x[c] < A.lo ? 2.0 * A.lo : 2.0 * A.hi) - x[c];
                if (INERTIAL) vn[c] = -vn[c];
            }
            x[c] = fmin(fmax(x[c], A.lo), A.hi);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) d[(P_X + c) * N + t] = x[c];
    if (dead) {
        status[t] = 0;
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d[(P_VO + c) * N + t] = vel[c];
        if (INERTIAL) {
            d[(P_V + c) * N + t] = vn[c];
            d[(P_FO + c) * N + t] = Fc[c];
        }
    }
}

// the second half: a = u(x) through the ghost-aware rows; tracers v = a, inertial F = (a - v) / tau + g
template <int ORDER, bool INERTIAL>
__global__ void __launch_bounds__(256) k_pmp_sample(PartGeom G, PartDecomp D, const real_t *__restrict__ u, const real_t *__restrict__ v,
                                                    const real_t *__restrict__ w, double *__restrict__ d,
                                                    const int *__restrict__ status, const int *__restrict__ cnt, int cap, double tau,
                                                    double gx, double gy, double gz)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= min(cnt[PMP_N], cap) || status[t] != 1) return;
    const long N = cap;
    const double x[3] = {d[(P_X + 0) * N + t], d[(P_X + 1) * N + t], d[(P_X + 2) * N + t]};
    double a[3];
    part_sample_mp<ORDER>(G, D, u, v, w, x, a);
    const double g[3] = {gx, gy, gz};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        d[(P_A + c) * N + t] = a[c];
        if (INERTIAL) d[(P_F + c) * N + t] = (a[c] - d[(P_V + c) * N + t]) / tau + g[c];
        else d[(P_V + c) * N + t] = a[c];
    }
}

// ---------------------------------------------------------------- migration along one direction
// 1. the class of every resident and the three counts of every block of 256 slots
__global__ void __launch_bounds__(256) k_pmp_classify(PartAxis A, PartDecomp D, int c, const double *__restrict__ d,
                                                      const int *__restrict__ status, int *__restrict__ cnt, int cap,
                                                      unsigned char *__restrict__ cls, int *__restrict__ blk, int nblk)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    int k = -1;
    if (t < min(cnt[PMP_N], cap)) {
        k = 0;
        if (status[t] != 2) {  // (a position that is not finite is compared with nothing)
            k = pmp_side(A, D, c, d[(long)(P_X + c) * cap + t]);
            if (k == 3) {
                atomicOr(&cnt[PMP_FLAGS], X3D_PARTICLES_FLAG_FAR);
                k = 0;
            }
        }
        cls[t] = (unsigned char)k;
    }
    const int c0 = __syncthreads_count(k == 0), c1 = __syncthreads_count(k == 1), c2 = __syncthreads_count(k == 2);
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = c0;
        blk[nblk + blockIdx.x] = c1;
        blk[2 * nblk + blockIdx.x] = c2;
    }
}

// 2. one block: the exclusive offsets of every block and class.  A class of leavers that does not fit its message stays where
// it is, as a whole, and the flag is set
__global__ void __launch_bounds__(1024) k_pmp_scan(int *__restrict__ blk, int nblk, int mig, int *__restrict__ cnt, int *__restrict__ mg)
{
    __shared__ int sh[3][1024];
    const int tid = threadIdx.x, per = (nblk + 1023) / 1024;
    const int b0 = min(tid * per, nblk), b1 = min(b0 + per, nblk);
    int s[3] = {0, 0, 0};
    for (int b = b0; b < b1; b++)
        for (int q = 0; q < 3; q++) s[q] += blk[q * nblk + b];
    for (int q = 0; q < 3; q++) sh[q][tid] = s[q];
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        int a[3] = {0, 0, 0};
        if (tid >= o)
            for (int q = 0; q < 3; q++) a[q] = sh[q][tid - o];
        __syncthreads();
        for (int q = 0; q < 3; q++) sh[q][tid] += a[q];
        __syncthreads();
    }
    const int T0 = sh[0][1023], T1 = sh[1][1023], T2 = sh[2][1023];
    const bool keep1 = T1 > mig, keep2 = T2 > mig;
    int p[3];
    for (int q = 0; q < 3; q++) p[q] = sh[q][tid] - s[q];  // exclusive
    int r0 = p[0] + (keep1 ? p[1] : 0) + (keep2 ? p[2] : 0), r1 = keep1 ? 0 : p[1], r2 = keep2 ? 0 : p[2];
    for (int b = b0; b < b1; b++) {
        const int c0 = blk[b], c1 = blk[nblk + b], c2 = blk[2 * nblk + b];
        blk[3 * nblk + b] = r0;
        blk[4 * nblk + b] = r1;
        blk[5 * nblk + b] = r2;
        r0 += c0 + (keep1 ? c1 : 0) + (keep2 ? c2 : 0);
        r1 += keep1 ? 0 : c1;
        r2 += keep2 ? 0 : c2;
    }
    if (tid == 0) {
        mg[0] = keep1; mg[1] = keep2; mg[2] = keep1 ? 0 : T1; mg[3] = keep2 ? 0 : T2;
        cnt[PMP_NMID] = T0 + (keep1 ? T1 : 0) + (keep2 ? T2 : 0);
        if (keep1 || keep2) atomicOr(&cnt[PMP_FLAGS], X3D_PARTICLES_FLAG_MIG);
    }
}

// 3. every resident to its slot, a function of the input order alone: the stayers to the front of the second set, the leavers
// as whole rows into the two messages ([0]: the count, then [nrow][mig] doubles, then id and status [2][mig] ints)
__global__ void __launch_bounds__(256) k_pmp_scatter(const double *__restrict__ d, const int *__restrict__ ints,
                                                     double *__restrict__ d2, int *__restrict__ ints2, int cap, int nrow,
                                                     const int *__restrict__ cnt, const unsigned char *__restrict__ cls,
                                                     const int *__restrict__ off, int nblk, const int *__restrict__ mg,
                                                     double *__restrict__ bufp, double *__restrict__ bufn, int mig)
{
    __shared__ int wt[3][4];
    const int t = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int k = -1;
    if (t < min(cnt[PMP_N], cap)) {
        k = cls[t];
        if ((k == 1 && mg[0]) || (k == 2 && mg[1])) k = 0;
    }
    int rank = 0;
    for (int q = 0; q < 3; q++) {
        const unsigned long long m = __ballot(k == q);
        if (k == q) rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wt[q][wave] = __popcll(m);
    }
    __syncthreads();
    if (t == 0) {
        reinterpret_cast<long long *>(bufp)[0] = mg[2];
        reinterpret_cast<long long *>(bufn)[0] = mg[3];
    }
    if (k < 0) return;
    for (int q = 0; q < wave; q++) rank += wt[k][q];
    const int slot = off[k * nblk + blockIdx.x] + rank;
    const long N = cap;
    if (k == 0) {
        if (slot >= cap) return;
        for (int r = 0; r < nrow; r++) d2[r * N + slot] = d[r * N + t];
        ints2[slot] = ints[t];
        ints2[N + slot] = ints[N + t];
    } else {
        if (slot >= mig) return;
        double *buf = k == 1 ? bufp : bufn;
        for (int r = 0; r < nrow; r++) buf[1 + (long)r * mig + slot] = d[r * N + t];
        int *bi = reinterpret_cast<int *>(buf + 1 + (long)nrow * mig);
        bi[slot] = ints[t];
        bi[mig + slot] = ints[N + t];
    }
}

// 4. the arrivals behind the stayers: those from pprev, then those from pnext, each in the sender's order.  What does not fit
// `capacity` is not taken and the flag is set
__global__ void __launch_bounds__(256) k_pmp_append(double *__restrict__ d, int *__restrict__ ints, int cap, int nrow,
                                                    int *__restrict__ cnt, const double *__restrict__ rp,
                                                    const double *__restrict__ rn, int mig)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int n = min(max(cnt[PMP_NMID], 0), cap);
    long long cp = reinterpret_cast<const long long *>(rp)[0], cn = reinterpret_cast<const long long *>(rn)[0];
    const bool bad = cp < 0 || cp > mig || cn < 0 || cn > mig;  // (not a count this code wrote)
    if (cp < 0 || cp > mig) cp = 0;
    if (cn < 0 || cn > mig) cn = 0;
    const int room = cap - n, tp = min((int)cp, room), tn = min((int)cn, room - tp);
    if (t == 0) {
        cnt[PMP_N] = n + tp + tn;
        if (tp < cp || tn < cn) atomicOr(&cnt[PMP_FLAGS], X3D_PARTICLES_FLAG_CAP);
        if (bad) atomicOr(&cnt[PMP_FLAGS], X3D_PARTICLES_FLAG_MIG);
    }
    const double *buf;
    int src, slot;
    if (t < mig) { buf = rp; src = t; if (src >= tp) return; slot = n + src; }
    else if (t < 2 * mig) { buf = rn; src = t - mig; if (src >= tn) return; slot = n + tp + src; }
    else return;
    const long N = cap;
    for (int r = 0; r < nrow; r++) d[r * N + slot] = buf[1 + (long)r * mig + src];
    const int *bi = reinterpret_cast<const int *>(buf + 1 + (long)nrow * mig);
    ints[slot] = bi[src];
    ints[N + slot] = bi[mig + src];
}

// the local cell key; particles that are not alive next to last, empty slots last
__global__ void __launch_bounds__(256) k_pmp_keys(PartGeom G, PartDecomp D, const double *__restrict__ d, const int *__restrict__ status,
                                                  const int *__restrict__ cnt, int cap, unsigned dead_key, unsigned *__restrict__ keys,
                                                  int *__restrict__ perm)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= cap) return;
    const long N = cap;
    unsigned key = dead_key + 1u;
    if (t < min(cnt[PMP_N], cap)) {
        key = dead_key;
        if (status[t] == 1) {
            const int i = part_cell(G.ax[0], d[(P_X + 0) * N + t]);
            const int j = min(max(part_cell(G.ax[1], d[(P_X + 1) * N + t]) - D.off[1], 0), D.nl[1] - 1);
            const int k = min(max(part_cell(G.ax[2], d[(P_X + 2) * N + t]) - D.off[2], 0), D.nl[2] - 1);
            key = ((unsigned)k * (unsigned)D.nl[1] + (unsigned)j) * (unsigned)D.nl[0] + (unsigned)i;
        }
    }
    keys[t] = key;
    perm[t] = t;
}

// x, v, a (nine rows of `capacity` doubles), id and status (two rows of `capacity` ints), then the local count and the flags
// (two ints)
__global__ void __launch_bounds__(256) k_pmp_pack(const double *__restrict__ d, const int *__restrict__ ints,
                                                  const int *__restrict__ cnt, int cap, double *__restrict__ out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= cap) return;
    const long N = cap;
#pragma unroll
    for (int r = 0; r < 9; r++) out[r * N + t] = d[r * N + t];
    int *oi = reinterpret_cast<int *>(out + 9 * N);
    oi[t] = ints[t];
    oi[N + t] = ints[N + t];
    if (t == 0) {
        oi[2 * N] = min(cnt[PMP_N], cap);
        oi[2 * N + 1] = cnt[PMP_FLAGS];
    }
}

// ---------------------------------------------------------------- host side
static void part_mp_free(x3d_particles *p)
{
    PartMp *m = p->mp;
    if (!m) return;
    for (int c = 1; c < 3; c++)
        if (m->frame[c]) hipFree(m->frame[c]);
    if (m->cnt) hipFree(m->cnt);
    if (m->cls) hipFree(m->cls);
    if (m->blk) hipFree(m->blk);
    if (m->mg) hipFree(m->mg);
    delete m;
    p->mp = nullptr;
}

// does this rank own the (wrapped, finite) position?  0, or the direction that says no + 1
static int part_mp_owned(const x3d_particles *p, const double x[3])
{
    const PartMp *m = p->mp;
    for (int c = 1; c < 3; c++) {
        const PartAxis &A = p->G.ax[c];
        if (m->D.np[c] > 1 && !pmp_owns(m->htab[c].data(), m->D.nl[c], m->D.np[c], A.periodic, A.L, A.hi, m->D.rank[c], x[c])) return c + 1;
    }
    return 0;
}

static double part_wrap_host(double x, double L)
{
    x = x - L * std::floor(x / L);
    if (x >= L) x = 0.0;
    if (x < 0.0) x = 0.0;
    return x;
}

// rows [nrow][m] of m particles, ids, statuses: what create and upload accept.  0 or an error code with the message set
static int part_mp_check(const x3d_particles *p, const char *who, const double *rows, int nrow, const int *id, const int *status, long m)
{
    for (int r = 0; r < nrow; r++) {
        const PartAxis *A = r < 3 ? &p->G.ax[r] : nullptr;
        for (long t = 0; t < m; t++) {
            const double v = rows[r * m + t];
            if ((status && status[t] == 2 && r < 3) ? false : !std::isfinite(v)) {
                x3d_set_error("%s: row %d holds a value that is not finite", who, r);
                return 2;
            }
            if (A && std::isfinite(v) && (A->periodic ? (v < 0.0 || v >= A->L) : (v < A->lo || v > A->hi))) {
                x3d_set_error("%s: a position lies outside the domain in direction %d", who, r + 1);
                return 2;
            }
        }
    }
    std::vector<int> seen(id, id + m);
    std::sort(seen.begin(), seen.end());
    for (long t = 0; t < m; t++) {
        if (seen[t] < 0 || seen[t] >= p->n || (t > 0 && seen[t] == seen[t - 1])) {
            x3d_set_error("%s: the ids are not distinct values of 0..n-1", who);
            return 2;
        }
        if (status && (status[t] < 0 || status[t] > 2)) {
            x3d_set_error("%s: unknown status %d", who, status[t]);
            return 2;
        }
        if (status && status[t] == 2) continue;  // (it stays where it died)
        const double x[3] = {rows[t], rows[m + t], rows[2 * m + t]};
        if (int bad = part_mp_owned(p, x)) {
            x3d_set_error("%s: particle %d is not owned by this rank (direction %d)", who, id[t], bad);
            return 2;
        }
    }
    return 0;
}

extern "C" int x3d_particles_mp_create(x3d_backend *b, const x3d_particles_params *prm, const x3d_particles_decomp *dc,
                                       const double *x0, const double *v0, const int *id, int m, x3d_particles **out)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && prm && dc && out && prm->coords[0] && prm->coords[1] && prm->coords[2], "x3d_particles_mp_create: null argument");
    X3D_REQUIRE(m == 0 || (x0 && id), "x3d_particles_mp_create: null argument");
    X3D_REQUIRE(prm->n >= 1 && prm->n <= X3D_PARTICLES_MAX, "x3d_particles_mp_create: %d particles, 1 to %d can be held", prm->n,
                X3D_PARTICLES_MAX);
    X3D_REQUIRE(prm->order == 2 || prm->order == 4, "x3d_particles_mp_create: order %d (2 or 4)", prm->order);
    X3D_REQUIRE(prm->wall == X3D_PARTICLES_REFLECT || prm->wall == X3D_PARTICLES_ABSORB, "x3d_particles_mp_create: unknown wall rule %d",
                prm->wall);
    X3D_REQUIRE(std::isfinite(prm->tau) && prm->tau >= 0.0, "x3d_particles_mp_create: tau must be finite and not negative");
    X3D_REQUIRE(std::isfinite(prm->g[0]) && std::isfinite(prm->g[1]) && std::isfinite(prm->g[2]),
                "x3d_particles_mp_create: gravity is not finite");
    X3D_REQUIRE(dc->capacity >= 1 && dc->capacity <= X3D_PARTICLES_MAX && dc->mig_capacity >= 1 && dc->mig_capacity <= X3D_PARTICLES_MAX,
                "x3d_particles_mp_create: capacity %d, mig_capacity %d (1 to %d each)", dc->capacity, dc->mig_capacity, X3D_PARTICLES_MAX);
    X3D_REQUIRE(m >= 0 && m <= dc->capacity && m <= prm->n, "x3d_particles_mp_create: %d particles for %d slots", m, dc->capacity);
    const int dims[3] = {b->nx, b->ny, b->nz};
    X3D_REQUIRE(dc->nproc[0] == 1, "x3d_particles_mp_create: x is never cut (nproc[0] = %d)", dc->nproc[0]);
    for (int c = 0; c < 3; c++) {
        X3D_REQUIRE(dc->nproc[c] >= 1 && dc->rank[c] >= 0 && dc->rank[c] < dc->nproc[c], "x3d_particles_mp_create: rank %d of %d in direction %d",
                    dc->rank[c], dc->nproc[c], c + 1);
        X3D_REQUIRE(dc->nproc[c] == 1 || dc->nlocal[c] >= 4, "x3d_particles_mp_create: a rank needs 4 vertices in a cut direction, direction %d has %d",
                    c + 1, dc->nlocal[c]);
        X3D_REQUIRE(dc->nlocal[c] == dims[c] && dc->nglobal[c] == dims[c] * dc->nproc[c] && dc->offset[c] == dims[c] * dc->rank[c],
                    "x3d_particles_mp_create: direction %d: %d vertices at %d of %d are not this backend's part of an even cut", c + 1,
                    dc->nlocal[c], dc->offset[c], dc->nglobal[c]);
        X3D_REQUIRE(dc->nglobal[c] >= prm->order, "x3d_particles_mp_create: direction %d has %d vertices, order %d needs %d", c + 1,
                    dc->nglobal[c], prm->order, prm->order);
        const double *t = prm->coords[c];
        for (int i = 0; i < dc->nglobal[c]; i++)
            X3D_REQUIRE(std::isfinite(t[i]) && (i == 0 || t[i] > t[i - 1]), "x3d_particles_mp_create: the coordinates of direction %d do not ascend",
                        c + 1);
        if (prm->periodic[c])
            X3D_REQUIRE(std::isfinite(prm->L[c]) && t[0] >= 0.0 && t[dc->nglobal[c] - 1] < prm->L[c],
                        "x3d_particles_mp_create: the vertices of periodic direction %d do not lie in [0, L)", c + 1);
    }
    X3D_REQUIRE((double)dims[0] * dims[1] * dims[2] < 4294967294.0, "x3d_particles_mp_create: the cell index does not fit 32 bits");
    x3d_particles *p = new x3d_particles();
    PartMp *mp = p->mp = new PartMp();
    p->b = b;
    p->n = prm->n; p->order = prm->order; p->inertial = prm->tau > 0.0; p->absorb = prm->wall == X3D_PARTICLES_ABSORB;
    p->nrow = p->inertial ? P_NROW_INERTIAL : P_NROW_TRACER;
    p->have_v0 = p->inertial && v0 != nullptr;
    p->tau = prm->tau;
    for (int c = 0; c < 3; c++) p->g[c] = prm->g[c];
    p->G.nxp = b->nxp; p->G.nyp = b->nyp;
    PartDecomp &D = mp->D;
    D.gh = prm->order == 4 ? 2 : 1;
    mp->capacity = dc->capacity; mp->mig = dc->mig_capacity;
    mp->nblk = (dc->capacity + 255) / 256;
    for (int c = 0; c < 3; c++) {
        PartAxis &A = p->G.ax[c];
        const double *t = prm->coords[c];
        const int N = dc->nglobal[c];
        A.n = N; A.periodic = prm->periodic[c] != 0; A.uniform = prm->uniform[c] != 0;
        A.lo = t[0]; A.hi = t[N - 1];
        A.L = A.periodic ? prm->L[c] : A.hi - A.lo;
        A.inv_h = A.periodic ? N / prm->L[c] : (N - 1) / (A.hi - A.lo);
        mp->htab[c].assign(t, t + N);
        D.off[c] = dc->offset[c]; D.nl[c] = dims[c]; D.np[c] = dc->nproc[c]; D.rank[c] = dc->rank[c];
    }
    const long cap = mp->capacity;
    std::vector<double> rows((size_t)p->nrow * cap, 0.0), chk((size_t)6 * (m > 0 ? m : 1), 0.0);
    for (int r = 0; r < 3; r++)
        for (long t = 0; t < m; t++) {
            const PartAxis &A = p->G.ax[r];
            double x = x0[r * (long)m + t];
            if (A.periodic && std::isfinite(x)) x = part_wrap_host(x, A.L);
            chk[r * (long)m + t] = rows[r * cap + t] = x;
            if (p->have_v0) chk[(3 + r) * (long)m + t] = rows[(P_V + r) * cap + t] = v0[r * (long)m + t];
        }
    if (int rc = part_mp_check(p, "x3d_particles_mp_create", chk.data(), 6, id, nullptr, m)) {
        part_free(p);
        return rc;
    }
    std::vector<int> ints((size_t)2 * cap, 0);
    for (long t = 0; t < m; t++) { ints[t] = id[t]; ints[cap + t] = 1; }
    hipError_t e = hipSuccess;
    size_t ntab = 0;
    for (int c = 0; c < 3; c++) ntab += dc->nglobal[c];
    auto alloc = [&e](void **q, size_t bytes) { if (e == hipSuccess) e = hipMalloc(q, bytes); };
    alloc(reinterpret_cast<void **>(&p->tabs), sizeof(double) * ntab);
    for (int s = 0; s < 2; s++) {
        alloc(reinterpret_cast<void **>(&p->d[s]), sizeof(double) * p->nrow * cap);
        alloc(reinterpret_cast<void **>(&p->ints[s]), sizeof(int) * 2 * cap);
    }
    alloc(reinterpret_cast<void **>(&p->keys), sizeof(unsigned) * 2 * cap);
    alloc(reinterpret_cast<void **>(&p->perm), sizeof(int) * 2 * cap);
    alloc(reinterpret_cast<void **>(&mp->cnt), sizeof(int) * PMP_NWORDS);
    alloc(reinterpret_cast<void **>(&mp->cls), (size_t)cap);
    alloc(reinterpret_cast<void **>(&mp->blk), sizeof(int) * 6 * mp->nblk);
    alloc(reinterpret_cast<void **>(&mp->mg), sizeof(int) * 4);
    const long ng = PMP_GL + D.gh;
    const long fe[3] = {0, D.np[1] > 1 ? 3 * ng * dims[2] * dims[0] : 0, D.np[2] > 1 ? 3 * ng * (dims[1] + ng) * dims[0] : 0};
    for (int c = 1; c < 3; c++)
        if (fe[c]) {
            alloc(reinterpret_cast<void **>(&mp->frame[c]), sizeof(real_t) * fe[c]);
            if (e == hipSuccess) e = hipMemset(mp->frame[c], 0, sizeof(real_t) * fe[c]);
        }
    D.fy = mp->frame[1]; D.fz = mp->frame[2];
    D.fy_comp = ng * dims[2] * dims[0]; D.fz_comp = ng * (dims[1] + ng) * dims[0];
    p->dead_key = (unsigned)((long)dims[0] * dims[1] * dims[2]);
    p->end_bit = 1;
    while (p->end_bit < 32 && ((p->dead_key + 1u) >> p->end_bit) != 0) p->end_bit++;
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(nullptr, p->tmp_bytes, p->keys, p->keys + cap, p->perm, p->perm + cap, (unsigned)cap, 0u, p->end_bit,
                                      b->stream);
    if (p->tmp_bytes == 0) p->tmp_bytes = 16;
    alloc(&p->tmp, p->tmp_bytes);
    if (e == hipSuccess) {
        size_t off = 0;
        for (int c = 0; c < 3 && e == hipSuccess; c++) {
            e = hipMemcpy(p->tabs + off, prm->coords[c], sizeof(double) * dc->nglobal[c], hipMemcpyHostToDevice);
            p->G.ax[c].c = p->tabs + off;
            off += dc->nglobal[c];
        }
    }
    const int words[PMP_NWORDS] = {m, m, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(mp->cnt, words, sizeof(words), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d[0], rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(p->d[1], 0, sizeof(double) * rows.size());
    if (e == hipSuccess) e = hipMemcpy(p->ints[0], ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(p->ints[1], 0, sizeof(int) * ints.size());
    if (e != hipSuccess) {
        part_free(p);
        x3d_set_error("x3d_particles_mp_create: %s", hipGetErrorString(e));
        return 1;
    }
    *out = p;
    return 0;
}

#define PMP_ARGS(name)                                                                                                           \
    X3D_REQUIRE(b && p, name ": null argument");                                                                                 \
    X3D_REQUIRE(p->b == b, name ": the particles belong to another backend");                                                    \
    X3D_REQUIRE(p->mp, name ": these particles live on one rank (x3d_particles_*)")

#define PMP_FIELD_ARGS(name)                                                                                                     \
    PMP_ARGS(name);                                                                                                              \
    X3D_REQUIRE(u && v && w && dims, name ": null argument");                                                                    \
    X3D_REQUIRE(dims[0] == b->nx && dims[1] == b->ny && dims[2] == b->nz,                                                        \
                name ": dims (%d,%d,%d) are not the vertices the particles were created for", dims[0], dims[1], dims[2])

#define PMP_DIR(name)                                                                                                            \
    X3D_REQUIRE((dir == 2 || dir == 3) && p->mp->D.np[dir - 1] > 1, name ": direction %d is not a cut y (2) or z (3)", dir)

extern "C" int x3d_particles_mp_ghost_pack(x3d_backend *b, x3d_particles *p, int dir, const real_t *u, const real_t *v, const real_t *w,
                                           const int dims[3], real_t *send_prev, real_t *send_next)
{
    X3D_RANGE(__func__);
    PMP_FIELD_ARGS("x3d_particles_mp_ghost_pack");
    PMP_DIR("x3d_particles_mp_ghost_pack");
    X3D_REQUIRE(send_prev && send_next, "x3d_particles_mp_ghost_pack: null argument");
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    const PartDecomp &D = p->mp->D;
    const long ng = PMP_GL + D.gh, nr = dir == 2 ? D.nl[2] : D.nl[1] + ng, total = 3 * ng * nr * D.nl[0];
    ProfScope ps(b, X3D_K_PACK);
    hipLaunchKernelGGL(k_pmp_ghost_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, b->stream, p->G, D, dir - 1, u, v, w,
                       send_prev, send_next);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_mp_ghost_unpack(x3d_backend *b, x3d_particles *p, int dir, const real_t *recv_prev, const real_t *recv_next)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_ghost_unpack");
    PMP_DIR("x3d_particles_mp_ghost_unpack");
    X3D_REQUIRE(recv_prev && recv_next, "x3d_particles_mp_ghost_unpack: null argument");
    const PartDecomp &D = p->mp->D;
    const long ng = PMP_GL + D.gh, nr = dir == 2 ? D.nl[2] : D.nl[1] + ng, total = 3 * ng * nr * D.nl[0];
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_pmp_ghost_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, b->stream, p->mp->frame[dir - 1],
                       recv_prev, recv_next, D.gh, (int)nr, D.nl[0]);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_mp_prime(x3d_backend *b, x3d_particles *p, const real_t *u, const real_t *v, const real_t *w,
                                      const int dims[3])
{
    X3D_RANGE(__func__);
    PMP_FIELD_ARGS("x3d_particles_mp_prime");
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    const int cap = p->mp->capacity;
    ProfScope ps(b, X3D_K_COPY);
    PART_LAUNCH(k_pmp_prime, cap, p->G, p->mp->D, u, v, w, p->d[p->cur], (const int *)(p->ints[p->cur] + cap), (const int *)p->mp->cnt, cap,
                p->have_v0, p->tau, p->g[0], p->g[1], p->g[2]);
    X3D_HIP(hipGetLastError());
    p->primed = 1;
    p->has_hist = 0;
    return 0;
}

extern "C" int x3d_particles_mp_move(x3d_backend *b, x3d_particles *p, double dt)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_move");
    X3D_REQUIRE(p->primed, "x3d_particles_mp_move: the state was neither primed nor loaded");
    X3D_REQUIRE(std::isfinite(dt) && dt > 0.0, "x3d_particles_mp_move: dt must be finite and positive");
    X3D_REQUIRE(!p->inertial || p->tau >= 2.0 * dt, "x3d_particles_mp_move: tau < 2 dt");
    const double c1 = p->has_hist ? 1.5 : 1.0, c0 = p->has_hist ? -0.5 : 0.0;
    const int cap = p->mp->capacity;
    const dim3 grid((unsigned)((cap + 255) / 256));
    ProfScope ps(b, X3D_K_COPY);
    if (p->inertial) hipLaunchKernelGGL(k_pmp_move<true>, grid, dim3(256), 0, b->stream, p->G, p->d[p->cur], p->ints[p->cur] + cap,
                                        (const int *)p->mp->cnt, cap, dt, c1, c0, p->absorb);
    else hipLaunchKernelGGL(k_pmp_move<false>, grid, dim3(256), 0, b->stream, p->G, p->d[p->cur], p->ints[p->cur] + cap,
                            (const int *)p->mp->cnt, cap, dt, c1, c0, p->absorb);
    X3D_HIP(hipGetLastError());
    p->has_hist = 1;
    return 0;
}

extern "C" int x3d_particles_mp_sample(x3d_backend *b, x3d_particles *p, const real_t *u, const real_t *v, const real_t *w,
                                       const int dims[3])
{
    X3D_RANGE(__func__);
    PMP_FIELD_ARGS("x3d_particles_mp_sample");
    X3D_REQUIRE(p->primed, "x3d_particles_mp_sample: the state was neither primed nor loaded");
    X3D_LAZY_IN(b, u);
    X3D_LAZY_IN(b, v);
    X3D_LAZY_IN(b, w);
    X3D_LAZY_EAGER(b);
    const int cap = p->mp->capacity;
    ProfScope ps(b, X3D_K_COPY);
    PART_LAUNCH(k_pmp_sample, cap, p->G, p->mp->D, u, v, w, p->d[p->cur], (const int *)(p->ints[p->cur] + cap), (const int *)p->mp->cnt, cap,
                p->tau, p->g[0], p->g[1], p->g[2]);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_mp_emigrate(x3d_backend *b, x3d_particles *p, int dir, double *send_prev, double *send_next)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_emigrate");
    PMP_DIR("x3d_particles_mp_emigrate");
    X3D_REQUIRE(send_prev && send_next && send_prev != send_next, "x3d_particles_mp_emigrate: two message buffers are needed");
    PartMp *m = p->mp;
    const int cap = m->capacity, cur = p->cur, c = dir - 1;
    const dim3 grid((unsigned)m->nblk);
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_pmp_classify, grid, dim3(256), 0, b->stream, p->G.ax[c], m->D, c, (const double *)p->d[cur],
                       (const int *)(p->ints[cur] + cap), m->cnt, cap, m->cls, m->blk, m->nblk);
    hipLaunchKernelGGL(k_pmp_scan, dim3(1), dim3(1024), 0, b->stream, m->blk, m->nblk, m->mig, m->cnt, m->mg);
    hipLaunchKernelGGL(k_pmp_scatter, grid, dim3(256), 0, b->stream, (const double *)p->d[cur], (const int *)p->ints[cur], p->d[1 - cur],
                       p->ints[1 - cur], cap, p->nrow, (const int *)m->cnt, (const unsigned char *)m->cls, (const int *)(m->blk + 3 * m->nblk),
                       m->nblk, (const int *)m->mg, send_prev, send_next, m->mig);
    X3D_HIP(hipGetLastError());
    p->cur = 1 - cur;
    return 0;
}

extern "C" int x3d_particles_mp_immigrate(x3d_backend *b, x3d_particles *p, int dir, const double *recv_prev, const double *recv_next)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_immigrate");
    PMP_DIR("x3d_particles_mp_immigrate");
    X3D_REQUIRE(recv_prev && recv_next, "x3d_particles_mp_immigrate: null argument");
    PartMp *m = p->mp;
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_pmp_append, dim3((unsigned)((2 * m->mig + 255) / 256)), dim3(256), 0, b->stream, p->d[p->cur], p->ints[p->cur],
                       m->capacity, p->nrow, m->cnt, recv_prev, recv_next, m->mig);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_mp_sort(x3d_backend *b, x3d_particles *p)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_sort");
    const int cap = p->mp->capacity, cur = p->cur;
    const dim3 grid((unsigned)((cap + 255) / 256));
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_pmp_keys, grid, dim3(256), 0, b->stream, p->G, p->mp->D, (const double *)p->d[cur], (const int *)(p->ints[cur] + cap),
                       (const int *)p->mp->cnt, cap, p->dead_key, p->keys, p->perm);
    X3D_HIP(hipGetLastError());
    size_t bytes = p->tmp_bytes;
    X3D_HIP(rocprim::radix_sort_pairs(p->tmp, bytes, p->keys, p->keys + cap, p->perm, p->perm + cap, (unsigned)cap, 0u, p->end_bit,
                                      b->stream));
    hipLaunchKernelGGL(k_particles_gather, grid, dim3(256), 0, b->stream, (const double *)p->d[cur], (const int *)p->ints[cur],
                       (const int *)(p->perm + cap), cap, p->nrow, p->d[1 - cur], p->ints[1 - cur]);
    X3D_HIP(hipGetLastError());
    p->cur = 1 - cur;
    return 0;
}

extern "C" int x3d_particles_mp_query(x3d_backend *b, const x3d_particles *p, int out[2])
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_query");
    X3D_REQUIRE(out, "x3d_particles_mp_query: null argument");
    X3D_HIP(hipStreamSynchronize(b->stream));
    b->n_sync++;
    int words[PMP_NWORDS];
    X3D_HIP(hipMemcpy(words, p->mp->cnt, sizeof(words), hipMemcpyDeviceToHost));
    out[0] = std::min(std::max(words[PMP_N], 0), p->mp->capacity);
    out[1] = words[PMP_FLAGS];
    return 0;
}

extern "C" int x3d_particles_mp_pack(x3d_backend *b, const x3d_particles *p, void *dst_dev, long capacity)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_pack");
    X3D_REQUIRE(dst_dev, "x3d_particles_mp_pack: null argument");
    const long cap = p->mp->capacity;
    X3D_REQUIRE(capacity >= 80L * cap + 8, "x3d_particles_mp_pack: the buffer holds %ld bytes, %ld are needed", capacity, 80L * cap + 8);
    X3D_REQUIRE(((size_t)dst_dev & 7) == 0, "x3d_particles_mp_pack: the buffer is not aligned to 8 bytes");
    if (int rc = x3d_snapshot_wait_for_copy_c(b, dst_dev)) return rc;
    ProfScope ps(b, X3D_K_PACK);
    hipLaunchKernelGGL(k_pmp_pack, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, b->stream, (const double *)p->d[p->cur],
                       (const int *)p->ints[p->cur], (const int *)p->mp->cnt, (int)cap, reinterpret_cast<double *>(dst_dev));
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_mp_download(x3d_backend *b, const x3d_particles *p, double *rows, int *id, int *status, int *n_local,
                                         int *flags, int *has_hist)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_download");
    X3D_REQUIRE(rows && id && status && n_local && flags && has_hist, "x3d_particles_mp_download: null argument");
    int q[2];
    if (int rc = x3d_particles_mp_query(b, p, q)) return rc;
    const long cap = p->mp->capacity, n = q[0];
    for (int r = 0; r < p->nrow && n > 0; r++)
        X3D_HIP(hipMemcpy(rows + r * n, p->d[p->cur] + r * cap, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (n > 0) {
        X3D_HIP(hipMemcpy(id, p->ints[p->cur], sizeof(int) * n, hipMemcpyDeviceToHost));
        X3D_HIP(hipMemcpy(status, p->ints[p->cur] + cap, sizeof(int) * n, hipMemcpyDeviceToHost));
    }
    *n_local = (int)n;
    *flags = q[1];
    *has_hist = p->has_hist;
    return 0;
}

extern "C" int x3d_particles_mp_upload(x3d_backend *b, x3d_particles *p, const double *rows, const int *id, const int *status, int m,
                                       int has_hist)
{
    X3D_RANGE(__func__);
    PMP_ARGS("x3d_particles_mp_upload");
    const long cap = p->mp->capacity;
    X3D_REQUIRE(m >= 0 && m <= cap, "x3d_particles_mp_upload: %d particles for %ld slots", m, cap);
    X3D_REQUIRE(m == 0 || (rows && id && status), "x3d_particles_mp_upload: null argument");
    if (int rc = part_mp_check(p, "x3d_particles_mp_upload", rows, p->nrow, id, status, m)) return rc;
    X3D_HIP(hipStreamSynchronize(b->stream));
    b->n_sync++;
    for (int r = 0; r < p->nrow && m > 0; r++)
        X3D_HIP(hipMemcpy(p->d[p->cur] + r * cap, rows + r * (long)m, sizeof(double) * m, hipMemcpyHostToDevice));
    if (m > 0) {
        X3D_HIP(hipMemcpy(p->ints[p->cur], id, sizeof(int) * m, hipMemcpyHostToDevice));
        X3D_HIP(hipMemcpy(p->ints[p->cur] + cap, status, sizeof(int) * m, hipMemcpyHostToDevice));
    }
    const int words[PMP_NWORDS] = {m, m, 0, 0};
    X3D_HIP(hipMemcpy(p->mp->cnt, words, sizeof(words), hipMemcpyHostToDevice));
    p->primed = 1;
    p->has_hist = has_hist != 0;
    return 0;
}

// ================================================================ two-way coupling
// The drag reaction of the inertial particles on the fluid, without atomics of any kind and with one fixed order of every sum.
//   build  keys (cell 2^24 + id, 64 bits) -> radix sort of (key, slot) -> the first particle of every occupied cell marked with
//          the cell's colour (i mod 2) + 2 (j mod 2) + 4 (k mod 2), every other position with 8 -> radix sort of (mark, position)
//          on 4 bits: stable, so the occupied cells come out by colour and, within a colour, by cell -> the nine colour offsets
//          -> one record of FB_NREC doubles per occupied cell, lane (corner, component) walking the cell's particles in key
//          order, that is in ascending id.  The state is not reordered.
//   add    colour after colour: within a colour no two cells share a vertex (even vertex counts in the periodic directions; a
//          non-periodic direction's last cell is n - 2), so every lane does a plain read-modify-write of its vertex.
// The number of occupied cells lives on the device; the launches are sized by n and loop over what the offsets say.
#define FB_NREC 24    // 8 corners x 3 components; lane = 3 corner + component, corner = alpha + 2 beta + 4 gamma
#define FB_KEY_ID 24  // bits of the id in a key
#define FB_BLOCKS (X3D_NCU * 8)

struct PartFb {
    double mass;
    double *inv;                // the three tables of 1 / d, one allocation
    const double *inv_d[3];
    unsigned long long *keys;   // [2][n]: keys in, sorted out
    int *slots;                 // [2][n]: 0..n-1 in, the slots in key order out
    unsigned *marks;            // [2][n]: colour marks in, sorted out
    int *pos;                   // [2][n]: 0..n-1 in, the positions of the cells' first particles, by colour, out
    unsigned *cells;            // [n]: the cell of each record
    int *coff;                  // [9]: the first record of each colour; [8]: the occupied cells
    double *rec;                // [n][FB_NREC]
    void *tmp;
    size_t tmp_bytes;
    unsigned end_bit;
    unsigned long long dead_cell;  // nx ny nz: the cell of a particle that is not alive
    int built;
};

static void part_fb_free(x3d_particles *p)
{
    PartFb *f = p->fb;
    if (!f) return;
    void *all[] = {f->inv, f->keys, f->slots, f->marks, f->pos, f->cells, f->coff, f->rec, f->tmp};
    for (void *q : all)
        if (q) hipFree(q);
    delete f;
    p->fb = nullptr;
}

struct FbGrid {
    int nx, ny, nz;
    long nxp, nyp;
    unsigned long long ncell;
};

__global__ void __launch_bounds__(256) k_fb_keys(PartGeom G, const double *__restrict__ d, const int *__restrict__ ints, int n,
                                                 unsigned long long dead_cell, unsigned long long *__restrict__ keys,
                                                 int *__restrict__ slots)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const long N = n;
    unsigned long long cell = dead_cell;
    if (ints[N + t] == 1) {  // (an alive particle's position is finite and inside: k_particles_advance)
        const unsigned long long i = (unsigned)part_cell(G.ax[0], d[(P_X + 0) * N + t]);
        const unsigned long long j = (unsigned)part_cell(G.ax[1], d[(P_X + 1) * N + t]);
        const unsigned long long k = (unsigned)part_cell(G.ax[2], d[(P_X + 2) * N + t]);
        cell = (k * (unsigned)G.ax[1].n + j) * (unsigned)G.ax[0].n + i;
    }
    keys[t] = (cell << FB_KEY_ID) | ((unsigned)ints[t] & ((1u << FB_KEY_ID) - 1u));
    slots[t] = t;
}

__global__ void __launch_bounds__(256) k_fb_marks(FbGrid g, const unsigned long long *__restrict__ keys, int n,
                                                  unsigned *__restrict__ marks, int *__restrict__ pos)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const unsigned long long cell = keys[t] >> FB_KEY_ID;
    unsigned mark = 8u;
    if (cell < g.ncell && (t == 0 || (keys[t - 1] >> FB_KEY_ID) != cell)) {
        const unsigned i = (unsigned)(cell % (unsigned)g.nx), j = (unsigned)((cell / (unsigned)g.nx) % (unsigned)g.ny);
        const unsigned k = (unsigned)(cell / ((unsigned long long)g.nx * (unsigned)g.ny));
        mark = (i & 1u) + 2u * (j & 1u) + 4u * (k & 1u);
    }
    marks[t] = mark;
    pos[t] = t;
}

// coff[c] = the number of sorted marks below c, c = 0 .. 8
__global__ void __launch_bounds__(64) k_fb_offsets(const unsigned *__restrict__ marks, int n, int *__restrict__ coff)
{
    const unsigned c = threadIdx.x;
    if (c > 8u) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (marks[mid] < c) lo = mid + 1; else hi = mid;
    }
    coff[c] = lo;
}

// w_1 of cell i of one direction
__device__ __forceinline__ double fb_w1(const PartAxis &A, int i, double x)
{
    const double lo = A.c[i], hi = i + 1 < A.n ? A.c[i + 1] : A.L;  // (i + 1 == n only in a periodic direction: the image of c[0])
    return (x - lo) / (hi - lo);
}

__global__ void __launch_bounds__(256) k_fb_records(PartGeom G, FbGrid g, const double *__restrict__ d,
                                                    const unsigned long long *__restrict__ keys, const int *__restrict__ slots,
                                                    const int *__restrict__ pos, const int *__restrict__ coff, int n, double mass,
                                                    double tau, unsigned *__restrict__ cells, double *__restrict__ rec)
{
    const long N = n;
    const long total = (long)min(max(coff[8], 0), n) * FB_NREC;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long q = e / FB_NREC;
        const int lane = (int)(e - q * FB_NREC), corner = lane / 3, comp = lane - 3 * corner;
        int t = pos[q];
        double sum = 0.0;
        unsigned long long cell = g.ncell;
        if (t >= 0 && t < n) cell = keys[t] >> FB_KEY_ID;
        if (cell < g.ncell) {
            const int i = (int)(cell % (unsigned)g.nx), j = (int)((cell / (unsigned)g.nx) % (unsigned)g.ny);
            const int k = (int)(cell / ((unsigned long long)g.nx * (unsigned)g.ny));
            for (; t < n && (keys[t] >> FB_KEY_ID) == cell; t++) {
                const int s = slots[t];
                if (s < 0 || s >= n) continue;  // (a permutation of 0..n-1; never an address from anything else)
                const double w1x = fb_w1(G.ax[0], i, d[(P_X + 0) * N + s]);
                const double w1y = fb_w1(G.ax[1], j, d[(P_X + 1) * N + s]);
                const double w1z = fb_w1(G.ax[2], k, d[(P_X + 2) * N + s]);
                const double wx = (corner & 1) ? w1x : 1.0 - w1x, wy = (corner & 2) ? w1y : 1.0 - w1y;
                const double wz = (corner & 4) ? w1z : 1.0 - w1z;
                const double D = mass * (d[(P_A + comp) * N + s] - d[(P_V + comp) * N + s]) / tau;
                sum += ((wx * wy) * wz) * D;
            }
        }
        rec[e] = sum;
        if (lane == 0) cells[q] = (unsigned)cell;
    }
}

__global__ void __launch_bounds__(256) k_fb_apply(FbGrid g, int px, int py, int pz, int colour, const int *__restrict__ coff,
                                                  const unsigned *__restrict__ cells, const double *__restrict__ rec,
                                                  const double *__restrict__ invx, const double *__restrict__ invy,
                                                  const double *__restrict__ invz, int ncap, real_t *du, real_t *dv, real_t *dw)
{
    const long lo = (long)min(max(coff[colour], 0), ncap) * FB_NREC, hi = (long)min(max(coff[colour + 1], 0), ncap) * FB_NREC;
    for (long e = lo + (long)blockIdx.x * 256 + threadIdx.x; e < hi; e += (long)gridDim.x * 256) {
        const long q = e / FB_NREC;
        const int lane = (int)(e - q * FB_NREC), corner = lane / 3, comp = lane - 3 * corner;
        const unsigned long long cell = cells[q];
        if (cell >= g.ncell) continue;
        int i = (int)(cell % (unsigned)g.nx) + (corner & 1), j = (int)((cell / (unsigned)g.nx) % (unsigned)g.ny) + ((corner >> 1) & 1);
        int k = (int)(cell / ((unsigned long long)g.nx * (unsigned)g.ny)) + ((corner >> 2) & 1);
        // node n of a periodic direction is node 0; a non-periodic direction's last cell is n - 2, so nothing else gets here
        if (i >= g.nx) { if (!px) continue; i = 0; }
        if (j >= g.ny) { if (!py) continue; j = 0; }
        if (k >= g.nz) { if (!pz) continue; k = 0; }
        const double val = -rec[e] * ((invx[i] * invy[j]) * invz[k]);
        real_t *blk = comp == 0 ? du : (comp == 1 ? dv : dw);
        const long off = i + g.nxp * ((long)j + g.nyp * (long)k);
        blk[off] = (real_t)((double)blk[off] + val);
    }
}

static FbGrid fb_grid(const x3d_particles *p)
{
    FbGrid g;
    g.nx = p->G.ax[0].n; g.ny = p->G.ax[1].n; g.nz = p->G.ax[2].n;
    g.nxp = p->G.nxp; g.nyp = p->G.nyp;
    g.ncell = p->fb->dead_cell;
    return g;
}

static unsigned fb_blocks(long lanes)
{
    const long want = (lanes + 255) / 256;
    return (unsigned)(want > FB_BLOCKS ? FB_BLOCKS : (want < 1 ? 1 : want));
}

#define FB_ARGS(name)                                                                                                            \
    X3D_REQUIRE(b && p, name ": null argument");                                                                                 \
    X3D_REQUIRE(p->b == b, name ": the particles belong to another backend");                                                    \
    X3D_REQUIRE(!p->mp, name ": two-way coupling is not built on several ranks")

extern "C" int x3d_particles_feedback_enable(x3d_backend *b, x3d_particles *p, double mass, const double *inv_dx, const double *inv_dy,
                                             const double *inv_dz)
{
    X3D_RANGE(__func__);
    FB_ARGS("x3d_particles_feedback_enable");
    X3D_REQUIRE(inv_dx && inv_dy && inv_dz, "x3d_particles_feedback_enable: null argument");
    X3D_REQUIRE(!p->fb, "x3d_particles_feedback_enable: already enabled");
    X3D_REQUIRE(p->inertial, "x3d_particles_feedback_enable: tracers (tau = 0) exert no drag");
    X3D_REQUIRE(std::isfinite(mass) && mass > 0.0, "x3d_particles_feedback_enable: the mass must be positive and finite");
    const double *tab[3] = {inv_dx, inv_dy, inv_dz};
    size_t ntab = 0;
    for (int c = 0; c < 3; c++) {
        const PartAxis &A = p->G.ax[c];
        X3D_REQUIRE(!A.periodic || A.n % 2 == 0,
                    "x3d_particles_feedback_enable: periodic direction %d has %d vertices, the cell colouring needs an even count", c + 1, A.n);
        for (int i = 0; i < A.n; i++)
            X3D_REQUIRE(std::isfinite(tab[c][i]) && tab[c][i] > 0.0, "x3d_particles_feedback_enable: 1 / d of direction %d is not positive and finite",
                        c + 1);
        ntab += (size_t)A.n;
    }
    // ---- nothing was allocated up to here
    PartFb *f = new PartFb();
    p->fb = f;
    f->mass = mass;
    f->dead_cell = (unsigned long long)p->G.ax[0].n * (unsigned long long)p->G.ax[1].n * (unsigned long long)p->G.ax[2].n;
    f->end_bit = FB_KEY_ID + 1;
    while (f->end_bit < 64 && (f->dead_cell >> (f->end_bit - FB_KEY_ID)) != 0) f->end_bit++;
    const size_t n = (size_t)p->n;
    hipError_t e = hipSuccess;
    auto alloc = [&e](void **q, size_t bytes) { if (e == hipSuccess) e = hipMalloc(q, bytes); };
    alloc(reinterpret_cast<void **>(&f->inv), sizeof(double) * ntab);
    alloc(reinterpret_cast<void **>(&f->keys), sizeof(unsigned long long) * 2 * n);
    alloc(reinterpret_cast<void **>(&f->slots), sizeof(int) * 2 * n);
    alloc(reinterpret_cast<void **>(&f->marks), sizeof(unsigned) * 2 * n);
    alloc(reinterpret_cast<void **>(&f->pos), sizeof(int) * 2 * n);
    alloc(reinterpret_cast<void **>(&f->cells), sizeof(unsigned) * n);
    alloc(reinterpret_cast<void **>(&f->coff), sizeof(int) * 9);
    alloc(reinterpret_cast<void **>(&f->rec), sizeof(double) * FB_NREC * n);
    size_t b1 = 0, b2 = 0;
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(nullptr, b1, f->keys, f->keys + n, f->slots, f->slots + n, (unsigned)n, 0u, f->end_bit, b->stream);
    if (e == hipSuccess)
        e = rocprim::radix_sort_pairs(nullptr, b2, f->marks, f->marks + n, f->pos, f->pos + n, (unsigned)n, 0u, 4u, b->stream);
    f->tmp_bytes = std::max<size_t>(std::max(b1, b2), 16);
    alloc(&f->tmp, f->tmp_bytes);
    size_t off = 0;
    for (int c = 0; c < 3 && e == hipSuccess; c++) {  // (the caller's tables may die with this call: synchronous copies)
        e = hipMemcpy(f->inv + off, tab[c], sizeof(double) * p->G.ax[c].n, hipMemcpyHostToDevice);
        f->inv_d[c] = f->inv + off;
        off += (size_t)p->G.ax[c].n;
    }
    if (e == hipSuccess) e = hipMemset(f->coff, 0, sizeof(int) * 9);
    if (e != hipSuccess) {
        part_fb_free(p);
        x3d_set_error("x3d_particles_feedback_enable: %s", hipGetErrorString(e));
        return 1;
    }
    return 0;
}

extern "C" int x3d_particles_feedback_build(x3d_backend *b, x3d_particles *p)
{
    X3D_RANGE(__func__);
    FB_ARGS("x3d_particles_feedback_build");
    X3D_REQUIRE(p->fb, "x3d_particles_feedback_build: two-way coupling was not enabled");
    X3D_REQUIRE(p->primed, "x3d_particles_feedback_build: the state was neither primed nor loaded");
    PartFb *f = p->fb;
    const int n = p->n, cur = p->cur;
    const dim3 grid((unsigned)((n + 255) / 256));
    const FbGrid g = fb_grid(p);
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_fb_keys, grid, dim3(256), 0, b->stream, p->G, (const double *)p->d[cur], (const int *)p->ints[cur], n, f->dead_cell,
                       f->keys, f->slots);
    X3D_HIP(hipGetLastError());
    size_t bytes = f->tmp_bytes;
    X3D_HIP(rocprim::radix_sort_pairs(f->tmp, bytes, f->keys, f->keys + n, f->slots, f->slots + n, (unsigned)n, 0u, f->end_bit, b->stream));
    hipLaunchKernelGGL(k_fb_marks, grid, dim3(256), 0, b->stream, g, (const unsigned long long *)(f->keys + n), n, f->marks, f->pos);
    X3D_HIP(hipGetLastError());
    bytes = f->tmp_bytes;
    X3D_HIP(rocprim::radix_sort_pairs(f->tmp, bytes, f->marks, f->marks + n, f->pos, f->pos + n, (unsigned)n, 0u, 4u, b->stream));
    hipLaunchKernelGGL(k_fb_offsets, dim3(1), dim3(64), 0, b->stream, (const unsigned *)(f->marks + n), n, f->coff);
    hipLaunchKernelGGL(k_fb_records, dim3(fb_blocks((long)n * FB_NREC)), dim3(256), 0, b->stream, p->G, g, (const double *)p->d[cur],
                       (const unsigned long long *)(f->keys + n), (const int *)(f->slots + n), (const int *)(f->pos + n),
                       (const int *)f->coff, n, f->mass, p->tau, f->cells, f->rec);
    X3D_HIP(hipGetLastError());
    f->built = 1;
    return 0;
}

extern "C" int x3d_particles_feedback_add(x3d_backend *b, x3d_particles *p, real_t *du, real_t *dv, real_t *dw, const int dims[3])
{
    X3D_RANGE(__func__);
    FB_ARGS("x3d_particles_feedback_add");
    X3D_REQUIRE(du && dv && dw && dims, "x3d_particles_feedback_add: null argument");
    X3D_REQUIRE(du != dv && du != dw && dv != dw, "x3d_particles_feedback_add: two derivative blocks are the same block");
    X3D_REQUIRE(p->fb && p->fb->built, "x3d_particles_feedback_add: the records were not built");
    X3D_REQUIRE(dims[0] == p->G.ax[0].n && dims[1] == p->G.ax[1].n && dims[2] == p->G.ax[2].n && dims[0] <= b->nxp && dims[1] <= b->nyp &&
                    dims[2] <= b->nzp,
                "x3d_particles_feedback_add: dims (%d,%d,%d) are not the vertices the particles were created for", dims[0], dims[1], dims[2]);
    X3D_LAZY_OUT(b, du, false);
    X3D_LAZY_OUT(b, dv, false);
    X3D_LAZY_OUT(b, dw, false);
    X3D_LAZY_EAGER(b);
    const PartFb *f = p->fb;
    const FbGrid g = fb_grid(p);
    // (the lists of the eight colours share the occupied cells: an eighth of the lanes each, on average)
    const unsigned blocks = fb_blocks(((long)p->n * FB_NREC + 7) / 8);
    ProfScope ps(b, X3D_K_BLAS1);
    for (int colour = 0; colour < 8; colour++)
        hipLaunchKernelGGL(k_fb_apply, dim3(blocks), dim3(256), 0, b->stream, g, p->G.ax[0].periodic, p->G.ax[1].periodic, p->G.ax[2].periodic,
                           colour, (const int *)f->coff, (const unsigned *)f->cells, (const double *)f->rec, f->inv_d[0], f->inv_d[1],
                           f->inv_d[2], p->n, du, dv, dw);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_particles_feedback_download(x3d_backend *b, const x3d_particles *p, int counts[9], unsigned *cells, double *records)
{
    X3D_RANGE(__func__);
    FB_ARGS("x3d_particles_feedback_download");
    X3D_REQUIRE(counts, "x3d_particles_feedback_download: null argument");
    X3D_REQUIRE(p->fb && p->fb->built, "x3d_particles_feedback_download: the records were not built");
    X3D_HIP(hipStreamSynchronize(b->stream));
    b->n_sync++;
    X3D_HIP(hipMemcpy(counts, p->fb->coff, sizeof(int) * 9, hipMemcpyDeviceToHost));
    const size_t nc = (size_t)std::min(std::max(counts[8], 0), p->n);
    if (cells && nc) X3D_HIP(hipMemcpy(cells, p->fb->cells, sizeof(unsigned) * nc, hipMemcpyDeviceToHost));
    if (records && nc) X3D_HIP(hipMemcpy(records, p->fb->rec, sizeof(double) * FB_NREC * nc, hipMemcpyDeviceToHost));
    return 0;
}
