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
static void part_free(x3d_particles *p)
{
    if (!p) return;
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
