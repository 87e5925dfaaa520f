// Immersed boundary and the cylinder case's per-sub-step boundary work, without the host.
//
// The reference's ibm_t%body (src/module/ibm.f90:148-170) multiplies u, v and w by a full-field mask that is 1.0 almost
// everywhere: three vecmult passes, 72 B/DoF, to zero the velocity at the few points inside the body.  x * 1.0 is x in
// IEEE arithmetic, so a kernel that visits only the 64-point x segments in which the mask differs from 1 gives the same
// bits.  x3d_ibm_create builds that work list on the host, once; the device keeps the list and the mask values of the
// listed segments, no full-size mask block.
//
// define_BC_cylinder / apply_BC_cylinder (src/case/cylinder.f90:109-243) take three slice reductions through the host,
// upload three blocks and stamp the faces with three launches whose scalars came from the host.  Here the two scalars
// stay in a device buffer (x3d_outflow_params) that the one stamping launch reads (x3d_cylinder_apply_bc), and the inlet
// plane is generated in place (x3d_inlet_noise).
#include "common.h"

#include <algorithm>

// ---------------------------------------------------------------- the work list
struct x3d_ibm {
    x3d_backend *b;
    int nx, ny, nz;
    long nseg, nmasked;
    int4 *seg;     // device [nseg]: (i0, j, k, valid points) of a segment, 0-based, i0 a multiple of 64; ascending in (k, j, i0)
    real_t *mask;  // device [nseg][64]: the mask values of the listed segments (1.0 beyond the row's end)
    double *part;  // device [(nseg + 3) / 4][3]: the workgroups' partial impulses of x3d_ibm_body_loads
    double *wgt;   // device [nx + ny + nz]: the quadrature weights w_x, w_y, w_z (x3d_ibm_set_weights), null until set
};

extern "C" int x3d_ibm_create(x3d_backend *b, const real_t *ep1_host, const int dims[3], x3d_ibm **out)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && ep1_host && dims && out, "x3d_ibm_create: null argument");
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_ibm_create: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    const int nx = dims[0], ny = dims[1], nz = dims[2];
    std::vector<int4> seg;
    std::vector<real_t> mask;
    long nmasked = 0;
    for (int k = 0; k < nz; k++)
        for (int j = 0; j < ny; j++) {
            const real_t *row = ep1_host + (size_t)nx * (j + (size_t)ny * k);
            for (int i0 = 0; i0 < nx; i0 += 64) {
                const int nv = std::min(64, nx - i0);
                int hit = 0;
                for (int l = 0; l < nv; l++) hit += row[i0 + l] != (real_t)1;
                if (!hit) continue;
                nmasked += hit;
                seg.push_back(make_int4(i0, j, k, nv));
                for (int l = 0; l < 64; l++) mask.push_back(l < nv ? row[i0 + l] : (real_t)1);
            }
        }
    x3d_ibm *m = new x3d_ibm();
    m->b = b;
    m->nx = nx; m->ny = ny; m->nz = nz;
    m->nseg = (long)seg.size();
    m->nmasked = nmasked;
    m->seg = nullptr;
    m->mask = nullptr;
    m->part = nullptr;
    m->wgt = nullptr;
    if (m->nseg > 0) {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&m->seg), sizeof(int4) * seg.size());
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->mask), sizeof(real_t) * mask.size());
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&m->part), sizeof(double) * 3 * ((seg.size() + 3) / 4));
        // (the host vectors die with this call: synchronous copies)
        if (e == hipSuccess) e = hipMemcpy(m->seg, seg.data(), sizeof(int4) * seg.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(m->mask, mask.data(), sizeof(real_t) * mask.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            if (m->seg) hipFree(m->seg);
            if (m->mask) hipFree(m->mask);
            if (m->part) hipFree(m->part);
            delete m;
            x3d_set_error("x3d_ibm_create: %s", hipGetErrorString(e));
            return 1;
        }
    }
    *out = m;
    return 0;
}

extern "C" int x3d_ibm_destroy(x3d_ibm *m)
{
    X3D_RANGE(__func__);
    if (!m) return 0;
    if (m->seg) hipFree(m->seg);
    if (m->mask) hipFree(m->mask);
    if (m->part) hipFree(m->part);
    if (m->wgt) hipFree(m->wgt);
    delete m;
    return 0;
}

extern "C" int x3d_ibm_counts(const x3d_ibm *m, long out[2])
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(m && out, "x3d_ibm_counts: null argument");
    out[0] = m->nseg;
    out[1] = m->nmasked;
    return 0;
}

// One wave per listed segment, one lane per point: a segment is 512 contiguous bytes of each of u, v, w (FP64) and of the
// packed mask.  The mask is read once and never again in this launch: non-temporal.  u, v, w go through the cache like
// any read-modify-write of a line the next kernel (the divergence's x operators) reads again.
__global__ void __launch_bounds__(256) k_ibm_body(real_t *__restrict__ u, real_t *__restrict__ v, real_t *__restrict__ w,
                                                  const int4 *__restrict__ seg, const real_t *__restrict__ mask, long nseg,
                                                  long nxp, long nyp)
{
    const long s = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + 4L * blockIdx.x;
    if (s >= nseg) return;
    const int ln = threadIdx.x & 63;
    const int4 e = seg[s];
    if (ln >= e.w) return;  // beyond the row's end: padding, or the next row -- never written
    const real_t m = __builtin_nontemporal_load(mask + s * 64 + ln);
    const long off = nxp * (e.y + nyp * (long)e.z) + e.x + ln;
    u[off] *= m;
    v[off] *= m;
    w[off] *= m;
}

extern "C" int x3d_ibm_body(x3d_backend *b, const x3d_ibm *m, real_t *u, real_t *v, real_t *w, const int dims[3])
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && m && u && v && w && dims, "x3d_ibm_body: null argument");
    X3D_REQUIRE(m->b == b, "x3d_ibm_body: the mask belongs to another backend");
    X3D_REQUIRE(dims[0] == m->nx && dims[1] == m->ny && dims[2] == m->nz,
                "x3d_ibm_body: dims (%d,%d,%d) are not the mask's (%d,%d,%d)", dims[0], dims[1], dims[2], m->nx, m->ny, m->nz);
    X3D_REQUIRE(u != v && u != w && v != w, "x3d_ibm_body: u, v, w must be three blocks");
    if (m->nseg == 0) return 0;  // a mask of ones: the identity
    X3D_LAZY_OUT(b, u, false);
    X3D_LAZY_OUT(b, v, false);
    X3D_LAZY_OUT(b, w, false);
    X3D_LAZY_EAGER(b);
    ProfScope ps(b, X3D_K_BLAS1);
    hipLaunchKernelGGL(k_ibm_body, dim3((unsigned)((m->nseg + 3) / 4)), dim3(256), 0, b->stream, u, v, w,
                       (const int4 *)m->seg, (const real_t *)m->mask, m->nseg, (long)b->nxp, (long)b->nyp);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- loads: the momentum the mask removes
extern "C" int x3d_ibm_set_weights(x3d_ibm *m, const double *wx, const double *wy, const double *wz)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(m && wx && wy && wz, "x3d_ibm_set_weights: null argument");
    const size_t n = (size_t)m->nx + m->ny + m->nz;
    std::vector<double> host(n);
    std::copy(wx, wx + m->nx, host.begin());
    std::copy(wy, wy + m->ny, host.begin() + m->nx);
    std::copy(wz, wz + m->nz, host.begin() + m->nx + m->ny);
    if (!m->wgt) X3D_HIP(hipMalloc(reinterpret_cast<void **>(&m->wgt), sizeof(double) * n));
    else X3D_HIP(hipStreamSynchronize(m->b->stream));  // (a launch that reads the table being replaced may still run)
    // (the host vector dies with this call: a synchronous copy)
    X3D_HIP(hipMemcpy(m->wgt, host.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    return 0;
}

// k_ibm_body's mapping and its expression for u, v, w (the same bits), and on the way the three impulses of the segment:
// term_c = (((1 - m) f_c) w_x[i]) (w_y[j] w_z[k]), every factor a double before any product.  A wave adds its 64 terms in a
// fixed shuffle tree (lanes beyond the row's end and waves beyond the list hold zeros), the workgroup's four waves are added
// in wave order, and workgroup g leaves the impulses of segments 4 g .. 4 g + 3 in part[g][0..2].  No atomics.
__global__ void __launch_bounds__(256) k_ibm_body_loads(real_t *__restrict__ u, real_t *__restrict__ v, real_t *__restrict__ w,
                                                        const int4 *__restrict__ seg, const real_t *__restrict__ mask, long nseg,
                                                        long nxp, long nyp, const double *__restrict__ wx,
                                                        const double *__restrict__ wy, const double *__restrict__ wz,
                                                        double *__restrict__ part)
{
    __shared__ double sm[4][3];
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long s = wv + 4L * blockIdx.x;
    const int ln = threadIdx.x & 63;
    double tu = 0.0, tv = 0.0, tw = 0.0;
    if (s < nseg) {
        const int4 e = seg[s];
        if (ln < e.w) {  // beyond the row's end: padding, or the next row -- never read, never written
            const real_t m = __builtin_nontemporal_load(mask + s * 64 + ln);
            const long off = nxp * (e.y + nyp * (long)e.z) + e.x + ln;
            const real_t fu = u[off], fv = v[off], fw = w[off];
            const double a = 1.0 - (double)m, wi = wx[e.x + ln], wjk = wy[e.y] * wz[e.z];
            tu = ((a * (double)fu) * wi) * wjk;
            tv = ((a * (double)fv) * wi) * wjk;
            tw = ((a * (double)fw) * wi) * wjk;
            u[off] = fu * m;
            v[off] = fv * m;
            w[off] = fw * m;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        tu += __shfl_down(tu, o);
        tv += __shfl_down(tv, o);
        tw += __shfl_down(tw, o);
    }
    if (ln == 0) { sm[wv][0] = tu; sm[wv][1] = tv; sm[wv][2] = tw; }
    __syncthreads();
    if (threadIdx.x < 3)
        part[3 * (long)blockIdx.x + threadIdx.x] =
            ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// One workgroup: thread t adds the partials t, t + 256, ... in ascending order, then the same shuffle tree and wave order as
// above -- an order fixed by nparts alone.  row[0..2] = the sums (accumulate = 0) or row[0..2] + the sums (accumulate = 1).
__global__ void __launch_bounds__(256) k_ibm_loads_finish(const double *__restrict__ part, long nparts, double *__restrict__ row,
                                                          int accumulate)
{
    __shared__ double sm[4][3];
    double tu = 0.0, tv = 0.0, tw = 0.0;
    for (long p = threadIdx.x; p < nparts; p += 256) {
        tu += part[3 * p + 0];
        tv += part[3 * p + 1];
        tw += part[3 * p + 2];
    }
    for (int o = 32; o > 0; o >>= 1) {
        tu += __shfl_down(tu, o);
        tv += __shfl_down(tv, o);
        tw += __shfl_down(tw, o);
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0) { sm[wv][0] = tu; sm[wv][1] = tv; sm[wv][2] = tw; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const double t = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
        row[threadIdx.x] = accumulate ? row[threadIdx.x] + t : t;
    }
}

extern "C" int x3d_ibm_body_loads(x3d_backend *b, const x3d_ibm *m, real_t *u, real_t *v, real_t *w, const int dims[3],
                                  double *row_dev, int accumulate)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && m && u && v && w && dims && row_dev, "x3d_ibm_body_loads: null argument");
    X3D_REQUIRE(m->b == b, "x3d_ibm_body_loads: the mask belongs to another backend");
    X3D_REQUIRE(dims[0] == m->nx && dims[1] == m->ny && dims[2] == m->nz,
                "x3d_ibm_body_loads: dims (%d,%d,%d) are not the mask's (%d,%d,%d)", dims[0], dims[1], dims[2], m->nx, m->ny,
                m->nz);
    X3D_REQUIRE(u != v && u != w && v != w, "x3d_ibm_body_loads: u, v, w must be three blocks");
    X3D_REQUIRE(m->wgt, "x3d_ibm_body_loads: x3d_ibm_set_weights has not been called on this mask");
    if (m->nseg == 0 && accumulate) return 0;  // a mask of ones adds zeros: nothing to launch
    if (m->nseg > 0) {
        X3D_LAZY_OUT(b, u, false);
        X3D_LAZY_OUT(b, v, false);
        X3D_LAZY_OUT(b, w, false);
    }
    X3D_LAZY_EAGER(b);
    const long nparts = (m->nseg + 3) / 4;
    if (nparts > 0) {  // (timed as x3d_ibm_body's launch is; the finishing launch counts as a reduction)
        ProfScope ps(b, X3D_K_BLAS1);
        hipLaunchKernelGGL(k_ibm_body_loads, dim3((unsigned)nparts), dim3(256), 0, b->stream, u, v, w, (const int4 *)m->seg,
                           (const real_t *)m->mask, m->nseg, (long)b->nxp, (long)b->nyp, (const double *)m->wgt,
                           (const double *)(m->wgt + m->nx), (const double *)(m->wgt + m->nx + m->ny), m->part);
    }
    {
        ProfScope ps(b, X3D_K_REDUCE);
        hipLaunchKernelGGL(k_ibm_loads_finish, dim3(1), dim3(256), 0, b->stream, (const double *)m->part, nparts, row_dev,
                           accumulate ? 1 : 0);
    }
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- outflow parameters
// compute_outflow_params (src/case/cylinder.f90:109-147) on the planes i = 1, nx - 1, nx of u, two stages like the other
// reductions of this library: stage 1 leaves, per workgroup, the two plane sums (FP64 in both flavours) and the maximum
// of the rows it owns -- an assignment that depends on the launch geometry only; stage 2, one workgroup, adds the parts
// in a fixed order and writes the two parameters.  No atomics, no host.  Each lane touches one element per row and plane:
// a cache line per access, inherent in the x-fastest layout.
__global__ void __launch_bounds__(256) k_outflow_stage1(const real_t *__restrict__ u, int nx, int ny, long nrow, long nxp,
                                                        long nyp, double *__restrict__ part)
{
    __shared__ double sm[4][3];
    double s_in = 0.0, s_out = 0.0, mx = -HUGE_VAL;
    for (long q = blockIdx.x * 256L + threadIdx.x; q < nrow; q += 256L * gridDim.x) {
        const long row = nxp * (q % ny + nyp * (q / ny));
        s_in += (double)u[row];
        s_out += (double)u[row + nx - 1];
        mx = fmax(mx, (double)u[row + nx - 2]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        s_in += __shfl_down(s_in, o);
        s_out += __shfl_down(s_out, o);
        mx = fmax(mx, __shfl_down(mx, o));
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0) { sm[wv][0] = s_in; sm[wv][1] = s_out; sm[wv][2] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x + 0] = (sm[0][0] + sm[1][0]) + (sm[2][0] + sm[3][0]);
        part[3 * blockIdx.x + 1] = (sm[0][1] + sm[1][1]) + (sm[2][1] + sm[3][1]);
        part[3 * blockIdx.x + 2] = fmax(fmax(sm[0][2], sm[1][2]), fmax(sm[2][2], sm[3][2]));
    }
}

// params[0] = out_vel = max(u[nx-1]) * gdt / dx ; params[1] = flow_rate_diff = (sum u[1] - sum u[nx]) / (ny * nz)
// (ny * nz of THIS rank, as the reference has it: :124-126)
__global__ void __launch_bounds__(256) k_outflow_stage2(const double *__restrict__ part, int nparts, real_t gdt, real_t dx,
                                                        double ny_nz, real_t *__restrict__ params)
{
    __shared__ double sm[4][3];
    double s_in = 0.0, s_out = 0.0, mx = -HUGE_VAL;
    for (int p = threadIdx.x; p < nparts; p += 256) {
        s_in += part[3 * p + 0];
        s_out += part[3 * p + 1];
        mx = fmax(mx, part[3 * p + 2]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        s_in += __shfl_down(s_in, o);
        s_out += __shfl_down(s_out, o);
        mx = fmax(mx, __shfl_down(mx, o));
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    if (ln == 0) { sm[wv][0] = s_in; sm[wv][1] = s_out; sm[wv][2] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double a = (sm[0][0] + sm[1][0]) + (sm[2][0] + sm[3][0]);
        const double c = (sm[0][1] + sm[1][1]) + (sm[2][1] + sm[3][1]);
        const real_t uxmax = (real_t)fmax(fmax(sm[0][2], sm[1][2]), fmax(sm[2][2], sm[3][2]));  // (exact: it is one of u's values)
        params[0] = uxmax * gdt / dx;
        params[1] = (real_t)((a - c) / ny_nz);
    }
}

extern "C" int x3d_outflow_params(x3d_backend *b, const real_t *u, const int dims[3], real_t gdt, real_t dx,
                                  const real_t **params_dev)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && u && dims && params_dev, "x3d_outflow_params: null argument");
    X3D_REQUIRE(dims[0] > 1 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_outflow_params: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    X3D_REQUIRE(dx != (real_t)0, "x3d_outflow_params: dx is zero");
    X3D_LAZY_IN(b, u);
    X3D_LAZY_EAGER(b);
    // (first call only; each pointer on its own, so that a failure between the two leaves nothing to allocate twice)
    if (!b->bc_part) X3D_HIP(hipMalloc(reinterpret_cast<void **>(&b->bc_part), sizeof(double) * 3 * X3D_BC_PARTS));
    if (!b->bc_params) X3D_HIP(hipMalloc(reinterpret_cast<void **>(&b->bc_params), sizeof(real_t) * 2));
    const long nrow = (long)dims[1] * dims[2];
    const int grid = (int)std::min<long>((nrow + 255) / 256, X3D_BC_PARTS);
    ProfScope ps(b, X3D_K_REDUCE);
    hipLaunchKernelGGL(k_outflow_stage1, dim3(grid), dim3(256), 0, b->stream, u, dims[0], dims[1], nrow, (long)b->nxp,
                       (long)b->nyp, b->bc_part);
    hipLaunchKernelGGL(k_outflow_stage2, dim3(1), dim3(256), 0, b->stream, (const double *)b->bc_part, grid, gdt, dx,
                       (double)nrow, b->bc_params);
    X3D_HIP(hipGetLastError());
    *params_dev = b->bc_params;
    return 0;
}

extern "C" int x3d_outflow_params_get(x3d_backend *b, real_t out[2])
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && out, "x3d_outflow_params_get: null argument");
    X3D_REQUIRE(b->bc_params, "x3d_outflow_params_get: x3d_outflow_params has not run on this backend");
    X3D_HIP(hipMemcpyAsync(out, b->bc_params, sizeof(real_t) * 2, hipMemcpyDeviceToHost, b->stream));
    X3D_HIP(hipStreamSynchronize(b->stream));
    b->n_sync++;
    return 0;
}

// ---------------------------------------------------------------- faces of the cylinder case
// field_set_face_from_field(X_FACE) (backend.hip, k_set_face_x_from) for u, v and w in one launch, c_end and
// flow_rate_diff read from the device: the same expression in the same order, so the same bits.
struct Face3 {
    real_t *f[3];
    const real_t *src[3];
};

__global__ void __launch_bounds__(256) k_cylinder_apply_bc(Face3 F, int nx, int ny, long nrow, long nxp, long nyp,
                                                           const real_t *__restrict__ params)
{
    const long q = blockIdx.x * 256L + threadIdx.x;
    if (q >= nrow) return;
    const real_t c_end = params[0], frd = params[1];
    const long row = nxp * (q % ny + nyp * (q / ny));
    real_t *f = F.f[blockIdx.y];
    f[row] = F.src[blockIdx.y][row];
    const real_t fd = f[row + nx - 1], fd1 = f[row + nx - 2];
    f[row + nx - 1] = fd - c_end * (fd - fd1) + frd;
}

extern "C" int x3d_cylinder_apply_bc(x3d_backend *b, real_t *u, real_t *v, real_t *w, const real_t *in_u, const real_t *in_v,
                                     const real_t *in_w, const int dims[3], const real_t *params_dev)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && u && v && w && in_u && in_v && in_w && dims && params_dev, "x3d_cylinder_apply_bc: null argument");
    X3D_REQUIRE(dims[0] > 2 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_cylinder_apply_bc: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    X3D_REQUIRE(u != v && u != w && v != w, "x3d_cylinder_apply_bc: u, v, w must be three blocks");
    X3D_REQUIRE(in_u != u && in_u != v && in_u != w && in_v != u && in_v != v && in_v != w && in_w != u && in_w != v && in_w != w,
                "x3d_cylinder_apply_bc: an inlet field is one of u, v, w");
    X3D_LAZY_IN(b, in_u);
    X3D_LAZY_IN(b, in_v);
    X3D_LAZY_IN(b, in_w);
    X3D_LAZY_OUT(b, u, false);
    X3D_LAZY_OUT(b, v, false);
    X3D_LAZY_OUT(b, w, false);
    X3D_LAZY_EAGER(b);
    Face3 F;
    F.f[0] = u; F.f[1] = v; F.f[2] = w;
    F.src[0] = in_u; F.src[1] = in_v; F.src[2] = in_w;
    const long nrow = (long)dims[1] * dims[2];
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_cylinder_apply_bc, dim3((unsigned)((nrow + 255) / 256), 3), dim3(256), 0, b->stream, F, dims[0],
                       dims[1], nrow, (long)b->nxp, (long)b->nyp, params_dev);
    X3D_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------- inlet plane
// plane i = 1 of f <- base + amp * (2 r - 1), r(j, k) = (mix64(mix64(seed + draw) + k * ny + j) >> 11) * 2^-53
// (define_BC_cylinder, src/case/cylinder.f90:200-210; the caller folds um into amp)
// FP64: r < 1, the values lie in [base - amp, base + amp).  FP32: the 53-bit integer is rounded to 24 bits first and can
// become 2^53, so r = 1 and base + amp itself can occur -- the interval is closed there, as it is for x3d_wall_noise.
__global__ void __launch_bounds__(256) k_inlet_noise(real_t *__restrict__ f, int ny, long nrow, long nxp, long nyp, real_t base,
                                                     real_t amp, unsigned long long key)
{
    const long q = blockIdx.x * 256L + threadIdx.x;
    if (q >= nrow) return;
    const real_t u01 = (real_t)(x3d_mix64(key + (unsigned long long)q) >> 11) * 0x1.0p-53;
    // (2 u01 - 1 is exact; the last step is spelled out as ONE fused operation so that the value does not depend on what
    //  the compiler chooses to contract: at most half an ulp from the host's two-rounding base + amp * (2 r - 1))
    f[nxp * (q % ny + nyp * (q / ny))] = fma_r(amp, (real_t)(2.0 * u01 - 1.0), base);
}

extern "C" int x3d_inlet_noise(x3d_backend *b, real_t *f, const int dims[3], real_t base, real_t amp, unsigned long long seed,
                               unsigned long long draw)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && f && dims, "x3d_inlet_noise: null argument");
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_inlet_noise: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    X3D_LAZY_OUT(b, f, false);  // (one plane is written: the rest of the block keeps its contents)
    X3D_LAZY_EAGER(b);
    const long nrow = (long)dims[1] * dims[2];
    ProfScope ps(b, X3D_K_COPY);
    hipLaunchKernelGGL(k_inlet_noise, dim3((unsigned)((nrow + 255) / 256)), dim3(256), 0, b->stream, f, dims[1], nrow,
                       (long)b->nxp, (long)b->nyp, base, amp, x3d_mix64(seed + draw));
    X3D_HIP(hipGetLastError());
    return 0;
}
