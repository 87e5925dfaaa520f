// Snapshots: the device side of the reference's snapshot manager (src/io/snapshot_manager.f90, write_fields;
// src/io/io_field_utils.f90:43-124, stride_data_to_buffer).  The reference copies every output field to the host whole,
// strides it there (one array pass per variable) and, for vort / qcrit, first fills two more full blocks
// (src/postprocess/postprocess.f90, compute_derived_fields).  Here ONE launch decimates, converts and packs every variable
// of a snapshot into one dense buffer -- |omega| and Q evaluated at the kept points only, no vort / qcrit block -- and ONE
// asynchronous copy on a second stream moves that buffer into pinned host memory; the compute stream never waits for it.
#include "common.h"

// ---------------------------------------------------------------- the pack kernel
// A wave owns one output row (variable v = blockIdx.y, kept z and y index from blockIdx.x and the wave number) and walks it
// along x: lane l takes the kept points l, l + 64, ... (stride_x > 1: scalar gathers, one point per lane) or, VEC, the pairs
// 2 l, 2 l + 128, ... through 16-byte loads as k_from_gradients has them.  Stores to the dense output are 64 lanes wide and
// contiguous.  The descriptor table travels as a kernel argument; blockIdx.y makes its index uniform.
struct SnapTab {
    x3d_snapshot_var v[X3D_SNAP_MAXVAR];
};
struct SnapGeom {
    int first[3], stride[3], count[3];
    long nxp, nxyp;  // row and plane pitch of the source blocks
};

// the formulas of k_from_gradients (backend.hip; src/backend/omp/backend.f90:616-649), g in the order of Grad9
template <bool QCRIT>
__device__ __forceinline__ real_t snap_derived(const real_t (&g)[9])
{
    const real_t dudx = g[0], dudy = g[1], dudz = g[2], dvdx = g[3], dvdy = g[4], dvdz = g[5], dwdx = g[6], dwdy = g[7],
                 dwdz = g[8];
    if (QCRIT) return -0.5 * (dudx * dudx + dvdy * dvdy + dwdz * dwdz) - dudy * dvdx - dudz * dwdx - dvdz * dwdy;
    return sqrt((dwdy - dvdz) * (dwdy - dvdz) + (dudz - dwdx) * (dudz - dwdx) + (dvdx - dudy) * (dvdx - dudy));
}

template <typename OUT, bool VEC>
__global__ void __launch_bounds__(256) k_snapshot_pack(SnapTab T, SnapGeom G, OUT *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // (kz, ky) of this wave
    const int cx = G.count[0], cy = G.count[1], cz = G.count[2];
    if (row >= (long)cy * cz) return;
    const int ky = (int)(row % cy), kz = (int)(row / cy);
    const x3d_snapshot_var &V = T.v[blockIdx.y];
    const long src0 = (long)(G.first[2] + kz * G.stride[2]) * G.nxyp + (long)(G.first[1] + ky * G.stride[1]) * G.nxp + G.first[0];
    OUT *__restrict__ o = out + ((long)blockIdx.y * cz * cy + row) * cx;
    const int kind = V.kind;
    const real_t scale = V.scale;
    if (VEC) {
        // stride_x = 1 and an even first_x: src0 is 16-byte aligned, the pair of the last odd point stays inside the row pitch
        const bool pair_store = (cx & 1) == 0;  // every output row then starts on an even element
        for (int i = 2 * lane; i < cx; i += 128) {
            real_t r0, r1;
            if (kind == X3D_SNAP_COPY) {
                const real2_t a = ldg_stream((const real2_t *)(V.src[0] + src0 + i));
                r0 = a.x * scale; r1 = a.y * scale;
            } else {
                real_t g0[9], g1[9];
#pragma unroll
                for (int m = 0; m < 9; m++) {
                    const real2_t a = ldg_stream((const real2_t *)(V.src[m] + src0 + i));
                    g0[m] = a.x; g1[m] = a.y;
                }
                if (kind == X3D_SNAP_QCRIT) { r0 = snap_derived<true>(g0); r1 = snap_derived<true>(g1); }
                else { r0 = snap_derived<false>(g0); r1 = snap_derived<false>(g1); }
            }
            if (pair_store) {
                typedef OUT out2v __attribute__((ext_vector_type(2)));
                const out2v w = {(OUT)r0, (OUT)r1};
                __builtin_nontemporal_store(w, reinterpret_cast<out2v *>(o + i));
            } else {
                o[i] = (OUT)r0;
                if (i + 1 < cx) o[i + 1] = (OUT)r1;
            }
        }
    } else {
        const int sx = G.stride[0];
        for (int i = lane; i < cx; i += 64) {
            const long s = src0 + (long)i * sx;
            real_t r;
            if (kind == X3D_SNAP_COPY) {
                r = __builtin_nontemporal_load(V.src[0] + s) * scale;
            } else {
                real_t g[9];
#pragma unroll
                for (int m = 0; m < 9; m++) g[m] = __builtin_nontemporal_load(V.src[m] + s);
                r = kind == X3D_SNAP_QCRIT ? snap_derived<true>(g) : snap_derived<false>(g);
            }
            __builtin_nontemporal_store((OUT)r, o + i);
        }
    }
}

// ---------------------------------------------------------------- copies in flight
// One slot per packed device buffer: ev_pack orders the copy behind the pack, ev_done is recorded behind the copy and is
// what x3d_snapshot_done / _wait look at -- and what the NEXT pack into the same buffer waits for, on the device.
// Who holds packed buffers on one backend (copyring.CopyRing slots): Snapshots 2, Checkpoints 1, and 2 for each series --
// Diagnostics, Loads, Probes: 9 with everything attached.  A ring slot that grows takes a new buffer and with it a new slot
// here, so the limit leaves room for that.
#define X3D_SNAP_SLOTS 16
struct SnapSlot {
    void *dev;
    hipEvent_t ev_pack, ev_done;
    bool copied;  // ev_done has been recorded at least once
};
struct x3d_snap {
    SnapSlot slot[X3D_SNAP_SLOTS];
    int nslot;
    hipStream_t own;  // the backend's copy stream, made on first use (non-blocking: the null stream does not join it)
};

static SnapSlot *snap_find(x3d_backend *b, const void *dev)
{
    x3d_snap *s = static_cast<x3d_snap *>(b->snap);
    if (!s) return nullptr;
    for (int i = 0; i < s->nslot; i++)
        if (s->slot[i].dev == dev) return &s->slot[i];
    return nullptr;
}

void x3d_snapshot_destroy_c(x3d_backend *b)
{
    x3d_snap *s = static_cast<x3d_snap *>(b->snap);
    if (!s) return;
    for (int i = 0; i < s->nslot; i++) {
        if (s->slot[i].copied) (void)hipEventSynchronize(s->slot[i].ev_done);  // (a pinned buffer may still be a target)
        (void)hipEventDestroy(s->slot[i].ev_pack);
        (void)hipEventDestroy(s->slot[i].ev_done);
    }
    if (s->own) (void)hipStreamDestroy(s->own);
    delete s;
    b->snap = nullptr;
}

int x3d_snapshot_wait_for_copy_c(x3d_backend *b, const void *dev)
{
    if (SnapSlot *s = snap_find(b, dev))
        if (s->copied) X3D_HIP(hipStreamWaitEvent(b->stream, s->ev_done, 0));
    return 0;
}

extern "C" int x3d_snapshot_pack(x3d_backend *b, const x3d_snapshot_var *vars, int nvar, const int dims[3],
                                 const int first[3], const int stride[3], const int count[3], int out_bytes, void *out)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && vars && dims && first && stride && count && out, "x3d_snapshot_pack: null argument");
    X3D_REQUIRE(nvar >= 1 && nvar <= X3D_SNAP_MAXVAR, "x3d_snapshot_pack: 1 .. %d variables (got %d)", X3D_SNAP_MAXVAR, nvar);
    X3D_REQUIRE(out_bytes == 4 || out_bytes == 8, "x3d_snapshot_pack: the output type is a 4- or 8-byte real (got %d)", out_bytes);
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "x3d_snapshot_pack: dims (%d,%d,%d) outside the block", dims[0], dims[1], dims[2]);
    for (int d = 0; d < 3; d++) {
        X3D_REQUIRE(stride[d] >= 1 && count[d] >= 1 && first[d] >= 0, "x3d_snapshot_pack: bad first / stride / count in direction %d",
                    d + 1);
        X3D_REQUIRE((long)first[d] + (long)(count[d] - 1) * stride[d] < dims[d],
                    "x3d_snapshot_pack: direction %d: first %d + (count %d - 1) * stride %d is outside dims %d", d + 1, first[d],
                    count[d], stride[d], dims[d]);
    }
    SnapTab T;
    memset(&T, 0, sizeof T);
    for (int v = 0; v < nvar; v++) {
        const int kind = vars[v].kind;
        X3D_REQUIRE(kind == X3D_SNAP_COPY || kind == X3D_SNAP_VORT || kind == X3D_SNAP_QCRIT,
                    "x3d_snapshot_pack: variable %d has an unknown kind %d", v, kind);
        T.v[v].kind = kind;
        T.v[v].scale = vars[v].scale;
        for (int m = 0; m < (kind == X3D_SNAP_COPY ? 1 : 9); m++) {
            X3D_REQUIRE(vars[v].src[m], "x3d_snapshot_pack: variable %d, source block %d is null", v, m);
            T.v[v].src[m] = vars[v].src[m];
        }
    }
    for (int v = 0; v < nvar; v++)
        for (int m = 0; m < (T.v[v].kind == X3D_SNAP_COPY ? 1 : 9); m++) X3D_LAZY_IN(b, T.v[v].src[m]);
    X3D_LAZY_EAGER(b);
    // a copy of this buffer's previous contents may still be in flight: the pack waits for it on the device
    if (int rc = x3d_snapshot_wait_for_copy_c(b, out)) return rc;
    SnapGeom G;
    for (int d = 0; d < 3; d++) { G.first[d] = first[d]; G.stride[d] = stride[d]; G.count[d] = count[d]; }
    G.nxp = b->nxp;
    G.nxyp = (long)b->nxp * b->nyp;
    bool vec = stride[0] == 1 && first[0] % 2 == 0;
    for (int v = 0; v < nvar; v++)  // (blocks are 16-byte aligned; any other source takes the scalar path)
        for (int m = 0; m < (T.v[v].kind == X3D_SNAP_COPY ? 1 : 9); m++)
            if ((size_t)T.v[v].src[m] % (2 * sizeof(real_t)) != 0) vec = false;
    const long rows = (long)count[1] * count[2];
    const dim3 grid((unsigned)((rows + 3) / 4), (unsigned)nvar), block(256);
    ProfScope ps(b, X3D_K_PACK);
    if (out_bytes == 8) {
        if (vec) hipLaunchKernelGGL((k_snapshot_pack<double, true>), grid, block, 0, b->stream, T, G, (double *)out);
        else hipLaunchKernelGGL((k_snapshot_pack<double, false>), grid, block, 0, b->stream, T, G, (double *)out);
    } else {
        if (vec) hipLaunchKernelGGL((k_snapshot_pack<float, true>), grid, block, 0, b->stream, T, G, (float *)out);
        else hipLaunchKernelGGL((k_snapshot_pack<float, false>), grid, block, 0, b->stream, T, G, (float *)out);
    }
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_snapshot_copy_async(x3d_backend *b, void *host_pinned, const void *dev, long nbytes, void *copy_stream,
                                       int *handle)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && host_pinned && dev && handle && nbytes > 0, "x3d_snapshot_copy_async: bad argument");
    X3D_LAZY_FLUSH(b);
    X3D_LAZY_EAGER(b);
    if (!b->snap) {
        x3d_snap *s = new x3d_snap();
        memset(s, 0, sizeof *s);
        b->snap = s;
    }
    x3d_snap *S = static_cast<x3d_snap *>(b->snap);
    hipStream_t cs = (hipStream_t)copy_stream;
    if (!cs || cs == b->stream) {
        if (!S->own) X3D_HIP(hipStreamCreateWithFlags(&S->own, hipStreamNonBlocking));
        cs = S->own;
    }
    SnapSlot *s = snap_find(b, dev);
    if (!s) {
        X3D_REQUIRE(S->nslot < X3D_SNAP_SLOTS, "x3d_snapshot_copy_async: more than %d packed buffers", X3D_SNAP_SLOTS);
        s = &S->slot[S->nslot];
        X3D_HIP(hipEventCreateWithFlags(&s->ev_pack, hipEventDisableTiming));
        X3D_HIP(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
        s->dev = const_cast<void *>(dev);
        s->copied = false;
        S->nslot++;
    }
    X3D_HIP(hipEventRecord(s->ev_pack, b->stream));
    X3D_HIP(hipStreamWaitEvent(cs, s->ev_pack, 0));
    X3D_HIP(hipMemcpyAsync(host_pinned, dev, (size_t)nbytes, hipMemcpyDeviceToHost, cs));
    X3D_HIP(hipEventRecord(s->ev_done, cs));
    s->copied = true;
    *handle = (int)(s - S->slot);
    return 0;
}

static int snap_slot_of(x3d_backend *b, int handle, SnapSlot **out)
{
    x3d_snap *S = b ? static_cast<x3d_snap *>(b->snap) : nullptr;
    X3D_REQUIRE(S && handle >= 0 && handle < S->nslot && S->slot[handle].copied, "x3d_snapshot: %d is not the handle of a copy",
                handle);
    *out = &S->slot[handle];
    return 0;
}

extern "C" int x3d_snapshot_done(x3d_backend *b, int handle, int *done)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && done, "x3d_snapshot_done: null argument");
    X3D_LAZY_FLUSH(b);
    X3D_LAZY_EAGER(b);
    SnapSlot *s = nullptr;
    if (int rc = snap_slot_of(b, handle, &s)) return rc;
    const hipError_t e = hipEventQuery(s->ev_done);
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();  // (not an error: the next launch check must not find it)
        *done = 0;
        return 0;
    }
    X3D_HIP(e);
    *done = 1;
    return 0;
}

extern "C" int x3d_snapshot_wait(x3d_backend *b, int handle)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b, "x3d_snapshot_wait: null argument");
    X3D_LAZY_FLUSH(b);
    X3D_LAZY_EAGER(b);
    SnapSlot *s = nullptr;
    if (int rc = snap_slot_of(b, handle, &s)) return rc;
    X3D_HIP(hipEventSynchronize(s->ev_done));
    b->n_sync++;
    return 0;
}
