// Checkpoints: the device side of the reference's checkpoint manager (src/io/checkpoint_manager.f90, write_fields /
// restart_checkpoint; src/io/io_manager.f90).  The reference pulls every field of the state to the host whole, one blocking
// get_field_data per variable, and on restart fills each block with 0 before set_field_data.  Here ONE launch packs the
// interiors of every block of the state (velocity, species, Adams-Bashforth history, statistics accumulators) into one dense
// buffer and, in the same pass, forms three integers per block -- two position-weighted sums of the elements' bit patterns
// and the count of NaN / Inf -- which ride behind the data through the asynchronous copy of snapshot.hip.  On restart the
// same sums are formed from the uploaded buffer before a single block is written, and ONE launch unpacks it.
//
// The sums are integer sums modulo 2^64: they do not depend on the order of the additions, so any reduction shape gives the
// same table.  With i the dense index of element e_i within its block:  s1 = sum bits(e_i),  s2 = sum bits(e_i) (2 i + 1).
// A wave forms, per row (or chunk) that starts at dense index i0, a = sum bits and c = sum bits (2 x + 1) with x the offset
// inside the row -- then s2's share is c + a * (2 i0): one 64-bit product per row instead of one per element.
#include "common.h"

typedef unsigned long long u64;
#define CKPT_V (16 / X3D_RB)  // elements per 16-byte access: 2 (FP64) or 4 (FP32)
typedef real_t ckpt_vec __attribute__((ext_vector_type(CKPT_V)));
#define CKPT_ROWS_PER_WAVE 8   // pack: a workgroup of four waves owns 32 consecutive rows and adds to the table once
#define CKPT_CHUNK 4096        // sums: dense elements per workgroup

struct CkptSrc {
    const real_t *p[X3D_CKPT_MAXBLOCK];
};
struct CkptDst {
    real_t *p[X3D_CKPT_MAXBLOCK];
};

__device__ __forceinline__ u64 ckpt_bits(real_t v)
{
#ifdef X3D_SINGLE_PREC
    return (u64)__float_as_uint(v);  // zero-extended
#else
    return (u64)__double_as_longlong(v);
#endif
}
__device__ __forceinline__ u64 ckpt_nonfinite(u64 bits)
{
#ifdef X3D_SINGLE_PREC
    return (bits & 0x7f800000ull) == 0x7f800000ull ? 1ull : 0ull;
#else
    return (bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull ? 1ull : 0ull;
#endif
}

// per-thread partial sums of one row / chunk: a = sum bits, c = sum bits (2 x + 1), nf = count of NaN / Inf
struct CkptAcc {
    u64 a, c, nf;
    __device__ __forceinline__ void add(real_t v, unsigned x)
    {
        const u64 bits = ckpt_bits(v);
        a += bits;
        c += bits * (u64)(2u * x + 1u);  // (x < 2^30: the factor fits 32 bits, the product is one mad_u64_u32 per half)
        nf += ckpt_nonfinite(bits);
    }
};

// the workgroup's three sums -> table[0..2], one vector atomic each from thread 0
__device__ __forceinline__ void ckpt_reduce_add(u64 s1, u64 s2, u64 nf, u64 *__restrict__ table)
{
    __shared__ u64 red[3][256];
    const int t = threadIdx.x;
    red[0][t] = s1; red[1][t] = s2; red[2][t] = nf;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w]; red[1][t] += red[1][t + w]; red[2][t] += red[2][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        if (red[0][0]) atomicAdd(&table[0], red[0][0]);
        if (red[1][0]) atomicAdd(&table[1], red[1][0]);
        if (red[2][0]) atomicAdd(&table[2], red[2][0]);
    }
}

// ---------------------------------------------------------------- pack
// blockIdx.y = the block of the state (its pointer is uniform per workgroup), blockIdx.x = a group of 32 rows (y, z);
// a wave walks its 8 rows along x.  Source rows start on 16 bytes (the row pitch is a multiple of 16 elements): the loads are
// 16 bytes wide when VEC, with a scalar tail of nx % CKPT_V elements; a dense row starts on 16 bytes only where
// (block * n + row * nx) % CKPT_V == 0 -- uniform per row -- and is stored 16 bytes wide there, element by element elsewhere.
template <bool VEC>
__global__ void __launch_bounds__(256) k_checkpoint_pack(CkptSrc S, int nx, int ny, long rows, long nxp, long nxyp,
                                                         real_t *__restrict__ out, u64 *__restrict__ table)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.y;
    const real_t *__restrict__ src = S.p[k];
    const long n = rows * nx;  // elements per block
    const long r0 = ((long)blockIdx.x * 4 + wave) * CKPT_ROWS_PER_WAVE;
    u64 s1 = 0, s2 = 0, nf = 0;
    for (long r = r0; r < r0 + CKPT_ROWS_PER_WAVE && r < rows; r++) {
        const long y = r % ny, z = r / ny;
        const real_t *__restrict__ s = src + z * nxyp + y * nxp;
        const long i0 = r * nx;               // dense index of the row's first element within the block
        real_t *__restrict__ o = out + (long)k * n + i0;
        CkptAcc A = {0, 0, 0};
        int done = 0;
        if (VEC) {
            const int nvec = nx / CKPT_V;
            const bool wide = (((long)k * n + i0) % CKPT_V) == 0;
            for (int j = lane; j < nvec; j += 64) {
                const ckpt_vec v = __builtin_nontemporal_load(reinterpret_cast<const ckpt_vec *>(s) + j);
#pragma unroll
                for (int e = 0; e < CKPT_V; e++) A.add(v[e], (unsigned)(j * CKPT_V + e));
                if (wide) {
                    __builtin_nontemporal_store(v, reinterpret_cast<ckpt_vec *>(o) + j);
                } else {
#pragma unroll
                    for (int e = 0; e < CKPT_V; e++) o[j * CKPT_V + e] = v[e];
                }
            }
            done = nvec * CKPT_V;
        }
        for (int x = done + lane; x < nx; x += 64) {  // the scalar tail (VEC), or the whole row
            const real_t v = __builtin_nontemporal_load(s + x);
            A.add(v, (unsigned)x);
            __builtin_nontemporal_store(v, o + x);
        }
        s1 += A.a;
        s2 += A.c + A.a * (u64)(2 * i0);
        nf += A.nf;
    }
    ckpt_reduce_add(s1, s2, nf, table + 3 * (long)k);
}

// ---------------------------------------------------------------- the sums of a dense buffer
// restart only: coalesced scalar loads (a block of an odd length starts off the 16-byte grid)
__global__ void __launch_bounds__(256) k_checkpoint_sums(const real_t *__restrict__ dense, long n, u64 *__restrict__ table)
{
    const int k = blockIdx.y;
    const real_t *__restrict__ d = dense + (long)k * n;
    const long i0 = (long)blockIdx.x * CKPT_CHUNK;
    CkptAcc A = {0, 0, 0};
    for (int x = threadIdx.x; x < CKPT_CHUNK && i0 + x < n; x += 256) A.add(d[i0 + x], (unsigned)x);
    ckpt_reduce_add(A.a, A.c + A.a * (u64)(2 * i0), A.nf, table + 3 * (long)k);
}

// ---------------------------------------------------------------- unpack
// the inverse: a wave owns one row of the PADDED block (blockIdx.x and the wave number; blockIdx.y = block) and writes all of
// it, the interior from the dense buffer and +0.0 everywhere else (row padding, rows and planes beyond dims).  Block rows
// are stored 16 bytes wide when VEC; the dense row is loaded 16 bytes wide where it starts on 16 bytes.
template <bool VEC>
__global__ void __launch_bounds__(256) k_checkpoint_unpack(CkptDst D, int nx, int ny, int nz, int nxp, int nyp, long prows,
                                                           const real_t *__restrict__ dense)
{
    const int lane = threadIdx.x & 63;
    const long pr = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // row of the padded block
    if (pr >= prows) return;
    const int k = blockIdx.y;
    const long y = pr % nyp, z = pr / nyp;
    real_t *__restrict__ dst = D.p[k] + pr * nxp;
    const bool inside = y < ny && z < nz;
    const long n = (long)nx * ny * nz;
    const long i0 = (z * ny + y) * nx;
    const real_t *__restrict__ s = dense + (long)k * n + i0;  // (not dereferenced unless inside)
    if (VEC) {
        const bool wide = inside && (((long)k * n + i0) % CKPT_V) == 0;
        for (int j = lane; j < nxp / CKPT_V; j += 64) {
            const int x0 = j * CKPT_V;
            ckpt_vec v;
            if (wide && x0 + CKPT_V <= nx) {
                v = __builtin_nontemporal_load(reinterpret_cast<const ckpt_vec *>(s) + j);
            } else {
#pragma unroll
                for (int e = 0; e < CKPT_V; e++) v[e] = (inside && x0 + e < nx) ? s[x0 + e] : (real_t)0;
            }
            __builtin_nontemporal_store(v, reinterpret_cast<ckpt_vec *>(dst) + j);
        }
    } else {
        for (int x = lane; x < nxp; x += 64) dst[x] = (inside && x < nx) ? s[x] : (real_t)0;
    }
}

// ---------------------------------------------------------------- entry points
static int ckpt_check(const x3d_backend *b, const char *who, int nblock, const int dims[3])
{
    X3D_REQUIRE(nblock >= 1 && nblock <= X3D_CKPT_MAXBLOCK, "%s: 1 .. %d blocks per launch (got %d)", who, X3D_CKPT_MAXBLOCK,
                nblock);
    X3D_REQUIRE(dims[0] > 0 && dims[0] <= b->nxp && dims[1] > 0 && dims[1] <= b->nyp && dims[2] > 0 && dims[2] <= b->nzp,
                "%s: dims (%d,%d,%d) outside the block", who, dims[0], dims[1], dims[2]);
    X3D_REQUIRE(dims[0] < (1 << 30), "%s: rows longer than the position weights are built for", who);
    return 0;
}

extern "C" int x3d_checkpoint_pack(x3d_backend *b, const x3d_real *const *blocks, int nblock, const int dims[3], void *out,
                                   unsigned long long *table)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && blocks && dims && out && table, "x3d_checkpoint_pack: null argument");
    if (int rc = ckpt_check(b, "x3d_checkpoint_pack", nblock, dims)) return rc;
    X3D_REQUIRE((size_t)out % sizeof(real_t) == 0 && (size_t)table % sizeof(u64) == 0,
                "x3d_checkpoint_pack: the buffer or the table is not aligned to its elements");
    CkptSrc S;
    memset(&S, 0, sizeof S);
    for (int k = 0; k < nblock; k++) {
        X3D_REQUIRE(blocks[k], "x3d_checkpoint_pack: block %d is null", k);
        S.p[k] = blocks[k];
    }
    for (int k = 0; k < nblock; k++) X3D_LAZY_IN(b, S.p[k]);
    X3D_LAZY_EAGER(b);
    // a copy of this buffer's previous contents may still be in flight: the pack waits for it on the device
    if (int rc = x3d_snapshot_wait_for_copy_c(b, out)) return rc;
    bool vec = (size_t)out % 16 == 0;
    for (int k = 0; k < nblock; k++)  // (blocks are 16-byte aligned; any other source takes the scalar path)
        if ((size_t)S.p[k] % 16 != 0) vec = false;
    const int nx = dims[0], ny = dims[1];
    const long rows = (long)ny * dims[2];
    const long per_wg = 4 * CKPT_ROWS_PER_WAVE;
    const dim3 grid((unsigned)((rows + per_wg - 1) / per_wg), (unsigned)nblock), block(256);
    X3D_HIP(hipMemsetAsync(table, 0, sizeof(u64) * 3 * (size_t)nblock, b->stream));
    ProfScope ps(b, X3D_K_PACK);
    const long nxp = b->nxp, nxyp = (long)b->nxp * b->nyp;
    if (vec)
        hipLaunchKernelGGL((k_checkpoint_pack<true>), grid, block, 0, b->stream, S, nx, ny, rows, nxp, nxyp, (real_t *)out, table);
    else
        hipLaunchKernelGGL((k_checkpoint_pack<false>), grid, block, 0, b->stream, S, nx, ny, rows, nxp, nxyp, (real_t *)out, table);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_checkpoint_sums(x3d_backend *b, const void *dense, int nblock, long n_per_block, unsigned long long *table)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && dense && table, "x3d_checkpoint_sums: null argument");
    X3D_REQUIRE(nblock >= 1 && nblock <= X3D_CKPT_MAXBLOCK, "x3d_checkpoint_sums: 1 .. %d blocks per launch (got %d)",
                X3D_CKPT_MAXBLOCK, nblock);
    X3D_REQUIRE(n_per_block > 0 && n_per_block < (1l << 42), "x3d_checkpoint_sums: bad block length %ld", n_per_block);
    X3D_REQUIRE((size_t)dense % sizeof(real_t) == 0 && (size_t)table % sizeof(u64) == 0,
                "x3d_checkpoint_sums: the buffer or the table is not aligned to its elements");
    X3D_LAZY_FLUSH(b);
    X3D_LAZY_EAGER(b);
    const dim3 grid((unsigned)((n_per_block + CKPT_CHUNK - 1) / CKPT_CHUNK), (unsigned)nblock), block(256);
    X3D_HIP(hipMemsetAsync(table, 0, sizeof(u64) * 3 * (size_t)nblock, b->stream));
    ProfScope ps(b, X3D_K_REDUCE);
    hipLaunchKernelGGL(k_checkpoint_sums, grid, block, 0, b->stream, (const real_t *)dense, n_per_block, table);
    X3D_HIP(hipGetLastError());
    return 0;
}

extern "C" int x3d_checkpoint_unpack(x3d_backend *b, x3d_real *const *blocks, int nblock, const int dims[3], long block_elems,
                                     const void *dense)
{
    X3D_RANGE(__func__);
    X3D_REQUIRE(b && blocks && dims && dense, "x3d_checkpoint_unpack: null argument");
    if (int rc = ckpt_check(b, "x3d_checkpoint_unpack", nblock, dims)) return rc;
    X3D_REQUIRE(block_elems == (long)b->nblock, "x3d_checkpoint_unpack: a block has %ld elements, the caller says %ld",
                (long)b->nblock, block_elems);
    X3D_REQUIRE((size_t)dense % sizeof(real_t) == 0, "x3d_checkpoint_unpack: the buffer is not aligned to its elements");
    CkptDst D;
    memset(&D, 0, sizeof D);
    for (int k = 0; k < nblock; k++) {
        X3D_REQUIRE(blocks[k], "x3d_checkpoint_unpack: block %d is null", k);
        for (int q = 0; q < k; q++) X3D_REQUIRE(blocks[k] != blocks[q], "x3d_checkpoint_unpack: blocks %d and %d are the same", q, k);
        D.p[k] = blocks[k];
    }
    for (int k = 0; k < nblock; k++) X3D_LAZY_OUT(b, D.p[k], true);
    X3D_LAZY_EAGER(b);
    bool vec = (size_t)dense % 16 == 0 && b->nxp % CKPT_V == 0;
    for (int k = 0; k < nblock; k++)
        if ((size_t)D.p[k] % 16 != 0) vec = false;
    const long prows = (long)b->nyp * b->nzp;
    const dim3 grid((unsigned)((prows + 3) / 4), (unsigned)nblock), block(256);
    ProfScope ps(b, X3D_K_PACK);
    if (vec)
        hipLaunchKernelGGL((k_checkpoint_unpack<true>), grid, block, 0, b->stream, D, dims[0], dims[1], dims[2], b->nxp, b->nyp,
                           prows, (const real_t *)dense);
    else
        hipLaunchKernelGGL((k_checkpoint_unpack<false>), grid, block, 0, b->stream, D, dims[0], dims[1], dims[2], b->nxp, b->nyp,
                           prows, (const real_t *)dense);
    X3D_HIP(hipGetLastError());
    return 0;
}
