// process_spectral_000, the mode operator of the all-periodic (000) Poisson solvers -- ONE copy for every kernel that
// applies it (poisson.hip, pfft.hip, sfft.hip and the fused transforms of fft512.hip):
//   src/backend/omp/kernels/spectral_processing.f90:36-99   three forward half-cell rotations (z, y, x), the division
//                                                           by the modified wave number, three backward rotations
// The operator is split at the division.  The normalisation and the division stay with the caller, in one of two forms:
//   form 1   v / nx / ny / nz ... -div / waves, zero where waves < 1e-16      (the reference's own divisions)
//   form 2   v * rn ... div * rw with rn = 1 / (nx ny nz) and the stored rw = -1 / waves (0 where waves < 1e-16)
#pragma once
#include "common.h"

// what one mode needs: its entries of the six rotation tables and the sign flips of the mirrored half of each axis
// ((k + 1) > n / 2 + 1).  fx is set only where the x axis is a full one (the z-first spectra: fft512.hip, ZH / YL);
// there the caller also swaps the roles of y and z by how it fills the struct.
struct Spec000Mode {
    real_t az, bz, ay, by, ax, bx;
    bool fz, fy, fx;
};

// Every p * q + r * s below is spelled with fma_r: under -ffp-contract=fast the compiler otherwise picks the fused
// product per call site (common.h).  The spelling is what the FP64 build of k_fft512<2, 8, ZH> (register layout) and
// k_fft512_peers<.., YL> chose before the copies were merged: the FIRST product as written in the reference is the
// fused one, except in the last line of the backward x rotation, where it is tr * ax.  (The table entry is written first
// in every fma_r: the same value, and the operand order with which the kernels keep the register counts they had.)
__device__ __forceinline__ void spec000_forward(real_t &div_r, real_t &div_c, const Spec000Mode &m)
{
    real_t tr, tc;
    tr = div_r; tc = div_c;  // z (:46-51)
    div_r = fma_r(m.bz, tr, tc * m.az); div_c = fma_r(m.bz, tc, -(tr * m.az));
    if (m.fz) { div_r = -div_r; div_c = -div_c; }
    tr = div_r; tc = div_c;  // y (:54-59)
    div_r = fma_r(m.by, tr, tc * m.ay); div_c = fma_r(m.by, tc, -(tr * m.ay));
    if (m.fy) { div_r = -div_r; div_c = -div_c; }
    tr = div_r; tc = div_c;  // x (:62-65)
    div_r = fma_r(m.bx, tr, tc * m.ax); div_c = fma_r(m.bx, tc, -(tr * m.ax));
    if (m.fx) { div_r = -div_r; div_c = -div_c; }
}

__device__ __forceinline__ void spec000_backward(real_t &div_r, real_t &div_c, const Spec000Mode &m)
{
    real_t tr, tc;
    tr = div_r; tc = div_c;  // z (:80-85)
    div_r = fma_r(m.bz, tr, -(tc * m.az)); div_c = fma_r(m.bz, -tc, -(tr * m.az));
    if (m.fz) { div_r = -div_r; div_c = -div_c; }
    tr = div_r; tc = div_c;  // y (:88-93)
    div_r = fma_r(m.by, tr, tc * m.ay); div_c = fma_r(m.by, tc, -(tr * m.ay));
    if (m.fy) { div_r = -div_r; div_c = -div_c; }
    tr = div_r; tc = div_c;  // x (:96-99)
    div_r = fma_r(m.bx, tr, tc * m.ax); div_c = fma_r(m.ax, tr, -(tc * m.bx));
    if (m.fx) { div_r = -div_r; div_c = -div_c; }
}
