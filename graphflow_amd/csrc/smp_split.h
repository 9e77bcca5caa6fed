// smp_split.h -- what the two split-operand kernel families of the fused SMP level share: the block products with their weight images
// (smp_level_c64_split.hip) and the weight gradients with their column bounds (smp_level_wgrad_split.hip).  Both carry an fp32 operand as
// two f16 halves (see the header of smp_level_c64_split.hip); here are the vector types, the power-of-two scales, the splits themselves,
// the geometry of a level's prebuilt weight images, and the two families' one read of GF_SMP_MASK_ZEROS (packed_rows).  What only one family uses -- thread
// counts, LDS layouts, the zero page and the scratch rows -- stays in that family's file.
#ifndef GF_SMP_SPLIT_H_INCLUDED
#define GF_SMP_SPLIT_H_INCLUDED

#include "gemm_lds.h"
#include "gf_internal.h"

namespace gf {

using lds_image::f16v;
using lds_image::f4v;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));

// power-of-two scale that puts a magnitude with biased exponent e into [2^13, 2^14), and its inverse (e clamped: magnitudes below
// 2^-113 are flushed by the f16 conversion, which is what the fp32 product of such operands underflows to as well)
template <unsigned EMIN = 14u>
__device__ __forceinline__ void pow2_scale(unsigned maxbits, float *s, float *inv) {
    unsigned e = maxbits >> 23;
    e = e < EMIN ? EMIN : e;
    *s = __uint_as_float((267u - e) << 23);
    *inv = __uint_as_float((e - 13u) << 23);
}
// The weight-gradient kernels fold a row's fp32 factor (tot, tr: up to ~2^10) into the column's scale BEFORE the multiply, so the
// scale of an all-zero column (a dead channel; every padded channel of gf_smp_create) must leave room for it: 2^126 x 30 = inf and
// inf x 0 = NaN.  Exponent floor 64: scale <= 2^76, a column whose largest magnitude is below 2^-63 keeps fewer than 22 bits.
__device__ __forceinline__ void pow2_scale_col(unsigned maxbits, float *s, float *inv) { pow2_scale<64u>(maxbits, s, inv); }
// (a, b) 2^k -> halves.  The LOW half is carried at 2^11 times its value (round 4): unscaled it goes subnormal for every element
// more than 2^17 below the block's largest (f16's smallest normal is 2^-14), which then kept one bit less per binary order -- ~15 bits
// at 2^24 : 1 inside a block.  Scaled, an element keeps its 22 bits down to 2^-27 of the block maximum (where h itself goes
// subnormal), i.e. over more range than an fp32 sum of the same terms resolves.  The two cross products  al' bh + ah bl'  are
// accumulated on their own, multiplied by 2^-11 (exact), and the main product  ah bh  is accumulated on top.
constexpr float kLowScale = 2048.f, kLowUnscale = 1.f / 2048.f;
__device__ __forceinline__ void split_pair2(float a, float b, float sa, float sb, h2 *h, h2 *l) {   // one scale per element
    const f2v x = {a * sa, b * sb};
    *h = __builtin_convertvector(x, h2);
    const f2v r = (x - __builtin_convertvector(*h, f2v)) * kLowScale;
    *l = __builtin_convertvector(r, h2);
}
__device__ __forceinline__ void split_pair(float a, float b, float s, h2 *h, h2 *l) { split_pair2(a, b, s, s, h, l); }
// the low half at its own value (the weight-gradient kernel: per-column exponents, see smp_wgrad_split); one scale per element
__device__ __forceinline__ void split_plain2(float a, float b, float sa, float sb, h2 *h, h2 *l) {
    const f2v x = {a * sa, b * sb};
    *h = __builtin_convertvector(x, h2);
    const f2v r = x - __builtin_convertvector(*h, f2v);
    *l = __builtin_convertvector(r, h2);
}
// The same split with the form of the residual FIXED (smp_wgrad_split).  Left to the compiler, `x - h` with x = a sa is contracted into
// fma(a, sa, -h) in some copies of the code and not in others -- the residual of the unrounded product is not the residual of the rounded
// one, so the low halves differ in their last bit -- and which copies changes with the code around them (it changed between the loop
// and its exits when the operand addressing moved to buffer descriptors).  FMA = true: h from the rounded product, l from the fused
// residual; false: both from the rounded product.  The kernel's tasks keep the forms the builds of record gave them.
template <bool FMA>
__device__ __forceinline__ void split_plain2_as(float a, float b, float sa, float sb, h2 *h, h2 *l) {
#pragma clang fp contract(off)
    const f2v x = {a * sa, b * sb};
    *h = __builtin_convertvector(x, h2);
    const f2v hf = __builtin_convertvector(*h, f2v);
    f2v r;
    if constexpr (FMA) r = f2v{__builtin_fmaf(a, sa, -hf[0]), __builtin_fmaf(b, sb, -hf[1])};
    else r = x - hf;
    *l = __builtin_convertvector(r, h2);
}

// images of both directions of up to kSpImgLevels levels in one launch: workgroup (direction, level); layout per (level, direction):
// imgH [kSpAll] | imgL [kSpAll] | winv (kSpPos floats in five uint4) -- ALL eighteen stacked blocks: positions 0..7 are the row products'
// (smp_rowpanel_split), 8..17 the per-(node,x) / per-node / compact products' (smp_small_split)
constexpr int kSpImgLevels = 8;
// (positions 18, 19, 20: the three extra products of SMP_2D_ver7 on the 18-slice level -- gf_smp::n_extra -- from their own weight blocks X)
constexpr int kSpPos = 21, kSpStacked = 18, kSpAll = kSpPos * 512;
constexpr int kSpImgStride = 2 * kSpAll + 6;   // uint4 per (level, direction): images, then kSpPos inverse scales in six uint4
// C = 128: a sub-block set holds the eight row products' positions only -- imgH [kSpAll128] | imgL [kSpAll128] | eight inverse scales in two uint4
constexpr int kSpAll128 = 8 * 512, kSpImgStride128 = 2 * kSpAll128 + 2;

// the level's packed transposed-row table with the presence bits (see smp_rowpanel_split) in place of the plain one: for levels of
// fewer than `row_limit` rows, unless GF_SMP_MASK_ZEROS=0 (read per call: the parity tests switch it).  THE read of that switch for
// the product and weight-gradient launches (row_products_kernel of smp_level_c64_split.hip, wgrad_packed of smp_level_wgrad_split.hip:
// each family's one decision)
inline bool packed_rows(const int *trowf, int rows, int row_limit) {
    return trowf && rows < row_limit && !env_is("GF_SMP_MASK_ZEROS", '0');
}

}  // namespace gf
#endif
