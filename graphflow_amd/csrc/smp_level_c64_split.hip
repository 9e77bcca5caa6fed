// smp_level_c64_split.hip -- the row-panel block products of the fused SMP level at C = 64 (and, templated on the channel count, C = 32:
// round 4) in the compact O layout, on the f16 matrix
// pipe with fp32-grade operands: every fp32 operand x is carried as TWO halves
//     x 2^k = h + l,   h = rn_f16(x 2^k),  l = rn_f16(x 2^k - h)          (22 significant bits, k a per-row / per-block exponent)
// and a product a b is evaluated as  ah bh + ah bl + al bh  (three v_mfma_f32_32x32x16_f16 with fp32 accumulation; products of
// f16 values are exact in fp32, the dropped al bl is 2^-22 of the term).  Against an fp64 product of the same operands the result
// is as close as the fp32 MFMA's (both are dominated by the fp32 accumulation; the arithmetic is emulated in tests/test_split_numerics.py
// and the kernels are held to the same 1e-5 bar by every SMP parity test, tests/test_smp_gpu.py::test_split_operand_products_*), while 64 columns of reduction cost 12 MFMAs of 8 passes instead of 32 of
// 16: the three product kernels of a level stop being bound by the fp32 matrix pipe (0.71 of its 157 TF/s peak, 0.83 of what the
// sustained clock allows -- no headroom) and become HBM streams.
//
// Same work decomposition as smp_rowpanel_c64 (smp_level_c64.hip): the eight 64 x 64 weight blocks live in LDS for the life of
// the workgroup -- here as two f16 fragment images (h and l, 64 KB each, scaled by a per-block power of two) -- and every wave
// walks 32-row panels alone: a lane owns half a row of a 64-column block, finds the row's exponent, splits its 32 values in
// registers, and runs the panel's products out of registers and LDS.  Row factors (tot / tr of the node, the row's and the
// block's exponents) multiply the product's 32 x 64 result on its way into the output accumulator.
#include <cstdlib>
#include <type_traits>

#include "gemm_lds.h"
#include "gf_internal.h"
#include "smp_internal.h"

namespace gf {
namespace {

using lds_image::f16v;
using lds_image::f4v;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef float f2v __attribute__((ext_vector_type(2)));

constexpr int kSpThreads = 512;            // two waves per SIMD, 256 registers each

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

// MASK: `trow` is the level's PACKED table (DevLevel::trowf) -- bits 0..29 the transposed row, bit 31 = the row's S_ab / T6 blocks
// hold data, bit 30 = those of the transposed row do.  Half of the rows at QM9 sizes are structurally zero in those two blocks
// (row (a, b) with b outside the field of a's source); the forward kernel then reads such a block from one 128-byte page of zeros
// that never leaves the caches instead: 1.1 of the 3.3 GB the kernel read per cfg3 step are not fetched.
// RULE: a select between a kernel argument and a `__device__` array (this page, sp_dump below) must be made, and the access issued, in
// the GLOBAL address space -- gf_global() on both sides, gf_ld_g / gf_st_g (gf_internal.h).  Selected as plain pointers the result is a
// generic pointer and every access through it a FLAT instruction: counted against LGKM_CNT as well, unordered against the LDS traffic
// these kernels live on, so the compiler drains its queues (lgkmcnt(0) / vmcnt(0)) where it would otherwise count them.  The same holds
// for an address that comes back from LDS as an integer (the row-class stores).
__device__ __attribute__((aligned(256))) const float sp_zero_page[64] = {};
// ... and the backward kernel sends the dS_ab / dT6 blocks of such rows -- gradients of structural zeros, which no consumer reads
// (the gather of df_{l-1} only visits rows (a, b) with b inside the field of a's source) -- to a scratch area that stays in L2:
// 0.73 of the 2.9 GB of dT are not written.  288 rows of 64 floats: a panel row r lands on scratch row (r & 255) + its offset
// inside the panel, spread over the cache channels.
constexpr int kSpDumpRows = 256 + 32;
__device__ __attribute__((aligned(256))) float sp_dump[kSpDumpRows * 64];
// The weight images of one direction: B fragment (pos, nh, c) gives lane (n, g) the eight values B[k = 32 g + 8 c + j][32 nh + n],
// j < 8, where B = W_pos (forward) or W_pos^T (backward) -- the k order a lane's half row of A supplies (see split_blk) -- as two f16
// halves at the block's exponent.  imgH / imgL / winv may be LDS (built by the product kernel itself) or global memory (built once
// per forward pass by smp_split_weight_images and copied by the product kernels: the build is ~30 us of strided reads per
// workgroup, and six launches per step paid it).  wmax: 8 words of LDS.
// CB = channels (64, or 32 since round 4): a block is CB x CB, a lane (row, half lh) of the A operand holds CB / 2 columns of its row,
// i.e. NC = CB / 16 k-chunks of eight, and the output has NH = CB / 32 column halves: NH NC 64 fragment entries per block, stored at
// a stride of 512 entries per position whatever CB is.
// LD (C = 128: a 64 x 64 sub-block of a 128 x 128 weight block, NPOS = 1): floats from one row of the block to the next
template <bool FWD, int NPOS, int CB = 64, int LD = CB>
__device__ __forceinline__ void build_weight_images(const float *__restrict__ Wst, uint4 *imgH, uint4 *imgL, float *winv, unsigned *wmax,
                                                    int tid) {
    constexpr int NC = CB / 16, NH = CB >= 32 ? CB / 32 : 1, E = NH * NC * 64;   // (CB = 16: one column half, columns 16..31 are zeros)
    static_assert(LD == CB || NPOS == 1, "a sub-block is built on its own");
    if (tid < NPOS) wmax[tid] = 0u;
    __syncthreads();
#pragma unroll 1
    for (int pos = 0; pos < NPOS; ++pos) {
        unsigned m = 0u;
        for (int i = tid; i < CB * CB; i += kSpThreads) {
            const unsigned b = __float_as_uint(Wst[LD == CB ? pos * CB * CB + i : (i / CB) * LD + i % CB]) & 0x7fffffffu;
            m = b > m ? b : m;
        }
        atomicMax(&wmax[pos], m);
    }
    __syncthreads();
    for (int t0 = tid; t0 < NPOS * E; t0 += kSpThreads) {
        const int pos = t0 / E, e = t0 % E;
        const int ln = e & 63, c = (e >> 6) % NC, nh = (e >> 6) / NC;
        const int t = pos * 512 + e;
        const int n = 32 * nh + (ln & 31), k0 = (CB / 2) * (ln >> 5) + 8 * c;
        float s, inv;
        pow2_scale(wmax[pos], &s, &inv);
        if (e == 0) winv[pos] = inv;
        const float *w = Wst + pos * CB * CB;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = n >= CB ? 0.f : FWD ? w[(k0 + j) * LD + n] : w[n * LD + k0 + j];
        unsigned hw[4], lw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            h2 h, l;
            split_pair(v[2 * j], v[2 * j + 1], s, &h, &l);
            hw[j] = __builtin_bit_cast(unsigned, h);
            lw[j] = __builtin_bit_cast(unsigned, l);
        }
        imgH[t] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
        imgL[t] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
    }
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
struct SplitImages {
    const float *Wst[kSpImgLevels];
    const float *X[kSpImgLevels];   // or null: no extra products
    uint4 *img[kSpImgLevels];   // [2 directions][kSpImgStride]
};
__global__ __launch_bounds__(kSpThreads) void smp_split_weight_images(SplitImages a, int C) {  // workgroup (direction, level, position)
    __shared__ unsigned wmax[1];
    uint4 *out = a.img[blockIdx.y] + (size_t)blockIdx.x * kSpImgStride;
    float *winv = reinterpret_cast<float *>(out + 2 * kSpAll) + blockIdx.z;
    if (blockIdx.z >= kSpStacked && !a.X[blockIdx.y]) return;   // (uniform)
    const float *w = blockIdx.z < kSpStacked ? a.Wst[blockIdx.y] + (size_t)blockIdx.z * C * C : a.X[blockIdx.y] + (size_t)(blockIdx.z - kSpStacked) * C * C;
    uint4 *H = out + blockIdx.z * 512, *L = out + kSpAll + blockIdx.z * 512;
    if (C == 64) {
        if (blockIdx.x == 0)
            build_weight_images<true, 1, 64>(w, H, L, winv, wmax, threadIdx.x);
        else
            build_weight_images<false, 1, 64>(w, H, L, winv, wmax, threadIdx.x);
    } else if (C == 16) {
        if (blockIdx.x == 0)
            build_weight_images<true, 1, 16>(w, H, L, winv, wmax, threadIdx.x);
        else
            build_weight_images<false, 1, 16>(w, H, L, winv, wmax, threadIdx.x);
    } else {
        if (blockIdx.x == 0)
            build_weight_images<true, 1, 32>(w, H, L, winv, wmax, threadIdx.x);
        else
            build_weight_images<false, 1, 32>(w, H, L, winv, wmax, threadIdx.x);
    }
}

// C = 128: every 128 x 128 block is four 64 x 64 sub-blocks, one image SET per (reduction half i, output half j) and level -- set q = 2 i + j
// at img + 2 q kSpImgStride128 (forward images, then backward images; positions 0..7 only: the row products', see kSpAll128).
// Forward, set (i, j) holds W[64 i .., 64 j ..]; backward it holds the transposed sub-block (W[64 j .., 64 i ..])^T, i.e. the one that takes
// columns [64 i, +64) of dO to columns [64 j, +64) of dT.  Workgroup (direction, level, 8 q + position).
__global__ __launch_bounds__(kSpThreads) void smp_split_weight_images_c128(SplitImages a) {
    __shared__ unsigned wmax[1];
    const int q = blockIdx.z >> 3, pos = blockIdx.z & 7, i = q >> 1, j = q & 1;
    uint4 *out = a.img[blockIdx.y] + (size_t)(2 * q + blockIdx.x) * kSpImgStride128;
    float *winv = reinterpret_cast<float *>(out + 2 * kSpAll128) + pos;
    const float *w = a.Wst[blockIdx.y] + (size_t)pos * 128 * 128;
    uint4 *H = out + pos * 512, *L = out + kSpAll128 + pos * 512;
    if (blockIdx.x == 0)
        build_weight_images<true, 1, 64, 128>(w + (size_t)64 * i * 128 + 64 * j, H, L, winv, wmax, threadIdx.x);
    else
        build_weight_images<false, 1, 64, 128>(w + (size_t)64 * j * 128 + 64 * i, H, L, winv, wmax, threadIdx.x);
}

// NF (round 5): factors per row in `rs` -- 2: (tot, tr) of the row's node; 8: one factor per stacked product 0..7, i.e. (tot, tot, tr, 1, 1,
// 1, 1, 1) times the node's slice-dropout factors of K0, K2, K6, K5, K9, K8, K12, K11 (RisiContraction_18_dropout: a dropped slice
// of the contraction is a zero factor on its block product, GraphFlow/RisiContraction_18_dropout.h:106-132)
#ifndef GF_SP_WHOLE_PANEL
#define GF_SP_WHOLE_PANEL 16   // (32: products-forward 0.36 -> 0.39 ms at C = 32)
#endif
// NX = 3 (CB <= 32, NF = 2): the extra products of SMP_2D_ver7 on the 18-slice level ride on the panel's fragments -- forward O_loc +=
// S_ab X_a + S_bc X_b + tr S_bc X_c, backward dS_ab += L X_a^T, dS_bc += L X_b^T + tr L X_c^T -- with the images of positions 18 .. 20
// CLS (the backward products with CB = 64, NF = 2, NX = 0, MASK and store_mask): panels of ONE row class.  `rcls` is the level's row-class
// buffer (smp_prepare.hip: row_class_count) -- the rows with S_ab / T6 data and the rows without as two padded lists of (row, packed
// word) -- and a wave's panel is 32 list entries: own-class panels run the full program and store every block, absent-class panels run
// products 4 and 1 + 6 of the eight (no dT6 / dS_ab product, no transposed dU, no store into the scratch rows).  A row's arithmetic
// does not depend on its panel: the results are the unclassed kernel's bit for bit.  Rows of a panel are no longer adjacent, so the
// stores take each row's address from the wave's LDS slot.  (The forward products lost on the same lists, 0.78 -> 0.99 ms: NOTES.md.)
// W = 2 (C = 128, CB = 64): one (i, j) pass of the four a 128 x 128 product is made of -- the rows are W times as wide, a block starts at
// CB W blk, and the pass reads columns [a_off, +64) of its operand blocks and writes columns [out_off, +64) of its output blocks with the
// weight images of sub-block (i, j).  ACC: the pass of the second reduction half -- its accumulators start from what the first pass stored.
// DZ (CLS): the L block of dO is not read.  At the top level of a plain model it is dz[row] = node_df[node(row)] * LeakyReLU'(z[row]) -- the
// read-out's vector of the row's node (dz.node_df, [nodes][64]: 4 MB at cfg3, L2 hits) times the slope from the row's sign words (dz.sgn,
// smp_combine_fwd_panels) -- and the kernel forms the lane's 32 floats itself: the same request shape, the operands and the product of
// combine-backward ((0 + v) * slope), the same bits.  dz.ent_node: the node of every class-list entry (smp_build_row_class_nodes).
template <bool FWD, bool MASK, int CB = 64, int NF = 2, int NX = 0, bool CLS = false, int W = 1, bool ACC = false, bool DZ = false>
__global__ __launch_bounds__(kSpThreads, 1) void smp_rowpanel_split(const float *__restrict__ A, const float *__restrict__ rs,
                                                                     const float *__restrict__ Wst, float *__restrict__ Out, int rows,
                                                                     const int *__restrict__ trow, int store_mask,
                                                                     const uint4 *__restrict__ wimg,    // or null: this direction's
                                                                     // images, built by smp_split_weight_images
                                                                     const int *__restrict__ rcls,      // CLS: the row classes
                                                                     int a_off, int out_off,            // W > 1: see above
                                                                     RowpanelDz dz) {                   // DZ: see above
    static_assert(W == 1 || (CB == 64 && NF == 2 && NX == 0 && !CLS), "sub-block passes: 64-channel panels, plain row factors");
    static_assert(!DZ || CLS, "dz formed in the kernel: the row-class panels");
    static_assert(W > 1 || !ACC, "");
    static_assert(!CLS || (!FWD && MASK && CB == 64 && NF == 2 && NX == 0), "row classes: the masked backward products at 64 channels");
    constexpr int LDA = (FWD ? 4 * CB : 2 * CB) * W, LDOUT = (FWD ? 2 * CB : 4 * CB) * W, BS = CB * W;   // BS: floats from a block to the next
    if constexpr (W == 1) a_off = out_off = 0;
    constexpr int ALL = W == 1 ? kSpAll : kSpAll128;   // entries of one half's images in the prebuilt set
    // values per lane and block, k-chunks, column halves, fragment entries per block.  CB = 16 (round 5: models of up to 16 channels, the
    // reference's own nChanels = 10): one k-chunk, one column half whose columns 16..31 are zero weights and are never stored
    constexpr int VPL = CB / 2, NC = CB / 16, NH = CB >= 32 ? CB / 32 : 1, E = NH * NC * 64;
    auto t_row = [](int t) { return MASK ? (t & 0x1fffffff) : t; };
    auto t_own = [](int t) { return MASK ? t < 0 : true; };
    auto t_tr = [](int t) { return MASK ? ((t >> 30) & 1) != 0 : true; };
    auto t_bc = [](int t) { return MASK ? ((t >> 29) & 1) != 0 : true; };   // the row's S_bc / T10 blocks hold data
    static_assert(NX == 0 || (NX == 3 && CB <= 32 && NF == 2), "the extra products: prebuilt images, plain row factors");
    constexpr int NP = 8 + NX;   // weight images in LDS
    // FWD with store_mask (the plain 64-channel program only): the rows of O without data in ANY block of T -- none of the three bits, exact
    // zeros that combine-forward does not request either (FusedRoute::skip_empty) -- go to the scratch rows, like the dS_ab / dT6 rows backward
    constexpr bool FWD_ROWMASK = FWD && MASK && CB == 64 && NF == 2 && NX == 0 && W == 1;
    extern __shared__ __attribute__((aligned(16))) uint4 sp_smem[];
    uint4 *imgH = sp_smem, *imgL = sp_smem + NP * E;
    float *winv = reinterpret_cast<float *>(sp_smem + 2 * NP * E);  // [NP] 2^-k of the weight blocks (padded to 16 floats)
    unsigned *wmax = reinterpret_cast<unsigned *>(winv + 16);       // [8]
    float *facs = winv + 32;                                        // [waves][32]: row factors on their way to the C layout
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int wave = tid >> 6;
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    unsigned long long *rowp = reinterpret_cast<unsigned long long *>(facs + (kSpThreads / 64) * 32);   // CLS: [waves][32] where the rows of the wave's panel are stored

    // ---- weight images (see build_weight_images): copied from the pass's prebuilt ones, or built here
    if (wimg) {
        for (int t = tid; t < NP * E; t += kSpThreads) {   // (512 entries apart per position in the prebuilt set, whatever CB is)
            const int pos = t / E, g = (pos < 8 ? pos : kSpStacked + pos - 8) * 512 + t % E;
            imgH[t] = wimg[g];
            imgL[t] = wimg[ALL + g];
        }
        if (tid < 2) reinterpret_cast<uint4 *>(winv)[tid] = wimg[2 * ALL + tid];
        if (NX > 0 && tid < NX) winv[8 + tid] = reinterpret_cast<const float *>(wimg + 2 * kSpAll)[kSpStacked + tid];
    } else {
        static_assert(E == 512 || true, "");
        if constexpr (CB == 64) build_weight_images<FWD, 8>(Wst, imgH, imgL, winv, wmax, tid);   // (other channel counts: prebuilt images only)
    }
    __syncthreads();

    const int npanels = (rows + 31) / 32;
    const int nwaves = gridDim.x * (kSpThreads / 64);
    float *myfac = facs + wave * 32;

    struct Raw {
        f4v a[VPL / 4];
    };
    struct Spl {
        uint4 h[NC], l[NC];  // eight f16 each
    };
    // columns [64 blk + 32 lh, +32) of row `li` of panel p, or of the given row (the transposed one).  Rows past the end read the
    // last row instead (unconditional loads: no branch per request); what is computed from them is never stored.
    auto load_raw_at = [&](Raw &R, int src_row, int blk, bool present) {
        __builtin_amdgcn_sched_barrier(0);  // (requests stay where the schedule below puts them: hoisted to the top of the panel
                                            //  they would all be live at once)
        asm volatile("" : "+v"(src_row));   // (nor is the address arithmetic on a prefetched row index moved up to its load)
        // (a select on the address: same requests, same registers.  Made on the address as an INTEGER and turned into a global pointer
        //  afterwards -- see the rule at sp_zero_page.  A select between two global POINTERS gives the same loads, but the compiler then
        //  re-associates the address arithmetic around it and the panel spills: 104 -> 284 bytes of scratch per lane forward, none -> 96
        //  in the row-class backward kernel.)
        unsigned long long sa = (unsigned long long)(A + (size_t)src_row * LDA + blk * BS + a_off + VPL * lh);
        if constexpr (MASK) sa = present ? sa : (unsigned long long)sp_zero_page;
        const GF_GLOBAL float *src = (const GF_GLOBAL float *)sa;
#pragma unroll
        for (int q = 0; q < VPL / 4; ++q) R.a[q] = gf_ld_g<1>(reinterpret_cast<const GF_GLOBAL f4v *>(src + 4 * q));
        __builtin_amdgcn_sched_barrier(0);
    };
    auto load_raw = [&](Raw &R, int p, int blk, bool present) {
        const int row = p * 32 + li;
        load_raw_at(R, row < rows ? row : rows - 1, blk, present);
    };
    // The transposed row of the lane's row of panel p.  Requested a panel ahead of the block request that uses it: a request
    // that waits for its own index waits for everything the wave has in flight before it (loads and stores return in order).
    auto fetch_trow = [&](int p) {
        const int row = p * 32 + li;
        return trow[row < rows ? row : rows - 1];
    };
    struct RowFac {   // the eight products' row factors (NF == 2: the ones are compile-time constants)
        float f[8];
    };
    auto load_scale = [&](int p) {
        int row = p * 32 + li;
        row = row < rows ? row : rows - 1;
        RowFac r;
        if constexpr (NF == 8) {
            const f4v a = *reinterpret_cast<const f4v *>(rs + (size_t)row * 8), b = *reinterpret_cast<const f4v *>(rs + (size_t)row * 8 + 4);
            r.f[0] = a[0], r.f[1] = a[1], r.f[2] = a[2], r.f[3] = a[3], r.f[4] = b[0], r.f[5] = b[1], r.f[6] = b[2], r.f[7] = b[3];
        } else {
            const float2 t = *reinterpret_cast<const float2 *>(rs + (size_t)row * 2);
            r.f[0] = r.f[1] = t.x, r.f[2] = t.y;
            r.f[3] = r.f[4] = r.f[5] = r.f[6] = r.f[7] = 1.f;
        }
        return r;
    };
    // raw block -> halves at the row's exponent (one exponent for the 64 columns of the row: both lane halves agree on it);
    // MFMA c takes the lane's columns [8 c, 8 c + 8) as k = 8 (lane >> 5) + j
    auto split_blk = [&](const Raw &R, Spl &S, float &inv) {
        __builtin_amdgcn_sched_barrier(0);  // (not earlier than written: a block split ahead of time is 32 more live registers)
        unsigned m = 0u;
#pragma unroll
        for (int q = 0; q < VPL / 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned b = __float_as_uint(R.a[q][j]) & 0x7fffffffu;
                m = b > m ? b : m;
            }
        const unsigned mo = (unsigned)__shfl_xor((int)m, 32);
        m = mo > m ? mo : m;
        float s;
        pow2_scale(m, &s, &inv);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            unsigned hw[4], lw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h2 h, l;
                const f4v v = R.a[2 * c + (j >> 1)];
                split_pair(v[2 * (j & 1)], v[2 * (j & 1) + 1], s, &h, &l);
                hw[j] = __builtin_bit_cast(unsigned, h);
                lw[j] = __builtin_bit_cast(unsigned, l);
            }
            S.h[c] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
            S.l[c] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // acc (two column halves) += rowfac * (S x block wpos).  `rowfac` is the lane's row factor (row li); the C/D layout of the
    // 32 x 32 MFMA wants it at rows (r & 3) + 8 (r >> 2) + 4 lh: through the wave's 32 floats of LDS (a wave's DS operations
    // execute in order).
    auto prod = [&](const Spl &S, float rowfac, int wpos, f16v &acc0, f16v &acc1) {
        __builtin_amdgcn_wave_barrier();
        myfac[li] = rowfac * winv[wpos];  // (both lane halves hold the row's factor: same value, same address, no branch)
        __builtin_amdgcn_wave_barrier();
        const uint4 *bh = imgH + (size_t)wpos * E + lane, *bl = imgL + (size_t)wpos * E + lane;
        // one column half at a time (sixteen registers of products in flight, not thirty-two: the panel's operand blocks and the
        // requests behind them take the rest of the wave's 256)
#pragma unroll
        for (int nh = 0; nh < NH; ++nh) {
            f16v t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0.f;
            // the cross products (low halves at 2^11, see split_pair) ...
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const h8 bhc = __builtin_bit_cast(h8, bh[(NC * nh + c) * 64]), blc = __builtin_bit_cast(h8, bl[(NC * nh + c) * 64]);
                const h8 ah = __builtin_bit_cast(h8, S.h[c]), al = __builtin_bit_cast(h8, S.l[c]);
                t = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bhc, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, blc, t, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] *= kLowUnscale;
            // ... and the main product on top, one dependent chain (its B fragments are read again: four more ds_read_b128, no
            // registers held; as two independent chains the compiler interleaved them and spilled hundreds of registers)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const h8 bhc = __builtin_bit_cast(h8, bh[(NC * nh + c) * 64]);
                const h8 ah = __builtin_bit_cast(h8, S.h[c]);
                t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bhc, t, 0, 0, 0);
            }
            f16v &acc = nh ? acc1 : acc0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f4v fac = *reinterpret_cast<const f4v *>(myfac + 8 * g + 4 * lh);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // (The masked and the plain build of a kernel must give the same bits, and every build the bits it always gave.  The
                    //  compiler contracts this update as it likes: it fuses all of them except two to ten per forward 32-channel build, in
                    //  both of its builds alike -- but with the masked operands loaded from global pointers it split four of them in
                    //  the masked 16-channel backward builds alone.  Those builds fuse by name, as they always compiled; the others keep
                    //  the expression they were built from.  tests/test_masked_operand_paths_gpu.py compares the pairs bit for bit.)
                    if constexpr (!FWD && CB == 16) acc[4 * g + j] = __builtin_fmaf(t[4 * g + j], fac[j], acc[4 * g + j]);
                    else acc[4 * g + j] += t[4 * g + j] * fac[j];
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    auto clear = [&](f16v &acc0, f16v &acc1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
    };
    // the accumulators of output block o of panel p at the start of its products: zeros, or (ACC) what the pass of the first reduction
    // half stored there -- the same elements this lane stores at the end (a row the masked store sends to the scratch rows is read all the
    // same: its sum goes nowhere)
    auto start = [&](int p, int o, f16v &acc0, f16v &acc1, auto full) {
        if constexpr (!ACC) {
            clear(acc0, acc1);
        } else {
            const int r0 = p * 32;
            const float *out = Out + (size_t)(r0 + 4 * lh) * LDOUT + o * BS + out_off + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2);
                const bool ok = decltype(full)::value || r0 + 4 * lh + rr < rows;
                acc0[r] = ok ? out[(size_t)rr * LDOUT] : 0.f;
                acc1[r] = ok ? out[(size_t)rr * LDOUT + 32] : 0.f;
            }
        }
    };
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    // (FULL: a panel wholly inside the matrix -- unconditional stores.  A conditional store or load anywhere in the panel loop
    //  makes the compiler give up counting the memory queue at the join: it then waits for vmcnt(0), requests just issued included,
    //  before every split.  The one partial panel of the matrix runs a second copy of the panel code.)
    auto store_out = [&](int p, int o, const f16v &acc0, const f16v &acc1, auto full, unsigned rowbits = 0xffffffffu) {
        const int r0 = p * 32;
        GF_GLOBAL float *out = gf_global(Out) + (size_t)(r0 + 4 * lh) * LDOUT + o * BS + out_off + li;
        if constexpr (CB < 32)   // lanes of the zero columns store into the scratch rows (a select on the address: every store is issued)
            out = li < CB ? out : gf_global(sp_dump) + (size_t)((r0 & 255) + 4 * lh) * 64 + li;
        if constexpr (MASK && (!FWD || FWD_ROWMASK) && decltype(full)::value) {
            if (rowbits != 0xffffffffu) {  // (uniform; the blocks without structural zeros pass all ones)
                // rows without data go to the scratch rows: a select on the address, every store is issued
                const unsigned mine = rowbits >> (4 * lh);
                GF_GLOBAL float *dump = gf_global(sp_dump) + (size_t)((r0 & 255) + 4 * lh) * 64 + li;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = (r & 3) + 8 * (r >> 2);
                    GF_GLOBAL float *dst = ((mine >> rr) & 1u) ? out + (size_t)rr * LDOUT : dump + rr * 64;
                    gf_st_g<2>(dst, acc0[r]);
                    if constexpr (NH == 2) gf_st_g<2>(dst + 32, acc1[r]);
                }
                return;
            }
        }
        if constexpr (decltype(full)::value) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2);
                gf_st_g<2>(out + (size_t)rr * LDOUT, acc0[r]);
                if constexpr (NH == 2) gf_st_g<2>(out + (size_t)rr * LDOUT + 32, acc1[r]);
            }
        } else {
            // (the partial panel skips the rows without data as the full ones do: until the stand-alone operator's test looked, it
            //  stored them -- numbers no consumer reads, but "not written" then held for every row except the level's last few)
            const unsigned mine = (MASK && (!FWD || FWD_ROWMASK)) ? rowbits >> (4 * lh) : 0xffffffffu;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2);
                if (r0 + 4 * lh + rr < rows && li < CB && ((mine >> rr) & 1u)) {
                    gf_st_g<2>(out + (size_t)rr * LDOUT, acc0[r]);
                    if constexpr (NH == 2) gf_st_g<2>(out + (size_t)rr * LDOUT + 32, acc1[r]);
                }
            }
        }
    };

    // One panel.  On entry Ra and Rb hold (requests for) the panel's first two blocks; every other block is requested as soon as
    // a raw buffer has been split, one to three products (0.4 - 1 us) ahead of its use, and the first two blocks of the wave's
    // next panel go out behind the panel's last ones.
    int tnext = CLS ? 0 : fetch_trow(blockIdx.x * (kSpThreads / 64) + wave);   // (CLS: the class lists carry the packed words)
    auto panel = [&](int p, Raw &Ra, Raw &Rb, auto full) {
        const int pn = p + nwaves;
        const int tcur = tnext;   // the transposed rows of this panel's rows (requested during the previous panel)
        tnext = fetch_trow(pn);
        const RowFac sc = load_scale(p);  // (used after the panel's first products)
        f16v acc0, acc1;
        Spl X, Y, Z;
        float iX, iY, iZ;
        if (FWD) {  // T blocks: 0 S_ab, 1 S_bc, 2 T6, 3 T10; outputs: 0 O_loc, 1 U.  Entry: Ra = S_ab, Rb = S_ab at the transposed rows
            const unsigned rowbits = (FWD_ROWMASK && store_mask) ? (unsigned)__ballot((tcur & 0xe0000000) != 0) : 0xffffffffu;
            split_blk(Ra, X, iX);
            load_raw(Ra, p, 1, t_bc(tcur));          // S_bc
            split_blk(Rb, Z, iZ);
            load_raw(Rb, p, 2, t_own(tcur));         // T6
            start(p, 1, acc0, acc1, full);
            prod(X, iX * sc.f[5], 5, acc0, acc1);
            prod(Z, iZ * sc.f[7], 7, acc0, acc1);
            split_blk(Ra, Y, iY);
            prod(Y, iY * sc.f[6], 6, acc0, acc1);
            store_out(p, 1, acc0, acc1, full, rowbits);
            start(p, 0, acc0, acc1, full);
            prod(X, iX * sc.f[0], 0, acc0, acc1);
            prod(X, iX * sc.f[2], 2, acc0, acc1);
            prod(Y, iY * sc.f[1], 1, acc0, acc1);
            if constexpr (NX == 3) {
                prod(X, iX, 8, acc0, acc1);
                prod(Y, iY, 9, acc0, acc1);
                prod(Y, iY * sc.f[2], 10, acc0, acc1);
            }
            load_raw(Ra, p, 3, t_bc(tcur));          // T10, once X and Y are dead: with two requests beside them the panel spills,
                                                     // and a scratch reload waits for the whole memory queue
            split_blk(Rb, Z, iZ);
            load_raw_at(Rb, t_row(tnext), 0, t_tr(tnext));   // S_ab of the next panel at its transposed rows
            prod(Z, iZ * sc.f[3], 3, acc0, acc1);
            split_blk(Ra, Z, iZ);
            load_raw(Ra, pn, 0, t_own(tnext));       // S_ab of the next panel
            prod(Z, iZ * sc.f[4], 4, acc0, acc1);
            store_out(p, 0, acc0, acc1, full, rowbits);
        } else {    // dO blocks: 0 L, 1 dU; outputs: 0 dS_ab, 1 dS_bc, 2 dT6, 3 dT10.  Entry: Ra = L, Rb = dU
            split_blk(Ra, X, iX);
            split_blk(Rb, Y, iY);
            // (rows whose S_ab / T6 blocks are structural zeros: bit i = row i of the panel has data; both lane halves hold the row's
            //  entry, the low word of the ballot is the panel's)
            // (the dS_bc / dT10 blocks of rows no source covers are stored all the same -- 8 % of the rows at level 3: masking them as
            //  well cost the kernel fifteen spills and more than it saved, 0.84 -> 0.91 ms)
            const unsigned rowbits = (MASK && store_mask) ? (unsigned)__ballot(t_own(tcur)) : 0xffffffffu;
            start(p, 2, acc0, acc1, full);
            prod(X, iX * sc.f[3], 3, acc0, acc1);
            store_out(p, 2, acc0, acc1, full, rowbits);
            start(p, 3, acc0, acc1, full);
            prod(X, iX * sc.f[4], 4, acc0, acc1);
            store_out(p, 3, acc0, acc1, full);
            start(p, 1, acc0, acc1, full);
            prod(X, iX * sc.f[1], 1, acc0, acc1);
            prod(Y, iY * sc.f[6], 6, acc0, acc1);
            if constexpr (NX == 3) {
                prod(X, iX, 9, acc0, acc1);
                prod(X, iX * sc.f[2], 10, acc0, acc1);
            }
            store_out(p, 1, acc0, acc1, full);
            // dU at the transposed rows: it only feeds dS_ab of this row, which is not stored where the row has no data.  (Requested
            // here, six products ahead of its use, not at the top of the panel: with the cross-product chain of round 4 the block's
            // thirty-two registers no longer fit beside X, Y and the first accumulators -- the compiler spilled twelve of them in the loop.)
            load_raw_at(Ra, t_row(tcur), 1, !(MASK && store_mask) || t_own(tcur));
            load_raw(Rb, pn, 1, !(MASK && store_mask) || t_bc(tnext));   // dU of the next panel (a row no source covers has nothing to
                                                                         // back-propagate: its whole dT row is a gradient of structural zeros)
            start(p, 0, acc0, acc1, full);
            prod(X, iX * sc.f[0], 0, acc0, acc1);
            prod(X, iX * sc.f[2], 2, acc0, acc1);
            prod(Y, iY * sc.f[5], 5, acc0, acc1);
            if constexpr (NX == 3) prod(X, iX, 8, acc0, acc1);
            split_blk(Ra, Z, iZ);
            load_raw(Ra, pn, 0, !(MASK && store_mask) || t_bc(tnext));   // L of the next panel
            prod(Z, iZ * sc.f[7], 7, acc0, acc1);
            store_out(p, 0, acc0, acc1, full, rowbits);
        }
    };
    if constexpr (CLS) {
        const int n_own_p = (rcls[0] + 31) >> 5, n_tot_p = n_own_p + ((rcls[1] + 31) >> 5), n_ent = 32 * n_tot_p;
        const int2 *ent = reinterpret_cast<const int2 *>(rcls + 4);
        unsigned long long *myrow = rowp + wave * 32;
        // the lane's entry of panel q (panels past the end read the last entry: requests made for them are never used): the packed
        // word, and through *rw the row with bit 31 set on a padding entry.  Fetched a panel ahead, like fetch_trow -- and the row with it,
        // so no block request waits for an index.
        int nd_next = 0;   // DZ: the node of the lane's row of the next panel, fetched with its entry
        auto fetch_entry = [&](int q, int *rw) {
            const int i = q * 32 + li;
            const int2 e = ent[i < n_ent ? i : n_ent - 1];
            if constexpr (DZ) nd_next = dz.ent_node[i < n_ent ? i : n_ent - 1];
            *rw = e.x;
            return e.y;
        };
        // DZ: the request for block L of `row` becomes the lane's 32 floats of the node's vector (a row no source covers: the zero page, as
        // load_raw_at) and the row's sign word of the lane's column half; dz_scale turns them into dz when the block is split
        unsigned sg_next = 0u;
        auto load_L_at = [&](Raw &R, int row, bool present) {
            if constexpr (!DZ) {
                load_raw_at(R, row, 0, present);
            } else {
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("" : "+v"(row));
                unsigned long long sa = (unsigned long long)(dz.node_df + (size_t)nd_next * CB + VPL * lh);
                sa = present ? sa : (unsigned long long)sp_zero_page;
                const GF_GLOBAL float *src = (const GF_GLOBAL float *)sa;
#pragma unroll
                for (int q = 0; q < VPL / 4; ++q) R.a[q] = gf_ld_g<1>(reinterpret_cast<const GF_GLOBAL f4v *>(src + 4 * q));
                sg_next = dz.sgn[(size_t)row * 2 + lh];
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto dz_scale = [&](Raw &R, unsigned sg) {
            if constexpr (DZ) {
#pragma unroll
                for (int q = 0; q < VPL / 4; ++q)
#pragma unroll
                    for (int j = 0; j < 4; ++j) R.a[q][j] = (0.f + R.a[q][j]) * (((sg >> (4 * q + j)) & 1u) ? 1.f : 0.01f);
            }
        };
        auto e_row = [](int rw) { return rw & 0x1fffffff; };
        auto scale_at = [&](int row) {
            const float2 t = *reinterpret_cast<const float2 *>(rs + (size_t)row * 2);
            RowFac r;
            r.f[0] = r.f[1] = t.x, r.f[2] = t.y;
            r.f[3] = r.f[4] = r.f[5] = r.f[6] = r.f[7] = 1.f;
            return r;
        };
        // where the lane's row is stored (a padding entry: one of the scratch rows), on its way to the C/D layout like the row factors
        auto post_rows = [&](int rw) {
            __builtin_amdgcn_wave_barrier();
            myrow[li] = (unsigned long long)(rw < 0 ? gf_global(sp_dump) + li * 64 : gf_global(Out) + (size_t)e_row(rw) * LDOUT);
            __builtin_amdgcn_wave_barrier();
        };
        auto store_rows = [&](int o, const f16v &acc0, const f16v &acc1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u64x2 a = *reinterpret_cast<const u64x2 *>(myrow + 8 * g + 4 * lh), b = *reinterpret_cast<const u64x2 *>(myrow + 8 * g + 4 * lh + 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    // (an address that went through LDS is an integer: rebuilt as a GLOBAL pointer, see gf_global)
                    GF_GLOBAL float *dst = (GF_GLOBAL float *)(j < 2 ? a[j & 1] : b[j & 1]) + o * CB + li;
                    gf_st_g<2>(dst, acc0[4 * g + j]);
                    gf_st_g<2>(dst + 32, acc1[4 * g + j]);
                }
            }
        };
        int p = blockIdx.x * (kSpThreads / 64) + wave;
        int rnext, tn = fetch_entry(p, &rnext);
        Raw Ra, Rb;   // on entry of a panel: Ra = L, Rb = dU (of a row no source covers: zeros, see `panel`)
        load_raw_at(Rb, e_row(rnext), 1, t_bc(tn));
        load_L_at(Ra, e_row(rnext), t_bc(tn));
        auto panel_own = [&](int q) {   // the program of `panel` below, its rows taken from the list; every row stores all four blocks
            const int qn = q + nwaves, rcur = rnext, tcur = tn;
            const unsigned sg = sg_next;
            tn = fetch_entry(qn, &rnext);
            const RowFac sc = scale_at(e_row(rcur));
            post_rows(rcur);
            f16v acc0, acc1;
            Spl X, Y, Z;
            float iX, iY, iZ;
            dz_scale(Ra, sg);
            split_blk(Ra, X, iX);
            split_blk(Rb, Y, iY);
            clear(acc0, acc1);
            prod(X, iX * sc.f[3], 3, acc0, acc1);
            store_rows(2, acc0, acc1);
            clear(acc0, acc1);
            prod(X, iX * sc.f[4], 4, acc0, acc1);
            store_rows(3, acc0, acc1);
            clear(acc0, acc1);
            prod(X, iX * sc.f[1], 1, acc0, acc1);
            prod(Y, iY * sc.f[6], 6, acc0, acc1);
            store_rows(1, acc0, acc1);
            load_raw_at(Ra, t_row(tcur), 1, t_own(tcur));  // dU at the transposed rows
            load_raw_at(Rb, e_row(rnext), 1, t_bc(tn));    // dU of the next panel
            clear(acc0, acc1);
            prod(X, iX * sc.f[0], 0, acc0, acc1);
            prod(X, iX * sc.f[2], 2, acc0, acc1);
            prod(Y, iY * sc.f[5], 5, acc0, acc1);
            split_blk(Ra, Z, iZ);
            load_L_at(Ra, e_row(rnext), t_bc(tn));         // L of the next panel
            prod(Z, iZ * sc.f[7], 7, acc0, acc1);
            store_rows(0, acc0, acc1);
        };
        auto panel_absent = [&](int q) {   // rows whose S_ab / T6 blocks are structural zeros: dT10 = 4 and dS_bc = 1 + 6 are all they store
            const int qn = q + nwaves, rcur = rnext;
            const unsigned sg = sg_next;
            tn = fetch_entry(qn, &rnext);
            const RowFac sc = scale_at(e_row(rcur));
            post_rows(rcur);
            f16v acc0, acc1;
            Spl X, Y;
            float iX, iY;
            dz_scale(Ra, sg);
            split_blk(Ra, X, iX);
            split_blk(Rb, Y, iY);
            load_raw_at(Rb, e_row(rnext), 1, t_bc(tn));
            load_L_at(Ra, e_row(rnext), t_bc(tn));
            clear(acc0, acc1);
            prod(X, iX * sc.f[4], 4, acc0, acc1);
            store_rows(3, acc0, acc1);
            clear(acc0, acc1);
            prod(X, iX * sc.f[1], 1, acc0, acc1);
            prod(Y, iY * sc.f[6], 6, acc0, acc1);
            store_rows(1, acc0, acc1);
        };
        // own panels first, absent panels (three products of eight, two stores of four) behind them, dealt from one range: the
        // workgroups stay balanced
        for (; p < n_own_p; p += nwaves) panel_own(p);
        for (; p < n_tot_p; p += nwaves) panel_absent(p);
        return;
    }
    if constexpr (CB <= GF_SP_WHOLE_PANEL) {
        // Sixteen channels (round 5): an operand block is 2 KB per wave and eight registers per lane, so two blocks in flight per wave
        // (what the schedule above keeps at 64 channels, where a block is 8 KB) leave the memory system idle -- 3 TB/s.  Here ALL of
        // a panel's blocks are requested one panel ahead (five raw buffers forward, three backward: forty / twenty-four registers), and
        // the transposed-row indices two panels ahead, so that no request waits behind the previous panel's stores.
        constexpr int NB = FWD ? 5 : 3;
        Raw R[NB];
        int p = blockIdx.x * (kSpThreads / 64) + wave;
        int t1 = tnext, t2 = fetch_trow(p + nwaves);   // of panel p, of the panel after it
        auto request = [&](int q, int t) {   // every block of panel q, whose packed transposed-row entries are t
            if constexpr (FWD) {
                load_raw(R[0], q, 0, t_own(t));
                load_raw_at(R[1], t_row(t), 0, t_tr(t));
                load_raw(R[2], q, 1, t_bc(t));
                load_raw(R[3], q, 2, t_own(t));
                load_raw(R[4], q, 3, t_bc(t));
            } else {
                const bool all = !(MASK && store_mask);
                load_raw(R[0], q, 0, all || t_bc(t));
                load_raw(R[1], q, 1, all || t_bc(t));
                load_raw_at(R[2], t_row(t), 1, all || t_own(t));
            }
        };
        auto panel16 = [&](int q, auto full) {
            const int qn = q + nwaves;
            const int tcur = t1;
            t1 = t2;
            t2 = fetch_trow(qn + nwaves);
            const RowFac sc = load_scale(q);
            Spl S[NB];
            float iv[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) split_blk(R[b], S[b], iv[b]);
            request(qn, t1);
            f16v acc0, acc1;
            if constexpr (FWD) {   // S: S_ab, S_ab at the transposed rows, S_bc, T6, T10
                clear(acc0, acc1);
                prod(S[0], iv[0] * sc.f[5], 5, acc0, acc1);
                prod(S[1], iv[1] * sc.f[7], 7, acc0, acc1);
                prod(S[2], iv[2] * sc.f[6], 6, acc0, acc1);
                store_out(q, 1, acc0, acc1, full);
                clear(acc0, acc1);
                prod(S[0], iv[0] * sc.f[0], 0, acc0, acc1);
                prod(S[0], iv[0] * sc.f[2], 2, acc0, acc1);
                prod(S[2], iv[2] * sc.f[1], 1, acc0, acc1);
                if constexpr (NX == 3) {
                    prod(S[0], iv[0], 8, acc0, acc1);
                    prod(S[2], iv[2], 9, acc0, acc1);
                    prod(S[2], iv[2] * sc.f[2], 10, acc0, acc1);
                }
                prod(S[3], iv[3] * sc.f[3], 3, acc0, acc1);
                prod(S[4], iv[4] * sc.f[4], 4, acc0, acc1);
                store_out(q, 0, acc0, acc1, full);
            } else {               // S: L, dU, dU at the transposed rows
                const unsigned rowbits = (MASK && store_mask) ? (unsigned)__ballot(t_own(tcur)) : 0xffffffffu;
                clear(acc0, acc1);
                prod(S[0], iv[0] * sc.f[3], 3, acc0, acc1);
                store_out(q, 2, acc0, acc1, full, rowbits);
                clear(acc0, acc1);
                prod(S[0], iv[0] * sc.f[4], 4, acc0, acc1);
                store_out(q, 3, acc0, acc1, full);
                clear(acc0, acc1);
                prod(S[0], iv[0] * sc.f[1], 1, acc0, acc1);
                prod(S[1], iv[1] * sc.f[6], 6, acc0, acc1);
                if constexpr (NX == 3) {
                    prod(S[0], iv[0], 9, acc0, acc1);
                    prod(S[0], iv[0] * sc.f[2], 10, acc0, acc1);
                }
                store_out(q, 1, acc0, acc1, full);
                clear(acc0, acc1);
                prod(S[0], iv[0] * sc.f[0], 0, acc0, acc1);
                prod(S[0], iv[0] * sc.f[2], 2, acc0, acc1);
                if constexpr (NX == 3) prod(S[0], iv[0], 8, acc0, acc1);
                prod(S[1], iv[1] * sc.f[5], 5, acc0, acc1);
                prod(S[2], iv[2] * sc.f[7], 7, acc0, acc1);
                store_out(q, 0, acc0, acc1, full, rowbits);
            }
        };
        request(p, t1);
        const int nfull16 = rows / 32;
        for (; p < nfull16; p += nwaves) panel16(p, std::true_type{});
        if (p < npanels) panel16(p, std::false_type{});
        return;
    }
    Raw R0, R1;
    int p = blockIdx.x * (kSpThreads / 64) + wave;
    load_raw(R0, p, 0, FWD ? t_own(tnext) : (!(MASK && store_mask) || t_bc(tnext)));
    if (FWD) load_raw_at(R1, t_row(tnext), 0, t_tr(tnext));
    else load_raw(R1, p, 1, !(MASK && store_mask) || t_bc(tnext));
    const int nfull = rows / 32;
    for (; p < nfull; p += nwaves) panel(p, R0, R1, std::true_type{});
    if (p < npanels) panel(p, R0, R1, std::false_type{});  // (the matrix's partial last panel: one wave of the grid)
}


// ---------------------------------------------------------------------------------------------------------------
// The small products of a level on the same machinery (round 3): per-(node,x) vectors, per-node scalars and the compact
// diagonal rows are [pairs | nodes | pairs of the level below] x 64..256 operands -- as 128-row tiles of the fp32 tile GEMM they
// were one latency chain of K / 32 steps per workgroup (40 us per launch at level 1 for 10 us of bytes).  Here a wave takes a
// 32-row panel, requests its whole operand at once, and multiplies from registers against weight images copied from the pass's
// prebuilt set (positions pos0.. of this direction).
//   PROG 0  Out[rows][64]          = sum_k In[rows][64 k ..] W_k      (k < 4)   Vout = Vt [K1;K3;K7;K10],  Sout = St [K4;K13;K14;K17]
//   PROG 1  Out[rows][64 k ..]     = In[rows][64] W_k^T               (k < 4)   dVt = dVout W^T,  dSt = dSout W^T   (transposed images)
//   PROG 2  Out[rows][64 k ..]     = In[rows][64 k ..] W_k            (k < 2)   Gc = [Fd K15 | Fc K16];  dFdc with the transposed images
// ---------------------------------------------------------------------------------------------------------------
constexpr int kSmThreads = 256;
// up to three products in ONE launch (a level's V, S and compact products: 17,000-row jobs are one round of latencies each, and
// three launches paid it three times): workgroups [wg0, wg0 + nwg) run job j
struct SmallJobs {
    const float *In[3];
    float *Out[3];
    int rows[3], pos0[3], prog[3], wg0[3], nwg[3];
    int n;
};
template <int PROG, int CB = 64>
__device__ __forceinline__ void small_split_body(const float *__restrict__ In, float *__restrict__ Out, int rows,
                                                 const uint4 *__restrict__ wimg, int pos0, int wg, int nwg) {
    constexpr int NPOS = PROG == 2 ? 2 : 4;
    constexpr int LDA = PROG == 0 ? 4 * CB : PROG == 1 ? CB : 2 * CB, LDOUT = PROG == 0 ? CB : PROG == 1 ? 4 * CB : 2 * CB;
    constexpr int VPL = CB / 2, NC = CB / 16, NH = CB >= 32 ? CB / 32 : 1, E = NH * NC * 64;   // (see smp_rowpanel_split)
    constexpr int NIN = PROG == 1 ? 1 : NPOS;
    extern __shared__ __attribute__((aligned(16))) uint4 sm_smem[];
    uint4 *imgH = sm_smem, *imgL = sm_smem + NPOS * E;
    float *winv = reinterpret_cast<float *>(sm_smem + 2 * NPOS * E);  // [NPOS] (room for 16)
    float *facs = winv + 16;                                             // [waves][32]
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lh = lane >> 5, wave = tid >> 6;
    for (int t = tid; t < NPOS * E; t += kSmThreads) {   // (512 entries apart per position in the prebuilt set)
        const int g = (pos0 + t / E) * 512 + t % E;
        imgH[t] = wimg[g];
        imgL[t] = wimg[kSpAll + g];
    }
    if (tid < NPOS) winv[tid] = reinterpret_cast<const float *>(wimg + 2 * kSpAll)[pos0 + tid];
    __syncthreads();
    float *myfac = facs + wave * 32;
    struct Raw {
        f4v a[VPL / 4];
    };
    struct Spl {
        uint4 h[NC], l[NC];
    };
    auto split_blk = [&](const Raw &R, Spl &S, float &inv) {
        unsigned m = 0u;
#pragma unroll
        for (int q = 0; q < VPL / 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned b = __float_as_uint(R.a[q][j]) & 0x7fffffffu;
                m = b > m ? b : m;
            }
        const unsigned mo = (unsigned)__shfl_xor((int)m, 32);
        m = mo > m ? mo : m;
        float sc;
        pow2_scale(m, &sc, &inv);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            unsigned hw[4], lw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h2 h, l;
                const f4v v = R.a[2 * c + (j >> 1)];
                split_pair(v[2 * (j & 1)], v[2 * (j & 1) + 1], sc, &h, &l);
                hw[j] = __builtin_bit_cast(unsigned, h);
                lw[j] = __builtin_bit_cast(unsigned, l);
            }
            S.h[c] = make_uint4(hw[0], hw[1], hw[2], hw[3]);
            S.l[c] = make_uint4(lw[0], lw[1], lw[2], lw[3]);
        }
    };
    auto prod = [&](const Spl &S, float rowfac, int wpos, f16v &acc0, f16v &acc1) {
        __builtin_amdgcn_wave_barrier();
        myfac[li] = rowfac * winv[wpos];
        __builtin_amdgcn_wave_barrier();
        const uint4 *bh = imgH + (size_t)wpos * E + lane, *bl = imgL + (size_t)wpos * E + lane;
#pragma unroll
        for (int nh = 0; nh < NH; ++nh) {
            f16v t;
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] = 0.f;
            // the cross products (low halves at 2^11, see split_pair) ...
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const h8 bhc = __builtin_bit_cast(h8, bh[(NC * nh + c) * 64]), blc = __builtin_bit_cast(h8, bl[(NC * nh + c) * 64]);
                const h8 ah = __builtin_bit_cast(h8, S.h[c]), al = __builtin_bit_cast(h8, S.l[c]);
                t = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bhc, t, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, blc, t, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) t[r] *= kLowUnscale;
            // ... and the main product on top, one dependent chain (its B fragments are read again: four more ds_read_b128, no
            // registers held; as two independent chains the compiler interleaved them and spilled hundreds of registers)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const h8 bhc = __builtin_bit_cast(h8, bh[(NC * nh + c) * 64]);
                const h8 ah = __builtin_bit_cast(h8, S.h[c]);
                t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bhc, t, 0, 0, 0);
            }
            f16v &acc = nh ? acc1 : acc0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f4v fac = *reinterpret_cast<const f4v *>(myfac + 8 * g + 4 * lh);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[4 * g + j] += t[4 * g + j] * fac[j];
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    const int npanels = (rows + 31) / 32;
    for (int p = wg * (kSmThreads / 64) + wave; p < npanels; p += nwg * (kSmThreads / 64)) {
        const int r0 = p * 32;
        const int row = r0 + li < rows ? r0 + li : rows - 1;   // (rows past the end re-read the last row; never stored)
        Raw R[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) {
            const float *src = In + (size_t)row * LDA + k * CB + VPL * lh;
#pragma unroll
            for (int q = 0; q < VPL / 4; ++q) R[k].a[q] = *reinterpret_cast<const f4v *>(src + 4 * q);
        }
        (void)NIN;
        auto store_out = [&](int o, const f16v &acc0, const f16v &acc1) {
            float *out = Out + (size_t)(r0 + 4 * lh) * LDOUT + o * CB + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = (r & 3) + 8 * (r >> 2);
                if (r0 + 4 * lh + rr < rows && li < CB) {
                    out[(size_t)rr * LDOUT] = acc0[r];
                    if constexpr (NH == 2) out[(size_t)rr * LDOUT + 32] = acc1[r];
                }
            }
        };
        f16v acc0, acc1;
        Spl X;
        float iX;
        if constexpr (PROG == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
#pragma unroll
            for (int k = 0; k < NPOS; ++k) {
                split_blk(R[k], X, iX);
                prod(X, iX, k, acc0, acc1);
            }
            store_out(0, acc0, acc1);
        } else if constexpr (PROG == 1) {
            split_blk(R[0], X, iX);
#pragma unroll
            for (int k = 0; k < NPOS; ++k) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
                prod(X, iX, k, acc0, acc1);
                store_out(k, acc0, acc1);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NPOS; ++k) {
                split_blk(R[k], X, iX);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
                prod(X, iX, k, acc0, acc1);
                store_out(k, acc0, acc1);
            }
        }
    }
}

template <int CB>
__global__ __launch_bounds__(kSmThreads, 2) void smp_small_split(SmallJobs jobs, const uint4 *__restrict__ wimg) {
    int j = 0;
    if (jobs.n > 1 && (int)blockIdx.x >= jobs.wg0[1]) j = 1;
    if (jobs.n > 2 && (int)blockIdx.x >= jobs.wg0[2]) j = 2;
    const int wg = (int)blockIdx.x - jobs.wg0[j];
    switch (jobs.prog[j]) {  // (uniform per workgroup)
        case 0: small_split_body<0, CB>(jobs.In[j], jobs.Out[j], jobs.rows[j], wimg, jobs.pos0[j], wg, jobs.nwg[j]); break;
        case 1: small_split_body<1, CB>(jobs.In[j], jobs.Out[j], jobs.rows[j], wimg, jobs.pos0[j], wg, jobs.nwg[j]); break;
        default: small_split_body<2, CB>(jobs.In[j], jobs.Out[j], jobs.rows[j], wimg, jobs.pos0[j], wg, jobs.nwg[j]); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Weight gradients of the fused level (compact layout), same split operands.  The eight row block products
//   dWst[p] = sum over rows of A_p[row]^T B_p[row],   A_p in T = [S_ab|S_bc|T6|T10],   B_p in {L, tot L, tr L, dU, dU[trow]}
// reduce over the ROWS, so a row's exponent cannot scale it (the terms of one MFMA accumulation must share their scale) -- but a
// COLUMN's can: every operand column carries one exponent for the whole level (see the kernel), derived from per-channel bounds that
// smp_wgrad_channel_maxima gathers: the largest |f_{l-1}| and |df_l| of each channel.
//
// A workgroup of eight waves takes every gridDim-th 16-row slice of the level, four slices in flight and ONE
// barrier per slice.  In the interval of slice i a thread splits its share of slice i + 1 (raw in registers, requested three
// intervals ago) and stores the halves TRANSPOSED ([column][row pair], laid out per kWsQuadSlot: conflict-free b32 stores and b128 fragment reads) into the
// other stage's four f16 images (A h / l: 256 columns, B h / l: 320 columns), requests its share of slice i + 4 into the
// registers just freed, and runs its wave's product on the images of slice i: a 64 x 64 output as 2 x 2 MFMA tiles, 12 MFMAs
// of 8 passes.  Partial images and their fold are those of smp_wgrad_c64: a fixed set of rows per image, fixed order, reproducible.
//
// Operands are ADDRESSED per slice, on the scalar unit: every slice of the workgroup is wave-uniform, so its rows of T and dO, the
// window of dO its gathered rows dU[trow] lie in (kTrowWindow rows on either side), and its entries of trow and of the row factors are
// reached through buffer descriptors built from blockIdx, gridDim and the loop counter; a lane adds a loop-constant offset (the
// gathered rows: (trow - window start) x row bytes).  Rows past the end of the level and structurally absent blocks (packed table)
// take an out-of-range offset and load zeros -- no 64-bit vector address, no row clamp, no page of zeros, no past-the-end factor
// (they were a quarter of the loop's instructions: NOTES.md, "Weight gradients: slice-based buffer loads").
// ---------------------------------------------------------------------------------------------------------------
constexpr int kWsThreads = 512, kWsSlice = 16;
constexpr int kWsACols = 256, kWsBCols = 320;
// The transposed image of 32 operand columns x 16 rows: a column is 8 words (f16 row pairs 0..7) = two 16-byte slots, the four columns
// of a quad lie 4 slots apart, and quad q of the block starts at slot kWsQuadSlot[q] (byte q of the constant) -- two quads interleaved
// fill 16 slots, the four such pairs are staggered by a slot or three.  Chosen by the bank rules of both accesses, so that nothing has to
// move between registers on the way in:
//   * the staging stores (ds_write_b32, banks = word % 32 over 32 lanes = 8 quads x 4 row pairs, every lane on the SAME column of its
//     quad): the quads' start slots are distinct mod 8 -- {0, 4, 5, 1, 6, 2, 3, 7} -- so the 32 lanes cover the 32 banks once;
//   * the fragment reads (ds_read_b128, slots mod 16 over the 16-lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of columns):
//     the quads {0, 3, 5, 6} start at slots 0, 1, 2, 3 mod 4 and so do the quads {1, 2, 4, 7}; with the columns 4 slots apart each
//     group covers the 16 slots once.
// 288 words per block (276 used) against the 384 of the [column][12 words] image it replaces, whose stores needed the lane's columns
// rotated through registers to separate the banks (two times eight v_cndmask per task).
constexpr unsigned long long kWsQuadSlot = 0x3713022611352400ull;   // quads 0..7: slots 0, 36, 53, 17, 38, 2, 19, 55
constexpr int kWsBlockWords = 288;
__device__ __forceinline__ int ws_col_word(int col) {   // word of (column, row pair 0) in its image
    const int q = (col >> 2) & 7;
    return (col >> 5) * kWsBlockWords + 4 * (int)((kWsQuadSlot >> (8 * q)) & 0xffu) + 16 * (col & 3);
}
constexpr int kWsAWords = kWsACols / 32 * kWsBlockWords, kWsBWords = kWsBCols / 32 * kWsBlockWords;   // one image (h or l)
constexpr int kWsStageWords = 2 * (kWsAWords + kWsBWords);
constexpr size_t kWsLds = 2 * (size_t)kWsStageWords * 4 + 2 * (kWsACols + kWsBCols) * sizeof(float);   // two stages + the column scales and their inverses
// THE gather window of the weight-gradient kernels (smp_wgrad_split, smp_wgrad_all): the rows a transposed row (e, x) lies from its row
// (x, e) at most.  Both kernels reach dU[trow] through a descriptor that spans this many rows below and above the slice; a row farther
// away loads zeros silently, so the contract -- |trow[r] - r| <= kTrowWindow -- is checked on the host before any launch of a
// caller-supplied table (check_tables of smp_level_ops.hip, kGatherWindow), and holds by construction inside a level, where trow
// stays in the row's own node of at most kFusedMaxField positions.
constexpr long long kTrowWindow = (long long)kFusedMaxField * kFusedMaxField;
// A caller-supplied table that leaves the window (gf_smp_level_wgrad_f32 takes any permutation of the rows) is served by smp_wgrad_split
// with ONE descriptor over all of dO instead -- WgradCall::any_trow -- while dO is smaller than kWgradWholeBytes (smp_internal.h).
constexpr size_t kWsWholeBytes = kWgradWholeBytes;
__constant__ int c_ws_ablk[8] = {0, 1, 0, 2, 3, 0, 1, 0};  // S_ab, S_bc, S_ab, T6, T10, S_ab, S_bc, S_ab
__constant__ int c_ws_bblk[8] = {1, 1, 2, 0, 0, 3, 3, 4};  // tot L, tot L, tr L, L, L, dU, dU, dU[trow]

// W = 2 (C = 128): one of the four independent 64 x 64 jobs of every product, dWst[p][64 i .., 64 j ..] = A_p[:, 64 i ..]^T B_p[:, 64 j ..] -- rows W
// times as wide, columns [a_off, +64) of the blocks of T, [b_off, +64) of the blocks of dO; the image lands at float out_off of its
// product's 128 x 128 partial image (the four jobs fill one set of images between them).  cmax: the bounds of THIS job's columns.
template <int W = 1>
__global__ __launch_bounds__(kWsThreads, 1) void smp_wgrad_split(const float *__restrict__ T, const float *__restrict__ dO,
                                                                  const float *__restrict__ rs, int rows,
                                                                  int window,   // rows dU[trow] may lie from its row: kTrowWindow, or
                                                                  // `rows` (any row of a dO smaller than kWsWholeBytes), see load_slice
                                                                  float *__restrict__ part, const int *__restrict__ trow,
                                                                  const unsigned *__restrict__ cmax,   // [kWsACols + kWsBCols] per-COLUMN magnitude
                                                                  // bounds (float bits) of the nine operand blocks over the level, see below; or
                                                                  // null: built here from the level's per-channel maxima
                                                                  const unsigned *__restrict__ chan,   // [128] max |f_{l-1}| | max |dz_l| per channel
                                                                  float smax, float max_tot, float max_tr,
                                                                  const unsigned *__restrict__ row_max,   // or null: {max |tot|, max |tr|} as float bits in
                                                                  // device memory (they replace max_tot / max_tr: the device-side table builder's)
                                                                  int packed,   // != 0: trow is the packed table (see smp_rowpanel_split); 2: and
                                                                  // dO of a row with none of its three bits was not written (FusedRoute::skip_empty)
                                                                  int a_off, int b_off, int out_off) {   // W > 1: see above
    if constexpr (W == 1) a_off = b_off = out_off = 0;
    constexpr int LDT = 256 * W, LDO = 128 * W, BS = 64 * W, LDW = 64 * W;   // rows of T, of dO; a block to the next; rows of an image
    extern __shared__ __attribute__((aligned(16))) unsigned ws_smem[];  // stage s: A h | A l | B h | B l; then the column scales
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // The workgroup's n-th slice is slice blockIdx.x + n gridDim.x of the level: at any time the workgroups read one contiguous
    // window of T and dO (4 MB), spread over every HBM channel.  (A contiguous row range per workgroup, as the fp32 kernel has,
    // makes 256 streams a multiple of 32 KB apart that advance in step: the loads alone then take 0.94 ms, 4.8 TB/s.)
    const int kend = rows;
    auto K = [&](int n) { return (long long)(blockIdx.x + (long long)n * gridDim.x) * kWsSlice; };

    // ---- the scales: ONE exponent per operand COLUMN for the whole level (round 4; rounds 2-3 kept one per 64-column block).  The
    // products reduce over the ROWS, so a column of A is a row of dW and a column of B a column of dW: scaling columns by powers of
    // two is exact and is undone per output element.  A quiet channel no longer shares its exponent with a loud one (the round-3
    // review's weak #1: with one exponent per block the small channels' low halves went subnormal 2^17 below the loud channel);
    // inside a column, an element keeps its 22 bits down to 2^-17 of the column's bound and the absolute error floor is 2^-38 of
    // the bound -- far below what the fp32 accumulation of that column's sum resolves.  The bounds need not be tight (sum s x the
    // largest |f_{l-1}| of the channel, etc.); a bound 2^10 above the true maximum still leaves the floor
    // at 2^-28 of it.
    float *sScale = reinterpret_cast<float *>(ws_smem + 2 * kWsStageWords), *sInv = sScale + kWsACols + kWsBCols;
    if (cmax) {
        for (int c = tid; c < kWsACols + kWsBCols; c += kWsThreads) pow2_scale_col(cmax[c], &sScale[c], &sInv[c]);
    } else {
        // from the per-channel maxima mf = max |f_{l-1}| and mdz = max |dz_l| (left by combine-forward of the level below and by this
        // level's combine-backward, reduced by level_channel_maxima):
        //   S_ab, S_bc = sums over <= smax positions of f_{l-1}          <= smax mf       T6, T10 = the same sums weighted by row sums
        //   of the gated adjacency (>= 0, they add up to tot)            <= max_tot mf
        //   L = dz <= mdz     tot L, tr L <= max_tot mdz, max_tr mdz     dU[e] = sum_y A+[y, e] dz[y] <= max_tot mdz   (and its gathered copy)
        if (row_max) {
            max_tot = __uint_as_float(row_max[0]);
            max_tr = __uint_as_float(row_max[1]);
        }
        for (int c = tid; c < kWsACols + kWsBCols; c += kWsThreads) {
            const bool isa = c < kWsACols;
            const int blk = (isa ? c : c - kWsACols) >> 6, ch = c & 63;
            const float m = __uint_as_float(chan[(isa ? 0 : 64) + ch]);
            const float fa = blk < 2 ? smax : max_tot;                                   // S_ab, S_bc | T6, T10
            const float fb = blk == 0 ? 1.f : blk == 2 ? max_tr : max_tot;               // L | tot L | tr L | dU | dU[trow]
            pow2_scale_col(__float_as_uint(m * (isa ? fa : fb)), &sScale[c], &sInv[c]);
        }
    }
    __syncthreads();

    // ---- staging tasks: one task = rows (k, k + 1) x 4 columns; a wave's task group = 8 column quads (128 B of a row) x the 8
    // row pairs of the slice.  A: group g = wave (8 groups of 32 columns: block g >> 1).  B: groups 0..9 = wave, wave + 8 (waves 0
    // and 1): block g >> 1 of {L, tot L, tr L, dU, dU[trow]}, column half g & 1.
    const int q_lo = lane & 7, pair = lane >> 3;
    struct Task {
        f4v v0, v1;  // rows k, k + 1
    };
    constexpr int NB = 2;
    struct Set {  // one slice's share of a thread: raw rows on their way from HBM
        Task ta, tb[NB];
        float f0, f1;  // the two rows' factor for the first B task (tot for the tot L copy, tr for the tr L copy, else unused)
    };
    const bool has_b1 = wave < 2;
    const int zbit = ((wave >> 1) & 1) == 0 ? 31 : 29;  // the wave stages S_ab / T6 (waves 0, 1, 4, 5) or S_bc / T10 (2, 3, 6, 7)
    const int a_quad = 8 * wave + q_lo;
    auto b_blk = [&](int e) { return (wave + 8 * e) >> 1; };
    auto b_quad = [&](int e) { return 8 * ((wave + 8 * e) & 1) + q_lo; };
    f4v a_scale, b_scale[NB];   // the scales of the lane's four columns
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a_scale[i] = sScale[4 * a_quad + i];
#pragma unroll
        for (int e = 0; e < NB; ++e) {
            const int blk = b_blk(e) < 5 ? b_blk(e) : 0;   // (waves 2..7 have no second task: any column)
            b_scale[e][i] = sScale[kWsACols + 64 * blk + 4 * b_quad(e) + i];
        }
    }
    // The gathered rows' indices (dU[trow]: waves 0 and 1, second task) are requested TWO requests ahead: a request that had to
    // wait for its own indices would wait for everything the wave has in flight before them (loads return in order) -- a full HBM
    // round trip inside every interval, which the barrier hands to all eight waves (measured: the interval WAS that round trip).
    //
    // Every request goes through a buffer descriptor whose base and size are wave-uniform: the slice K(m) rides in the descriptor (or
    // in the scalar offset), a lane's offset is a loop constant, and whatever must not be fetched -- a row past the end of the level,
    // a structurally absent block of the packed table, the second "task" of waves 2..7 -- gets an offset out of the descriptor's
    // range and loads zeros without a request leaving the wave.  No 64-bit address, row clamp or select is formed on the vector unit.
    constexpr int kOor = (int)kWsWholeBytes;            // beyond every descriptor below (the window's spans 8,208 rows of 1 KiB)
    constexpr unsigned kRsrcFlags = 0x00020000;
    constexpr int kAuxA = (GF_NT_SITES & 4) ? 2 : 0;   // the rows of T are read once: streamed (aux bit 1 = nt); dO is read five times
    // the first row of the workgroup's m-th slice, `rows` when the slice lies past the end (then every entry is out of range).  32-bit
    // unsigned on purpose -- the scalar unit compares no 64-bit integers; a workgroup requests at most six slices past the end, far
    // less than 2^31 rows
    auto first_row = [&](int m) {
        const unsigned k = (blockIdx.x + (unsigned)m * gridDim.x) * (unsigned)kWsSlice;
        return __builtin_amdgcn_readfirstlane((int)(k < (unsigned)rows ? k : (unsigned)rows));
    };
    const __amdgpu_buffer_rsrc_t rTr = __builtin_amdgcn_make_buffer_rsrc(const_cast<int *>(trow), 0, (unsigned)rows * 4u, kRsrcFlags);
    const __amdgpu_buffer_rsrc_t rRs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(rs), 0, (unsigned)rows * 8u, kRsrcFlags);
    int ia0 = 0, ia1 = 0, ib0 = 0, ib1 = 0;  // trow of the rows (k, k + 1) of the wave's next / next-but-one request
    const int off_tr = 8 * pair;             // rows (2 pair, 2 pair + 1) of a slice in the table of 4-byte entries
    auto fetch_trow = [&](int m, int &t0, int &t1) {   // (entries past the end read 0: their rows of T are zeros, see load_slice)
        const int ks = first_row(m);
        t0 = __builtin_amdgcn_raw_buffer_load_b32(rTr, off_tr, ks * 4, 0);
        t1 = __builtin_amdgcn_raw_buffer_load_b32(rTr, off_tr + 4, ks * 4, 0);
    };
    // a lane's constant byte offsets: its two rows of T in the slice's descriptor, of dO behind the window's scalar offset
    const int a_col = W == 1 ? 4 * a_quad : (a_quad >> 4) * BS + a_off + ((4 * a_quad) & 63);   // the quad's first column in its row of T
    const int off_a = 2 * pair * (LDT * 4) + a_col * 4;
    const int b0_col = (b_blk(0) >= 3 ? BS : 0) + b_off + 4 * b_quad(0);   // first task: L (blocks 0..2) or dU (3) of the lane's own rows
    const int off_b = 2 * pair * (LDO * 4) + b0_col * 4;
    const int g_col = (BS + b_off + 4 * b_quad(1)) * 4;                     // second task (waves 0, 1): dU of the gathered rows
    const int off_rs = 16 * pair + 4 * (b_blk(0) == 2 ? 1 : 0);             // the row's factor: tot, or tr for the tr L copy
    // NO branch in a request or around it: every wave issues the same loads every interval (waves 2..7 issue a second "task" that is
    // never stored, at an out-of-range offset: an issue slot and no traffic).  With a conditional load
    // anywhere in the loop the compiler cannot count what is in flight at the join and waits for vmcnt(0) before every split --
    // the whole queue, the requests just issued included (the interval was one HBM round trip for that reason, too).
    auto load_slice = [&](Set &S, int m) {  // the workgroup's m-th slice; calls come with consecutive m
        // (packed table: bit 31 of a row's entry = its S_ab / T6 blocks hold data; the waves that stage those blocks do not fetch the
        //  rows without -- 0.73 GB a cfg3 step)
        const int g0 = packed ? (ia0 & 0x1fffffff) : ia0, g1 = packed ? (ia1 & 0x1fffffff) : ia1;
        // (absent: bit 31 clear for the S_ab / T6 waves, bit 29 clear for the S_bc / T10 waves)
        const bool z0 = packed && !((ia0 >> zbit) & 1), z1 = packed && !((ia1 >> zbit) & 1);
        // the gathered dU row meets S_ab of its row only: a row without data skips the gather as well (and waves 2..7 have none)
        const bool zg0 = !has_b1 || (packed && ia0 >= 0), zg1 = !has_b1 || (packed && ia1 >= 0);
        // an empty row (no data in any block of T): its dO was not stored and meets zeros only -- not requested either
        const bool ze0 = packed > 1 && !(ia0 & 0xe0000000), ze1 = packed > 1 && !(ia1 & 0xe0000000);
        ia0 = ib0, ia1 = ib1;
        fetch_trow(m + 2, ib0, ib1);
        // the slice's descriptors, on the scalar unit: rows [k0, min(k0 + 16, rows)) of T, and the window of dO that holds the slice's
        // own rows and every row they may gather: [max(0, k0 - kTrowWindow), min(rows, k0 + 16 + kTrowWindow))
        const int k0 = first_row(m);
        const int left = rows - k0 < kWsSlice ? rows - k0 : kWsSlice;   // (0 past the end)
        const int w0 = __builtin_amdgcn_readfirstlane(k0 > window ? k0 - window : 0);
        const unsigned w1u = (unsigned)k0 + (unsigned)kWsSlice + (unsigned)window;   // (k0, window <= rows < 2^31)
        const int w1 = __builtin_amdgcn_readfirstlane((int)(w1u < (unsigned)rows ? w1u : (unsigned)rows));
        const __amdgpu_buffer_rsrc_t rT =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(T + (size_t)k0 * LDT), 0, (unsigned)(left * (LDT * 4)), kRsrcFlags);
        // (window = rows: the descriptor spans all of dO, which the launcher admits below kWsWholeBytes only -- kOor stays out of range)
        const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(dO + (size_t)w0 * LDO), 0,
                                                                             left > 0 ? (unsigned)((w1 - w0) * (LDO * 4)) : 0u, kRsrcFlags);
        const int own = (k0 - w0) * (LDO * 4);
        S.ta.v0 = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rT, z0 ? kOor : off_a, 0, kAuxA));
        S.ta.v1 = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rT, z1 ? kOor : off_a + LDT * 4, 0, kAuxA));
        S.f0 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rRs, off_rs, k0 * 8, 0));
        S.f1 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rRs, off_rs + 8, k0 * 8, 0));
        S.tb[0].v0 = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rD, ze0 ? kOor : off_b, own, 0));
        S.tb[0].v1 = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rD, ze1 ? kOor : off_b + LDO * 4, own, 0));
        // (unsigned: the zero entry of a row past the end may wrap -- harmless, its rows of T are zeros and the descriptor bounds it)
        const int og0 = (int)((unsigned)(g0 - w0) * (unsigned)(LDO * 4) + (unsigned)g_col);
        const int og1 = (int)((unsigned)(g1 - w0) * (unsigned)(LDO * 4) + (unsigned)g_col);
        S.tb[1].v0 = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rD, zg0 ? kOor : og0, 0, 0));
        S.tb[1].v1 = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rD, zg1 ? kOor : og1, 0, 0));
    };
    // word (column col0 + i, pair) of the images <- halves of (row k, row k + 1) at column col0 + i: the four columns of the lane's quad
    // are 16 words apart (ws_col_word), one address and four immediate offsets per image -- conflict-free as issued, see kWsQuadSlot
    // (sc: the columns' scales; f0, f1: what rows k and k + 1 are multiplied by besides -- the row's factor for the tot L / tr L copies,
    //  1 otherwise: it rides in the one multiply the split starts with.  Rows past the end of the level arrive as zeros.)
    auto store_task = [&](const f4v &v0, const f4v &v1, unsigned *H, unsigned *L, int col0, const f4v &sc, float f0, float f1, auto fma) {
        const int w = ws_col_word(col0) + pair;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h2 h, l;
            split_plain2_as<decltype(fma)::value>(v0[i], v1[i], sc[i] * f0, sc[i] * f1, &h, &l);
            H[w + 16 * i] = __builtin_bit_cast(unsigned, h);
            L[w + 16 * i] = __builtin_bit_cast(unsigned, l);
        }
    };
    // rows past the range arrived as zeros; the scaled copies of L take their row factors (fp32 factor times a power of two: the
    // product the fp32 kernel forms, rounded once)
    auto store_slice = [&](const Set &S, unsigned *stage) {
        unsigned *Ah = stage, *Al = Ah + kWsAWords, *Bh = Al + kWsAWords, *Bl = Bh + kWsBWords;
        // (which task takes its low half from a fused residual is fixed here, not left to the compiler: see split_plain2_as)
        store_task(S.ta.v0, S.ta.v1, Ah, Al, 4 * a_quad, a_scale, 1.f, 1.f, std::true_type());
        const bool scaled = b_blk(0) == 1 || b_blk(0) == 2;   // (the second task is the gathered dU: no factor)
        store_task(S.tb[0].v0, S.tb[0].v1, Bh, Bl, 64 * b_blk(0) + 4 * b_quad(0), b_scale[0], scaled ? S.f0 : 1.f, scaled ? S.f1 : 1.f, std::false_type());
        if (has_b1) store_task(S.tb[1].v0, S.tb[1].v1, Bh, Bl, 64 * b_blk(1) + 4 * b_quad(1), b_scale[1], 1.f, 1.f, std::true_type());
    };

    f16v acc[2][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = acc[0][1][r] = acc[1][0][r] = acc[1][1][r] = 0.f;
    const int ablk = c_ws_ablk[wave], bblk = c_ws_bblk[wave];
    auto products = [&](const unsigned *stage) {
        const unsigned *Ah = stage, *Al = Ah + kWsAWords, *Bh = Al + kWsAWords, *Bl = Bh + kWsBWords;
        const int ao = ws_col_word(ablk * 64 + li) + 4 * lg, bo = ws_col_word(bblk * 64 + li) + 4 * lg;   // (the next 32 columns: a block on)
        h8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            ah[t] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4 *>(Ah + ao + t * kWsBlockWords));
            al[t] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4 *>(Al + ao + t * kWsBlockWords));
            bh[t] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4 *>(Bh + bo + t * kWsBlockWords));
            bl[t] = __builtin_bit_cast(h8, *reinterpret_cast<const uint4 *>(Bl + bo + t * kWsBlockWords));
        }
        // (plain low halves here -- split_plain2 -- not the 2^11-scaled ones of the row-panel kernels: with per-column exponents the
        //  subnormal floor sits 2^-38 below the column's bound, and the three products go straight into the accumulator)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
            }
    };
    // interval of the workgroup's slice n: Ra holds slice n + 1; the requests of slices n + 2 and n + 3 are in the other two sets
    auto interval = [&](Set &Ra, int n) {
        store_slice(Ra, ws_smem + ((n + 1) & 1) * kWsStageWords);  // (past the end: zeros)
        load_slice(Ra, n + 4);
        products(ws_smem + (n & 1) * kWsStageWords);
        __syncthreads();
    };
    if (K(0) < kend) {
        Set S0, S1, S2;
        fetch_trow(0, ia0, ia1);
        fetch_trow(1, ib0, ib1);
        load_slice(S0, 0);
        load_slice(S1, 1);
        load_slice(S2, 2);
        store_slice(S0, ws_smem);
        load_slice(S0, 3);
        __syncthreads();
        // now: images of slice 0 in stage 0; S1 = slice 1, S2 = slice 2, S0 = slice 3
        int left = (int)((kend - K(0) + (long long)gridDim.x * kWsSlice - 1) / ((long long)gridDim.x * kWsSlice));  // slices of this workgroup
        int n = 0;
        for (; left >= 3; n += 3, left -= 3) {  // (nothing conditional inside: see load_slice)
            interval(S1, n);
            interval(S2, n + 1);
            interval(S0, n + 2);
        }
        if (left >= 1) interval(S1, n);
        if (left >= 2) interval(S2, n + 1);
    }
    // back to fp32 units: row k of the product is column k of its A block, column n column n of its B block.
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float *out = part + ((size_t)blockIdx.x * 8 + wave) * (LDW * LDW) + out_off + li;
    const float *ia = sInv + ablk * 64, *ib = sInv + kWsACols + bblk * 64;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const float ub = ib[32 * nt + li];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * lg;
                out[row * LDW + 32 * nt] = acc[mt][nt][r] * (ia[row] * ub);
            }
        }
}


// ---------------------------------------------------------------------------------------------------------------
// The same eight products at the other channel counts the row-panel kernels serve (CB = 32 / 16; round 5), with ONE wave doing all
// eight for its slices and the operands loaded STRAIGHT into MFMA layout.  Both operands of  dW = A^T B  reduce over the ROWS, and
// v_mfma_f32_32x32x16_f16 wants from lane (c = lane & 31, g = lane >> 5) the eight reduction indices k = 8 g .. 8 g + 7 of column c --
// eight ROWS of one column: one dword load per row hands the wave fully used row segments, the lane splits its eight values in
// registers, and the fragments go to the pipe (no transposed LDS image, no barrier per slice).  A wave keeps the eight accumulators
// (128 registers; one wave per SIMD, four per workgroup), requests the seven blocks of its slice once, splits nine operands (four of
// T; L, tot L, tr L, dU, dU[trow] -- or eight factor-scaled ones under slice dropout, NF = 8) and runs the 24 MFMAs.  (A wave per
// product, round 4, requested and split every shared block up to five times and was VALU-bound: NOTES.md.)
//   * Buffer addressing with the descriptor REBASED per slice (wave-uniform scalar arithmetic): lane offsets are constants, the row
//     of a request rides in its scalar offset, rows past the end of the level are out of range (they load zeros), and a row whose
//     block is structurally zero (packed table, see smp_rowpanel_split) gets an out-of-range offset.  The gathered rows dU[trow] lie
//     inside the row's own node (< s^2 <= 4096 rows away, kTrowWindow: 1024 until round 6, when nodes of up to 64 positions joined the
//     fused level): their descriptor starts that many rows below the slice.  Any level size.
//   * CB = 16: a 32 x 32 tile has room for TWO 16-column operands, so a slice is 32 rows there and the lanes of columns 16..31 carry
//     the operands of its second sixteen rows: the tile's diagonal quadrants are the two half-slices' products (the off-diagonal ones
//     mix the halves and are ignored) and are added at the end -- half the instructions per row of a half-empty tile.
//   * The four waves of a workgroup take its slices in turn; their images are added in wave order through LDS: the same partial
//     images (8 x CB x CB floats per workgroup), same fold as the staged kernel, and the result does not depend on timing.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kW8Threads = 256;
// NX = 3 (SMP_2D_ver7 on the 18-slice level, gf_smp::n_extra): three more products on operands the slice already holds as fragments --
// S_ab^T L, S_bc^T L, S_bc^T (tr L) -- whose images go to `xpart` (three per workgroup), folded by the caller into dX.
template <int CB, int NF, int NX = 0>
__global__ __launch_bounds__(kW8Threads, 1) void smp_wgrad_all(const float *__restrict__ T, const float *__restrict__ dO,
                                                                const float *__restrict__ rs, int rows, float *__restrict__ part,
                                                                const int *__restrict__ trow, const unsigned *__restrict__ cmax,
                                                                const unsigned *__restrict__ chan, float smax,
                                                                const unsigned *__restrict__ row_max, int packed, float *__restrict__ xpart = nullptr) {
    static_assert(CB == 32 || CB == 16, "one 32 x 32 tile per product");
    static_assert(NX == 0 || (NX == 3 && NF == 2), "the extra products take the plain (tot, tr) row factors");
    constexpr int NP = 8 + NX;
    constexpr int ACOLS = 4 * CB, BCOLS = 5 * CB;
    constexpr int SL = CB == 16 ? 2 * kWsSlice : kWsSlice;   // rows of a slice (CB = 16: two half-slices per tile, see above)
    constexpr int TROW = 16 * CB, DROW = 8 * CB;             // bytes of a row of T, of dO
    constexpr int NBF = NF == 8 ? 8 : 5;                     // B fragments per slice
    __shared__ float sScale[ACOLS + BCOLS], sInv[ACOLS + BCOLS];
    __shared__ float sImg[NP * CB * CB];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, lg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = (CB == 16 && li >= 16) ? 1 : 0;
    const int lc = CB == 16 ? (li & 15) : li;
    const int rb = 8 * lg + 16 * hi;
    if (cmax) {
        for (int c = tid; c < ACOLS + BCOLS; c += kW8Threads) pow2_scale_col(cmax[c], &sScale[c], &sInv[c]);
    } else {
        const float max_tot = __uint_as_float(row_max[0]), max_tr = __uint_as_float(row_max[1]);
        for (int c = tid; c < ACOLS + BCOLS; c += kW8Threads) {
            const bool isa = c < ACOLS;
            const int blk = (isa ? c : c - ACOLS) / CB, ch = c % CB;
            const float m = __uint_as_float(chan[(isa ? 0 : CB) + ch]);
            const float fa = blk < 2 ? smax : max_tot;
            const float fb = blk == 0 ? 1.f : blk == 2 ? max_tr : max_tot;
            pow2_scale_col(__float_as_uint(m * (isa ? fa : fb)), &sScale[c], &sInv[c]);
        }
    }
    __syncthreads();
    float sa[4], sb[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) sa[k] = sScale[CB * k + lc];
#pragma unroll
    for (int k = 0; k < 5; ++k) sb[k] = sScale[ACOLS + CB * k + lc];

    constexpr int kOut = 0x40000000;
    const long long nsl = ((long long)rows + SL - 1) / SL;
    auto slice_of = [&](int m) { return (long long)blockIdx.x + ((long long)wave + 4ll * m) * gridDim.x; };   // the wave's m-th slice
    struct Idx {
        int t[8];
    };
    struct Fac {
        float f[8][NF == 8 ? 8 : 2];
    };
    struct Raw {
        float a[4][8], l[8], u[8], g[8];   // S_ab, S_bc, T6, T10 | L | dU | dU[trow]
    };
    const __amdgpu_buffer_rsrc_t rTr = __builtin_amdgcn_make_buffer_rsrc(const_cast<int *>(trow), 0, (unsigned)rows * 4u, 0x00020000);
    constexpr int rsb = 4 * NF;
    const __amdgpu_buffer_rsrc_t rRs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(rs), 0, (unsigned)rows * (unsigned)rsb, 0x00020000);
    auto ld1 = [](__amdgpu_buffer_rsrc_t r, int voff, int soff) {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
    };
    typedef int i4v __attribute__((ext_vector_type(4)));
    auto first_row = [&](int m) {
        const long long k0 = slice_of(m) * SL;
        return k0 < rows ? (int)k0 : rows;   // (past the end: every entry out of range)
    };
    auto load_idx = [&](Idx &I, int m) {
        const int ks = first_row(m);
        const i4v t0 = __builtin_bit_cast(i4v, __builtin_amdgcn_raw_buffer_load_b128(rTr, 4 * rb, ks * 4, 0));
        const i4v t1 = __builtin_bit_cast(i4v, __builtin_amdgcn_raw_buffer_load_b128(rTr, 4 * rb + 16, ks * 4, 0));
        I.t[0] = t0[0], I.t[1] = t0[1], I.t[2] = t0[2], I.t[3] = t0[3], I.t[4] = t1[0], I.t[5] = t1[1], I.t[6] = t1[2], I.t[7] = t1[3];
    };
    auto load_fac = [&](Fac &F, int m) {   // the lane's eight rows are consecutive: rsb bytes each
        const int ks = first_row(m);
#pragma unroll
        for (int q = 0; q < 8 * NF / 4; ++q) {
            const f4v v = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rRs, rsb * rb + 16 * q, ks * rsb, 0));
#pragma unroll
            for (int e = 0; e < 4; ++e) F.f[(4 * q + e) / NF][(4 * q + e) % NF] = v[e];
        }
    };
    auto load_raw = [&](Raw &R, const Idx &I, int m) {
        const long long k0 = slice_of(m) * SL;
        const bool live = k0 < rows;
        long long left = (long long)rows - k0;
        left = left < 0 ? 0 : left > SL ? SL : left;
        const long long k0c = live ? k0 : 0;
        const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(T + (size_t)k0c * ACOLS), 0, (unsigned)(left * TROW), 0x00020000);
        const long long g0 = k0c > kTrowWindow ? k0c - kTrowWindow : 0;
        long long g1 = k0c + SL + kTrowWindow;
        g1 = g1 > rows ? rows : g1;
        const __amdgpu_buffer_rsrc_t rD = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(dO + (size_t)g0 * 2 * CB), 0, live ? (unsigned)((g1 - g0) * DROW) : 0u, 0x00020000);
        const int own = (int)(k0c - g0) * DROW;
        const int ig0 = (int)g0;
        const int offA = rb * TROW + lc * 4, offL = rb * DROW + lc * 4, offU = offL + CB * 4;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = I.t[j];
            const bool p31 = !packed || ((t >> 31) & 1), p29 = !packed || ((t >> 29) & 1);
            const int v31 = p31 ? offA : kOut, v29 = p29 ? offA : kOut;
            const int tr = packed ? (t & 0x1fffffff) : t;
            const int vg = p31 ? (tr - ig0) * DROW + (CB + lc) * 4 : kOut;   // dU[trow] only meets S_ab of ITS row
            R.a[0][j] = ld1(rT, v31, j * TROW);
            R.a[1][j] = ld1(rT, v29 + CB * 4, j * TROW);
            R.a[2][j] = ld1(rT, v31 + 2 * CB * 4, j * TROW);
            R.a[3][j] = ld1(rT, v29 + 3 * CB * 4, j * TROW);
            R.l[j] = ld1(rD, offL, own + j * DROW);
            R.u[j] = ld1(rD, offU, own + j * DROW);
            R.g[j] = ld1(rD, vg, 0);
        }
    };
    f16v acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][r] = 0.f;
    auto frag = [&](const float (&v)[8], float sc, const Fac *F, int col, h8 *H, h8 *L) {
        unsigned hw[4], lw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h2 h, l;
            split_plain2(v[2 * i], v[2 * i + 1], F ? sc * F->f[2 * i][col] : sc, F ? sc * F->f[2 * i + 1][col] : sc, &h, &l);
            hw[i] = __builtin_bit_cast(unsigned, h);
            lw[i] = __builtin_bit_cast(unsigned, l);
        }
        *H = __builtin_bit_cast(h8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
        *L = __builtin_bit_cast(h8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
    };
    // products 0..7: A block c_ws_ablk, B operand c_ws_bblk (0 L, 1 tot L, 2 tr L, 3 dU, 4 dU[trow]) -- compile-time copies
    // (extra products 8, 9, 10: S_ab with L, S_bc with L, S_bc with tr L)
    constexpr int kA[11] = {0, 1, 0, 2, 3, 0, 1, 0, 0, 1, 1}, kB[11] = {1, 1, 2, 0, 0, 3, 3, 4, 0, 0, 2};
    const long long first = (long long)blockIdx.x + (long long)wave * gridDim.x;
    if (first < nsl) {
        const int mine = (int)((nsl - first + 4ll * gridDim.x - 1) / (4ll * gridDim.x));   // slices of this wave
        Idx I0, I1;
        Fac F0, F1;
        Raw R0, R1;
        load_idx(I0, 0);
        load_idx(I1, 1);
        load_fac(F0, 0);
        load_raw(R0, I0, 0);
        load_idx(I0, 2);
        load_fac(F1, 1);
        load_raw(R1, I1, 1);
        // One slice: the B fragments first (they serve several products), then block after block of T -- split, multiply -- so that at
        // most one A fragment is live beside them (with all nine fragments built before the first MFMA the wave needed more than its
        // 256 VGPRs: the allocator parked values loaded by the requests IN FLIGHT in AGPRs, and every such copy waits for its load --
        // the queue was drained once per pair of slices).  The next-but-one slice is requested as soon as the last raw register is free.
        auto mfma3 = [&](int p, const h8 &ah, const h8 &al, const h8 &bh, const h8 &bl) {
            acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[p], 0, 0, 0);
        };
        auto step = [&](Raw &R, Fac &Fcur, Idx &Inext2, Idx &Inext3, int m) {
            h8 bh[NBF], bl[NBF];
            if constexpr (NF == 8) {
#pragma unroll
                for (int p = 0; p < 8; ++p) frag(kB[p] == 3 ? R.u : kB[p] == 4 ? R.g : R.l, sb[kB[p]], &Fcur, p, &bh[p], &bl[p]);
            } else {
                frag(R.l, sb[0], nullptr, 0, &bh[0], &bl[0]);
                frag(R.l, sb[1], &Fcur, 0, &bh[1], &bl[1]);
                frag(R.l, sb[2], &Fcur, 1, &bh[2], &bl[2]);
                frag(R.u, sb[3], nullptr, 0, &bh[3], &bl[3]);
                frag(R.g, sb[4], nullptr, 0, &bh[4], &bl[4]);
            }
#pragma unroll
            for (int k = 0; k < NBF; ++k) asm volatile("" : "+v"(bh[k]), "+v"(bl[k]));
            auto bsel = [&](int p) { return NF == 8 ? p : kB[p]; };
            h8 ah, al;
            frag(R.a[0], sa[0], nullptr, 0, &ah, &al);   // S_ab: products 0, 2, 5, 7
            asm volatile("" : "+v"(ah), "+v"(al));
            __builtin_amdgcn_sched_barrier(0);
            mfma3(0, ah, al, bh[bsel(0)], bl[bsel(0)]);
            mfma3(2, ah, al, bh[bsel(2)], bl[bsel(2)]);
            mfma3(5, ah, al, bh[bsel(5)], bl[bsel(5)]);
            mfma3(7, ah, al, bh[bsel(7)], bl[bsel(7)]);
            if constexpr (NX == 3) mfma3(8, ah, al, bh[0], bl[0]);
            h8 ch, cl;
            frag(R.a[1], sa[1], nullptr, 0, &ch, &cl);   // S_bc: products 1, 6
            asm volatile("" : "+v"(ch), "+v"(cl));
            __builtin_amdgcn_sched_barrier(0);
            mfma3(1, ch, cl, bh[bsel(1)], bl[bsel(1)]);
            mfma3(6, ch, cl, bh[bsel(6)], bl[bsel(6)]);
            if constexpr (NX == 3) {
                mfma3(9, ch, cl, bh[0], bl[0]);
                mfma3(10, ch, cl, bh[2], bl[2]);
            }
            h8 dh, dl, eh, el;
            frag(R.a[2], sa[2], nullptr, 0, &dh, &dl);   // T6: product 3
            frag(R.a[3], sa[3], nullptr, 0, &eh, &el);   // T10: product 4
            asm volatile("" : "+v"(dh), "+v"(dl), "+v"(eh), "+v"(el));
            __builtin_amdgcn_sched_barrier(0);
            load_idx(Inext3, m + 3);
            load_fac(Fcur, m + 2);
            load_raw(R, Inext2, m + 2);
            __builtin_amdgcn_sched_barrier(0);
            mfma3(3, dh, dl, bh[bsel(3)], bl[bsel(3)]);
            mfma3(4, eh, el, bh[bsel(4)], bl[bsel(4)]);
        };
        for (int m = 0; m < mine; m += 2) {
            step(R0, F0, I0, I1, m);
            step(R1, F1, I1, I0, m + 1);
        }
    }
    // the four waves' images, added in wave order (back in fp32 units: row k of a product is column k of its A block, column n
    // column n of its B block)
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const float *ia = sInv + kA[p] * CB, ub = sInv[ACOLS + kB[p] * CB + lc];
                float *img = sImg + p * CB * CB + lc;
                if constexpr (CB == 16) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * lg;   // 0 .. 15
                        const float second = acc[p][r + 8];
                        const float v = (acc[p][r] + __shfl_xor(second, 16)) * (ia[row] * ub);
                        if (li < 16) img[row * CB] = w == 0 ? v : img[row * CB] + v;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2) + 4 * lg;
                        const float v = acc[p][r] * (ia[row] * ub);
                        img[row * CB] = w == 0 ? v : img[row * CB] + v;
                    }
                }
            }
        }
        __syncthreads();
    }
    float *out = part + (size_t)blockIdx.x * 8 * (CB * CB);
    for (int i = tid; i < 8 * CB * CB / 4; i += kW8Threads)
        *reinterpret_cast<f4v *>(out + 4 * i) = *reinterpret_cast<const f4v *>(sImg + 4 * i);
    if constexpr (NX > 0) {
        float *xo = xpart + (size_t)blockIdx.x * NX * (CB * CB);
        for (int i = tid; i < NX * CB * CB / 4; i += kW8Threads)
            *reinterpret_cast<f4v *>(xo + 4 * i) = *reinterpret_cast<const f4v *>(sImg + 8 * CB * CB + 4 * i);
    }
}

// ---- the column bounds of a level's operand blocks (cmax of smp_wgrad_split / smp_wgrad_all) ----------------------------------
// THE column-maxima loop (four rows in flight per thread): the largest |x| of columns [0, 64) of X [rows][ld] over the rows this
// workgroup takes, reduced through LDS and added to out[64] (float bits, atomicMax: out starts at 0).  256 threads.
__device__ __forceinline__ void col_absmax64_body(const float *__restrict__ X, long long rows, int ld, unsigned *__restrict__ out) {
    __shared__ unsigned red[64];
    if (threadIdx.x < 64) red[threadIdx.x] = 0u;
    __syncthreads();
    const int q = threadIdx.x & 15;   // channel quad
    f4v m = {0.f, 0.f, 0.f, 0.f};
    const long long step = (long long)gridDim.x * 16;
    for (long long r0 = (long long)blockIdx.x * 16 + (threadIdx.x >> 4); r0 < rows; r0 += 4 * step) {
        f4v v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long r = r0 + u * step;
            v[u] = *reinterpret_cast<const f4v *>(X + (size_t)(r < rows ? r : r0) * ld + 4 * q);   // (past the end: row r0 again)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], fabsf(v[u][j]));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) atomicMax(&red[4 * q + j], __float_as_uint(m[j]));
    __syncthreads();
    if (threadIdx.x < 64 && red[threadIdx.x]) atomicMax(&out[threadIdx.x], red[threadIdx.x]);
}
// 64 columns of one operand (the exact bounds: wgrad_exact_bounds)
__global__ __launch_bounds__(256) void col_absmax64(const float *__restrict__ X, long long rows, int ld, unsigned *__restrict__ out) {
    col_absmax64_body(X, rows, ld, out);
}
// both per-channel maxima of a 64-channel level in ONE launch: blockIdx.y = 0: X0 [rows0][64] -> out[0, 64), 1: X1 [rows1][64] -> out[64, 128)
__global__ __launch_bounds__(256) void level_channel_maxima(const float *__restrict__ X0, long long rows0, const float *__restrict__ X1,
                                                            long long rows1, unsigned *__restrict__ out) {
    col_absmax64_body(blockIdx.y ? X1 : X0, blockIdx.y ? rows1 : rows0, 64, out + 64 * blockIdx.y);
}
// the same for other row widths, one row in flight: X0 [rows0][ld0], X1 [rows1][ld1], columns [0, C) of each -> out[0, C) | out[C, 2 C)
// (C % 4 == 0, C <= 64)
__global__ __launch_bounds__(256) void level_channel_maxima_ld(const float *__restrict__ X0, long long rows0, int ld0, const float *__restrict__ X1,
                                                               long long rows1, int ld1, int C, unsigned *__restrict__ out) {
    __shared__ unsigned red[64];
    const float *X = blockIdx.y ? X1 : X0;
    const long long rows = blockIdx.y ? rows1 : rows0;
    const int ld = blockIdx.y ? ld1 : ld0, nq = C / 4, rpb = 256 / nq;   // rows per block pass
    if (threadIdx.x < 64) red[threadIdx.x] = 0u;
    __syncthreads();
    const int q = threadIdx.x % nq, rr = threadIdx.x / nq;
    f4v m = {0.f, 0.f, 0.f, 0.f};
    if (rr < rpb)
        for (long long r = (long long)blockIdx.x * rpb + rr; r < rows; r += (long long)gridDim.x * rpb) {
            const f4v v = *reinterpret_cast<const f4v *>(X + (size_t)r * ld + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], fabsf(v[j]));
        }
#pragma unroll
    for (int j = 0; j < 4; ++j) atomicMax(&red[4 * q + j], __float_as_uint(m[j]));
    __syncthreads();
    if ((int)threadIdx.x < C && red[threadIdx.x]) atomicMax(&out[C * blockIdx.y + threadIdx.x], red[threadIdx.x]);
}
__global__ void rowscale_absmax(const float *__restrict__ rs, int rows, unsigned *__restrict__ out) {   // out[0..1] = max |tot|, |tr|
    float a = 0.f, b = 0.f;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        a = fmaxf(a, fabsf(rs[2 * (size_t)r]));
        b = fmaxf(b, fabsf(rs[2 * (size_t)r + 1]));
    }
    atomicMax(&out[0], __float_as_uint(a));
    atomicMax(&out[1], __float_as_uint(b));
}
// The exact column maxima spread over the nine operand blocks of a weight-gradient job, CB columns each: mt = the column maxima of
// T = [S_ab | S_bc | T6 | T10], mo those of dO = [L | dU], mx[0..1] = the largest |tot|, |tr|.  One job per block of the launch, its
// bounds `stride` words behind the job before: [S_ab | S_bc | T6 | T10 | L | tot L | tr L | dU | dU[trow]].  sub = 0: the one job of a
// level of CB channels.  sub = 64 (C = 128): job blockIdx.x = 2 i + j of smp_wgrad_split<2> takes columns [sub i, +CB) of the blocks of
// T and [sub j, +CB) of those of dO, whose blocks are CB + sub columns wide.
__global__ void wgrad_bounds_exact(const unsigned *__restrict__ mt, const unsigned *__restrict__ mo, const unsigned *__restrict__ mx,
                                   unsigned *__restrict__ cmax, int CB, int stride, int sub) {
    const int c = threadIdx.x, i = blockIdx.x >> 1, j = blockIdx.x & 1;   // 64 threads
    if (c >= CB) return;
    cmax += blockIdx.x * stride;
    const int W = CB + sub;
    const float tot = __uint_as_float(mx[0]), tr = __uint_as_float(mx[1]);
    for (int k = 0; k < 4; ++k) cmax[CB * k + c] = mt[W * k + sub * i + c];
    const float l = __uint_as_float(mo[sub * j + c]), u = __uint_as_float(mo[W + sub * j + c]);
    cmax[4 * CB + c] = __float_as_uint(l);
    cmax[5 * CB + c] = __float_as_uint(tot * l);
    cmax[6 * CB + c] = __float_as_uint(tr * l);
    cmax[7 * CB + c] = cmax[8 * CB + c] = __float_as_uint(u);
}

}  // namespace

bool smp_split_products(const gf_ctx *ctx) {  // (read per call: the parity tests switch it)
    if (ctx && ctx->fp32_products) return false;  // GF_OPT_SMP_FP32_PRODUCTS
    return !env_is("GF_SMP_SPLIT", '0');
}

// the level's packed transposed-row table with the presence bits (see smp_rowpanel_split) in place of the plain one: for levels of
// fewer than `row_limit` rows, unless GF_SMP_MASK_ZEROS=0 (read per call: the parity tests switch it).  THE read of that switch for
// the product and weight-gradient launches (wgrad_packed below: the weight gradients' one decision)
static bool packed_rows(const int *trowf, int rows, int row_limit) {
    return trowf && rows < row_limit && !env_is("GF_SMP_MASK_ZEROS", '0');
}

size_t smp_split_image_bytes(int C) { return (C == 128 ? 8 * (size_t)kSpImgStride128 : 2 * (size_t)kSpImgStride) * sizeof(uint4); }   // (128: four sub-block sets)
template <int C>
static gf_status launch_small_split(gf_ctx *ctx, const char *name, int total, size_t lds, const SmallJobs &jb, const uint4 *img) {
    gf_status st = opt_in_lds(ctx, smp_small_split<C>, lds);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, name, smp_small_split<C>, dim3((unsigned)total), dim3(kSmThreads), lds, jb, img);
    return GF_OK;
}
// the small products of a level in one launch (see smp_small_split): n <= 3 jobs of prog 0 / 1 / 2 on `rows[j]` rows with the weight
// images from stacked position pos0[j] on; `transposed` picks the backward images; wimg = the level's prebuilt images
gf_status smp_small_split_c64(gf_ctx *ctx, bool transposed, int n, const int *prog, const float *const *In, float *const *Out, const int *rows,
                              const int *pos0, const void *wimg, const char *name, int C) {
    const uint4 *img = static_cast<const uint4 *>(wimg) + (transposed ? kSpImgStride : 0);
    SmallJobs jb;
    jb.n = 0;
    int total = 0;
    for (int j = 0; j < n && jb.n < 3; ++j) {
        if (rows[j] < 1) continue;
        const int npanels = (rows[j] + 31) / 32, per = kSmThreads / 64, want = (npanels + per - 1) / per;
        const int k = jb.n++;
        jb.In[k] = In[j], jb.Out[k] = Out[j], jb.rows[k] = rows[j], jb.pos0[k] = pos0[j], jb.prog[k] = prog[j];
        jb.wg0[k] = total;
        jb.nwg[k] = want < 512 ? want : 512;   // (persistent: a workgroup copies 32 - 64 KB of weight images before its first panel)
        total += jb.nwg[k];
    }
    if (total == 0) return GF_OK;
    const size_t lds = 2 * (size_t)4 * (C >= 32 ? C / 32 : 1) * (C / 16) * 64 * 16 + 16 * sizeof(float) + (kSmThreads / 64) * 32 * sizeof(float);
    switch (C) {
    case 16: return launch_small_split<16>(ctx, name, total, lds, jb, img);
    case 32: return launch_small_split<32>(ctx, name, total, lds, jb, img);
    case 64: return launch_small_split<64>(ctx, name, total, lds, jb, img);
    }
    return fail(ctx, GF_ERR_UNSUPPORTED, "smp_small_split: %d channels", C);
}

// the split weight images (both directions) of n levels' stacked weights in one launch; img[i]: smp_split_image_bytes() each
gf_status smp_split_build_images(gf_ctx *ctx, const float *const *Wst, void *const *img, int n, int C, const float *const *X) {
    for (int i0 = 0; i0 < n; i0 += kSpImgLevels) {
        SplitImages a;
        const int m = n - i0 < kSpImgLevels ? n - i0 : kSpImgLevels;
        for (int i = 0; i < m; ++i) {
            a.Wst[i] = Wst[i0 + i];
            a.X[i] = X ? X[i0 + i] : nullptr;
            a.img[i] = static_cast<uint4 *>(img[i0 + i]);
        }
        if (C == 128)   // (four sub-block sets of the eight row products' blocks: smp_split_weight_images_c128)
            GF_LAUNCH(ctx, "smpf_stack_w", smp_split_weight_images_c128, dim3(2, m, 32), dim3(kSpThreads), 0, a);
        else
            GF_LAUNCH(ctx, "smpf_stack_w", smp_split_weight_images, dim3(2, m, kSpPos), dim3(kSpThreads), 0, a, C);
    }
    return GF_OK;
}

// the kernel arguments of smp_rowpanel_split that do not select an instantiation
struct RowpanelArgs {
    int grid;
    const float *A, *rowscale, *Wst;
    float *Out;
    int rows;
    const int *trow;   // the plain or (mask) the packed table
    int store_mask;
    const uint4 *img;   // this direction's weight images, or null
};
template <bool F, bool M, int CB, int NF, int NX, bool CLS = false, int W = 1, bool ACC = false, bool DZ = false>
static gf_status launch_rowpanel_split(gf_ctx *ctx, const RowpanelArgs &a, const int *rcls = nullptr, int a_off = 0, int out_off = 0,
                                       RowpanelDz dz = RowpanelDz()) {
    const size_t lds = 2 * (size_t)(8 + NX) * (CB >= 32 ? CB / 32 : 1) * (CB / 16) * 64 * 16 + 32 * sizeof(float) + (kSpThreads / 64) * 32 * sizeof(float) +
                       (CLS ? (kSpThreads / 64) * 32 * sizeof(float *) : 0);
    gf_status st = opt_in_lds(ctx, smp_rowpanel_split<F, M, CB, NF, NX, CLS, W, ACC, DZ>, lds);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, F ? "smpf_products_fwd" : "smpf_products_bwd", (smp_rowpanel_split<F, M, CB, NF, NX, CLS, W, ACC, DZ>), dim3((unsigned)a.grid), dim3(kSpThreads),
              lds, a.A, a.rowscale, a.Wst, a.Out, a.rows, a.trow, a.store_mask, a.img, rcls, a_off, out_off, dz);
    return GF_OK;
}
// C = 128: the four (reduction half i, output half j) passes of a level's products, each the 64-channel program on its sub-blocks; for an
// output half the pass of i = 1 adds to what i = 0 stored -- a fixed order, the same bits every run.  img: the level's four image sets.
template <bool F, bool M>
static gf_status launch_rowpanel_c128(gf_ctx *ctx, RowpanelArgs a, const uint4 *sets) {
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) {
            a.img = sets + (size_t)(2 * (2 * i + j) + (F ? 0 : 1)) * kSpImgStride128;
            const gf_status st = i == 0 ? launch_rowpanel_split<F, M, 64, 2, 0, false, 2, false>(ctx, a, nullptr, 64 * i, 64 * j)
                                        : launch_rowpanel_split<F, M, 64, 2, 0, false, 2, true>(ctx, a, nullptr, 64 * i, 64 * j);
            if (st != GF_OK) return st;
        }
    return GF_OK;
}
template <int CB, int NF, int NX = 0>
static gf_status launch_rowpanel_split(gf_ctx *ctx, bool forward, bool mask, const RowpanelArgs &a) {
    if (forward) return mask ? launch_rowpanel_split<true, true, CB, NF, NX>(ctx, a) : launch_rowpanel_split<true, false, CB, NF, NX>(ctx, a);
    return mask ? launch_rowpanel_split<false, true, CB, NF, NX>(ctx, a) : launch_rowpanel_split<false, false, CB, NF, NX>(ctx, a);
}

// Panels of one row class (see the kernel): the masked backward products at C = 64 with the level's class lists, when the gradients
// of structural zeros are skipped -- otherwise every row runs the full program and writes all four blocks, and the classes buy
// nothing.  GF_SMP_ROW_CLASSES=0 (read per call): the unclassed kernel.
static bool rowpanel_classed(bool forward, int rows, const int *trowf, bool skip_zero_grads, int C, int nf, int nx, const int *rowcls) {
    return rowcls && !forward && skip_zero_grads && C == 64 && nf == 2 && nx == 0 && packed_rows(trowf, rows, 1 << 29) && !env_is("GF_SMP_ROW_CLASSES", '0');
}
bool smp_rowpanel_dz_applies(const gf_ctx *ctx, int rows, const int *trow, const int *trowf, bool skip_zero_grads, int C, int nf, int nx, const int *rowcls) {
    return trow && smp_split_products(ctx) && rowpanel_classed(false, rows, trowf, skip_zero_grads, C, nf, nx, rowcls);
}

// Row-panel products of a fused SMP level at C = 64, compact layout (O = [O_loc | U]; trow = the transposed-row table of the
// level): forward O from T = [S_ab|S_bc|T6|T10], or backward dT from dO.  Every output element is produced by one wave in a
// fixed order: results do not depend on the grid size.
gf_status smp_rowpanel_split_c64(gf_ctx *ctx, bool forward, const float *A, const float *rowscale, const float *Wst, float *Out,
                                 int rows, const int *trow, int cus, const int *trowf, bool skip_zero_grads, const void *wimg, int C, int nf, int nx,
                                 const int *rowcls, const RowpanelDz *dz, bool skip_empty) {
    const int per = kSpThreads / 64;
    const bool classed = rowpanel_classed(forward, rows, trowf, skip_zero_grads, C, nf, nx, rowcls);
    const int npanels = (rows + 31) / 32 + (classed ? 1 : 0);   // (two padded lists: one panel more at the most)
    const int want = (npanels + per - 1) / per;
    // C = 64: one persistent workgroup per CU (the weight images take 128 KB of LDS); C = 32 (32 KB of images): two
    const int slots = C == 64 ? cus : 2 * cus;   // (C = 32 / 16: one or two per CU measured equal)
    const int grid = want < slots ? want : slots;
    if (C != 64 && !wimg) return fail(ctx, GF_ERR_UNSUPPORTED, "smp_rowpanel_split: %d channels need the level's prebuilt weight images", C);
    const bool mask = packed_rows(trowf, rows, 1 << 29);
    if (C == 128) {   // four sub-block passes of the 64-channel program (launch_rowpanel_c128); the row classes are not used
        if (nf != 2 || nx != 0) return fail(ctx, GF_ERR_UNSUPPORTED, "smp_rowpanel_split: %d row factors / %d extra products at 128 channels", nf, nx);
        const int want128 = ((rows + 31) / 32 + per - 1) / per;
        const RowpanelArgs a = {want128 < cus ? want128 : cus, A, rowscale, Wst, Out, rows, mask ? trowf : trow, skip_zero_grads ? 1 : 0, nullptr};
        const uint4 *sets = static_cast<const uint4 *>(wimg);
        if (forward) return mask ? launch_rowpanel_c128<true, true>(ctx, a, sets) : launch_rowpanel_c128<true, false>(ctx, a, sets);
        return mask ? launch_rowpanel_c128<false, true>(ctx, a, sets) : launch_rowpanel_c128<false, false>(ctx, a, sets);
    }
    // (store_mask: backward, the gradients of structural zeros are not stored; forward, 64 channels: the rows of O without any data are not)
    const RowpanelArgs a = {grid, A, rowscale, Wst, Out, rows, mask ? trowf : trow, (forward ? (skip_empty && mask && C == 64) : skip_zero_grads) ? 1 : 0,
                            wimg ? static_cast<const uint4 *>(wimg) + (forward ? 0 : kSpImgStride) : nullptr};
    if (nx != 0) {   // the extra products of SMP_2D_ver7 on the 18-slice level (see the kernel)
        if (nx != 3 || nf != 2 || !(C == 32 || C == 16) || !wimg)
            return fail(ctx, GF_ERR_UNSUPPORTED, "smp_rowpanel_split: %d extra products at %d channels / %d row factors", nx, C, nf);
        return C == 32 ? launch_rowpanel_split<32, 2, 3>(ctx, forward, mask, a) : launch_rowpanel_split<16, 2, 3>(ctx, forward, mask, a);
    }
    if (nf != 2 && !(nf == 8 && (C == 32 || C == 16))) return fail(ctx, GF_ERR_UNSUPPORTED, "smp_rowpanel_split: %d row factors at %d channels", nf, C);
    if (nf == 8)   // (per-product row factors: the slice-dropout towers, computed at 32 or 16 channels)
        return C == 32 ? launch_rowpanel_split<32, 8>(ctx, forward, mask, a) : launch_rowpanel_split<16, 8>(ctx, forward, mask, a);
    switch (C) {
    case 64:
        if (classed && dz) return launch_rowpanel_split<false, true, 64, 2, 0, true, 1, false, true>(ctx, a, rowcls, 0, 0, *dz);
        if (dz) return fail(ctx, GF_ERR_INVALID, "smp_rowpanel_split: dz is formed by the row-class kernel only");
        if (classed) return launch_rowpanel_split<false, true, 64, 2, 0, true>(ctx, a, rowcls);
        return launch_rowpanel_split<64, 2>(ctx, forward, mask, a);
    case 32: return launch_rowpanel_split<32, 2>(ctx, forward, mask, a);
    case 16: return launch_rowpanel_split<16, 2>(ctx, forward, mask, a);
    }
    return fail(ctx, GF_ERR_UNSUPPORTED, "smp_rowpanel_split: %d channels", C);
}

// ---------------------------------------------------------------------------------------------------------------
// The weight gradients of a fused level's eight row block products, every channel count of the family: ONE entry point
// (smp_wgrad_partials), ONE exact-bounds step (wgrad_exact_bounds), the two size queries, and the question whether the call reads the
// absent blocks of T (smp_wgrad_reads_absent_blocks) -- answered from the same kernel choice and the same packed_rows decision the
// launch makes.  smp_internal.h: WgradCall.
// ---------------------------------------------------------------------------------------------------------------
namespace {

// which kernel a call runs
enum class WgradKernel { None, Fp32, Split64, All, Split128 };
WgradKernel wgrad_kernel(const gf_ctx *ctx, const WgradCall &a) {
    switch (a.C) {
    // 64 channels: the split-operand kernel where it has bounds to take its column exponents from, else the fp32 matrix pipe
    case 64: return a.trow && smp_split_products(ctx) && (a.bounds.level(64) || a.words) ? WgradKernel::Split64 : WgradKernel::Fp32;
    case 32:
    case 16: return WgradKernel::All;
    case 128: return WgradKernel::Split128;   // four sub-block launches of the 64-channel kernel, exact bounds only
    }
    return WgradKernel::None;
}
// ... whether it takes the level's maxima (else exact bounds from the operands themselves)
bool wgrad_level_bounds(WgradKernel k, const WgradCall &a) { return (k == WgradKernel::Split64 || k == WgradKernel::All) && a.bounds.level(a.C); }
// ... and whether it walks the level's PACKED table, reading an absent S_ab / T6 block from the zero page: one row limit per kernel
// (smp_wgrad_all keeps one bit more of a packed entry for itself)
bool wgrad_packed(WgradKernel k, const WgradCall &a) {
    return k != WgradKernel::Fp32 && packed_rows(a.trowf, a.rows, k == WgradKernel::All ? 1 << 28 : 1 << 29);
}

// The scratch words of a call: [0, mo) column maxima of T [rows][4 C], [mo, mx) of dO [rows][2 C], mx: max |tot|, |tr|, then from
// `cmax` on the nine blocks' bounds of every job (wgrad_bounds_exact).  32 and 16 channels share one layout; [0, 2 C) of it also holds
// the level's channel maxima (WgradScales::chan) of a model's level.
struct WgradWords {
    int mo, mx, cmax, jobs;
    size_t total;
};
WgradWords wgrad_words(int C) {
    if (C == 128) return {512, 768, 1024, 4, 1024 + 4 * (size_t)(kWsACols + kWsBCols)};
    return {256, 384, 512, 1, 512 + 9 * (size_t)(C == 64 ? 64 : 32)};
}

// Exact column bounds of the operand blocks from the operands themselves (one extra pass over T and dO: T must hold its structural
// zeros), C = 16 / 32 / 64 / 128, into words + wgrad_words(C).cmax.  The column maxima -- the next speed target named in NOTES.md -- are
// taken HERE and nowhere else: 64 columns a launch of col_absmax64 (16 channels: the two operands are one narrow pass each).
gf_status wgrad_exact_bounds(gf_ctx *ctx, const WgradCall &a) {
    const int C = a.C;
    const WgradWords w = wgrad_words(C);
    unsigned *words = a.words;
    GF_HIP_TRY(ctx, hipMemsetAsync(words, 0, sizeof(unsigned) * w.cmax, ctx->stream));
    if (C >= 32) {
        const long long g0 = ((long long)a.rows + 15) / 16;
        const unsigned g = (unsigned)(g0 < 1 ? 1 : g0 > 1024 ? 1024 : g0);
        for (int k = 0; k < 4 * C / 64; ++k)
            GF_LAUNCH(ctx, "smpf_colmax", col_absmax64, dim3(g), dim3(256), 0, a.T + 64 * k, (long long)a.rows, 4 * C, words + 64 * k);
        for (int k = 0; k < 2 * C / 64; ++k)
            GF_LAUNCH(ctx, "smpf_colmax", col_absmax64, dim3(g), dim3(256), 0, a.dO + 64 * k, (long long)a.rows, 2 * C, words + w.mo + 64 * k);
    } else {
        const long long g0 = ((long long)a.rows + 63) / 64;
        const unsigned g = (unsigned)(g0 < 1 ? 1 : g0 > 256 ? 256 : g0);
        GF_LAUNCH(ctx, "smpf_colmax", level_channel_maxima_ld, dim3(g, 1), dim3(256), 0, a.T, (long long)a.rows, 4 * C, (const float *)nullptr, 0ll, 0, 4 * C, words);
        GF_LAUNCH(ctx, "smpf_colmax", level_channel_maxima_ld, dim3(g, 1), dim3(256), 0, a.dO, (long long)a.rows, 2 * C, (const float *)nullptr, 0ll, 0, 2 * C,
                  words + w.mo);
    }
    GF_LAUNCH(ctx, "smpf_colmax", rowscale_absmax, dim3(64), dim3(256), 0, a.rowscale, a.rows, words + w.mx);
    const int CB = C == 128 ? 64 : C;
    GF_LAUNCH(ctx, "smpf_colmax", wgrad_bounds_exact, dim3(w.jobs), dim3(64), 0, words, words + w.mo, words + w.mx, words + w.cmax, CB, 9 * CB, C == 128 ? 64 : 0);
    return GF_OK;
}

// workgroups (= partial image sets) of the C = 32 / 16 weight-gradient launch for a level of `rows` rows.  smp_wgrad_all keeps one wave
// per SIMD (its eight accumulators): ONE workgroup per CU -- measured at C = 32, cfg3: 0.44 ms with 256 workgroups, 0.53 with 512 (the
// second half waits for whole CUs), 0.72 with 1024.
int wgrad_all_splits(gf_ctx *ctx, long long rows) {
    static int cu_count[64] = {};
    const int di = ctx->device & 63;
    if (!cu_count[di]) {
        if (hipDeviceGetAttribute(&cu_count[di], hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cu_count[di] < 1) cu_count[di] = 256;
    }
    const long long cap = cu_count[di];
    const long long slices = (rows + 15) / 16, want = slices / 8;
    return (int)(want < 1 ? 1 : want > cap ? cap : want);
}
// the partial images of a call, and the rows of one (0: smp_wgrad_all deals slices, not ranges).  They depend on `rows` only (and the
// device's CU count): results are reproducible.  64 / 128 channels: one workgroup per CU, at least 8 slices each.
struct WgradPlan {
    int splits, kchunk;
};
WgradPlan wgrad_plan(gf_ctx *ctx, int rows, int C) {
    if (C == 32 || C == 16) return {wgrad_all_splits(ctx, rows), 0};
    const int target = 256, slice = C == 128 ? kWsSlice : lds_image::BK;
    int kchunk = ((rows + target - 1) / target + slice - 1) / slice * slice;
    if (kchunk < 8 * slice) kchunk = 8 * slice;
    return {(rows + kchunk - 1) / kchunk, kchunk};
}

// one launch of smp_wgrad_all: nf row factors per row of rowscale; xpart: with the three extra products of SMP_2D_ver7
template <int CB>
gf_status launch_wgrad_all(gf_ctx *ctx, const WgradCall &a, int splits, const int *tr, const unsigned *cmax, const WgradScales &b, int packed, float *xpart) {
    if (xpart) {
        GF_LAUNCH(ctx, "smpf_wgrad", (smp_wgrad_all<CB, 2, 3>), dim3((unsigned)splits), dim3(kW8Threads), 0, a.T, a.dO, a.rowscale, a.rows, a.part, tr, cmax, b.chan,
                  b.smax, b.row_max, packed, xpart);
    } else if (a.nf == 8) {
        GF_LAUNCH(ctx, "smpf_wgrad", (smp_wgrad_all<CB, 8>), dim3((unsigned)splits), dim3(kW8Threads), 0, a.T, a.dO, a.rowscale, a.rows, a.part, tr, cmax, b.chan,
                  b.smax, b.row_max, packed);
    } else {
        GF_LAUNCH(ctx, "smpf_wgrad", (smp_wgrad_all<CB, 2>), dim3((unsigned)splits), dim3(kW8Threads), 0, a.T, a.dO, a.rowscale, a.rows, a.part, tr, cmax, b.chan,
                  b.smax, b.row_max, packed);
    }
    return GF_OK;
}
// W = 1: the 64-channel launch; W = 2: the four (i, j) sub-block launches at 128 channels, each with its own job's bounds
template <int W>
gf_status launch_wgrad_split(gf_ctx *ctx, const WgradCall &a, const WgradPlan &p, const int *tr, const unsigned *cmax, const WgradScales &b, int packed) {
    const gf_status st = opt_in_lds(ctx, smp_wgrad_split<W>, kWsLds);
    if (st != GF_OK) return st;
    if (a.any_trow && (size_t)a.rows * 2 * a.C * sizeof(float) >= kWsWholeBytes)
        return fail(ctx, GF_ERR_INVALID, "smp_wgrad_partials: a table beyond the gather window of %lld rows on a dO of 1 GiB or more", kTrowWindow);
    const int window = a.any_trow ? a.rows : (int)kTrowWindow;
    for (int q = 0; q < W * W; ++q) {
        const int i = q >> 1, j = q & 1;
        GF_LAUNCH(ctx, "smpf_wgrad", smp_wgrad_split<W>, dim3((unsigned)p.splits), dim3(kWsThreads), kWsLds, a.T, a.dO, a.rowscale, a.rows, window, a.part, tr,
                  cmax ? cmax + q * (kWsACols + kWsBCols) : cmax, b.chan, b.smax, b.max_tot, b.max_tr, b.row_max, packed, 64 * i, 64 * j, 64 * i * 128 + 64 * j);
    }
    return GF_OK;
}

}  // namespace

size_t smp_wgrad_words(int C, bool exact) { return C == 64 && !exact ? 128 : wgrad_words(C).total; }

// (the eight products' images, the extra products' behind them, each with the room splitk_fold's second stage takes behind its images)
size_t smp_wgrad_part_floats(gf_ctx *ctx, int rows, int C, int nx) {
    const size_t splits = (size_t)wgrad_plan(ctx, rows, C).splits;
    return (splits + (splits + 31) / 32) * (size_t)(8 + nx) * C * C;
}

bool smp_wgrad_reads_absent_blocks(const gf_ctx *ctx, const WgradCall &a) {
    const WgradKernel k = wgrad_kernel(ctx, a);
    // the fp32 kernel does not mask; exact bounds are maxima over ALL of T; a split kernel masks iff it walks the packed table
    return !wgrad_level_bounds(k, a) || !wgrad_packed(k, a);
}

gf_status smp_wgrad_partials(gf_ctx *ctx, const WgradCall &a, FoldGroup *out, FoldGroup *xout) {
    const size_t CC = (size_t)a.C * a.C;
    *out = {a.part, 0, 8 * CC};
    if (xout) *xout = {nullptr, 0, 3 * CC};
    if (a.rows < 1) return GF_OK;
    const WgradKernel k = wgrad_kernel(ctx, a);
    if (k == WgradKernel::None) return fail(ctx, GF_ERR_UNSUPPORTED, "smp_wgrad_partials: %d channels", a.C);
    if (a.nf != 2 && !(a.nf == 8 && k == WgradKernel::All)) return fail(ctx, GF_ERR_UNSUPPORTED, "smp_wgrad_partials: %d row factors at %d channels", a.nf, a.C);
    const bool level = wgrad_level_bounds(k, a), exact = !level && k != WgradKernel::Fp32;
    if (exact && a.nf != 2) return fail(ctx, GF_ERR_UNSUPPORTED, "smp_wgrad_partials: exact column bounds with per-product row factors");
    if (exact && !a.words) return fail(ctx, GF_ERR_INVALID, "smp_wgrad_partials: exact column bounds without their scratch words");
    const WgradPlan p = wgrad_plan(ctx, a.rows, a.C);
    if ((size_t)p.splits * 8 * CC > a.part_floats)
        return fail(ctx, GF_ERR_NOMEM, "smp_wgrad_partials: %d partial images, room for %zu", p.splits, a.part_floats / (8 * CC));
    out->splits = p.splits;
    // SMP_2D_ver7's three extra products ride in smp_wgrad_all (their operands are fragments it already holds): three more images per
    // workgroup -- where the kernel has them (plain row factors) and the workspace the room; else the caller's own products
    float *xpart = nullptr;
    if (xout && k == WgradKernel::All && a.nf == 2 && smp_wgrad_part_floats(ctx, a.rows, a.C, 3) <= a.part_floats) {
        xpart = a.part + smp_wgrad_part_floats(ctx, a.rows, a.C, 0);
        *xout = {xpart, p.splits, 3 * CC};
    }
    if (exact) {
        const gf_status st = wgrad_exact_bounds(ctx, a);
        if (st != GF_OK) return st;
    }
    const unsigned *cmax = exact ? a.words + wgrad_words(a.C).cmax : nullptr;
    const WgradScales b = level ? a.bounds : WgradScales();
    const bool mask = wgrad_packed(k, a);
    const int *tr = mask ? a.trowf : a.trow;
    switch (k) {
    case WgradKernel::Fp32: return smp_wgrad_fp32_c64(ctx, a.T, a.dO, a.rowscale, a.rows, p.kchunk, p.splits, a.part, a.trow);
    case WgradKernel::Split64: return launch_wgrad_split<1>(ctx, a, p, tr, cmax, b, mask ? (a.skip_empty ? 2 : 1) : 0);
    case WgradKernel::Split128: return launch_wgrad_split<2>(ctx, a, p, tr, cmax, b, mask ? 1 : 0);
    default: break;
    }
    return a.C == 32 ? launch_wgrad_all<32>(ctx, a, p.splits, tr, cmax, b, mask ? 1 : 0, xpart) : launch_wgrad_all<16>(ctx, a, p.splits, tr, cmax, b, mask ? 1 : 0, xpart);
}

// words: [0, C) largest |f_{l-1}| per channel, [C, 2 C) largest |dz_l| per channel, accumulated here with atomicMax (the caller zeroes
// them).  fprev [prev_rows][ld0]: f_{l-1} or the per-panel maxima its combine-forward left; dsrc [drows][ld1]: the per-workgroup maxima
// of this level's combine-backward.  One launch: the four-rows-in-flight kernel for 64-float rows of 64 channels, else the general one.
gf_status smp_wgrad_channel_maxima(gf_ctx *ctx, const float *fprev, long long prev_rows, int ld0, const float *dsrc, long long drows, int ld1, int C,
                                   unsigned *words) {
    const long long big = prev_rows > drows ? prev_rows : drows, g0 = (big + 63) / 64;
    const unsigned g = (unsigned)(g0 < 1 ? 1 : g0 > 256 ? 256 : g0);
    if (C == 64 && ld0 == 64 && ld1 == 64)
        GF_LAUNCH(ctx, "smpf_colmax", level_channel_maxima, dim3(g, 2), dim3(256), 0, fprev, prev_rows, dsrc, drows, words);
    else
        GF_LAUNCH(ctx, "smpf_colmax", level_channel_maxima_ld, dim3(g, 2), dim3(256), 0, fprev, prev_rows, ld0, dsrc, drows, ld1, C, words);
    return GF_OK;
}

}  // namespace gf
