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
//
// Here: the weight-image kernels, smp_rowpanel_split, smp_small_split, their launchers, and the products' ONE entry point
// (smp_row_products, at the end).  The split arithmetic and the image geometry: smp_split.h.  The weight gradients of the same products:
// smp_level_wgrad_split.hip.
#include <cstdlib>
#include <type_traits>

#include "gemm_lds.h"
#include "gf_internal.h"
#include "smp_internal.h"
#include "smp_split.h"

namespace gf {
namespace {

constexpr int kSpThreads = 512;            // two waves per SIMD, 256 registers each

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

// images of both directions of up to kSpImgLevels levels in one launch: workgroup (direction, level, position); the layout per (level,
// direction): smp_split.h
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

}  // namespace

bool smp_split_products(const gf_ctx *ctx) {  // (read per call: the parity tests switch it)
    if (ctx && ctx->fp32_products) return false;  // GF_OPT_SMP_FP32_PRODUCTS
    return !env_is("GF_SMP_SPLIT", '0');
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

// ---------------------------------------------------------------------------------------------------------------
// The eight row block products of a fused level, every channel count of the family: ONE entry point (smp_row_products) and ONE choice
// (row_products_kernel) -- which kernel a call runs, whether it walks the packed table, and, where no kernel takes the call, the status
// and the reason.  The launch switches on it; the stand-alone operators' refusals (smp_row_products_admissible) and the reverse sweep's
// question whether the kernel can form dz (smp_row_products_can_form_dz) are answers of the same function.  smp_internal.h: RowProductsCall.
// ---------------------------------------------------------------------------------------------------------------
namespace {

// Split: smp_rowpanel_split with plain row factors (64 / 32 / 16 channels); SplitExtras: with SMP_2D_ver7's three extra products (32 / 16);
// SplitFac8: one row factor per product (32 / 16); Classed: panels of one row class (64, backward); ClassedDz: ... forming dz itself;
// Split128: four sub-block passes of the 64-channel program; Fp32: smp_rowpanel_c64 (smp_level_c64.hip)
enum class RowProductsKernel { None, Fp32, Split, SplitExtras, SplitFac8, Classed, ClassedDz, Split128 };
struct RowProductsChoice {
    RowProductsKernel kernel = RowProductsKernel::None;
    bool mask = false;          // the launch walks the level's PACKED table (packed_rows)
    gf_status status = GF_OK;   // kernel == None: the refusal
    char reason[160] = {0};
};
RowProductsChoice refuse(gf_status st, const char *fmt, ...) {
    RowProductsChoice r;
    r.status = st;
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(r.reason, sizeof(r.reason), fmt, ap);
    va_end(ap);
    return r;
}
RowProductsChoice row_products_kernel(const gf_ctx *ctx, const RowProductsCall &c) {
    using K = RowProductsKernel;
    const bool small = c.C == 32 || c.C == 16, dz = c.dz.node_df != nullptr;
    if (!(c.trow && smp_split_products(ctx))) {   // the fp32 matrix pipe: 64 channels, plain row factors, every row stored, dO read whole
        if (c.skip_empty) return refuse(GF_ERR_INVALID, "smp_row_products: only the split row-panel kernel leaves the empty rows unstored");
        if (dz) return refuse(GF_ERR_INVALID, "smp_row_products: dz is formed by the split row-class kernel only");
        if (c.C != 64 || c.nf != 2 || c.nx != 0)
            return refuse(GF_ERR_UNSUPPORTED, "smp_row_products: %d channels / %d row factors / %d extra products on the fp32 matrix pipe", c.C, c.nf, c.nx);
        return {K::Fp32};
    }
    if (c.C != 64 && !c.wimg) return refuse(GF_ERR_UNSUPPORTED, "smp_row_products: %d channels need the level's prebuilt weight images", c.C);
    const bool mask = packed_rows(c.trowf, c.rows, 1 << 29);
    if (c.C == 128) {   // four sub-block passes of the 64-channel program (launch_rowpanel_c128); the row classes are not used
        if (c.nf != 2 || c.nx != 0) return refuse(GF_ERR_UNSUPPORTED, "smp_row_products: %d row factors / %d extra products at 128 channels", c.nf, c.nx);
        return {K::Split128, mask};
    }
    if (c.nx != 0) {   // the extra products of SMP_2D_ver7 on the 18-slice level (see the kernel)
        if (c.nx != 3 || c.nf != 2 || !small) return refuse(GF_ERR_UNSUPPORTED, "smp_row_products: %d extra products at %d channels / %d row factors", c.nx, c.C, c.nf);
        return {K::SplitExtras, mask};
    }
    if (c.nf != 2 && !(c.nf == 8 && small)) return refuse(GF_ERR_UNSUPPORTED, "smp_row_products: %d row factors at %d channels", c.nf, c.C);
    if (c.nf == 8) return {K::SplitFac8, mask};   // (per-product row factors: the slice-dropout towers, computed at 32 or 16 channels)
    if (small) return {K::Split, mask};
    if (c.C != 64) return refuse(GF_ERR_UNSUPPORTED, "smp_row_products: %d channels", c.C);
    // Panels of one row class (see the kernel): the masked backward products at C = 64 with the level's class lists, when the gradients
    // of structural zeros are skipped -- otherwise every row runs the full program and writes all four blocks, and the classes buy
    // nothing.  GF_SMP_ROW_CLASSES=0 (read per call, here only): the unclassed kernel.
    const bool classed = c.rowcls && !c.forward && c.skip_zero_grads && mask && !env_is("GF_SMP_ROW_CLASSES", '0');
    if (dz && !classed) return refuse(GF_ERR_INVALID, "smp_row_products: dz is formed by the row-class kernel only");
    return {classed ? (dz ? K::ClassedDz : K::Classed) : K::Split, mask};
}

}  // namespace

gf_status smp_row_products_admissible(gf_ctx *ctx, const RowProductsCall &c) {
    const RowProductsChoice k = row_products_kernel(ctx, c);
    return k.kernel == RowProductsKernel::None ? fail(ctx, k.status, "%s", k.reason) : GF_OK;
}

bool smp_row_products_can_form_dz(const gf_ctx *ctx, const RowProductsCall &c) {
    RowProductsCall plain = c;
    plain.dz = RowpanelDz();
    return row_products_kernel(ctx, plain).kernel == RowProductsKernel::Classed;
}

gf_status smp_row_products(gf_ctx *ctx, const RowProductsCall &c) {
    using K = RowProductsKernel;
    if (c.rows < 1) return GF_OK;
    const RowProductsChoice k = row_products_kernel(ctx, c);
    if (k.kernel == K::None) return fail(ctx, k.status, "%s", k.reason);
    if (k.kernel == K::Fp32) return smp_row_products_fp32_c64(ctx, c.forward, c.A, c.rowscale, c.Wst, c.Out, c.rows, c.trow);
    const bool forward = c.forward, mask = k.mask, classed = k.kernel == K::Classed || k.kernel == K::ClassedDz;
    const int per = kSpThreads / 64, cus = device_cu_count(ctx);
    const int npanels = (c.rows + 31) / 32 + (classed ? 1 : 0);   // (two padded lists: one panel more at the most)
    const int want = (npanels + per - 1) / per;
    // C = 64: one persistent workgroup per CU (the weight images take 128 KB of LDS); C = 32 (32 KB of images): two
    const int slots = c.C == 64 ? cus : 2 * cus;   // (C = 32 / 16: one or two per CU measured equal)
    const int grid = want < slots ? want : slots;
    if (k.kernel == K::Split128) {
        const int want128 = ((c.rows + 31) / 32 + per - 1) / per;
        const RowpanelArgs a = {want128 < cus ? want128 : cus, c.A, c.rowscale, c.Wst, c.Out, c.rows, mask ? c.trowf : c.trow, c.skip_zero_grads ? 1 : 0, nullptr};
        const uint4 *sets = static_cast<const uint4 *>(c.wimg);
        if (forward) return mask ? launch_rowpanel_c128<true, true>(ctx, a, sets) : launch_rowpanel_c128<true, false>(ctx, a, sets);
        return mask ? launch_rowpanel_c128<false, true>(ctx, a, sets) : launch_rowpanel_c128<false, false>(ctx, a, sets);
    }
    // (store_mask: backward, the gradients of structural zeros are not stored; forward, 64 channels: the rows of O without any data are not)
    const RowpanelArgs a = {grid, c.A, c.rowscale, c.Wst, c.Out, c.rows, mask ? c.trowf : c.trow, (forward ? (c.skip_empty && mask && c.C == 64) : c.skip_zero_grads) ? 1 : 0,
                            c.wimg ? static_cast<const uint4 *>(c.wimg) + (forward ? 0 : kSpImgStride) : nullptr};
    switch (k.kernel) {
    case K::SplitExtras: return c.C == 32 ? launch_rowpanel_split<32, 2, 3>(ctx, forward, mask, a) : launch_rowpanel_split<16, 2, 3>(ctx, forward, mask, a);
    case K::SplitFac8: return c.C == 32 ? launch_rowpanel_split<32, 8>(ctx, forward, mask, a) : launch_rowpanel_split<16, 8>(ctx, forward, mask, a);
    case K::ClassedDz: return launch_rowpanel_split<false, true, 64, 2, 0, true, 1, false, true>(ctx, a, c.rowcls, 0, 0, c.dz);
    case K::Classed: return launch_rowpanel_split<false, true, 64, 2, 0, true>(ctx, a, c.rowcls);
    default: break;   // Split
    }
    return c.C == 64 ? launch_rowpanel_split<64, 2>(ctx, forward, mask, a) : c.C == 32 ? launch_rowpanel_split<32, 2>(ctx, forward, mask, a) : launch_rowpanel_split<16, 2>(ctx, forward, mask, a);
}

}  // namespace gf
