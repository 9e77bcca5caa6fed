// smp_level_wgrad_split.hip -- the weight gradients of the fused SMP level's eight row block products (C = 16 / 32 / 64 / 128, compact O
// layout) on the f16 matrix pipe with two-half fp32 operands: the kernels (smp_wgrad_split at 64 and, as four sub-block jobs, 128 channels;
// smp_wgrad_all at 32 / 16), the column bounds their per-column exponents come from, and the family's ONE entry point, smp_wgrad_partials
// (smp_internal.h: WgradCall).  The split arithmetic and what it shares with the products of smp_level_c64_split.hip: smp_split.h.
#include <cstdlib>
#include <type_traits>

#include "gemm_lds.h"
#include "gf_internal.h"
#include "smp_internal.h"
#include "smp_split.h"

namespace gf {
namespace {

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
    const long long cap = device_cu_count(ctx);
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
