// smp_fused_tables.hip -- the table kernels of the fused SMP level (smp_fused.hip): tables-forward for the size classes and for the nodes
// above 32 positions, the vector sums, the zero fill of the blocks tables-forward skips, tables-backward, and their launchers.
#include "smp_fused_internal.h"

using namespace gf::dev;

namespace gf {
namespace {

// Totals of two tables over the four c-groups (16-lane rows) of a wave in ONE butterfly: v_permlane16_swap of (u, v) leaves
// {u.r0, v.r0, u.r2, v.r2} and {u.r1, v.r1, u.r3, v.r3}, whose sum pairs rows 0+1 and 2+3 of u in the even rows and of v in
// the odd rows; the xor-32 step finishes both.  Even c-groups end up with the total of u, odd ones with the total of v:
// half the lane traffic of reducing each table to all lanes.
__device__ __forceinline__ f4 fold_two_tables(f4 u, f4 v) {
    f4 z;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(u[k]), __float_as_uint(v[k]), false, false);
        z[k] = xor32_sum(__uint_as_float(r[0]) + __uint_as_float(r[1]));
    }
    return z;
}

// x of lane ^ 8 (a rotation by eight inside each 16-lane row: one DPP move per dword)
__device__ __forceinline__ f4 dpp_xor8(f4 v) {
    f4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r[k] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[k]), 0x128 /* row_ror:8 */, 0xf, 0xf, true));
    return r;
}

__device__ __forceinline__ f4 dpp_ror4(f4 v) {   // x of lane + 4 inside each 16-lane row (row_ror:4)
    f4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        r[k] = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[k]), 0x124 /* row_ror:4 */, 0xf, 0xf, true));
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
// T1w: tables-forward (s <= 4 NI, NI in {1, 2, 4, 8}).  One WAVE per (node, b): a workgroup covers four consecutive b of one
// node and shares the node's selection maps and row sums in LDS.  Lane = (c-group cg, channel quad fl) as in r18_fwd_slab;
// every row a of the slab P[:, b, :, :] is GATHERED straight from f_{l-1}[src(n, a)] through the selection map pi_a
// (P[a][b][c] = F_a[pi_a(b)][pi_a(c)] or 0), one row prefetched ahead.  A wave walks all rows a itself, so the sums over a
// stay in its registers: no cross-wave reduction, one barrier in the whole kernel.  (A workgroup-per-pair variant with the
// rows split over four waves paid about ten barriers of prologue/epilogue and was slower in every size class: 3.3 -> 2.6 ms
// for s <= 16, 0.73 -> 0.54 ms for 16 < s <= 32 at cfg3.)
// ---------------------------------------------------------------------------------------------------------------
#ifndef GF_TF_OCC
#define GF_TF_OCC 4   // waves per SIMD of the classes s <= 16 (five: the per-node kernel spills, 0.94 -> 1.08 ms)
#endif
// VEC (round 4, ALLOK only): the sums over b that smp_vectors used to collect in a pass of its own -- rowsum_a[x] = sum_b S_ab[x, b],
// D8[x] = sum_b P[x, b, b] and the per-node scalars -- are kept as the rows go by: every wave adds its (a, b) terms to LDS accumulators
// of its OWN (two 16-byte read-modify-writes per row, plain DS operations in wave order: no atomics; the lanes outside c-group 0 work
// on a slot nobody reads, so the row loop stays branch-free), the four waves' partials are folded in a fixed order after one barrier.
// tables-forward 0.90 -> 1.04 ms, smp_vectors (0.38 ms a cfg3 step, 1 GB of traffic) gone.  Measured and not kept: one read-modify-write
// per row with c-group 2 taking the diagonal element over lane ^ 32 (1.19 ms: the exchange sits on the row's critical path); the
// row sums only, D8 gathered from the compact diagonal table in the epilogue as smp_vectors did (1.10 ms).
// LPC (round 4): lanes per position -- 16 (64-channel windows) or 8 (32-channel windows: at C = 32 every lane has channels and a wave
// load covers eight positions; the sixteen-lane mapping left half of the lanes idle there).
template <int NI, bool ALLOK, bool VEC = false, int LPC = 16>  // ALLOK: C is a multiple of the window (4 LPC channels) -- every lane has channels
__global__ __launch_bounds__(kThreads, NI <= 4 ? GF_TF_OCC : 2) void smp_tables_fwd_w(  // (NI = 4 sat at 130 VGPRs: capped to 128 -> 4 waves per SIMD)
    const float *__restrict__ fprev, const float *__restrict__ rsum,
                                                             float *__restrict__ T, float *__restrict__ Vt,
                                                             float *__restrict__ scal, const long long *__restrict__ pair_src_row,
                                                             const int *__restrict__ pair_src_s, const short *__restrict__ pi,
                                                             const int4 *__restrict__ recs,  // two per node, in launch order (build_tf_records)
                                                             int C, int nwin,
                                                             int zeros_kept,  // != 0: the structurally-zero rows (a, b) hold their zeros
                                                             const unsigned char *__restrict__ rowflag,  // with zeros_kept: bit 1 =
                                                             // row (b, c) has data in S_bc / T10 (the others are not stored either)
                                                             float *__restrict__ St) {  // VEC: [nodes][4C] per-node scalars
    static_assert(!VEC || ALLOK, "the folded vector sums need every lane to have channels");
    constexpr int PPW = 64 / LPC, CWIN = 4 * LPC;   // positions per wave load, channels per window
    static_assert(LPC == 16 || ((LPC == 8 || LPC == 4) && ALLOK), "eight / four lanes per position: whole 32- / 16-channel windows only");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = lane / LPC, fl = lane % LPC;
    // launch order: molecule-major inside the size class, one contiguous run of it per XCD (blockIdx % 8): the source
    // tensors f_{l-1}[w] of a molecule are gathered by ~s consumers each, which then share an L2
    unsigned tile;
    {
        const unsigned nb = gridDim.x, qq = nb / 8, r = nb % 8, x = blockIdx.x % 8;
        tile = (x < r ? x * (qq + 1) : r * (qq + 1) + (x - r) * qq) + blockIdx.x / 8;
    }
    // ONE workgroup per node (round 3; it was one per four b): measured with every row but a wave's own skipped, two thirds of the
    // kernel's time were the workgroup's fixed costs -- three dependent table reads to find the node, the staging of its maps, the
    // barrier -- paid s / 4 times per node.  The node's record is one 32-byte read, the maps are staged once, and each wave walks
    // b = wave, wave + 4, ... on its own.
    const int win = (int)(tile % nwin);
    const int4 r0 = recs[2 * (tile / nwin)], r1 = recs[2 * (tile / nwin) + 1];
    const int N = r0.y;
    const size_t rowbase = ((size_t)(unsigned)r1.y << 32) | (unsigned)r1.x, pairbase = ((size_t)(unsigned)r1.w << 32) | (unsigned)r1.z;
    const int f = win * CWIN + 4 * fl;
    const bool fok = f < C;
    const int fld = fok ? f : 0;
    constexpr bool allok = ALLOK;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    // The address chain of a row is LDS reads only, and few of them: per row a the source tensor's descriptor words, per (a, c) the
    // BYTE offset of column pi_a(c) inside a row of the source (kAbsent -- beyond any source tensor, the buffer load returns 0 --
    // where pi_a(c) < 0 and in the padding c >= N), rows padded to the class's 4 NI positions so that a lane's NI reads are
    // unconditional and a constant 16 bytes apart.  (Round 3: the maps were shorts read one at a time behind a lane mask, each waited
    // for, multiplied and selected before its request went out: ~45 VALU and five LDS round trips per row in front of the loads.)
    constexpr int ST = PPW * NI;
    constexpr int kAbsent = 0x40000000;
    float *sR = smem;                                               // [N]
    int4 *sRow = reinterpret_cast<int4 *>(smem + ((N + 3) & ~3));   // [N] {address lo, hi, bytes, s_w} of f_{l-1}[src(n, a)]
    int *sOff = reinterpret_cast<int *>(sRow + N);                  // [N][ST]
    const int nthreads = kThreads;
    for (int i = tid; i < N; i += nthreads) {
        sR[i] = rsum[pairbase + i];
        const int sw = pair_src_s[pairbase + i];
        const unsigned long long addr = reinterpret_cast<unsigned long long>(fprev + pair_src_row[pairbase + i] * C);
        sRow[i] = make_int4((int)(unsigned)addr, (int)(unsigned)(addr >> 32), sw * sw * C * 4, sw);
    }
    for (int i = tid; i < N * ST; i += nthreads) {
        const int a = i / ST, c = i % ST;
        const int p = (c < N) ? pi[rowbase + a * N + c] : -1;
        sOff[i] = p >= 0 ? p * C * 4 : kAbsent;
    }
    unsigned char *sFlag = reinterpret_cast<unsigned char *>(sOff + N * ST);  // [N][N] the node's row flags
    const bool skip_bc = zeros_kept && rowflag;
    if (skip_bc)
        for (int i = tid; i < N * N; i += nthreads) sFlag[i] = rowflag[rowbase + i];
    // VEC: per wave, [N][rowsum | D8][64 floats] accumulators and a 64-float slot the lanes outside c-group 0 read and write instead
    f4 *sAcc = reinterpret_cast<f4 *>(smem + ((((N + 3) & ~3) + 4 * N + N * ST + ((N * N + 3) >> 2) + 3) & ~3));
    const int nwv = nthreads / 64;
    f4 *wacc = sAcc + (size_t)wave * N * (2 * LPC), *wdummy = sAcc + (size_t)nwv * N * (2 * LPC) + wave * (2 * LPC);
    if constexpr (VEC)
        for (int i = lane; i < N * (2 * LPC); i += 64) wacc[i] = splat(0.f);
    __syncthreads();

    float rc[NI];
    int cc[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = i * PPW + cg;
        cc[i] = (c < N) ? c : -1;
        rc[i] = (c < N && fok) ? sR[c] : 0.f;
    }
    for (int b = wave; b < N; b += nthreads / 64) {
    f4 sbc[NI], t10[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) sbc[i] = t10[i] = splat(0.f);
    f4 dgsum = splat(0.f);

    // Row a of the slab through a buffer descriptor of the source tensor f_{l-1}[src(n, a)] (wave-uniform base and row offset,
    // 32-bit lane offsets): a structurally-zero position gets an out-of-range offset and the hardware returns 0 -- no 64-bit
    // address arithmetic and no selects in the loop.  Only rows with pi_a(b) >= 0 are ever requested (`present` below), and every
    // lane requests: no branch, nothing for the compiler to lose count of the memory queue over.
    const int lane_off = fok ? fld * 4 : kAbsent;        // (lanes without channels -- C % 64 != 0 -- fetch nothing)
    const int diag_off = (cg < 2) ? lane_off : kAbsent;  // (the diagonal entries are c-groups 0 and 1's)
    auto load_row = [&](int a, f4(&v)[NI], f4 &dg) {
        const int4 ri = sRow[a];
        const int *orow = sOff + a * ST;
        const int ob = orow[b];
        int oc[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) oc[i] = orow[cg + PPW * i];
        const int od = orow[(cg == 0) ? b : a];  // pi_a(b) for c-group 0, pi_a(a) for the others
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)ri.x), hi = __builtin_amdgcn_readfirstlane((unsigned)ri.y);
        const int bytes = __builtin_amdgcn_readfirstlane(ri.z), sw = __builtin_amdgcn_readfirstlane(ri.w);
        const float *src = reinterpret_cast<const float *>(((unsigned long long)hi << 32) | lo);
        const __amdgpu_buffer_rsrc_t rs = make_rsrc(src, (size_t)(unsigned)bytes);
        const int rowoff = __builtin_amdgcn_readfirstlane(ob) * sw;  // row pi_a(b) of the source: pi_a(b) C 4 bytes x s_w
#pragma unroll
        for (int i = 0; i < NI; ++i) v[i] = buf_ld4(rs, oc[i] + lane_off, rowoff);
        dg = buf_ld4(rs, od + diag_off, rowoff);
    };

    // two row buffers used alternately (the loop is unrolled by two: no register copies between rows)
    f4 bufA[NI], bufB[NI], dA, dB;
    // (after fold_two_tables the EVEN 16-lane rows of the wave hold the S_ab total, the odd rows the T6 total)
    float *const tcol = T + (rowbase + b) * (size_t)(T_COLS * C) + f + (((lane >> 4) & 1) ? T_T6 : T_SAB) * C;  // (+ a N ldt per row)
    const size_t tstep = (size_t)N * (T_COLS * C);
    // Rows (a, b) whose source does not contain vertex b (pi_a(b) < 0) are structurally zero -- about 40 % of them at QM9
    // sizes: they are never loaded or summed, only their two table entries are written as zeros.  `present` is wave-uniform
    // (b is the wave's, a the loop's): bit a = row a has data.  The row of the node's own vertex (a == b) always has.
    unsigned present = (unsigned)__ballot(lane < N && sOff[(lane < N ? lane : 0) * ST + b] != kAbsent);
    present = __builtin_amdgcn_readfirstlane(present);
    if (allok) {
        if (!zeros_kept)  // (the zeros of these rows are already in the buffer, written once for this batch: DevLevel::t_zeros)
            for (unsigned z = ~present & (N >= 32 ? 0xffffffffu : ((1u << N) - 1u)); z; z &= z - 1)
                st4(tcol + (__builtin_ctz(z)) * tstep, splat(0.f));
    } else if (fok && cg < 2) {
        for (unsigned z = ~present & (N >= 32 ? 0xffffffffu : ((1u << N) - 1u)); z; z &= z - 1)
            st4(T + (rowbase + (size_t)__builtin_ctz(z) * N + b) * (size_t)(T_COLS * C) + f + (cg ? T_T6 : T_SAB) * C, splat(0.f));
    }
    auto row_step = [&](int a, int an, const f4(&cur)[NI], const f4 &dcur, f4(&nxt)[NI], f4 &dnxt, auto own_row) {
        load_row(an >= 0 ? an : a, nxt, dnxt);
        const float ra = sR[a];
        f4 sab = splat(0.f), t6 = splat(0.f);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const f4 v = cur[i];
            sbc[i] += v;
            t10[i] += ra * v;
            sab += v;
            t6 += rc[i] * v;
        }
        if constexpr (LPC <= 8) {   // the two c-groups of a 16-lane row first (lane ^ 8: a rotation by eight inside the row, on the VALU)
            sab += dpp_xor8(sab);
            t6 += dpp_xor8(t6);
        }
        if constexpr (LPC == 4) {   // ... four of them: the pairs' sums rotated by four (v[l] + v[l+8] + v[l+4] + v[l+12])
            sab += dpp_ror4(sab);
            t6 += dpp_ror4(t6);
        }
        const f4 both = fold_two_tables(sab, t6);  // even 16-lane rows: S_ab[a,b], odd rows: T6[a,b]
        dgsum += dcur;
        if (allok) {
            // every lane stores (c-groups 0/2 the S_ab block, 1/3 the T6 block; the pairs write identical values to the same
            // address): a store that all paths issue can be COUNTED by the compiler, so waiting for the next row's loads
            // (vmcnt is in order over loads and stores) need not include it; lane-conditional stores cannot (-5 %)
            gf_st_s<32>(reinterpret_cast<f4 *>(tcol + a * tstep), both);  // table row (a, b)
            if constexpr (VEC) {   // c-group 0 holds S_ab[a, b] and P[a, b, b]: into the wave's accumulators of row a
                f4 *slot = (cg == 0) ? wacc + a * (2 * LPC) + fl : wdummy + fl;
                const f4 r = slot[0] + both, d8 = slot[LPC] + dcur;
                slot[0] = r;
                slot[LPC] = d8;
            }
            if constexpr (decltype(own_row)::value) {  // a == b: the peeled first row
                if (cg == 0) st4(scal + ((pairbase + b) * 4 + 3) * (size_t)C + f, dcur);
                if (cg == 2 * (16 / LPC)) st4(scal + ((pairbase + b) * 4 + 1) * (size_t)C + f, both);   // (a c-group of an even row other than 0)
            }
        } else if (fok) {
            float *trow = T + (rowbase + (size_t)a * N + b) * (size_t)(T_COLS * C) + f;  // table row (a, b)
            if (cg == 0) {
                st4(trow + T_SAB * C, both);
                if (a == b) st4(scal + ((pairbase + b) * 4 + 3) * (size_t)C + f, dcur);
            } else if (cg == 1) {
                st4(trow + T_T6 * C, both);
            } else if (cg == 2) {
                if (a == b) st4(scal + ((pairbase + b) * 4 + 1) * (size_t)C + f, both);
            }
        }
    };
    {
        auto pop = [&]() {  // next present row, or -1
            if (!present) return -1;
            const int a = __builtin_ctz(present);
            present &= present - 1;
            return a;
        };
        if (ALLOK) {
            // Row a = b (the node's own vertex: always present) first, outside the loop, with its two extra stores; the loop over
            // the other rows then has no conditional store and is entered with the memory queue its back edge leaves (a row's
            // requests and one store): the compiler counts the queue (vmcnt(N)) instead of draining it -- stores included --
            // at the top of every pair of rows.  (Row order changes the order of the sums over a, not their terms.)
            present &= ~(1u << b);
            // (one row requested ahead; two, with three buffers in rotation, spilled: NOTES.md, "Switches retired")
            int a = b, an = pop();
            load_row(a, bufA, dA);
            row_step(a, an, bufA, dA, bufB, dB, std::true_type{});
            while (an >= 0) {
                a = an;
                an = pop();
                row_step(a, an, bufB, dB, bufA, dA, std::false_type{});
                if (an < 0) break;
                a = an;
                an = pop();
                row_step(a, an, bufA, dA, bufB, dB, std::false_type{});
            }
        } else {
            int a = pop();
            load_row(a, bufA, dA);
            for (;;) {
                int an = pop();
                row_step(a, an, bufA, dA, bufB, dB, std::false_type{});
                if (an < 0) break;
                a = an;
                an = pop();
                row_step(a, an, bufB, dB, bufA, dA, std::false_type{});
                if (an < 0) break;
                a = an;
            }
        }
    }
    f4 cs = splat(0.f);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (cc[i] >= 0) {
            cs += sbc[i];
            if (fok && (!skip_bc || (sFlag[b * N + cc[i]] & 2))) {
                float *trow = T + (rowbase + (size_t)b * N + cc[i]) * (size_t)(T_COLS * C) + f;  // table row (b, c)
                gf_st_s<32>(reinterpret_cast<f4 *>(trow + T_SBC * C), sbc[i]);
                gf_st_s<32>(reinterpret_cast<f4 *>(trow + T_T10 * C), t10[i]);
            }
        }
    }
    cs = reduce_cgroups<LPC>(cs);
    // diagonal sums: lanes of c-group 0 hold sum_a P[a,b,b], c-group 1 holds sum_a P[a,b,a]
    const f4 dactot = shfl_xor4(dgsum, LPC);  // c-group 0 lanes receive c-group 1's sum
    if (cg == 0 && fok) {
        float *v = Vt + (pairbase + b) * 4 * (size_t)C + f;
        st4(v + 1 * C, cs);
        st4(v + 3 * C, dactot);
        float *sc = scal + (pairbase + b) * 4 * (size_t)C + f;
        st4(sc + 0 * C, cs);
        st4(sc + 2 * C, dgsum);
    }
    }  // b
    if constexpr (VEC) {
        __syncthreads();   // (every wave's accumulators and partial scalars are complete and visible to the workgroup)
        const int node = r0.x;
        for (int i = tid; i < N * (2 * LPC); i += nthreads) {   // (row a, rowsum | D8, float4 q): the waves' partials in wave order
            const int a = i / (2 * LPC), rem = i % (2 * LPC);
            f4 v = sAcc[(size_t)a * (2 * LPC) + rem];
            for (int w = 1; w < nwv; ++w) v += sAcc[((size_t)w * N + a) * (2 * LPC) + rem];
            st4(Vt + (pairbase + a) * 4 * (size_t)C + (rem / LPC) * 2 * C + win * CWIN + 4 * (rem % LPC), v);
        }
        if (tid < 4 * LPC) {   // per-node scalars: the sum over b of the partials, in the order of b (as smp_vectors formed it)
            const int k = tid / LPC, q = tid % LPC;
            const auto one = [](int) { return 1.f; };
            st4(St + (size_t)node * 4 * C + k * C + win * CWIN + 4 * q,
                batched_sum(scal + pairbase * 4 * (size_t)C + k * C + win * CWIN + 4 * q, (size_t)4 * C, 0, N, one));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// tables-forward for the FEW nodes above 32 positions (33 .. 64; round 6): smp_tables_fwd_w keeps a wave's sums over a in registers by
// consumer position -- 4 NI positions, NI <= 8 -- and a 48-atom molecule's level-3 fields reach 35.  One workgroup per (node, b), plain
// loops, every sum in index order; the same outputs as smp_tables_fwd_w<NI, true, false> (the sums over b are smp_vectors', launched
// over these nodes behind it):
//   T[(a, b)] = [S_ab | . | T6 | .]  for the rows with an image (pi_a(b) >= 0; the others: zeros unless the level keeps them masked)
//   T[(b, c)] = [. | S_bc | . | T10] for the rows some source covers (all of them when the level does not mask)
//   Vt[(n, b)] blocks 1, 3 = sum_c S_bc[b, c], sum_a P[a, b, a];  scal[(n, b)] = {sum_c S_bc[b, c], S_ab[b, b], sum_a P[a, b, b], P[b, b, b]}
// with P[a, b, c] = f_{l-1}[w_a][pi_a(b)][pi_a(c)] or 0 (SMP_omega.h:641-651, RisiContraction_18.h:98-322 factorised as in DESIGN.md 4.5).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smp_tables_fwd_big(const float *__restrict__ fprev, const float *__restrict__ rsum, float *__restrict__ T,
                                                          float *__restrict__ Vt, float *__restrict__ scal,
                                                          const long long *__restrict__ pair_src_row, const int *__restrict__ pair_src_s,
                                                          const short *__restrict__ pi, const int *__restrict__ pair_node,
                                                          const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                          const long long *__restrict__ node_pair, long long pair0, int C, int zeros_kept,
                                                          const unsigned char *__restrict__ rowflag) {
    const long long e = pair0 + blockIdx.x;
    const int n = pair_node[e], N = node_s[n];
    const size_t rowbase = (size_t)node_row[n], pairbase = (size_t)node_pair[n];
    const int b = (int)(e - (long long)pairbase), nl = C >> 2, tid = threadIdx.x;
    extern __shared__ __attribute__((aligned(16))) float big_smem[];
    float *sBC = big_smem;                       // [N][C] S_bc[b, c], then: P[a, b, b]
    float *sAC = sBC + (size_t)N * C;            // [N][C] P[a, b, a]
    float *sR = sAC + (size_t)N * C;             // [N]
    long long *sSrc = reinterpret_cast<long long *>(sR + ((N + 3) & ~3));   // [N] first float of f_{l-1}[w_a]
    int *sSw = reinterpret_cast<int *>(sSrc + N);                           // [N]
    short *sPi = reinterpret_cast<short *>(sSw + N);                        // [N][N] pi_a(x)
    for (int i = tid; i < N; i += 256) {
        sR[i] = rsum[pairbase + i];
        sSrc[i] = pair_src_row[pairbase + i] * C;
        sSw[i] = pair_src_s[pairbase + i];
    }
    for (int i = tid; i < N * N; i += 256) sPi[i] = pi[rowbase + i];
    __syncthreads();
    const bool skip_bc = zeros_kept && rowflag;
    // rows (b, c): sums over the sources a
    for (int it = tid; it < N * nl; it += 256) {
        const int c = it / nl, f = 4 * (it - c * nl);
        f4 sbc = splat(0.f), t10 = splat(0.f);
        for (int a = 0; a < N; ++a) {
            const int pb = sPi[a * N + b], pc = sPi[a * N + c];
            if (pb >= 0 && pc >= 0) {
                const f4 v = ld4(fprev + sSrc[a] + ((size_t)pb * sSw[a] + pc) * C + f);
                sbc += v;
                t10 += sR[a] * v;
            }
        }
        st4(sBC + (size_t)c * C + f, sbc);
        if (!skip_bc || (rowflag[rowbase + (size_t)b * N + c] & 2)) {
            float *trow = T + (rowbase + (size_t)b * N + c) * (size_t)(T_COLS * C) + f;
            st4(trow + T_SBC * C, sbc);
            st4(trow + T_T10 * C, t10);
        }
    }
    __syncthreads();
    f4 cs = splat(0.f);
    if (tid < nl)
        for (int c = 0; c < N; ++c) cs += ld4(sBC + (size_t)c * C + 4 * tid);
    __syncthreads();   // (sBC is reused below)
    // rows (a, b): sums over c; the two diagonal elements of the row on the way
    for (int it = tid; it < N * nl; it += 256) {
        const int a = it / nl, f = 4 * (it - a * nl);
        const int pb = sPi[a * N + b];
        f4 sab = splat(0.f), t6 = splat(0.f), dbb = splat(0.f), dac = splat(0.f);
        if (pb >= 0) {
            const float *src = fprev + sSrc[a] + (size_t)pb * sSw[a] * C + f;
            for (int c = 0; c < N; ++c) {
                const int pc = sPi[a * N + c];
                if (pc >= 0) {
                    const f4 v = ld4(src + (size_t)pc * C);
                    sab += v;
                    t6 += sR[c] * v;
                    if (c == b) dbb = v;
                    if (c == a) dac = v;
                }
            }
        }
        if (pb >= 0 || !zeros_kept) {
            float *trow = T + (rowbase + (size_t)a * N + b) * (size_t)(T_COLS * C) + f;
            st4(trow + T_SAB * C, sab);
            st4(trow + T_T6 * C, t6);
        }
        st4(sBC + (size_t)a * C + f, dbb);
        st4(sAC + (size_t)a * C + f, dac);
        if (a == b) {   // the node's own vertex: always present
            st4(scal + ((pairbase + b) * 4 + 3) * (size_t)C + f, dbb);
            st4(scal + ((pairbase + b) * 4 + 1) * (size_t)C + f, sab);
        }
    }
    __syncthreads();
    if (tid < nl) {
        const int f = 4 * tid;
        f4 dgsum = splat(0.f), dactot = splat(0.f);
        for (int a = 0; a < N; ++a) {
            dgsum += ld4(sBC + (size_t)a * C + f);
            dactot += ld4(sAC + (size_t)a * C + f);
        }
        float *v = Vt + (pairbase + b) * 4 * (size_t)C + f;
        st4(v + 1 * C, cs);
        st4(v + 3 * C, dactot);
        float *sc = scal + (pairbase + b) * 4 * (size_t)C + f;
        st4(sc + 0 * C, cs);
        st4(sc + 2 * C, dgsum);
    }
}
static size_t tables_big_lds(int N, int C) {
    return sizeof(float) * (2 * (size_t)N * C + ((N + 3) & ~3)) + sizeof(long long) * N + sizeof(int) * N + sizeof(short) * (size_t)N * N + 32;
}

// rowsum_a[x] = sum_b S_ab[x,b], D8[x] = sum_b Dbb[x,b] per (node, x); scalars per node = sum over b of the partials.
// Items = (x, float4 lane); the s loads of an item are issued in batches of 8 (batched_sum).
__global__ __launch_bounds__(256) void smp_vectors(const float *__restrict__ T, float *__restrict__ Vt,
                                                   const float *__restrict__ scal, float *__restrict__ St,
                                                   const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                   const long long *__restrict__ node_pair, int C,
                                                   const float *__restrict__ Fdc, const long long *__restrict__ pair_src_pair,
                                                   const short *__restrict__ pi) {
    const int n = blockIdx.x;
    const int s = node_s[n], nl = C / 4;
    const size_t rowbase = (size_t)node_row[n], pairbase = (size_t)node_pair[n];
    const auto one = [](int) { return 1.f; };
    for (int i = threadIdx.x; i < s * nl; i += blockDim.x) {
        const int fl = i % nl, x = i / nl;
        const float *t = T + (rowbase + (size_t)x * s) * (size_t)(T_COLS * C) + T_SAB * C + 4 * fl;
        f4 rs = splat(0.f), d8 = splat(0.f);
        {  // D8[x] = sum_b P[x,b,b] = sum over the images pi_x(b) of f_{l-1}[w_x][p,p]  (compact table Fdc); the rows (x, b) with
           // pi_x(b) < 0 are structurally zero in S_ab as well: only the others are read (half of the 0.73 GB block at QM9 sizes)
            const float *fd = Fdc + (size_t)pair_src_pair[pairbase + x] * 2 * C + 4 * fl;
            const short *map = pi + rowbase + (size_t)x * s;
            for (int b0 = 0; b0 < s; b0 += 8) {
                f4 v[8], u[8];
                bool ok[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int p = (b0 + j < s) ? map[b0 + j] : -1;
                    ok[j] = p >= 0;
                    v[j] = ld4(fd + (size_t)(ok[j] ? p : 0) * 2 * C);
                    u[j] = ld4(ok[j] ? t + (size_t)(b0 + j) * (T_COLS * C) : fd);  // (absent: a line the lane has just read)
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (ok[j]) d8 += v[j], rs += u[j];
            }
        }
        st4(Vt + (pairbase + x) * 4 * (size_t)C + 0 * C + 4 * fl, rs);
        st4(Vt + (pairbase + x) * 4 * (size_t)C + 2 * C + 4 * fl, d8);
    }
    for (int i = threadIdx.x; i < C; i += blockDim.x)  // 4C floats = C float4
        st4(St + (size_t)n * 4 * C + 4 * i, batched_sum(scal + pairbase * 4 * (size_t)C + 4 * i, (size_t)4 * C, 0, s, one));
}

// zeros into the S_ab / T6 blocks of the rows (a, b), and the S_bc / T10 blocks of the rows (b, c), that tables-forward never
// writes: once per prepared batch (DevLevel::t_zeros; rowflag bits 0 / 1 = the row has data in the first / second pair of blocks)
constexpr int kZeroFillRows = 64;   // rows per workgroup: eight per pass (a thread was launched per (row, float4): 62 M threads at cfg3's level 3)
template <int CB>   // channels: 64 or 32
__global__ __launch_bounds__(256) void tables_zero_fill(float *__restrict__ T, const unsigned char *__restrict__ rowflag, long long rows) {
    constexpr int NQ = CB / 4, RPP = 256 / (2 * NQ), NP = kZeroFillRows / RPP;   // float4 per block, rows per pass, passes
    const int q = threadIdx.x % (2 * NQ);  // 2 NQ float4 = two CB-column blocks
    const long long row0 = (long long)blockIdx.x * kZeroFillRows + threadIdx.x / (2 * NQ);
    int fl[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {   // (all flags first: one round trip)
        const long long row = row0 + RPP * p;
        fl[p] = row < rows ? rowflag[row] : 3;
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const long long row = row0 + RPP * p;
        if (!(fl[p] & 1)) st4(T + row * (T_COLS * CB) + (q < NQ ? T_SAB * CB + 4 * q : T_T6 * CB + 4 * (q - NQ)), splat(0.f));
        if (!(fl[p] & 2)) st4(T + row * (T_COLS * CB) + (q < NQ ? T_SBC * CB + 4 * q : T_T10 * CB + 4 * (q - NQ)), splat(0.f));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// tables-backward.  Workgroup per (node, b): dP[:, b, :, :] from the table gradients.  Streaming phase as r18_bwd_slab.
//   dP[a,b,c] = X[a] + Y[c] + G5[a] r[c] + G9[c] r[a] + [c==b] Z1[a] + [c==a] Z2[a]
//   X[a]  = dS_ab[a,b] + d rowsum[a] + d colsum[b] + d total + [a==b] d s14
//   Y[c]  = dS_bc[b,c]     G5[a] = dT6[a,b]     G9[c] = dT10[b,c]
//   Z1[a] = dDbb[a,b] + dD8[a] + d s15 + [a==b] d s18          Z2[a] = dDac[a,b] + dD11[b]
// ---------------------------------------------------------------------------------------------------------------
template <int LPC, int NI>
__global__ __launch_bounds__(kThreads, 3) void smp_tables_bwd(const float *__restrict__ dT, const float *__restrict__ dVt,
                                                              const float *__restrict__ dSt, const float *__restrict__ A,
                                                              float *__restrict__ dP, const short *__restrict__ pi, Ragged R,
                                                              int C, int nwin) {
    constexpr int PPW = 64 / LPC;
    constexpr int CW = 4 * LPC;
    constexpr int NGRP = kThreads / LPC;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = lane / LPC, fl = lane % LPC;
    const int grp = tid / LPC;
    const Where W = locate(R, nwin);
    const int N = W.N, b = W.i;
    const size_t rowbase = W.rowbase, pbase = W.pbase, pairbase = W.pairbase;
    const int f = W.win * CW + 4 * fl;
    const bool fok = f < C;
    const int fc = fok ? f : 0;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AdjLds L = load_adjacency<false>(smem, A + rowbase, N);
    float *sX = smem + adj_lds_floats(N);
    float *sG5 = sX + N * CW;
    float *sZ1 = sG5 + N * CW;
    float *sZ2 = sZ1 + N * CW;
    // Selection maps of the node: dP[a][b][c] is only ever read by the consumer gather where pi_a(b) and pi_a(c) exist
    // (the promoted tensor is zero elsewhere, about two thirds of it at QM9 sizes), so only those positions are written.
    short *sPi = reinterpret_cast<short *>(sZ2 + N * CW);
    for (int i = tid; i < N * N; i += kThreads) sPi[i] = pi[rowbase + i];
    {
        const float *ds = dSt + (size_t)W.node * 4 * C + fc;
        const f4 dtotal = ld4(ds + 0 * C), ds14 = ld4(ds + 1 * C), ds15 = ld4(ds + 2 * C), ds18 = ld4(ds + 3 * C);
        const float *dvb = dVt + (pairbase + b) * 4 * (size_t)C + fc;
        const f4 dcol = ld4(dvb + 1 * C), dd11 = ld4(dvb + 3 * C);
        for (int a = grp; a < N; a += NGRP) {
            const float *t = dT + (rowbase + (size_t)a * N + b) * (size_t)(T_COLS * C) + fc;  // table row (a, b)
            const float *dva = dVt + (pairbase + a) * 4 * (size_t)C + fc;
            f4 x = ld4(t + T_SAB * C) + ld4(dva + 0 * C) + dcol + dtotal;
            // (the D_bb / D_ac table gradients reach df_{l-1} through the compact path: dFdc in the consumer gather)
            f4 z1 = ld4(dva + 2 * C) + ds15;
            if (a == b) {
                x += ds14;
                z1 += ds18;
            }
            const f4 m = fok ? splat(1.f) : splat(0.f);
            st4(sX + a * CW + 4 * fl, x * m);
            st4(sG5 + a * CW + 4 * fl, ld4(t + T_T6 * C) * m);
            st4(sZ1 + a * CW + 4 * fl, z1 * m);
            st4(sZ2 + a * CW + 4 * fl, dd11 * m);
        }
    }
    __syncthreads();

    f4 yv[NI], g9[NI];
    float rc[NI];
    int coff[NI], cxs[NI];
    bool live[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = i * PPW + cg;
        const bool ok = c < N;
        const int cx = ok ? c : 0;
        cxs[i] = cx;
        live[i] = ok && fok;
        coff[i] = cx * C + fc;
        rc[i] = L.r[cx];
        const float *t = dT + (rowbase + (size_t)b * N + cx) * (size_t)(T_COLS * C) + fc;  // table row (b, c)
        yv[i] = ld4(t + T_SBC * C);
        g9[i] = ld4(t + T_T10 * C);
    }
    const int ib = b / PPW, cgb = b % PPW;
    float *dPg = dP + pbase * C + (size_t)b * N * C;
    const size_t rowStride = (size_t)N * N * C;
    for (int a = wave; a < N; a += kWaves) {
        const short *map = sPi + a * N;
        if (map[b] < 0) continue;  // wave-uniform: the whole row (a, b, :) of the promoted tensor is structurally zero
        float *row = dPg + a * rowStride;
        const f4 xa = ld4(sX + a * CW + 4 * fl), g5a = ld4(sG5 + a * CW + 4 * fl);
        const float ra = L.r[a];
        const int ia = a / PPW, cga = a % PPW;
        const f4 z1 = ld4(sZ1 + a * CW + 4 * fl) * ((cg == cgb) ? 1.f : 0.f);
        const f4 z2 = ld4(sZ2 + a * CW + 4 * fl) * ((cg == cga) ? 1.f : 0.f);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            f4 o = xa + yv[i] + g5a * rc[i] + g9[i] * ra;
            if (i == ib) o += z1;
            if (i == ia) o += z2;
            if (live[i] && map[cxs[i]] >= 0) st4(row + coff[i], o);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// tables-forward of a level whose sources are ALL single vertices (level 1: the sources are the level-0 nodes).  Then
// P[a, b, c] = f_0[src(n, b)] where a == b == c and 0 elsewhere, and every output of smp_tables_fwd_w<NI, true, true, LPC> is a copy of
// a row of f_0, that row times r[b], a zero, or -- the per-node scalars -- the sum of the node's source rows in the order of b:
//   T[(b, b)] = [f | f | r f | r f],  Vt[(n, b)] = [f | f | f | f],  scal[(n, b)] = [f | f | f | f],  St[n] = 4 x sum_b f
// and the zeros of the rows (a, b), a != b, under the policy of that kernel (none where the level keeps its zeros; S_bc / T10 only on
// the rows flagged as covered).  The general kernel spends a workgroup, its staged maps and two barriers per node on this; here LPC
// lanes take a (node, b) pair -- no LDS, no barrier -- and behind the pairs one lane group per node forms St.  The sums of the general
// kernel have one non-zero term each, so the values are its values (a zero may differ in sign: it adds its term to +0).
// One difference on non-finite data: the general kernel forms St with batched_sum, which pads a batch of eight with 0 x (a re-read
// row) -- NaN if f_0 holds an Inf or a NaN there -- and this kernel skips the padding terms: with finite f_0 the same bits, with an
// Inf or NaN in f_0 St may differ (both are already non-finite downstream of that row).
// C = 4 LPC channels (one window).
// ---------------------------------------------------------------------------------------------------------------
template <int LPC>
__global__ __launch_bounds__(256) void smp_tables_fwd_single(const float *__restrict__ fprev, const float *__restrict__ rsum, float *__restrict__ T,
                                                             float *__restrict__ Vt, float *__restrict__ scal, float *__restrict__ St,
                                                             const long long *__restrict__ pair_src_row, const int *__restrict__ pair_node,
                                                             const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                             const long long *__restrict__ node_pair, long long pair_lo, int npairs, int node_lo,
                                                             int nnodes, int zeros_kept, const unsigned char *__restrict__ rowflag) {
    constexpr int C = 4 * LPC, GPB = 256 / LPC;
    constexpr size_t ldt = (size_t)T_COLS * C;
    const int fl = (int)threadIdx.x % LPC;
    const long long g = (long long)blockIdx.x * GPB + (int)threadIdx.x / LPC;
    if (g < npairs) {
        const long long pe = pair_lo + g;
        const int n = pair_node[pe], N = node_s[n];
        const long long pairbase = node_pair[n], rowbase = node_row[n];
        const int b = (int)(pe - pairbase);
        const f4 v = ld4(fprev + pair_src_row[pe] * C + 4 * fl);
        const f4 vz = v + splat(0.f), rz = rsum[pe] * v + splat(0.f);   // (as the sums that start from +0 leave them)
        const bool skip_bc = zeros_kept && rowflag;
        float *Tn = T + (size_t)rowbase * ldt + 4 * fl;
        for (int x = 0; x < N; ++x) {
            if (x == b) continue;
            if (!zeros_kept) {   // row (a = x, b): no image
                st4(Tn + ((size_t)x * N + b) * ldt + T_SAB * C, splat(0.f));
                st4(Tn + ((size_t)x * N + b) * ldt + T_T6 * C, splat(0.f));
            }
            if (!skip_bc || (rowflag[rowbase + b * N + x] & 2)) {   // row (b, c = x)
                st4(Tn + ((size_t)b * N + x) * ldt + T_SBC * C, splat(0.f));
                st4(Tn + ((size_t)b * N + x) * ldt + T_T10 * C, splat(0.f));
            }
        }
        float *td = Tn + ((size_t)b * N + b) * ldt;
        st4(td + T_SAB * C, vz);
        st4(td + T_T6 * C, rz);
        if (!skip_bc || (rowflag[rowbase + b * N + b] & 2)) {
            st4(td + T_SBC * C, vz);
            st4(td + T_T10 * C, rz);
        }
        float *vt = Vt + (size_t)pe * 4 * C + 4 * fl, *sc = scal + (size_t)pe * 4 * C + 4 * fl;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            st4(vt + k * C, vz);
            st4(sc + k * C, k == 3 ? v : vz);   // (block 3 is the loaded row itself)
        }
    } else if (g < (long long)npairs + nnodes) {
        const int n = node_lo + (int)(g - npairs), N = node_s[n];
        const long long pairbase = node_pair[n];
        f4 s = splat(0.f);
        for (int b0 = 0; b0 < N; b0 += 8) {
            f4 t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = ld4(fprev + pair_src_row[pairbase + (b0 + j < N ? b0 + j : 0)] * C + 4 * fl);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (b0 + j < N) s += t[j];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) st4(St + (size_t)n * 4 * C + k * C + 4 * fl, s);
    }
}

template <int LPC>
size_t tables_bwd_lds(int N) {
    constexpr int CW = 4 * LPC;
    return sizeof(float) * ((size_t)adj_lds_floats(N) + 4 * (size_t)N * CW) + sizeof(short) * (size_t)N * N + 16;
}

Ragged ragged_for(const gf_smp::DevLevel &d, long long lo, int smax) {
    Ragged R = {d.pair_node, d.node_s, d.node_p, d.node_row, d.node_pair, lo, smax};
    return R;
}

// launch names of tables-forward: one per NI, as rocprof lists kernels by symbol (the bench's "dominant kernel" is the
// symbol with the largest time per step; it sums these four for the kernel's own roofline line)
template <int NI>
constexpr const char *tables_fwd_name() {
    return NI == 1 ? "smpf_tables_fwd_ni1" : NI == 2 ? "smpf_tables_fwd_ni2" : NI == 4 ? "smpf_tables_fwd_ni4" : "smpf_tables_fwd_ni8";
}
// One size class at LPC lanes per position (64 / LPC positions per wave load, classes of 4 NI, 8 NI, 16 NI positions for LPC = 16, 8, 4).
// fold: the kernel keeps the sums over b of smp_vectors itself (VEC; always at 8 and 4 lanes).
template <int NI, int LPC>
gf_status launch_tables_fwd_class(gf_smp *s, int l, const SizeClass &c, bool fold) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    constexpr int PPW = 64 / LPC, CW = 4 * LPC;
    const int C = s->cfg.nChanels, nwin = (C + CW - 1) / CW;
    // nodes of the class: nodes are sorted by size, so the class is a contiguous node range -- and the same range of positions in
    // the level's (class, molecule) order, which is the order of the records (build_tf_records)
    const int n_lo = h.pair_node[(size_t)c.lo], n_hi = (c.hi < (long long)h.pairs) ? h.pair_node[(size_t)c.hi] : h.nNodes;
    if (n_hi <= n_lo) return GF_OK;
    const dim3 grid((unsigned)((n_hi - n_lo) * nwin));
    const size_t lds = sizeof(float) * ((c.smax + 3) & ~3) + 16 * (size_t)c.smax + sizeof(int) * (size_t)c.smax * PPW * NI + 16 +
                       (size_t)c.smax * c.smax + 16;
    const int flags = d.t_zeros ? 1 : 0;   // (only ever set at 64 / 32 / 16 channels, where the kernel folds: fused_route)
    if (!fold) {
        if constexpr (LPC == 16)
            GF_LAUNCH(ctx, tables_fwd_name<NI>(), (smp_tables_fwd_w<NI, false>), grid, dim3(kThreads), lds, s->lv[l - 1].f, d.rsum, d.Q, d.Vt, d.scal,
                      d.pair_src_row, d.pair_src_s, d.pi, d.tf_recs + 2 * (size_t)n_lo, C, nwin, flags, (const unsigned char *)nullptr, (float *)nullptr);
        return GF_OK;
    }
    // a level of single-vertex sources (level 1) at one window of channels: a lane group per (node, b) pair (GF_SMP_LEVEL1=0: the kernel below)
    const std::vector<gfsmp::Bucket> &src = s->lay.level[l - 1].buckets;
    if (!src.empty() && src.back().s == 1 && C == CW && smp_level1_switch()) {
        const long long work = (c.hi - c.lo) + (n_hi - n_lo);
        constexpr int GPB = 256 / LPC;
        GF_LAUNCH(ctx, tables_fwd_name<NI>(), smp_tables_fwd_single<LPC>, dim3((unsigned)((work + GPB - 1) / GPB)), dim3(256), 0, s->lv[l - 1].f, d.rsum,
                  d.Q, d.Vt, d.scal, d.St, d.pair_src_row, d.pair_node, d.node_s, d.node_row, d.node_pair, (long long)c.lo, (int)(c.hi - c.lo), n_lo,
                  n_hi - n_lo, flags, flags ? d.rowflag : (const unsigned char *)nullptr);
        ++s->single_launches;
        return GF_OK;
    }
    const int nwv = kThreads / 64;
    const size_t lds_v = ((lds + 15) & ~(size_t)15) + 16 + (size_t)nwv * ((size_t)c.smax * (32 * LPC) + 32 * LPC);
    gf_status st = opt_in_lds(ctx, smp_tables_fwd_w<NI, true, true, LPC>, lds_v);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, tables_fwd_name<NI>(), (smp_tables_fwd_w<NI, true, true, LPC>), grid, dim3(kThreads), lds_v, s->lv[l - 1].f, d.rsum, d.Q, d.Vt, d.scal,
              d.pair_src_row, d.pair_src_s, d.pi, d.tf_recs + 2 * (size_t)n_lo, C, nwin, flags, flags ? d.rowflag : (const unsigned char *)nullptr, d.St);
    return GF_OK;
}

template <int NI>
gf_status launch_tables_bwd_class(gf_smp *s, int l, const SizeClass &c, const float *dT) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, nwin = (C + 63) / 64;
    const size_t lds = tables_bwd_lds<16>(c.smax);
    gf_status st = opt_in_lds(ctx, smp_tables_bwd<16, NI>, lds);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "smpf_tables_bwd", (smp_tables_bwd<16, NI>), dim3((unsigned)((c.hi - c.lo) * nwin)), dim3(kThreads), lds, dT,
              d.dVt, d.dSt, d.adj, s->P, d.pi, ragged_for(d, c.lo, c.smax), C, nwin);
    return GF_OK;
}
}  // namespace

std::vector<SizeClass> classes_of(const gfsmp::LevelLayout &h, int ppw) {
    std::vector<SizeClass> out;
    size_t k = 0;
    for (int cls = 1; cls <= 8 && k < h.buckets.size(); cls *= 2) {
        const size_t k0 = k;
        int smax = 0;
        // (never beyond 32 positions, whatever the lanes per position: the nodes above take smp_tables_fwd_big -- big_part)
        while (k < h.buckets.size() && h.buckets[k].s <= cls * ppw && h.buckets[k].s <= 32) smax = h.buckets[k++].s;
        if (k == k0) continue;
        SizeClass c;
        c.lo = h.node_pair[h.buckets[k0].first_node];
        c.hi = (k < h.buckets.size()) ? h.node_pair[h.buckets[k].first_node] : (long long)h.pairs;
        c.smax = smax;
        c.ni = cls;
        out.push_back(c);
    }
    return out;
}

// the class's NI at the route's lanes per position: NI = 1, 2, 4, 8 at sixteen lanes, 1, 2, 4 at eight (s <= 8, 16, 32), 1, 2 at four
gf_status launch_tables_fwd(gf_smp *s, int l, const SizeClass &c, const FusedRoute &r) {
    const bool fold = r.fold_vectors;
    if (r.lpc == 4) return c.ni == 1 ? launch_tables_fwd_class<1, 4>(s, l, c, fold) : launch_tables_fwd_class<2, 4>(s, l, c, fold);
    if (r.lpc == 8)
        return c.ni == 1 ? launch_tables_fwd_class<1, 8>(s, l, c, fold)
             : c.ni == 2 ? launch_tables_fwd_class<2, 8>(s, l, c, fold) : launch_tables_fwd_class<4, 8>(s, l, c, fold);
    switch (c.ni) {
        case 1: return launch_tables_fwd_class<1, 16>(s, l, c, fold);
        case 2: return launch_tables_fwd_class<2, 16>(s, l, c, fold);
        case 4: return launch_tables_fwd_class<4, 16>(s, l, c, fold);
        default: return launch_tables_fwd_class<8, 16>(s, l, c, fold);
    }
}

// the nodes above 32 positions (none at QM9 sizes): their own tables-forward, see smp_tables_fwd_big
gf_status launch_tables_fwd_big(gf_smp *s, int l, const BigPart &big) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels;
    const size_t lds_b = tables_big_lds(big.smax, C);
    gf_status st = opt_in_lds(ctx, smp_tables_fwd_big, lds_b);
    if (st != GF_OK) return st;
    const int flags = d.t_zeros ? 1 : 0;   // (as launch_tables_fwd_class)
    GF_LAUNCH(ctx, "smpf_tables_fwd_big", smp_tables_fwd_big, dim3((unsigned)big.pairs), dim3(256), lds_b, s->lv[l - 1].f, d.rsum, d.Q, d.Vt, d.scal,
              d.pair_src_row, d.pair_src_s, d.pi, d.pair_node, d.node_s, d.node_row, d.node_pair, big.pair0, C, flags,
              flags ? d.rowflag : (const unsigned char *)nullptr);
    return GF_OK;
}

gf_status launch_vectors(gf_smp *s, int l, const FusedRoute &r, const BigPart &big) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const int C = s->cfg.nChanels;
    const float *T = d.Q;
    if (!r.fold_vectors)
        GF_LAUNCH(ctx, "smpf_vectors", smp_vectors, dim3(h.nNodes), dim3(node_block(h, C)), 0, T, d.Vt, d.scal, d.St, d.node_s, d.node_row,
                  d.node_pair, C, d.Fdc, d.pair_src_pair, d.pi);
    else if (big.nodes > 0)   // (smp_tables_fwd_w folds these sums itself; the big nodes' kernel leaves them to smp_vectors)
        GF_LAUNCH(ctx, "smpf_vectors", smp_vectors, dim3(big.nodes), dim3(256), 0, T, d.Vt, d.scal, d.St + (size_t)big.n0 * 4 * C, d.node_s + big.n0,
                  d.node_row + big.n0, d.node_pair + big.n0, C, d.Fdc, d.pair_src_pair, d.pi);
    return GF_OK;
}

gf_status launch_tables_bwd(gf_smp *s, int l, const SizeClass &c, const float *dT) {
    switch (c.ni) {
        case 1: return launch_tables_bwd_class<1>(s, l, c, dT);
        case 2: return launch_tables_bwd_class<2>(s, l, c, dT);
        case 4: return launch_tables_bwd_class<4>(s, l, c, dT);
        default: return launch_tables_bwd_class<8>(s, l, c, dT);
    }
}

// zeros into the blocks of T that tables-forward skips (DevLevel::t_zeros), unless they are there already
gf_status smp_fused_ensure_zero_fill(gf_smp *s, int l) {
    gf_smp::DevLevel &d = s->lv[l];
    if (!d.t_zeros || d.t_filled || !d.rowflag) return GF_OK;
    const long long rows = s->lay.level[l].rows;
    const int C = s->cfg.nChanels;
    void (*const fill)(float *, const unsigned char *, long long) = C == 16 ? tables_zero_fill<16> : C == 64 ? tables_zero_fill<64> : tables_zero_fill<32>;
    GF_LAUNCH(s->ctx, "smpf_tables_fill", fill, dim3((unsigned)((rows + kZeroFillRows - 1) / kZeroFillRows)), dim3(256), 0, d.Q, d.rowflag, rows);
    d.t_filled = true;
    return GF_OK;
}

// per-batch tables of smp_bwd_gather_v2, built on the device at prepare time on the handle's upload stream (behind the uploads
// of the consumer lists they are derived from)
// records of tables-forward: two int4 per node, in the level's (size class, molecule) order (mol_order):
//   {node, s, 0, 0}  {first row lo, hi, first pair lo, hi}
__global__ void build_tf_records(const int *__restrict__ mol_order, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                 const long long *__restrict__ node_pair, int4 *__restrict__ recs, int nodes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nodes) return;
    const int n = mol_order[i];
    const long long r = node_row[n], p = node_pair[n];
    recs[2 * i] = make_int4(n, node_s[n], 0, 0);
    recs[2 * i + 1] = make_int4((int)(unsigned)(r & 0xffffffffll), (int)(r >> 32), (int)(unsigned)(p & 0xffffffffll), (int)(p >> 32));
}

gf_status smp_build_tf_records(gf_smp *s, int l, hipStream_t stream) {
    gf_smp::DevLevel &d = s->lv[l];
    const int nodes = s->lay.level[l].nNodes;
    if (!d.tf_recs || nodes == 0) return GF_OK;
    hipLaunchKernelGGL(build_tf_records, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, stream, d.mol_order, d.node_s, d.node_row,
                       d.node_pair, d.tf_recs, nodes);
    GF_LAUNCH_CHECK(s->ctx, "build_tf_records");
    return GF_OK;
}

}  // namespace gf
