// smp_fused_gather.hip -- the consumer gather of the fused SMP level (smp_fused.hip): df_{l-1} from the table gradients of level l, dP never
// materialised; its per-batch record tables.
#include "smp_fused_internal.h"

using namespace gf::dev;

namespace gf {
namespace {

// ---------------------------------------------------------------------------------------------------------------
// consumer gather with tables-backward folded in.  Per SOURCE node w of level l-1:
//   df_{l-1}[w][p,q] = [p==q] dFd[p] + [q==c_w] dFc[p] + sum over consumers (n,a), in consumer order, of dP_n[a, b, c]
// with b = inv(p), c = inv(q) both present, and dP_n[a,b,c] EVALUATED from the table gradients by the formula above
// smp_tables_bwd (same expression; only the two diagonal terms are summed separately) instead of being written by one
// kernel and read back by the next.  A lane owns (p, 4 channels) and keeps the accumulators of its row in registers.
// The [c == b] and [c == a] terms of dP land on fixed positions of the row: c == b means q == p (inv is injective), and c == a means
// q == c_w (the source's own vertex sits at position a of the consumer): they are summed over the consumers in two extra
// accumulators, which start from the compact-path gradients of the same two positions, and join the row at the end.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kGatherMaxS = 64;   // (32 until round 6)

// ---------------------------------------------------------------------------------------------------------------
// Nothing but memory requests and sums inside the consumer loop (round 3).  Round 2's kernel (a workgroup per source, consumer lists
// staged in LDS behind barriers, one launch per size class) spent three dependent round trips per consumer at three waves per SIMD: it
// was latency-bound (rocprof: the loop's instructions accounted for a tenth of its time), not issue-bound.  Here:
//   * everything wave-uniform about a consumer comes from two per-batch tables built on the device at prepare time
//     (build_gather_records): an 8-dword header per consumer entry (size, index, row / pair bases, node, r[a]) and a 4-dword record
//     per (entry, source position q): byte offset of the consumer's row (b = 0, c = inv(q)), r[c], presence m, m r[a].  They are
//     read with SCALAR loads, the header one consumer ahead: no LDS, no barrier, no readfirstlane, no per-lane address arithmetic
//     per position -- a position's two requests are buffer loads with a per-lane row offset (b s ldt) and a scalar column offset;
//   * the lane's own index b = inv(p) is requested one consumer ahead;
//   * ALL requests of a consumer (ten row terms + two per position, QB = SW positions at a time for SW <= 16) are issued before
//     the first sum: one round trip per consumer, 26 - 42 KB in flight per wave;
//   * absent positions (uniform) read the consumer's row c = 0 and are multiplied by m = 0; absent b (per lane) sends every
//     request of the lane out of range (zeros): no branch anywhere in the loop, so the memory queue is counted, not drained.
// Held against the two-kernel form (tables-backward writes dP, promote_backward gathers it: GF_SMP_BWD_GATHER=0) by
// tests/test_smp_gpu.py::test_folded_backward_gather_equals_the_two_kernel_path.
// ---------------------------------------------------------------------------------------------------------------
struct GatherTables {
    const int4 *hdr;   // [entries][2]: {s, a, row lo, row hi} {pair base lo, hi, node, r[a] bits}
    const int4 *qrec;  // gather_pad(s_w) records per entry: {row-c byte offset (0 when absent), r[c] bits, m bits, m r[a] bits}
};

// block per source node w: its consumer entries' headers and records (positions past s_w and absent positions: m = 0, row 0)
__global__ __launch_bounds__(64) void build_gather_records(const int *__restrict__ prev_s, const long long *__restrict__ cons_ptr,
                                     const long long *__restrict__ cons_qbase, const int *__restrict__ cons_s,
                                     const int *__restrict__ cons_a, const long long *__restrict__ cons_row,
                                     const long long *__restrict__ cons_pair, const int *__restrict__ pair_node,
                                     const long long *__restrict__ cons_inv_off, const short *__restrict__ inv,
                                     const float *__restrict__ rsum, int ldt_bytes, int4 *__restrict__ hdr, int4 *__restrict__ qrec) {
    const int w = blockIdx.x, sw = prev_s[w];
    const int pad = gfsmp::gather_pad(sw);
    const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1], qb = cons_qbase[w];
    for (long long ce = c0 + threadIdx.x; ce < c1; ce += blockDim.x) {
        const long long row = cons_row[ce], pe = cons_pair[ce], pb = pe - cons_a[ce];
        hdr[2 * ce] = make_int4(cons_s[ce], cons_a[ce], (int)(unsigned)(row & 0xffffffffll), (int)(row >> 32));
        hdr[2 * ce + 1] = make_int4((int)(unsigned)(pb & 0xffffffffll), (int)(pb >> 32), pair_node[pe], __float_as_int(rsum[pe]));
    }
    const long long n = (c1 - c0) * pad;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const long long ce = c0 + i / pad;
        const int q = (int)(i % pad);
        const long long pe = cons_pair[ce], pb = pe - cons_a[ce];
        const int c = q < sw ? (int)inv[cons_inv_off[ce] + q] : -1;
        // A position q without an image (or padding) multiplies what it loads by m = 0 -- but it still loads: from the row of the
        // FIRST position that has an image, a row (b, c') every b of this entry shares a source with (the entry's own), i.e. one that
        // is written every step (the backward products do not store the S_bc / T10 gradients of rows no source covers).
        int cfirst = 0;
        for (int k = 0; k < sw; ++k) {
            const int ck = (int)inv[cons_inv_off[ce] + k];
            if (ck >= 0) {
                cfirst = ck;
                break;
            }
        }
        const float ra = rsum[pe], rho = c >= 0 ? rsum[pb + c] : 0.f, m = c >= 0 ? 1.f : 0.f;
        qrec[qb + i] = make_int4((c >= 0 ? c : cfirst) * ldt_bytes, __float_as_int(rho), __float_as_int(m), __float_as_int(m * ra));
    }
}

// Scalar loads written out (s_load_dwordx4 + an explicit wait that "produces" the loaded values, so that nothing reads them before
// it).  Left to the compiler, a uniform global load becomes a scalar load only when it can prove that no store of the kernel
// clobbers it -- which it gives up on behind a scheduling barrier, behind a struct of pointers, and in every path of a switch but
// the first (observed): the fallback is a per-lane load plus a readfirstlane waterfall per use, ten times the instructions.
typedef int si4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ si4 s_load4(const int4 *p) {  // p must be wave-uniform
    si4 r;
    asm volatile("s_load_dwordx4 %0, %1, 0x0" : "=s"(r) : "s"(p));
    return r;
}
__device__ __forceinline__ void s_wait2(si4 &a, si4 &b) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(a), "+s"(b)); }
template <int N>
__device__ __forceinline__ void s_wait(si4 (&r)[N]) {
    if constexpr (N == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r[0]));
    else if constexpr (N == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r[0]), "+s"(r[1]));
    else if constexpr (N == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r[0]), "+s"(r[1]), "+s"(r[2]), "+s"(r[3]));
    else if constexpr (N == 5) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r[0]), "+s"(r[1]), "+s"(r[2]), "+s"(r[3]), "+s"(r[4]));
    else if constexpr (N == 6)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(r[0]), "+s"(r[1]), "+s"(r[2]), "+s"(r[3]), "+s"(r[4]), "+s"(r[5]));
    else {
        static_assert(N == 8, "batch sizes of the gather");
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+s"(r[0]), "+s"(r[1]), "+s"(r[2]), "+s"(r[3]), "+s"(r[4]), "+s"(r[5]), "+s"(r[6]), "+s"(r[7]));
    }
}

__device__ __forceinline__ f4 gbuf_ld4_once(__amdgpu_buffer_rsrc_t r, int voff_bytes) {
    return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, voff_bytes, 0, (GF_NT_SITES & 128) ? 2 : 0));
}
constexpr int kOor = 0x40000000;  // a lane offset no consumer's tables reach (<= 32 x 32 rows of 16 C bytes): the load returns 0

#define GF_GATHER_PARAMS                                                                                                          \
    const float *__restrict__ dT, const float *__restrict__ dVt, const float *__restrict__ dSt, float *__restrict__ dfprev,            \
        const float *__restrict__ dFdc, const int *__restrict__ prev_s, const long long *__restrict__ prev_row,                      \
        const long long *__restrict__ prev_pair, const int *__restrict__ prev_center, const long long *__restrict__ cons_ptr,        \
        const long long *__restrict__ cons_inv_off, const long long *__restrict__ cons_qbase, const short *__restrict__ inv,         \
        GatherTables G, int C
#define GF_GATHER_ARGS dT, dVt, dSt, dfprev, dFdc, prev_s, prev_row, prev_pair, prev_center, cons_ptr, cons_inv_off, cons_qbase, inv, G, C

// one source node w: SWP = gfsmp::gather_pad(s_w) accumulators and records per consumer; QB positions requested together.
// (The pointers stay individual __restrict__ kernel parameters: handed over in a struct they lose the no-alias guarantee against
//  the store of df, and the uniform table loads are then no longer selected as scalar loads.)
// One wave-sized work item: lanes [64 chunk, 64 chunk + 64) of source w's (row p, channel quad) space.  RS = records per consumer
// entry of this source (SWP, or 32 for the sources of 17 .. 32 positions, which run as two items of sixteen positions each:
// positions [qoff, qoff + 16)).
template <int SWP, int QB, int RS = SWP>
__device__ __forceinline__ void gather_source(GF_GATHER_PARAMS, int w, int chunk, int qoff = 0) {
    static_assert(SWP % QB == 0, "whole batches");
    const int sw = prev_s[w], cw = prev_center[w];
    const int nl = C >> 2, items = sw * nl;
    const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1];
    const int C4 = C * 4, ldtb = T_COLS * C4;  // bytes of a C-block, of a row of dT
    float *dst = dfprev + prev_row[w] * C;
    const float *dfd = dFdc + (size_t)prev_pair[w] * 2 * C;
    const long long ioff0 = c0 < c1 ? cons_inv_off[c0] : 0;  // (the entries of a source are consecutive in inv: sw shorts each)
    const int4 *qr0 = G.qrec + cons_qbase[w];
    {
        const int it = chunk * 64 + (int)(threadIdx.x & 63);
        const bool live = it < items;
        const int p = live ? it / nl : 0, f4b = 16 * (live ? it % nl : 0);
        f4 acc[SWP], accd = splat(0.f), accc = splat(0.f);
#pragma unroll
        for (int q = 0; q < SWP; ++q) acc[q] = splat(0.f);
        if (live) {
            accd = ld4(dfd + (size_t)p * 2 * C + (f4b >> 2));
            accc = ld4(dfd + (size_t)p * 2 * C + C + (f4b >> 2));
        }
        if (c0 < c1) {
            si4 h0 = s_load4(G.hdr + 2 * c0), h1 = s_load4(G.hdr + 2 * c0 + 1);
            s_wait2(h0, h1);
            int b = inv[ioff0 + p];  // (idle lanes read position 0 and are sent out of range below: no branch around a request)
            b = live ? b : -1;
            for (long long ce = c0; ce < c1; ++ce) {
                // header and lane index of the NEXT consumer (clamped re-read at the end: unconditional)
                const long long cn = ce + 1 < c1 ? ce + 1 : ce;
                si4 n0 = s_load4(G.hdr + 2 * cn), n1 = s_load4(G.hdr + 2 * cn + 1);  // (waited for at the end of this consumer)
                int bn = inv[ioff0 + (cn - c0) * sw + p];
                bn = live ? bn : -1;
                const int s = h0.x, a = h0.y;
                const long long urow = ((long long)h0.w << 32) | (unsigned)h0.z, upb = ((long long)h1.y << 32) | (unsigned)h1.x;
                const int unode = h1.z;
                const __amdgpu_buffer_rsrc_t rT = make_rsrc(dT + (size_t)urow * (T_COLS * C), (size_t)s * s * ldtb);
                const __amdgpu_buffer_rsrc_t rV = make_rsrc(dVt + (size_t)upb * 4 * C, (size_t)s * 4 * C4);
                const __amdgpu_buffer_rsrc_t rS = make_rsrc(dSt + (size_t)unode * 4 * C, (size_t)4 * C4);
                const bool has = b >= 0;
                const int tab = has ? (a * s + b) * ldtb + f4b : kOor;  // row (a, b) of the consumer's tables
                const int va = has ? a * 4 * C4 + f4b : kOor, vb = has ? b * 4 * C4 + f4b : kOor;
                const int vs = has ? f4b : kOor, vd = (has && p == cw) ? f4b : kOor;  // a == b  <=>  p is the source's own vertex
                const int tb = has ? b * s * ldtb + f4b : kOor;                          // row (b, 0)
                // (the S_ab / T6 gradient blocks of row (a, b) are read by this source alone, once: streamed -- GF_NT_SITES 128 -- so that they
                //  do not push the S_bc / T10 blocks, which every source of the consumer re-reads, out of the L2)
                const f4 l0 = gbuf_ld4_once(rT, tab + T_SAB * C4), g5 = gbuf_ld4_once(rT, tab + T_T6 * C4);
                const f4 l1 = buf_ld4(rV, va, 0), l4 = buf_ld4(rV, va + 2 * C4, 0);
                const f4 l2 = buf_ld4(rV, vb + C4, 0), z2 = buf_ld4(rV, vb + 3 * C4, 0);
                const f4 l3 = buf_ld4(rS, vs, 0), l5 = buf_ld4(rS, vs + 2 * C4, 0);
                const f4 l6 = buf_ld4(rS, vd + C4, 0), l7 = buf_ld4(rS, vd + 3 * C4, 0);
                const int4 *qr = qr0 + (ce - c0) * RS + qoff;
                f4 x = splat(0.f);
#pragma unroll
                for (int q0 = 0; q0 < SWP; q0 += QB) {
                    f4 y[QB], g9[QB];
                    si4 rec[QB];
#pragma unroll
                    for (int j = 0; j < QB; ++j) rec[j] = s_load4(qr + q0 + j);
                    s_wait(rec);  // (behind the row terms' requests; also lands the next header)
#pragma unroll
                    for (int j = 0; j < QB; ++j) {
                        y[j] = buf_ld4(rT, tb + T_SBC * C4, rec[j].x);
                        g9[j] = buf_ld4(rT, tb + T_T10 * C4, rec[j].x);
                    }
                    if (q0 == 0) x = ((l0 + l1) + (l2 + l3)) + l6;
#pragma unroll
                    for (int j = 0; j < QB; ++j) {
                        const float rho = __int_as_float(rec[j].y), m = __int_as_float(rec[j].z), mra = __int_as_float(rec[j].w);
                        acc[q0 + j] += m * (x + y[j]) + g5 * rho + g9[j] * mra;
                    }
                    // (no sched_barrier between the batches: the intrinsic counts as a memory clobber, after which the uniform
                    //  record loads of the loop are no longer selected as scalar loads but as per-lane loads + waterfall loops)
                }
                accd += (l4 + l5) + l7;
                accc += z2;
                s_wait2(n0, n1);
                h0 = n0;
                h1 = n1;
                b = bn;
            }
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < SWP; ++q)
                if (qoff + q < sw) {
                    f4 o = acc[q];
                    if (qoff + q == p) o += accd;
                    if (qoff + q == cw) o += accc;
                    gf_st_s<64>(reinterpret_cast<f4 *>(dst + ((size_t)p * sw + qoff + q) * C + (f4b >> 2)), o);
                }
        }
    }
}

// ONE launch per level, molecule by molecule (gfsmp::LevelLayout::gather_items): the rows (b, c) of a consumer are re-read by each of its
// ~s sources, of whatever size -- launched per size class, a molecule's table gradients were fetched from HBM once per class (rocprof:
// 1.24 -> 1.53 ms for the same kernel when the classes of the launch order were refined).  Every wave of the grid takes one work item
// of the level's list: (source, 64-lane chunk of its (p, channel quad) rows, eight positions q) -- a source of more than eight positions
// is several items, all sources molecule-major (smp_prep.cpp).  Waves are independent (no LDS, no barrier): a workgroup is just four
// consecutive items, whatever their sources' sizes; nothing is launched for rows a source does not have (idle waves of a
// workgroup-per-source grid cost 0.15 - 0.3 ms of wave launches per step).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void smp_bwd_gather_all(GF_GATHER_PARAMS,
                                                                                                      const int2 *__restrict__ items,
                                                                                                      int n_items) {
    // launch order: each XCD (blockIdx % 8) takes a contiguous run of the list
    unsigned blk;
    {
        const unsigned nb = gridDim.x, q = nb / 8, r = nb % 8, x = blockIdx.x % 8;
        blk = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + blockIdx.x / 8;
    }
    const int i = __builtin_amdgcn_readfirstlane((int)(blk * 4 + (threadIdx.x >> 6)));
    if (i >= n_items) return;
    const int2 item = items[i];
    const int w = __builtin_amdgcn_readfirstlane(item.x), chunk = __builtin_amdgcn_readfirstlane(item.y & 0xffff);
    const int qc = __builtin_amdgcn_readfirstlane(item.y >> 16);   // which eight positions q of the source (sources above eight positions)
    const int sw = prev_s[w];
    // Round 4: at most EIGHT accumulators per item -- a source of more positions runs as ceil(s_w / 8) items of eight positions q each
    // (the row terms of a consumer are requested by each of them: L1 hits).  128 registers, four waves per SIMD instead of three: the
    // kernel waits on its gathers (holding it to two waves per SIMD costs 20 %), and the sixteen-accumulator path set its budget.
    switch (gfsmp::gather_pad(sw)) {
        case 1: gather_source<1, 1>(GF_GATHER_ARGS, w, chunk); break;
        case 2: gather_source<2, 2>(GF_GATHER_ARGS, w, chunk); break;
        case 4: gather_source<4, 4>(GF_GATHER_ARGS, w, chunk); break;
        case 5: gather_source<5, 5>(GF_GATHER_ARGS, w, chunk); break;
        case 6: gather_source<6, 6>(GF_GATHER_ARGS, w, chunk); break;
        case 8: gather_source<8, 8>(GF_GATHER_ARGS, w, chunk); break;
        case 10:
            if (qc == 0) gather_source<8, 8, 10>(GF_GATHER_ARGS, w, chunk, 0);
            else gather_source<2, 2, 10>(GF_GATHER_ARGS, w, chunk, 8);
            break;
        case 12:
            if (qc == 0) gather_source<8, 8, 12>(GF_GATHER_ARGS, w, chunk, 0);
            else gather_source<4, 4, 12>(GF_GATHER_ARGS, w, chunk, 8);
            break;
        case 16: gather_source<8, 8, 16>(GF_GATHER_ARGS, w, chunk, 8 * qc); break;
        case 32: gather_source<8, 8, 32>(GF_GATHER_ARGS, w, chunk, 8 * qc); break;
        default: gather_source<8, 8, 64>(GF_GATHER_ARGS, w, chunk, 8 * qc); break;   // (sources of 33 .. 64 positions: level 4 of a 48-atom molecule)
    }
}

// ---------------------------------------------------------------------------------------------------------------
// A level whose sources are ALL single vertices (level 1: the sources are the level-0 nodes).  Every source is one item of the list
// and has one row (p = q = 0) of C / 4 = NL channel quads: as a wave of its own it runs with NL of 64 lanes live and pays one memory
// round trip per consumer for that quarter (at C = 64) of a wave's requests.  Here a wave takes 64 / NL CONSECUTIVE items, NL lanes
// each.  What was wave-uniform per source is now uniform per lane group only, so
//   * headers and records come by ordinary (per-lane, group-broadcast) loads, all of them one consumer ahead, and
//   * one buffer resource spans each table of the whole level: a consumer's base joins the lane offset (the launcher takes this kernel
//     only while those offsets stay below kOorAll);
//   * the loop runs to the longest consumer list of the wave; a group that is through requests nothing (every offset out of range)
//     and adds nothing.
// Per source the consumers come in the same order and the sums are the expression of gather_source<1, 1>, term for term.
// ---------------------------------------------------------------------------------------------------------------
// The offset of a lane that requests nothing: beyond every whole-level table this kernel is launched on (the launcher checks
// bytes < kOorAll).  Bit 31 is set on purpose: a raw buffer load range-checks voffset + the instruction's immediate as an UNSIGNED
// 32-bit byte offset against num_records, so the value is 2 GiB, not negative, whatever the builtin's `int` parameter suggests; the
// block constants added to it (at most 3 C 4 + 12 bytes: static_assert below) cannot wrap it, and an immediate the compiler folds
// out of the sum is added by the hardware as an unsigned 12-bit field -- the same sum.
constexpr unsigned kOorAll = 0x80000000u;
static_assert((unsigned long long)kOorAll + 3ull * 64 * 4 + 16 <= 0xffffffffull, "block offsets added to kOorAll stay below 2^32 (C <= 64)");
template <int NL>
__global__ __launch_bounds__(256) void smp_bwd_gather_single(GF_GATHER_PARAMS, const int2 *__restrict__ items, int n_items, unsigned bytesT,
                                                             unsigned bytesV, unsigned bytesS) {
    constexpr int PER = 64 / NL;   // sources per wave
    unsigned blk;
    {
        const unsigned nb = gridDim.x, q = nb / 8, r = nb % 8, x = blockIdx.x % 8;
        blk = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + blockIdx.x / 8;
    }
    const int lane = (int)(threadIdx.x & 63);
    const int i0 = (int)(blk * 4 + (threadIdx.x >> 6)) * PER;
    if (i0 >= n_items) return;   // (wave-uniform)
    const int i = i0 + lane / NL;
    const bool live = i < n_items;   // (the ragged last wave)
    const int w = live ? items[i].x : 0;
    const int cw = prev_center[w];
    const int f4b = 16 * (lane % NL), C4 = C * 4, ldtb = T_COLS * C4;
    const long long c0r = cons_ptr[w], c1r = cons_ptr[w + 1];
    const int cnt = live ? (int)(c1r - c0r) : 0;
    // (a group without consumers reads entry 0 of the tables, which exists whenever any lane of the wave enters the loop)
    const long long c0 = cnt > 0 ? c0r : 0, ioff0 = cnt > 0 ? cons_inv_off[c0r] : 0, qb = cnt > 0 ? cons_qbase[w] : 0;
    f4 acc = splat(0.f), accd = splat(0.f), accc = splat(0.f);
    if (live) {
        const float *dfd = dFdc + (size_t)prev_pair[w] * 2 * C;
        accd = ld4(dfd + (f4b >> 2));
        accc = ld4(dfd + C + (f4b >> 2));
    }
    const __amdgpu_buffer_rsrc_t rT = make_rsrc(dT, bytesT), rV = make_rsrc(dVt, bytesV), rS = make_rsrc(dSt, bytesS);
    int4 h0 = make_int4(0, 0, 0, 0), h1 = h0, rec = h0;
    int b = -1;
    if (__builtin_amdgcn_ballot_w64(cnt > 0) != 0) {
        h0 = G.hdr[2 * c0], h1 = G.hdr[2 * c0 + 1], rec = G.qrec[qb];
        b = inv[ioff0];
    }
    for (int k = 0; __builtin_amdgcn_ballot_w64(k < cnt) != 0; ++k) {
        const bool on = k < cnt;
        const int kn = (k + 1 < cnt) ? k + 1 : (cnt > 0 ? cnt - 1 : 0);
        const int4 n0 = G.hdr[2 * (c0 + kn)], n1 = G.hdr[2 * (c0 + kn) + 1], recn = G.qrec[qb + kn];
        const int bn = inv[ioff0 + kn];
        const int s = h0.x, a = h0.y;
        const long long urow = ((long long)h0.w << 32) | (unsigned)h0.z, upb = ((long long)h1.y << 32) | (unsigned)h1.x;
        const unsigned baseT = (unsigned)(urow * ldtb), baseV = (unsigned)(upb * 4 * C4), baseS = (unsigned)h1.z * 4u * (unsigned)C4;
        const bool has = on && b >= 0;
        const unsigned tab = has ? baseT + (unsigned)((a * s + b) * ldtb + f4b) : kOorAll;   // row (a, b) of the consumer's tables
        const unsigned va = has ? baseV + (unsigned)(a * 4 * C4 + f4b) : kOorAll, vb = has ? baseV + (unsigned)(b * 4 * C4 + f4b) : kOorAll;
        const unsigned vs = has ? baseS + (unsigned)f4b : kOorAll, vd = (has && cw == 0) ? baseS + (unsigned)f4b : kOorAll;
        const unsigned tb = has ? baseT + (unsigned)(b * s * ldtb + f4b) + (unsigned)rec.x : kOorAll;   // row (b, c)
        const f4 l0 = gbuf_ld4_once(rT, (int)(tab + T_SAB * C4)), g5 = gbuf_ld4_once(rT, (int)(tab + T_T6 * C4));
        const f4 l1 = buf_ld4(rV, (int)va, 0), l4 = buf_ld4(rV, (int)(va + 2 * C4), 0);
        const f4 l2 = buf_ld4(rV, (int)(vb + C4), 0), z2 = buf_ld4(rV, (int)(vb + 3 * C4), 0);
        const f4 l3 = buf_ld4(rS, (int)vs, 0), l5 = buf_ld4(rS, (int)(vs + 2 * C4), 0);
        const f4 l6 = buf_ld4(rS, (int)(vd + C4), 0), l7 = buf_ld4(rS, (int)(vd + 3 * C4), 0);
        const f4 y = buf_ld4(rT, (int)(tb + T_SBC * C4), 0), g9 = buf_ld4(rT, (int)(tb + T_T10 * C4), 0);
        const f4 x = ((l0 + l1) + (l2 + l3)) + l6;
        const float rho = __int_as_float(rec.y), m = __int_as_float(rec.z), mra = __int_as_float(rec.w);
        if (on) {
            acc += m * (x + y) + g5 * rho + g9 * mra;
            accd += (l4 + l5) + l7;
            accc += z2;
        }
        h0 = n0;
        h1 = n1;
        rec = recn;
        b = bn;
    }
    if (live) {
        f4 o = acc;
        o += accd;   // (q == p: the one position)
        if (cw == 0) o += accc;
        gf_st_s<64>(reinterpret_cast<f4 *>(dfprev + prev_row[w] * C + (f4b >> 2)), o);
    }
}

}  // namespace

gf_status smp_build_gather_records(gf_smp *s, int l, hipStream_t stream) {
    gf_smp::DevLevel &d = s->lv[l];
    const gf_smp::DevLevel &pv = s->lv[l - 1];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    if (!d.cons_hdr || h.pairs == 0) return GF_OK;
    const int C = s->cfg.nChanels;
    hipLaunchKernelGGL(build_gather_records, dim3((unsigned)s->lay.level[l - 1].nNodes), dim3(64), 0, stream, pv.node_s, d.cons_ptr,
                       d.cons_qbase, d.cons_s, d.cons_a, d.cons_row, d.cons_pair, d.pair_node, d.cons_inv_off, d.inv, d.rsum,
                       T_COLS * C * 4, d.cons_hdr, d.cons_qrec);
    GF_LAUNCH_CHECK(s->ctx, "build_gather_records");
    return GF_OK;
}

// the folded gather keeps a source node's row of accumulators in registers: receptive fields of level l-1 up to 32
bool smp_fused_gather_enabled(const gf_smp *s, int l) {
    const gfsmp::LevelLayout &hp = s->lay.level[l - 1];
    return s->bwd_gather && !hp.buckets.empty() && hp.buckets.back().s <= kGatherMaxS;
}

// df_{l-1} from the table gradients of level l without materialising dP (see smp_bwd_gather)
gf_status smp_fused_gather_backward(gf_smp *s, int l) {
    const gfsmp::LevelLayout &h = s->lay.level[l], &hp = s->lay.level[l - 1];
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels;
    const float *dT = d.Q + (size_t)h.rows * T_COLS * C + (size_t)h.rows * O_COLS * C;
    if (!d.cons_hdr) return fail(s->ctx, GF_ERR_INVALID, "smp_fused_gather_backward: level %d has no gather records", l);
    if (!hp.buckets.empty() && hp.buckets.back().s > kGatherMaxS) return fail(s->ctx, GF_ERR_UNSUPPORTED, "smp_fused_gather_backward: receptive field > 64");
    const gf_smp::DevLevel &pv = s->lv[l - 1];
    gf_ctx *ctx = s->ctx;
    const GatherTables G = {d.cons_hdr, d.cons_qrec};
    const int n_items = (int)(hp.gather_items.size() / 2);
    // single-vertex sources only (level 1): 64 / (C / 4) sources per wave, while one buffer resource per table reaches the whole level
    const size_t bT = (size_t)h.rows * T_COLS * C * 4, bV = (size_t)h.pairs * 4 * C * 4, bS = (size_t)h.nNodes * 4 * C * 4;
    const bool single = n_items > 0 && !hp.buckets.empty() && hp.buckets.back().s == 1 && (C == 64 || C == 32 || C == 16) &&
                        bT < kOorAll && bV < kOorAll && bS < kOorAll && smp_level1_switch();
    if (single) {
#define GF_GATHER_SINGLE(NL_)                                                                                                              \
    GF_LAUNCH(ctx, "smpf_bwd_gather", smp_bwd_gather_single<NL_>, dim3((unsigned)((n_items + 4 * (64 / NL_) - 1) / (4 * (64 / NL_)))),       \
              dim3(256), 0, dT, d.dVt, d.dSt, pv.df, d.dFdc, pv.node_s, pv.node_row, pv.node_pair, pv.node_center, d.cons_ptr,              \
              d.cons_inv_off, d.cons_qbase, d.inv, G, C, reinterpret_cast<const int2 *>(pv.gather_items), n_items, (unsigned)bT,            \
              (unsigned)bV, (unsigned)bS)
        if (C == 64) GF_GATHER_SINGLE(16);
        else if (C == 32) GF_GATHER_SINGLE(8);
        else GF_GATHER_SINGLE(4);
#undef GF_GATHER_SINGLE
        ++s->single_launches;
    } else if (n_items > 0)
        GF_LAUNCH(ctx, "smpf_bwd_gather", smp_bwd_gather_all, dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, dT, d.dVt, d.dSt, pv.df,
                  d.dFdc, pv.node_s, pv.node_row, pv.node_pair, pv.node_center, d.cons_ptr, d.cons_inv_off, d.cons_qbase, d.inv, G, C,
                  reinterpret_cast<const int2 *>(pv.gather_items), n_items);
    return GF_OK;
}

}  // namespace gf
