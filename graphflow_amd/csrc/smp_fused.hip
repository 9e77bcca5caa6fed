// smp_fused.hip -- fused SMP level: promotion + RisiContraction_18 + K-projection + bias + LeakyReLU without ever
// materialising the promoted stack P (sum s^3 C floats) or the 18-slice contraction output Q (18 sum s^2 C floats).
//
// Same mathematics as the op-by-op pipeline of smp.hip (GraphFlow/SMP_omega.h:630-670), regrouped:
//   Q_k = (N x N table) x (factor depending on A)  for every one of the 18 cases, and the
//   K-projection is linear, so   sum_k Q_k K^(k)   is evaluated as
//     tables  T = [S_ab | S_bc | T6 | T10]                   four N x N x C tables per node, built by ONE pass that gathers
//                                                             the promoted tensors straight from f_{l-1}
//     compact G15 = Fd K15, G16 = Fc K16 on the sum-s rows of the level below: the diagonal tables D_bb[x,y] = P[x,y,y] and
//             D_ac[x,y] = P[x,y,x] are gathers of f_{l-1}[w_x][p,p] and f_{l-1}[w_x][p,centre]  (see diag_gather_fwd)
//     GEMMs   O_loc = tot [S_ab|S_bc][K0;K2] + tr S_ab K6 + [T6|T10][K5;K9]     (tot, tr as per-row factors of the operand)
//             Z = [S_ab|S_bc][K8;K12]   Z' = S_ab K11                              8 C x C block products on the rows, not 18
//             V = [rowsum_a|colsum_b|D8|D11][K1;K3;K7;K10]  (per (node,x))   S = [total|s14|s15|s18][K4;K13;K14;K17] (per node)
//     combine f_l[x,y] = LeakyReLU(b + O_loc[x,y] + sum_e A[y,e] (Z[x,e] + Z'[e,x] + G15[x,e] + G16[e,x]) + r[y] V[x] + A[x,y] S)
// The reverse sweep mirrors it: combine-backward -> compact gradients -> block GEMMs (dT, dK) -> smp_bwd_gather, the
// consumer gather of df_{l-1} that evaluates dP from the table gradients on the fly (dP is not materialised either; the
// two-kernel form tables-backward -> promote_backward remains for GF_SMP_BWD_GATHER=0 and receptive fields > 32).
// HBM traffic per level drops from about (2 S + 40 R) C floats to about 19 R C, GEMM flops from 18 to 8 units
// (R = sum s^2, S = sum s^3).
#include "smp_fused_internal.h"

using namespace gf::dev;

namespace gf {
namespace {

// stacked weight layout: position p holds block K^(kperm[p]); groups are contiguous
//   [0,2) tot | [2,3) tr | [3,5) dir | [5,8) Z | [8,10) Z' | [10,14) V | [14,18) S
__constant__ int c_kperm[18] = {0, 2, 6, 5, 9, 8, 12, 11, 15, 16, 1, 3, 7, 10, 4, 13, 14, 17};

// ---------------------------------------------------------------------------------------------------------------
// Compact-diagonal variant.  D_bb[x,y] = P[x,y,y] = f_{l-1}[w_x][p,p] and D_ac[x,y] = P[x,y,x] = f_{l-1}[w_x][p,c] with
// p = pi_x(y) and c = the position of w_x's own vertex in its receptive field: both tables are gathers of sum-s vectors per
// source node.  So D_bb K15 and D_ac K16 are computed ONCE on those vectors ([pairs of level l-1] rows instead of
// [rows of level l]: 24x fewer at level 3 of cfg3), combine-forward gathers the products, and the reverse sweep collects
// their gradients with a consumer gather.  T and dT lose two of their six blocks and the row GEMMs two of ten products.
//   Fdc[pr] = [ f[w][p,p] | f[w][p,c_w] ]   (pr = node_pair(l-1)[w] + p)        Gc = [ Fd K15 | Fc K16 ]
// ---------------------------------------------------------------------------------------------------------------
__global__ void diag_gather_fwd(const float *__restrict__ fprev, float *__restrict__ Fdc, const int *__restrict__ node_s,
                                const long long *__restrict__ node_row, const long long *__restrict__ node_pair,
                                const int *__restrict__ node_center, int C) {
    const int w = blockIdx.x;
    const int s = node_s[w], c = node_center[w], nl = C / 4;
    const float *src = fprev + (size_t)node_row[w] * C;
    float *dst = Fdc + (size_t)node_pair[w] * 2 * C;
    for (int i = threadIdx.x; i < s * nl; i += blockDim.x) {
        const int fl = i % nl, p = i / nl;
        st4(dst + (size_t)p * 2 * C + 4 * fl, ld4(src + ((size_t)p * s + p) * C + 4 * fl));
        st4(dst + (size_t)p * 2 * C + C + 4 * fl, ld4(src + ((size_t)p * s + c) * C + 4 * fl));
    }
}

// dGc[pr] = [ sum_cons dU_n[a, inv(p)] | sum_cons dU_n[inv(p), a] ]  over the consumers (n, a) of source node w, in consumer
// order (deterministic).  dU_n[x, e] is the Z block of dO at row (x, e) (written by combine-backward).
// (individual __restrict__ kernel parameters, also for the launch that shares this body with smp_reduce_pairs: handed over in a struct the
//  pointers lose their no-alias guarantee -- measured in round 6: 0.20 -> 0.26 ms per cfg3 step for this kernel)
#define GF_DIAGB_PARAMS                                                                                                               \
    const float *__restrict__ dO, float *__restrict__ dGc, const int *__restrict__ prev_s, const long long *__restrict__ prev_pair,       \
        const long long *__restrict__ cons_ptr, const long long *__restrict__ cons_row, const int *__restrict__ cons_s,                  \
        const int *__restrict__ cons_a, const long long *__restrict__ cons_inv_off, const short *__restrict__ inv, int C, int ocols,     \
        const float *__restrict__ nodefac, /* or null: slice-dropout factors [nodes][18] of the CONSUMERS' level */                       \
        const long long *__restrict__ cons_pair, const int *__restrict__ pair_node /* (with nodefac: consumer -> node) */
#define GF_DIAGB_ARGS dO, dGc, prev_s, prev_pair, cons_ptr, cons_row, cons_s, cons_a, cons_inv_off, inv, C, ocols, nodefac, cons_pair, pair_node
__device__ __forceinline__ void diag_gather_bwd_body(GF_DIAGB_PARAMS, int w) {
    const int sw = prev_s[w], nl = C / 4;
    const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1];
    const size_t ldo = (size_t)ocols * C;
    float *dst = dGc + (size_t)prev_pair[w] * 2 * C;
    for (int i = threadIdx.x; i < sw * nl; i += blockDim.x) {
        const int fl = i % nl, p = i / nl;
        f4 a15 = splat(0.f), a16 = splat(0.f);
        for (long long e0 = c0; e0 < c1; e0 += 4) {  // four consumers' loads in flight (clamped address + select), same order
            f4 u[4], v[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = (e0 + j < c1) ? e0 + j : e0;
                const int ip = inv[cons_inv_off[e] + p];
                ok[j] = e0 + j < c1 && ip >= 0;
                const int s = cons_s[e], a = cons_a[e], ix = ok[j] ? ip : 0;
                const float *base = dO + (size_t)cons_row[e] * ldo + O_Z * C + 4 * fl;
                u[j] = ld4(base + ((size_t)a * s + ix) * ldo);
                v[j] = ld4(base + ((size_t)ix * s + a) * ldo);
                if (nodefac) {   // (uniform) the consumer node's factors of slices 15 and 16
                    const float *nf = nodefac + (size_t)pair_node[cons_pair[e]] * 18;
                    u[j] = u[j] * nf[15];
                    v[j] = v[j] * nf[16];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ok[j]) {
                    a15 += u[j];
                    a16 += v[j];
                }
        }
        st4(dst + (size_t)p * 2 * C + 4 * fl, a15);
        st4(dst + (size_t)p * 2 * C + C + 4 * fl, a16);
    }
}
__global__ void diag_gather_bwd(GF_DIAGB_PARAMS) { diag_gather_bwd_body(GF_DIAGB_ARGS, (int)blockIdx.x); }

// ---- slice dropout on the fused level (round 5; RisiContraction_18_dropout, GraphFlow/RisiContraction_18_dropout.h:106-132, 465-471) ----
// The reference zeroes (train) or scales by nKept / 18 (test) single slices k of a node's contraction output.  The factorised level never
// forms a slice, but every slice is one block product K^(k) applied to one table, so a node's slice factor m_k is a per-node factor on that
// product: the eight row products take it through an eight-column row-factor table (smp_rowpanel_split / smp_wgrad_all, NF = 8), the
// vector / scalar products through their operands (Vt, St and their gradients are scaled block by block), the two compact diagonal
// products where the consumer gathers them (combine-forward, diag_gather_bwd).
//   nodefac[n][k] = bit k of keep[n] ? scale : 0        rowfac8[row] = (tot m0, tot m2, tr m6, m5, m9, m8, m12, m11) of the row's node
__global__ __launch_bounds__(64) void build_dropout_factors(const unsigned *__restrict__ keep, float scale, const float2 *__restrict__ node_scale,
                                                            const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                            float *__restrict__ nodefac, float *__restrict__ rowfac8) {
    const int n = blockIdx.x, s = node_s[n];
    const unsigned bits = keep[n];
    auto m = [&](int k) { return ((bits >> k) & 1u) ? scale : 0.f; };
    if (threadIdx.x < 18) nodefac[(size_t)n * 18 + threadIdx.x] = m((int)threadIdx.x);
    const float2 tt = node_scale[n];
    const f4 lo = {tt.x * m(0), tt.x * m(2), tt.y * m(6), m(5)}, hi = {m(9), m(8), m(12), m(11)};
    float *dst = rowfac8 + (size_t)node_row[n] * 8;
    for (int i = threadIdx.x; i < s * s; i += blockDim.x) {
        st4(dst + (size_t)i * 8, lo);
        st4(dst + (size_t)i * 8 + 4, hi);
    }
}
// X [rows][4 C] *= the node's factors of slices (k0, k1, k2, k3), block by block; row_node == nullptr: row r belongs to node r
__global__ void scale_node_blocks(float *__restrict__ X, const int *__restrict__ row_node, const float *__restrict__ nodefac, int k0, int k1,
                                  int k2, int k3, int C, long long rows) {
    const int nq = C / 4;   // float4 per block
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * 4 * nq) return;
    const long long row = i / (4 * nq);
    const int blk = (int)(i % (4 * nq)) / nq;
    const int node = row_node ? row_node[row] : (int)row;
    const int k = blk == 0 ? k0 : blk == 1 ? k1 : blk == 2 ? k2 : k3;
    const float f = nodefac[(size_t)node * 18 + k];
    f4 v = ld4(X + i * 4);
    st4(X + i * 4, v * f);
}

// stacked[p] = K^(kperm[p])  (gather; the gradients take the inverse permutation in smp_fold_level).  Block k of the level weight is
// K[(k C + ci) C + co] in the SMP_omega layout [18C][C] and K[co 18C + k C + ci] in the CustomMatMulTensor layout [C][18C]
// (custom != 0, SMP_2D_ver8): the stacked copy is [ci][co] either way, so the block GEMMs do not care.
__device__ __forceinline__ size_t weight_index(int k, int r, int C, int custom) {
    const int ci = r / C, co = r % C;
    return custom ? (size_t)co * 18 * C + (size_t)k * C + ci : ((size_t)k * C + ci) * C + co;
}
// every level's stacked copy in one launch (the parameters are fixed for the whole forward pass)
constexpr int kStackLevels = 8;
struct StackAll {
    const float *K[kStackLevels];
    float *stacked[kStackLevels];
    int n;
};
__global__ void stack_weights_all(StackAll a, int C, int custom) {
    const int CC = C * C;
    const float *K = a.K[blockIdx.y];
    float *st = a.stacked[blockIdx.y];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 18 * CC; i += gridDim.x * blockDim.x)
        st[i] = K[weight_index(c_kperm[i / CC], i % CC, C, custom)];
}

// One pass over the per-(node,x) partials of combine-backward for a block of nodes [n0, n1):
//   dSout[n] = sum_x dSpart[(n,x)]
//   colpart[block] = sum over the block's pairs of dbpart    (folded in order by smp_fold_level)
// 256 threads = row groups x C/4 float4 lanes (C % 4 == 0, C <= 1024); the groups are folded through LDS in a fixed order.
#define GF_REDP_PARAMS                                                                                                              \
    const float *__restrict__ dSpart, const float *__restrict__ dbpart, float *__restrict__ dSout, float *__restrict__ colpart,          \
        const int *__restrict__ node_s, const long long *__restrict__ node_pair, int Cr, int nodes, int nodes_per_block
#define GF_REDP_ARGS dSpart, dbpart, dSout, colpart, node_s, node_pair, Cr, nodes, nodes_per_block
__device__ __forceinline__ void reduce_pairs_body(GF_REDP_PARAMS, int bid, float *red) {
    const int C = Cr;
    const int n0 = bid * nodes_per_block, n1 = (n0 + nodes_per_block < nodes) ? n0 + nodes_per_block : nodes;
    const int nl = C / 4, ng = 256 / nl;
    const int g = threadIdx.x / nl, fl = threadIdx.x % nl;
    const auto one = [](int) { return 1.f; };
    if (g < ng) {
        for (int n = n0 + g; n < n1; n += ng)
            st4(dSout + (size_t)n * C + 4 * fl, batched_sum(dSpart + (size_t)node_pair[n] * C + 4 * fl, (size_t)C, 0, node_s[n], one));
        const long long p0 = node_pair[n0], p1 = (n1 < nodes) ? node_pair[n1] : node_pair[n1 - 1] + node_s[n1 - 1];
        const int cnt = (int)((p1 - p0 - g + ng - 1) / ng);
        st4(red + g * C + 4 * fl, batched_sum(dbpart + ((size_t)p0 + g) * C + 4 * fl, (size_t)ng * C, 0, cnt > 0 ? cnt : 0, one));
    }
    __syncthreads();
    if (g == 0) {
        f4 t = ld4(red + 4 * fl);
        for (int k = 1; k < ng; ++k) t += ld4(red + k * C + 4 * fl);
        st4(colpart + (size_t)bid * C + 4 * fl, t);
    }
}
__global__ __launch_bounds__(256) void smp_reduce_pairs(GF_REDP_PARAMS) {
    __shared__ __attribute__((aligned(16))) float red[1024];
    reduce_pairs_body(GF_REDP_ARGS, (int)blockIdx.x, red);
}
// Both in ONE launch (round 6): they are independent (each reads what combine-backward left), small and latency-bound -- the column
// partials' workgroups first, then a workgroup per source node of the level below.  GF_SMP_FUSE_SMALL=0: two launches.
__global__ __launch_bounds__(256) void smp_reduce_pairs_and_diag_gather(GF_REDP_PARAMS, int nb, GF_DIAGB_PARAMS) {
    __shared__ __attribute__((aligned(16))) float red[1024];
    if ((int)blockIdx.x < nb) reduce_pairs_body(GF_REDP_ARGS, (int)blockIdx.x, red);
    else diag_gather_bwd_body(GF_DIAGB_ARGS, (int)blockIdx.x - nb);
}

// End of a level's reverse sweep: every partial image of its weight and bias gradients folded in ONE launch, in a fixed
// order, straight into the caller's gradient buffers:
//   stacked positions [0,8)  <- the row-range images of smp_wgrad_c64          (n = 8 C^2)
//   [8,9), [9,10)            <- dK15, dK16 on the compact rows                  (n = C^2 each)
//   [10,14), [14,18)         <- the per-(node,x) and per-node products          (n = 4 C^2 each)
//   bias                     <- the column partials of smp_reduce_pairs         (n = C)
// dK_l[weight_index(kperm[p], .)] += sum (the inverse of stack_weights_all's permutation), db_l += sum.
// 256 threads = 64 outputs x 4 split quarters: a quarter sums its run of images in order (8 loads in flight), the four
// quarters are then added in order through LDS -- the summation tree depends on the image count only.
constexpr int kFoldGroups = 6;
struct FoldArgs {
    const float *part[kFoldGroups];
    int splits[kFoldGroups];
    unsigned n[kFoldGroups], first[kFoldGroups];  // outputs [first, first + n) of the stacked index space (bias at 18 C^2)
    int ngroups;
};
__global__ __launch_bounds__(256) void smp_fold_level(FoldArgs a, float *__restrict__ dK, float *__restrict__ db, int C, int custom,
                                                      unsigned total) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, qtr = threadIdx.x >> 6;
    const unsigned i = blockIdx.x * 64u + e;
    float acc = 0.f;
    if (i < total) {
        int g = 0;
#pragma unroll
        for (int k = 1; k < kFoldGroups; ++k)
            if (k < a.ngroups && i >= a.first[k]) g = k;
        const unsigned j = i - a.first[g];
        if (j < a.n[g]) {
            const int S = a.splits[g], per = (S + 3) / 4;
            const int s0 = qtr * per, s1 = (s0 + per < S) ? s0 + per : S;
            const float *p = a.part[g] + j;
            const size_t stride = a.n[g];
            for (int sb = s0; sb < s1; sb += 8) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (sb + k < s1) ? p[(size_t)(sb + k) * stride] : 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += v[k];
            }
        }
    }
    red[qtr][e] = acc;
    __syncthreads();
    if (qtr == 0 && i < total) {
        const float v = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        const unsigned CC = (unsigned)C * C;
        if (i < 18 * CC)
            dK[weight_index(c_kperm[i / CC], (int)(i % CC), C, custom)] += v;
        else
            db[i - 18 * CC] += v;
    }
}

}  // namespace

// the dedicated C = 64 kernels of the block products (weights resident in LDS, rows in registers; output-stationary weight gradients).
// GF_SMP_ROWPANEL=0 (read per call: the parity tests switch it) selects the grouped tiled GEMM launches every other channel count uses.
// Round 4: the split-operand row-panel products also run at C = 32 (32 x 32 blocks: one column half, two k-chunks per lane; weight
// gradients on smp_wgrad_all<32>); the fp32-pipe variants, the panel combine and the small-product kernels stay C = 64 only.
// C = 128: the same family as four 64-channel sub-block passes per product (smp_level_c64_split.hip: W = 2), on the split pipe only and
// for the plain 18-slice model (no towers, slice dropout or embedded ver6 / ver7 model), unless GF_SMP_C128=0 (smp_c128_switch): then the grouped GEMMs.
static bool smp_c128_kernels(const gf_smp *s) {
    if (s->cfg.nChanels != 128 || s->cfg.nContractions != 18 || s->cfg.physics || s->drop_on || s->n_extra || s->dup_channels) return false;
    if (!smp_split_products(s->ctx) || !smp_c128_switch() || !s->wbound || (int)s->lv.size() <= s->cfg.nLevels) return false;
    for (int l = 1; l <= s->cfg.nLevels; ++l)
        if (!s->lv[l].trow || !s->lv[l].wimg) return false;   // (the transposed-row tables and the four image sets: smp_prepare.hip)
    return true;
}
static bool smp_c64_kernels(const gf_smp *s) {
    if (env_is("GF_SMP_ROWPANEL", '0')) return false;
    if (s->cfg.nChanels == 128) return smp_c128_kernels(s);
    return s->cfg.nChanels == 64 || ((s->cfg.nChanels == 32 || s->cfg.nChanels == 16) && smp_split_products(s->ctx) && s->wbound != nullptr);
}

// Every path decision of one call of the level, and every environment switch the level reads (the remaining ones: smp_fused_supported).
// Evaluated once at the entry of smp_fused_forward_level and once at the entry of smp_fused_backward_level: the tests flip the switches
// between calls of one process, so nothing here is cached in the handle.
FusedRoute fused_route(const gf_smp *s, int l) {
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels;
    const long long rows = s->lay.level[l].rows;
    FusedRoute r;
    r.panels = smp_c64_kernels(s);
    // compact projected matrix O = [O_loc | U] (2C) instead of [O_loc | Z | Z'] (3C): the row-panel product kernels gather the
    // transposed rows themselves; the tiled launches keep the three-block layout
    r.ocols = r.panels ? 2 : O_COLS;
    r.split = smp_split_products(s->ctx);
    r.fold_vectors = smp_tables_fold_vectors(s);
    r.lpc = !r.fold_vectors ? 16 : smp_quarter_window(C) ? 4 : smp_half_window(C) ? 8 : 16;
    // The structurally-zero rows of the S_ab / T6 blocks (half of the rows at QM9 sizes, 0.73 GB of zeros a step at cfg3) are the
    // same rows every step of a prepared batch and nothing else writes there: their zeros go in once, tables-forward skips them.
    // Round 4: and they are not even written that once while every reader of T skips them -- the split product kernels and the packed
    // weight-gradient kernel read an absent block from a page of zeros, the sums over b never visit one -- which is the default path; a
    // reader that does not mask (fp32 pipe, tiled GEMMs) gets the fill before it runs (fwd_zero_rows, or where the reverse sweep finds one).
    r.skip_zero_rows = (C == 64 || ((C == 32 || C == 16) && r.fold_vectors)) && d.rowflag && !env_is("GF_SMP_MASK_ZEROS", '0');
    r.readers_mask = r.panels && r.split && d.trowf && d.trow && rows < (1ll << 29);
    r.small_split = smp_panel_channels(C) && d.wimg_ready;   // wave per 32-row panel on the f16 pipe (smp_small_split)
    r.drop = s->drop_on;   // (smp_fused_supported: only where the factor tables exist)
    r.nf = r.drop ? 8 : 2;
    // (32 / 16 channels, prebuilt images, no slice dropout)
    r.extras_in_kernel = s->n_extra && (C == 32 || C == 16) && r.panels && d.wimg_ready && d.wimg && !r.drop && r.split && d.trow;
    // wave per row panel, the adjacency product on the matrix pipe; a level beyond the panel kernels' 32-bit offsets, or another channel
    // count: the workgroup kernels for every node
    r.panel_combine = smp_panel_channels(C) && r.panels && d.fwd_pan && rows * 512 < 0x3fffffffll;
    r.gather = smp_fused_gather_enabled(s, l);
    r.fuse_small = !env_is("GF_SMP_FUSE_SMALL", '0');
    r.sign_mask = smp_sign_mask(s, l);
    // The EMPTY rows of the level -- none of bits 31 / 30 / 29 of trowf: no data in any block of T, 17 % of cfg3's rows -- have exact zeros
    // in O and a dO nobody reads.  Neither is stored or read where EVERY writer and reader of the region in this call masks them: the
    // split forward products, the two panel combine kernels, smp_wgrad_split on the level's maxima (exact bounds scan all of dO) and the
    // masked backward products (classed: the driver's lists leave the rows out; unclassed: dO is read where a source covers the row).
    // Excluded: the workgroup combine kernels (nodes above 32 positions), slice dropout, the extra products and transposed channels of
    // the embedded `_10` / `_50` models, every other channel count.  GF_SMP_EMPTY_ROWS=0 (read per call): everything moves as before.
    r.skip_empty = C == 64 && r.panels && r.split && r.readers_mask && r.panel_combine && r.gather && r.skip_zero_rows && !r.drop && !s->n_extra &&
                   !s->dup_channels && !s->lay.level[l].buckets.empty() && s->lay.level[l].buckets.back().s <= 32 && d.pan_live && d.rowcls && s->wbound && d.dzmax &&
                   !env_is("GF_SMP_EMPTY_ROWS", '0');
    return r;
}

static BigPart big_part(const gfsmp::LevelLayout &h) {
    BigPart b;
    b.n0 = h.nNodes, b.row0 = h.rows, b.pair0 = h.pairs, b.quad0 = (int)h.quad_node.size();
    long long q = 0;
    for (const gfsmp::Bucket &bk : h.buckets) {
        if (bk.s > 32) {
            b.n0 = bk.first_node;
            break;
        }
        q += (long long)bk.count * ((bk.s + 3) / 4);   // (quads are in node order, ceil(s / 4) per node: smp_prep.cpp)
    }
    if (b.n0 < h.nNodes) {
        b.nodes = h.nNodes - b.n0;
        b.row0 = h.node_row[(size_t)b.n0], b.pair0 = h.node_pair[(size_t)b.n0];
        b.pairs = h.pairs - b.pair0;
        b.quad0 = (int)q, b.quads = (int)h.quad_node.size() - (int)q;
        b.smax = h.buckets.back().s;
    }
    return b;
}

// every level's block-permuted weight copy in one launch (gf_smp_forward, before the first level)
gf_status smp_fused_stack_all(gf_smp *s, const std::vector<const float *> &K) {
    const int L = s->cfg.nLevels, C = s->cfg.nChanels;
    for (int l0 = 1; l0 <= L; l0 += kStackLevels) {
        StackAll a;
        a.n = 0;
        for (int l = l0; l <= L && a.n < kStackLevels; ++l) {
            if (smp_level_kind(s, l) != LevelKind::Fused18) continue;
            a.K[a.n] = K[l];
            a.stacked[a.n] = s->lv[l].Wst;
            ++a.n;
        }
        if (a.n > 0)
            GF_LAUNCH(s->ctx, "smpf_stack_w", stack_weights_all, dim3(64, a.n), dim3(256), 0, a, C, s->cfg.custom_matmul);
    }
    // ... and the split product kernels' weight images of every level, both directions (the backward pass reuses them)
    for (int l = 1; l <= L; ++l) s->lv[l].wimg_ready = false;
    if ((smp_panel_channels(C) || C == 128) && smp_c64_kernels(s) && smp_split_products(s->ctx)) {
        std::vector<const float *> w, x;
        std::vector<void *> im;
        for (int l = 1; l <= L; ++l)
            if (smp_level_kind(s, l) == LevelKind::Fused18 && s->lv[l].wimg) {
                w.push_back(s->lv[l].Wst);
                x.push_back((s->n_extra && s->extra_w) ? s->extra_w + (size_t)(l - 1) * 3 * C * C : nullptr);   // (images 18 .. 20: SMP_2D_ver7's extra products)
                im.push_back(s->lv[l].wimg);
                s->lv[l].wimg_ready = true;
            }
        if (!w.empty()) {
            gf_status st = smp_split_build_images(s->ctx, w.data(), im.data(), (int)w.size(), C, x.data());
            if (st != GF_OK) return st;
        }
    }
    return GF_OK;
}

bool smp_fused_supported(const gf_smp *s, int l) {
    const int C = s->cfg.nChanels;
    if (C % 4 != 0 || C > 1024) return false;
    if (s->cfg.nContractions != 18) return false;  // SMP_2D_ver6 / ver7 (_10 / _50): op-by-op levels
    if (!s->cfg.square()) return false;            // a tower at its own halving channel counts (GF_SMP_PAD_CHANNELS=0): op-by-op levels
    const gfsmp::LevelLayout &h = s->lay.level[l];
    if (h.buckets.empty()) return false;
    if (s->drop_on) {   // RisiContraction_18_dropout: fused where the per-product row factors exist (round 5: the split row-panel kernels at
        // 32 / 16 channels -- the towers' padded widths -- with the panel combine-forward and the level's device-built statistics), else op by op
        const gf_smp::DevLevel &d = s->lv[l];
        if (!((C == 32 || C == 16) && smp_c64_kernels(s) && d.rowfac8 && d.nodefac && d.fwd_pan && d.dzmax && d.row_max && d.trow && s->bwd_gather) ||
            env_is("GF_SMP_FUSED_DROPOUT", '0'))
            return false;
    }
    if (h.buckets.back().s <= 32) return true;  // 8 * PPW at LPC = 16
    // Round 6: fields of 33 .. 64 positions at 64 / 32 / 16 (padded) channels -- the nodes above 32 run tables-forward on smp_tables_fwd_big and the two combine steps
    // on the workgroup kernels (big_part); the gather wants the SOURCES (level l - 1) within 32, the split row-panel products their packed tables
    const gf_smp::DevLevel &d = s->lv[l];
    return h.buckets.back().s <= kFusedMaxField && smp_panel_channels(C) && smp_tables_fold_vectors(s) && smp_c64_kernels(s) &&
           smp_split_products(s->ctx) && smp_fused_gather_enabled(s, l) && d.trow && d.trowf && d.rowflag && d.dzmax && d.row_max && d.fwd_pan &&
           !env_is("GF_SMP_BIG_FIELDS", '0');
}

// ---- what the steps of both drivers share ----
// Q buffer of the level ([rows][18C]) is carved as  T [rows][4C] | O / dO [rows][3C] | dT [rows][4C]
static float *level_T(const gf_smp *s, int l) { return s->lv[l].Q; }
static float *level_O(const gf_smp *s, int l) { return s->lv[l].Q + (size_t)s->lay.level[l].rows * T_COLS * s->cfg.nChanels; }
static float *level_dT(const gf_smp *s, int l) { return level_O(s, l) + (size_t)s->lay.level[l].rows * O_COLS * s->cfg.nChanels; }

// one plain product of a grouped launch: no K pieces, no row factors
static GemmSpec gemm_spec(const float *A, const float *B, float *Cm, int M, int N, int K, int lda, int ldb, int ldc) {
    const GemmSpec z = {A, B, Cm, M, N, K, lda, ldb, ldc, 0, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, nullptr, 0, {-1, -1, -1, -1}};
    return z;
}

// The five row products of the level where they run one by one on the tiled GEMMs (the grouped launches name the same blocks as K pieces):
//   O[:, ocol] (+)= fac T[:, tcol .. tcol + kb) Wst[wpos .. wpos + kb)      fac = column scol of the level's rowscale table, or none
//   O_LOC = tot [S_ab|S_bc][K0;K2] + tr S_ab K6 + [T6|T10][K5;K9]     Z = [S_ab|S_bc][K8;K12]     Z' = S_ab K11
// The weight gradients are T-block^T dO-block per entry, the table gradients dO-block Wst-block^T (bwd_table_grads).
struct RowProduct {
    int tcol, kb, wpos, ocol, scol, acc;
};
static const RowProduct kRowProducts[5] = {{T_SAB, 2, 0, O_LOC, 0, 0}, {T_SAB, 1, 2, O_LOC, 1, 1}, {T_T6, 2, 3, O_LOC, -1, 1},
                                           {T_SAB, 2, 5, O_Z, -1, 0},  {T_SAB, 1, 7, O_ZP, -1, 0}};

// Slice dropout: the vector / scalar slices' factors ride on the operands -- Vt blocks (1, 3, 7, 10), St blocks (4, 13, 14, 17); the
// reverse sweep scales the gradients of the scaled operands by the same factors once more.
static gf_status dropout_scale(gf_smp *s, int l, float *Vt, float *St) {
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, pairs = (int)s->lay.level[l].pairs, nodes = s->lay.level[l].nNodes;
    const long long nv = (long long)pairs * C, ns = (long long)nodes * C;
    GF_LAUNCH(s->ctx, "smpf_dropout_scale", scale_node_blocks, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, Vt, d.pair_node, d.nodefac, 1, 3, 7, 10, C,
              (long long)pairs);
    GF_LAUNCH(s->ctx, "smpf_dropout_scale", scale_node_blocks, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, St, (const int *)nullptr, d.nodefac, 4, 13, 14,
              17, C, (long long)nodes);
    return GF_OK;
}

gf_status smp_fused_copy_projected(gf_smp *s, int l, float *out) {
    if (!s->lv[l].Q || !s->lv[l].fwd_c64) return fail(s->ctx, GF_ERR_INVALID, "level %d has no compact projected matrix (no fused forward on the row-panel kernels)", l);
    const size_t bytes = (size_t)s->lay.level[l].rows * 2 * s->cfg.nChanels * sizeof(float);
    GF_HIP_TRY(s->ctx, hipMemcpyAsync(out, level_O(s, l), bytes, hipMemcpyDeviceToDevice, s->ctx->stream));
    return GF_OK;
}

// ---- the forward pass of a level, step by step ----
static gf_status fwd_zero_rows(gf_smp *s, int l, const FusedRoute &r) {
    s->lv[l].t_zeros = r.skip_zero_rows;
    return (r.skip_zero_rows && !r.readers_mask) ? smp_fused_ensure_zero_fill(s, l) : GF_OK;
}

static gf_status fwd_dropout_factors(gf_smp *s, int l) {
    const gf_smp::DevLevel &d = s->lv[l];
    GF_LAUNCH(s->ctx, "smpf_dropout_factors", build_dropout_factors, dim3(s->lay.level[l].nNodes), dim3(64), 0, d.keep_mask, s->drop_scale,
              reinterpret_cast<const float2 *>(d.node_scale), d.node_s, d.node_row, d.nodefac, d.rowfac8);
    return GF_OK;
}

static gf_status fwd_tables(gf_smp *s, int l, const FusedRoute &r, const BigPart &big) {
    for (const SizeClass &c : classes_of(s->lay.level[l], 64 / r.lpc)) {
        const gf_status st = launch_tables_fwd(s, l, c, r);
        if (st != GF_OK) return st;
    }
    return big.nodes > 0 ? launch_tables_fwd_big(s, l, big) : GF_OK;
}

// Fdc = [f[w][p,p] | f[w][p,c_w]] of the level below (read by smp_vectors and by the compact products)
static gf_status fwd_diag_gather(gf_smp *s, int l) {
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const gfsmp::LevelLayout &hp = s->lay.level[l - 1];
    const int C = s->cfg.nChanels;
    GF_LAUNCH(s->ctx, "smpf_diag_gather", diag_gather_fwd, dim3(hp.nNodes), dim3(node_block(hp, C)), 0, pv.f, d.Fdc, pv.node_s, pv.node_row, pv.node_pair,
              pv.node_center, C);
    return GF_OK;
}

// V = Vt [K1;K3;K7;K10], S = St [K4;K13;K14;K17], Gc = [Fd K15 | Fc K16]: the small products of the level, ONE launch
static gf_status fwd_small_products(gf_smp *s, int l, const FusedRoute &r) {
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, pairs = (int)s->lay.level[l].pairs, nodes = s->lay.level[l].nNodes, prevPairs = (int)s->lay.level[l - 1].pairs;
    const size_t CC = (size_t)C * C;
    if (r.small_split) {
        const int prog[3] = {0, 2, 0}, nrows[3] = {pairs, prevPairs, nodes}, pos0[3] = {10, 8, 14};
        const float *in[3] = {d.Vt, d.Fdc, d.St};
        float *out[3] = {d.Vout, d.Gc, d.Sout};
        return smp_small_split_c64(s->ctx, false, 3, prog, in, out, nrows, pos0, d.wimg, "smpf_small_nn", C);
    }
    const GemmSpec sm[4] = {gemm_spec(d.Vt, d.Wst + 10 * CC, d.Vout, pairs, C, 4 * C, 4 * C, C, C),
                            gemm_spec(d.St, d.Wst + 14 * CC, d.Sout, nodes, C, 4 * C, 4 * C, C, C),
                            gemm_spec(d.Fdc, d.Wst + 8 * CC, d.Gc, prevPairs, C, C, 2 * C, C, 2 * C),
                            gemm_spec(d.Fdc + C, d.Wst + 9 * CC, d.Gc + C, prevPairs, C, C, 2 * C, C, 2 * C)};
    return gemm_grouped_free(s->ctx, false, sm, 4, "smpf_small_nn");
}

// the row-panel family's call for level l in one direction: forward O from T, backward dT from dO (without dz: bwd_table_grads asks for it)
static RowProductsCall row_products_call(const gf_smp *s, int l, const FusedRoute &r, bool forward) {
    const gf_smp::DevLevel &d = s->lv[l];
    RowProductsCall c = {forward, forward ? level_T(s, l) : level_O(s, l), r.drop ? d.rowfac8 : d.rowscale, d.Wst, forward ? level_O(s, l) : level_dT(s, l),
                         (int)s->lay.level[l].rows, d.trow};
    c.trowf = d.trowf, c.rowcls = d.rowcls;
    c.wimg = d.wimg_ready ? d.wimg : nullptr;
    c.C = s->cfg.nChanels, c.nf = r.nf, c.nx = r.extras_in_kernel ? 3 : 0;
    // (backward, with the consumer gather reading dT: the gradients of the structurally-zero S_ab / T6 rows have no reader: not written)
    c.skip_zero_grads = !forward && r.gather;
    c.skip_empty = forward && r.skip_empty;
    return c;
}

// block products: A = T column range, B = stacked weights, C = O column block.  The row-panel family (weights in LDS), else one grouped
// launch (every row panel of T is fetched from HBM once and shared through L2 by the three products), separate launches as a fallback.
static gf_status fwd_row_products(gf_smp *s, int l, const FusedRoute &r) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, rows = (int)s->lay.level[l].rows;
    const size_t CC = (size_t)C * C;
    float *T = level_T(s, l), *O = level_O(s, l);
    if (r.panels) return smp_row_products(ctx, row_products_call(s, l, r, true));
    const int ldt = T_COLS * C, ldo = O_COLS * C;   // (the tiled launches always use the three-block layout)
    const long long tC = C, wCC = (long long)CC;
    const GemmSpec sp[3] = {
        // O_LOC: three K pieces, the first two row-scaled
        {T, d.Wst, O + O_LOC * C, rows, C, 5 * C, ldt, C, ldo, 3, {T_SAB * tC, T_SAB * tC, T_T6 * tC, 0}, {0 * wCC, 2 * wCC, 3 * wCC, 0},
         {2 * C, C, 2 * C, 0}, d.rowscale, 2, {0, 1, -1, -1}},
        // Z (stack 5, 6), Z' (stack 7); the D_bb K15 / D_ac K16 terms come from Gc
        gemm_spec(T + T_SAB * C, d.Wst + 5 * CC, O + O_Z * C, rows, C, 2 * C, ldt, C, ldo),
        gemm_spec(T + T_SAB * C, d.Wst + 7 * CC, O + O_ZP * C, rows, C, C, ldt, C, ldo),
    };
    if (gemm_grouped_supported(sp, 3, false, false)) return gemm_grouped_rows(ctx, false, false, sp, 3, rows);
    for (const RowProduct &g : kRowProducts) {
        const gf_status st = gemm_rs(ctx, false, false, rows, C, g.kb * C, T + g.tcol * C, ldt, 0, d.Wst + g.wpos * CC, C, 0, O + g.ocol * C, ldo, 0, 1, g.acc,
                                     d.rowscale, 2, g.scol);
        if (st != GF_OK) return st;
    }
    return GF_OK;
}

// SMP_2D_ver7 on the 18-slice level: O_loc += S_ab X_a + S_bc X_b + tr S_bc X_c (gf_smp::n_extra), plain fp32 GEMMs on T
static gf_status fwd_extra_products(gf_smp *s, int l, const FusedRoute &r) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, rows = (int)s->lay.level[l].rows;
    const size_t CC = (size_t)C * C;
    float *T = level_T(s, l), *O = level_O(s, l);
    if (!s->extra_w) return fail(ctx, GF_ERR_INVALID, "fused level %d: the extra products' weights are not bound", l);
    gf_status st = smp_fused_ensure_zero_fill(s, l);   // (these readers do not mask the absent S_ab blocks)
    if (st != GF_OK) return st;
    const float *X = s->extra_w + (size_t)(l - 1) * 3 * CC;
    const int ldt = T_COLS * C, ldO = r.ocols * C;
    static_assert(T_SBC == T_SAB + 1, "[S_ab | S_bc] [X_a; X_b] as one product of depth 2 C");
    // ONE launch: three K pieces (S_ab X_a, S_bc X_b, tr S_bc X_c), accumulated into O_loc; two launches where the segmented form
    // does not apply (16 channels: a piece is shorter than the GEMM's k-step)
    const GemmSpec xs = {T, X, O + O_LOC * C, rows, C, 3 * C, ldt, C, ldO, 3, {(long long)T_SAB * C, (long long)T_SBC * C, (long long)T_SBC * C, 0},
                         {0, (long long)CC, 2 * (long long)CC, 0}, {C, C, C, 0}, d.rowscale, 2, {-1, -1, 1, -1}};
    if (gemm_grouped_supported(&xs, 1, false, false)) return gemm_grouped_rows(ctx, false, false, &xs, 1, rows, 1);
    st = gemm_rs(ctx, false, false, rows, C, 2 * C, T + T_SAB * C, ldt, 0, X, C, 0, O + O_LOC * C, ldO, 0, 1, 1, nullptr, 0, -1);
    if (st == GF_OK) st = gemm_rs(ctx, false, false, rows, C, C, T + T_SBC * C, ldt, 0, X + 2 * CC, C, 0, O + O_LOC * C, ldO, 0, 1, 1, d.rowscale, 2, 1);
    return st;
}

static gf_status fwd_combine(gf_smp *s, int l, const FusedRoute &r, const BigPart &big, const float *bl) {
    const gf_smp::DevLevel &d = s->lv[l];
    const float *O = level_O(s, l);
    if (!r.panel_combine) {
        if (r.drop) return fail(s->ctx, GF_ERR_UNSUPPORTED, "fused level %d: slice dropout needs the panel combine-forward", l);
        return launch_combine_fwd(s, l, all_quads(s->lay.level[l]), "smpf_combine_fwd", big.nodes > 0, O, bl, r.ocols, nullptr);
    }
    // the top level leaves the readout's partial sums behind, the others the per-channel maxima the level above scales its
    // weight-gradient operands with
    float *psum = (l == s->cfg.nLevels || s->cfg.physics) ? d.psum : nullptr;   // (a tower reads every level out)
    const float *nodefac = r.drop ? d.nodefac : nullptr;
    const gf_status st = smp_combine_fwd_panels_c64(s, l, O, bl, psum, d.pmax, nodefac, r.skip_empty);
    if (st != GF_OK) return st;
    if (psum) s->lv[l].psum_ready = true;
    if (d.pmax && big.nodes == 0) s->lv[l].pmax_ready = true;   // (maxima of the panels only: a level with bigger nodes is scanned)
    // the nodes above 32 positions: workgroup per (node, four x), a 64-position build
    return big.nodes > 0 ? launch_combine_fwd(s, l, big_quads(big), "smpf_combine_fwd_big", true, O, bl, r.ocols, nodefac) : GF_OK;
}

gf_status smp_fused_forward_level(gf_smp *s, int l, const float *Kl, const float *bl) {
    const gf_smp::DevLevel &d = s->lv[l];
    const FusedRoute r = fused_route(s, l);
    const BigPart big = big_part(s->lay.level[l]);
    // what this pass runs the level's products on decides the layout of O / dO (two or three blocks) at C = 32: the reverse sweep
    // follows the forward's choice, not the option's value at the time it runs (round-4 advice)
    s->lv[l].fwd_c64 = r.panels;
    if (r.skip_empty) ++s->empty_row_calls;
    gf_status st = fwd_zero_rows(s, l, r);
    if (st == GF_OK && r.drop) st = fwd_dropout_factors(s, l);
    if (st == GF_OK) st = fwd_tables(s, l, r, big);
    if (st == GF_OK) st = fwd_diag_gather(s, l);
    if (st == GF_OK) st = launch_vectors(s, l, r, big);
    if (st == GF_OK && r.drop) st = dropout_scale(s, l, d.Vt, d.St);
    if (st == GF_OK) st = fwd_small_products(s, l, r);
    if (st == GF_OK) st = fwd_row_products(s, l, r);
    if (st == GF_OK && s->n_extra && !r.extras_in_kernel) st = fwd_extra_products(s, l, r);
    if (st == GF_OK) st = fwd_combine(s, l, r, big, bl);
    return st;
}

// ---- the reverse sweep of a level, step by step ----
static gf_status bwd_refusals(gf_smp *s, int l, const FusedRoute &r) {
    // Slice dropout in TEST mode scales the forward values by nKept / 18 (RisiContraction_18_dropout.h:465-471) and its backward() does
    // not (:480-): a reverse sweep there is neither a derivative nor something the reference's drivers ever run (Predict is forward only).
    // The fused level carries one factor table per pass; the op-by-op levels reproduce that sweep (GF_SMP_FUSED_DROPOUT=0).
    if (s->drop_on && s->drop_scale != 1.f)
        return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_backward: fused level %d under slice dropout in test mode (scale %.4f): set GF_SMP_FUSED_DROPOUT=0 "
                                                "for the reference's unscaled test-mode sweep", l, (double)s->drop_scale);
    // The forward pass wrote O in the layout of ITS product kernels; at C = 32 those exist on the split path only, so an option flipped
    // between the two passes would make this sweep read dO in the other layout: refused instead of differentiated wrongly.  Past this
    // point r.panels IS the forward's choice (DevLevel::fwd_c64).
    if (s->lv[l].fwd_c64 != r.panels)
        return fail(s->ctx, GF_ERR_INVALID, "gf_smp_backward: the product kernels' option (GF_OPT_SMP_FP32_PRODUCTS / GF_SMP_SPLIT / GF_SMP_ROWPANEL / GF_SMP_C128) "
                                            "changed since the forward pass of level %d", l);
    return GF_OK;
}

// combine-backward: dO and the per-(node, x) partials from dF.  On the forward's row panels where they exist (one wave per panel, every
// request up front; the workgroup kernel then serves the nodes above 32 positions), else the workgroup kernel for every node.  Leaves in
// dz_rows / dz_ld (and dz_rows2 / dz_off2 / dz_ld2) where the weight gradients find the column maxima of |dz|.
static gf_status bwd_combine(gf_smp *s, int l, const FusedRoute &r, const BigPart &big, const float *dfrows, const float *node_df) {
    gf_smp::DevLevel &d = s->lv[l];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const int C = s->cfg.nChanels;
    // the workgroup kernels write one row of their window's width per workgroup
    const int wg_ld = smp_half_window(C) ? 32 : 64, wg_nwin = smp_half_window(C) ? C / 32 : (C + 63) / 64;
    float *dO = level_O(s, l);
    float *dzmax = (s->wbound && d.dzmax && r.panels) ? d.dzmax : (float *)nullptr;
    if (!r.panel_combine) {
        d.dz_rows = (long long)h.quad_node.size();
        d.dz_rows2 = 0;
        d.dz_ld = wg_ld;
        return launch_combine_bwd(s, l, all_quads(h), "smpf_combine_bwd", dfrows, node_df, dO, r.ocols, dzmax);
    }
    gf_status st = smp_combine_bwd_panels_c64(s, l, dfrows, node_df, dO, dzmax, r.skip_empty);
    if (st != GF_OK) return st;
    d.dz_rows = d.fwd_npanels;
    d.dz_ld = C;
    d.dz_rows2 = 0;
    if (big.nodes == 0) return GF_OK;
    // the nodes above 32 positions: their column maxima behind the panels' (at C = 64 the panels' width -- one table; at 32 / 16
    // channels a second set, dz_rows2)
    float *dz2 = dzmax ? dzmax + (size_t)d.fwd_npanels * C : (float *)nullptr;
    st = launch_combine_bwd(s, l, big_quads(big), "smpf_combine_bwd_big", dfrows, node_df, dO, r.ocols, dz2);
    if (st != GF_OK) return st;
    if (C == 64) {
        d.dz_rows = d.fwd_npanels + big.quads;
    } else {
        d.dz_rows2 = big.quads * wg_nwin;
        d.dz_off2 = (long long)d.fwd_npanels * C;
        d.dz_ld2 = wg_ld;
    }
    return GF_OK;
}

// <= 256 column partials of the bias gradient per level: nodes per workgroup of smp_reduce_pairs, and the workgroups
static int colpart_blocks(int nodes, int *npb) {
    *npb = (nodes + 255) / 256;
    return (nodes + *npb - 1) / *npb;
}

// dSout per node + the column partials of the bias gradient, and dGc: both in one launch, or (GF_SMP_FUSE_SMALL=0) one each
static gf_status bwd_reduce_and_diag_gather(gf_smp *s, int l, const FusedRoute &r) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const gfsmp::LevelLayout &hp = s->lay.level[l - 1];
    const int C = s->cfg.nChanels, nodes = s->lay.level[l].nNodes, prevNodes = hp.nNodes;
    int npb;
    const int nb = colpart_blocks(nodes, &npb);
    float *colpart = s->colpart + (size_t)l * 256 * C;
    const float *dO = level_O(s, l);
    const float *nfac = r.drop ? d.nodefac : (const float *)nullptr;
    if (r.fuse_small && prevNodes > 0) {
        GF_LAUNCH(ctx, "smpf_diag_gather_bwd", smp_reduce_pairs_and_diag_gather, dim3((unsigned)(nb + prevNodes)), dim3(256), 0, d.dSpart, d.dbpart, d.dSout,
                  colpart, d.node_s, d.node_pair, C, nodes, npb, nb, dO, d.dGc, pv.node_s, pv.node_pair, d.cons_ptr, d.cons_row, d.cons_s, d.cons_a,
                  d.cons_inv_off, d.inv, C, r.ocols, nfac, d.cons_pair, d.pair_node);
    } else {
        GF_LAUNCH(ctx, "smpf_reduce_pairs", smp_reduce_pairs, dim3(nb), dim3(256), 0, d.dSpart, d.dbpart, d.dSout, colpart, d.node_s,
                  d.node_pair, C, nodes, npb);
        GF_LAUNCH(ctx, "smpf_diag_gather_bwd", diag_gather_bwd, dim3(prevNodes), dim3(node_block(hp, C)), 0, dO, d.dGc, pv.node_s, pv.node_pair,
                  d.cons_ptr, d.cons_row, d.cons_s, d.cons_a, d.cons_inv_off, d.inv, C, r.ocols, nfac, d.cons_pair, d.pair_node);
    }
    return GF_OK;
}

// ONE NT launch: dFdc = [dG15 K15^T | dG16 K16^T], dVt = dVout [K1;K3;K7;K10]^T, dSt = dSout [K4;..]^T
static gf_status bwd_small_nt(gf_smp *s, int l, const FusedRoute &r) {
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, pairs = (int)s->lay.level[l].pairs, nodes = s->lay.level[l].nNodes, prevPairs = (int)s->lay.level[l - 1].pairs;
    const size_t CC = (size_t)C * C;
    if (r.small_split) {
        const int prog[3] = {1, 2, 1}, nrows[3] = {pairs, prevPairs, nodes}, pos0[3] = {10, 8, 14};
        const float *in[3] = {d.dVout, d.dGc, d.dSout};
        float *out[3] = {d.dVt, d.dFdc, d.dSt};
        return smp_small_split_c64(s->ctx, true, 3, prog, in, out, nrows, pos0, d.wimg, "smpf_small_nt", C);
    }
    const GemmSpec nt[4] = {gemm_spec(d.dGc, d.Wst + 8 * CC, d.dFdc, prevPairs, C, C, 2 * C, C, 2 * C),
                            gemm_spec(d.dGc + C, d.Wst + 9 * CC, d.dFdc + C, prevPairs, C, C, 2 * C, C, 2 * C),
                            gemm_spec(d.dVout, d.Wst + 10 * CC, d.dVt, pairs, 4 * C, C, C, C, 4 * C),
                            gemm_spec(d.dSout, d.Wst + 14 * CC, d.dSt, nodes, 4 * C, C, C, C, 4 * C)};
    return gemm_grouped_free(s->ctx, true, nt, 4, "smpf_small_nt");
}

// Partial images of the eight row products' weight gradients, for bwd_fold: the row-panel family's kernels into the workspace
// (smp_wgrad_partials picks the kernel), or the grouped split-K launch (its own ordered reduction) into the stacked image, one "image".
// *x_done: the extra products' weight gradients came out of the same kernel.
static gf_status bwd_weight_grads(gf_smp *s, int l, const FusedRoute &r, FoldGroup *rowg, bool *x_done) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int C = s->cfg.nChanels, rows = (int)h.rows;
    const size_t CC = (size_t)C * C;
    const int ldt = T_COLS * C, ldo = O_COLS * C;
    float *T = level_T(s, l), *dO = level_O(s, l);
    gf_status st;
    if (!r.panels) {
        GemmSpec sp[5];
        for (int i = 0; i < 5; ++i) {
            const RowProduct &g = kRowProducts[i];
            sp[i] = gemm_spec(T + g.tcol * C, dO + g.ocol * C, d.dWst + g.wpos * CC, g.kb * C, C, rows, ldt, ldo, C);
            sp[i].rs = g.scol >= 0 ? d.rowscale : nullptr;
            sp[i].rs_ld = 2;
            sp[i].scol[0] = g.scol;
        }
        if (C <= 64 && gemm_grouped_supported(sp, 5, true, false)) {
            st = gemm_grouped_splitk(ctx, sp, 5, rows, d.dWst, 0);
            if (st != GF_OK) return st;
        } else {
            for (const RowProduct &g : kRowProducts) {
                st = gemm_rs(ctx, true, false, g.kb * C, C, rows, T + g.tcol * C, ldt, 0, dO + g.ocol * C, ldo, 0, d.dWst + g.wpos * CC, C, 0, 1, 0,
                             d.rowscale, 2, g.scol);
                if (st != GF_OK) return st;
            }
        }
        // (the split launches above used the workspace from its base; their reductions have been issued, and the launches
        //  that follow are ordered behind them on the same stream)
        rowg->part = d.dWst;
        rowg->splits = 1;
        rowg->n = 8 * CC;
        return GF_OK;
    }
    float *ws = static_cast<float *>(ctx->ws);
    const size_t ws_floats = ctx->ws_bytes / sizeof(float);
    // scratch words of the level: its channel maxima, and the exact bounds' where the level may take them (a 64-channel level never does)
    unsigned *words = s->wbound ? s->wbound + (size_t)l * smp_wgrad_words(C, C != 64) : nullptr;
    WgradCall wc = {T, dO, r.drop ? d.rowfac8 : d.rowscale, rows, C, r.nf, d.trow, d.trowf, WgradScales(), C == 64 ? nullptr : words, ws, ws_floats};
    // The operand columns' exponents come from the largest |f_{l-1}| and |dz_l| of every channel where the level has them: the per-panel
    // maxima combine-forward of the level below left behind (f_{l-1} itself was read for them: 94 MB at cfg3's level 3) or f_0, and
    // the per-workgroup maxima of this level's combine-backward -- 17 - 19 MB of partials at cfg3's level 3 -- reduced by one small
    // launch.  The 32- / 16-channel kernel wants the row factors' maxima on the device (device-built tables); 128 channels: exact only.
    if (words && d.dzmax && r.split && (C == 64 || ((C == 32 || C == 16) && d.row_max))) {
        if (C != 64) GF_HIP_TRY(ctx, hipMemsetAsync(words, 0, sizeof(unsigned) * 64, ctx->stream));   // (64: once per forward, smp.hip)
        const bool pm = pv.pmax && pv.pmax_ready;
        st = smp_wgrad_channel_maxima(ctx, pm ? pv.pmax : pv.f, pm ? (long long)pv.fwd_npanels : (long long)s->lay.level[l - 1].rows, C, d.dzmax,
                                      d.dz_rows, d.dz_ld, C, words);
        if (st != GF_OK) return st;
        if (d.dz_rows2 > 0) {   // (the big nodes' workgroups at 32 / 16 channels: maxima of another row width, folded into the same words)
            st = smp_wgrad_channel_maxima(ctx, pv.f, 0, C, d.dzmax + d.dz_off2, d.dz_rows2, d.dz_ld2, C, words);
            if (st != GF_OK) return st;
        }
        wc.bounds.chan = words;
        wc.bounds.smax = (float)h.buckets.back().s;
        wc.bounds.max_tot = d.max_tot, wc.bounds.max_tr = d.max_tr, wc.bounds.row_max = d.row_max;
    }
    if (r.skip_empty && !wc.bounds.level(C)) return fail(ctx, GF_ERR_INVALID, "fused level %d: empty rows skipped without the level's maxima", l);
    wc.skip_empty = r.skip_empty;
    if (smp_wgrad_reads_absent_blocks(ctx, wc)) {   // (see fused_route: then T needs its structural zeros)
        st = smp_fused_ensure_zero_fill(s, l);
        if (st != GF_OK) return st;
    }
    // SMP_2D_ver7 on the 18-slice level: its three extra products ride in the same kernel where it has them, folded straight into dX
    // (not under slice dropout: the extra products take the plain (tot, tr) row factors)
    FoldGroup xg = {nullptr, 0, 0};
    st = smp_wgrad_partials(ctx, wc, rowg, (s->n_extra && s->extra_g && !r.drop) ? &xg : nullptr);
    if (st != GF_OK) return st;
    if (xg.splits) {
        st = splitk_fold(ctx, xg.part, s->extra_g + (size_t)(l - 1) * 3 * CC, xg.n, xg.splits, 0);
        if (st != GF_OK) return st;
        *x_done = true;
    }
    return GF_OK;
}

// ONE TN launch: dK15, dK16, Vt^T dVout, St^T dSout, each split over its own rows, into the workspace behind the row products' images
static gf_status bwd_small_tn(gf_smp *s, int l, size_t used, FoldGroup *small) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, pairs = (int)s->lay.level[l].pairs, nodes = s->lay.level[l].nNodes, prevPairs = (int)s->lay.level[l - 1].pairs;
    float *ws = static_cast<float *>(ctx->ws);
    const size_t ws_floats = ctx->ws_bytes / sizeof(float);
    // (C = ws + used for the alignment check only: the launcher places the images itself)
    const GemmSpec tn[4] = {gemm_spec(d.Fdc, d.dGc, ws + used, C, C, prevPairs, 2 * C, 2 * C, C),
                            gemm_spec(d.Fdc + C, d.dGc + C, ws + used, C, C, prevPairs, 2 * C, 2 * C, C),
                            gemm_spec(d.Vt, d.dVout, ws + used, 4 * C, C, pairs, 4 * C, C, C),
                            gemm_spec(d.St, d.dSout, ws + used, 4 * C, C, nodes, 4 * C, C, C)};
    return gemm_grouped_free_tn(ctx, tn, 4, ws + used, ws_floats - used, small, "smpf_small_tn");
}

// Every partial image of the level's weight and bias gradients folded, un-stacked and added into dK_l / db_l in ONE launch
static gf_status bwd_fold(gf_smp *s, int l, const FoldGroup &rowg, const FoldGroup *small, float *dKl, float *dbl) {
    const int C = s->cfg.nChanels;
    const size_t CC = (size_t)C * C;
    int npb;
    const int nb = colpart_blocks(s->lay.level[l].nNodes, &npb);
    const FoldGroup colg = {s->colpart + (size_t)l * 256 * C, nb, (size_t)C};
    const FoldGroup *grp[kFoldGroups] = {&rowg, &small[0], &small[1], &small[2], &small[3], &colg};
    const unsigned firsts[kFoldGroups] = {0u, (unsigned)(8 * CC), (unsigned)(9 * CC), (unsigned)(10 * CC), (unsigned)(14 * CC), (unsigned)(18 * CC)};
    FoldArgs fa;
    fa.ngroups = kFoldGroups;
    for (int g = 0; g < kFoldGroups; ++g) {
        fa.part[g] = grp[g]->part;
        fa.splits[g] = grp[g]->splits;
        fa.n[g] = (unsigned)grp[g]->n;
        fa.first[g] = firsts[g];
    }
    const unsigned total = (unsigned)(18 * CC + C);
    GF_LAUNCH(s->ctx, "smpf_fold", smp_fold_level, dim3((total + 63) / 64), dim3(256), 0, fa, dKl, dbl, C, s->cfg.custom_matmul, total);
    return GF_OK;
}

// table gradients dT from dO.  dz_vec (or null): combine-backward's gradient was this per-node vector alone and the level's sign words
// are this pass's -- the backward products then form the dz block of dO themselves instead of reading it, where the row-class kernel
// runs them.  The tiled launches: one grouped launch, or the transposes of kRowProducts one by one.
static gf_status bwd_table_grads(gf_smp *s, int l, const FusedRoute &r, const float *dz_vec) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, rows = (int)s->lay.level[l].rows;
    const size_t CC = (size_t)C * C;
    float *dO = level_O(s, l), *dT = level_dT(s, l);
    if (r.panels) {
        RowProductsCall call = row_products_call(s, l, r, false);
        if (dz_vec && d.rowcls_node && smp_row_products_can_form_dz(ctx, call)) call.dz = {dz_vec, d.sgn, d.rowcls_node};
        return smp_row_products(ctx, call);
    }
    const int ldt = T_COLS * C, ldo = O_COLS * C;
    const long long oC = C, wCC = (long long)CC;
    const GemmSpec dg[3] = {
        {dO, d.Wst, dT + T_SAB * C, rows, C, 4 * C, ldo, C, ldt, 4, {O_LOC * oC, O_LOC * oC, O_Z * oC, O_ZP * oC},
         {0 * wCC, 2 * wCC, 5 * wCC, 7 * wCC}, {C, C, C, C}, d.rowscale, 2, {0, 1, -1, -1}},
        {dO, d.Wst, dT + T_SBC * C, rows, C, 2 * C, ldo, C, ldt, 2, {O_LOC * oC, O_Z * oC, 0, 0}, {1 * wCC, 6 * wCC, 0, 0}, {C, C, 0, 0},
         d.rowscale, 2, {0, -1, -1, -1}},
        {dO, d.Wst, dT + T_T6 * C, rows, 2 * C, C, ldo, C, ldt, 1, {O_LOC * oC, 0, 0, 0}, {3 * wCC, 0, 0, 0}, {C, 0, 0, 0}, nullptr, 0,
         {-1, -1, -1, -1}},
    };
    if (gemm_grouped_supported(dg, 3, false, true)) return gemm_grouped_rows(ctx, false, true, dg, 3, rows);
    // Z first (it writes dS_ab and dS_bc), the others accumulate, [T6|T10] last (written once); a row-scaled product of two table blocks
    // runs block by block
    static const int order[5] = {3, 0, 1, 4, 2};
    for (const int i : order) {
        const RowProduct &g = kRowProducts[i];
        const int pieces = (g.scol >= 0) ? g.kb : 1, acc = (i == 3 || i == 2) ? 0 : 1;
        for (int p = 0; p < pieces; ++p) {
            const gf_status st = gemm_rs(ctx, false, true, rows, (g.kb / pieces) * C, C, dO + g.ocol * C, ldo, 0, d.Wst + (g.wpos + p) * CC, C, 0,
                                         dT + (g.tcol + p) * C, ldt, 0, 1, acc, d.rowscale, 2, g.scol);
            if (st != GF_OK) return st;
        }
    }
    return GF_OK;
}

// the extra products of SMP_2D_ver7 (see the forward): dX = T-block^T L, dT-blocks += L X^T -- what the level's own kernels did not do
static gf_status bwd_extra_products(gf_smp *s, int l, const FusedRoute &r, bool x_wgrad_done) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, rows = (int)s->lay.level[l].rows;
    const size_t CC = (size_t)C * C;
    const bool x_bwd_done = r.extras_in_kernel;   // (their share of dT came out of the backward row-panel kernel)
    float *T = level_T(s, l), *dO = level_O(s, l), *dT = level_dT(s, l);
    gf_status st;
    if (!s->extra_w || !s->extra_g) return fail(ctx, GF_ERR_INVALID, "fused level %d: the extra products' weights are not bound", l);
    if (!x_wgrad_done) {   // (the GEMM that reads T does not mask the absent S_ab blocks)
        st = smp_fused_ensure_zero_fill(s, l);
        if (st != GF_OK) return st;
    }
    const float *X = s->extra_w + (size_t)(l - 1) * 3 * CC;
    float *dX = s->extra_g + (size_t)(l - 1) * 3 * CC;
    const int ldt = T_COLS * C, ldO = r.ocols * C;
    const float *Lg = dO + O_LOC * C;
    // ([X_a; X_b] is one [2 C][C] matrix and [S_ab | S_bc] one [rows][2 C] operand: two products per direction instead of three)
    // d[X_a; X_b] = [S_ab | S_bc]^T L and dX_c = (tr S_bc)^T L: one split launch over the rows, ordered fold
    GemmSpec wg[2] = {gemm_spec(T + T_SAB * C, Lg, nullptr, 2 * C, C, rows, ldt, ldO, C), gemm_spec(T + T_SBC * C, Lg, nullptr, C, C, rows, ldt, ldO, C)};
    wg[1].rs = d.rowscale, wg[1].rs_ld = 2, wg[1].scol[0] = 1;
    // dT[S_ab] += L X_a^T; dT[S_bc] += L X_b^T + tr L X_c^T (two K pieces): one launch
    GemmSpec bg[2] = {gemm_spec(Lg, X, dT + T_SAB * C, rows, C, C, ldO, C, ldt), gemm_spec(Lg, X, dT + T_SBC * C, rows, C, 2 * C, ldO, C, ldt)};
    bg[1].nseg = 2, bg[1].b_off[0] = (long long)CC, bg[1].b_off[1] = 2 * (long long)CC;
    bg[1].klen[0] = bg[1].klen[1] = C, bg[1].rs = d.rowscale, bg[1].rs_ld = 2, bg[1].scol[0] = -1, bg[1].scol[1] = 1;
    if (gemm_grouped_supported(wg, 2, true, false) && gemm_grouped_supported(bg, 2, false, true) && C <= 64) {
        st = x_wgrad_done ? GF_OK : gemm_grouped_splitk(ctx, wg, 2, rows, dX, 0);
        // (the dS_ab rows of structural zeros were not written by the product kernel: what accumulates there is never read either)
        if (st == GF_OK && !x_bwd_done) st = gemm_grouped_rows(ctx, false, true, bg, 2, rows, 1);
    } else {
        st = x_wgrad_done ? GF_OK : gemm_rs(ctx, true, false, 2 * C, C, rows, T + T_SAB * C, ldt, 0, Lg, ldO, 0, dX, C, 0, 1, 0, nullptr, 0, -1);
        if (st == GF_OK && !x_wgrad_done) st = gemm_rs(ctx, true, false, C, C, rows, T + T_SBC * C, ldt, 0, Lg, ldO, 0, dX + 2 * CC, C, 0, 1, 0, d.rowscale, 2, 1);
        if (st == GF_OK && !x_bwd_done) st = gemm_rs(ctx, false, true, rows, 2 * C, C, Lg, ldO, 0, X, C, 0, dT + T_SAB * C, ldt, 0, 1, 1, nullptr, 0, -1);
        if (st == GF_OK && !x_bwd_done) st = gemm_rs(ctx, false, true, rows, C, C, Lg, ldO, 0, X + 2 * CC, C, 0, dT + T_SBC * C, ldt, 0, 1, 1, d.rowscale, 2, 1);
    }
    return st;
}

// dP into s->P for promote_backward (the two-kernel form of the gather: GF_SMP_BWD_GATHER=0, or sources above the gather's reach)
static gf_status bwd_tables(gf_smp *s, int l) {
    gf_status st = ensure_P(s);
    if (st != GF_OK) return st;
    for (const SizeClass &c : classes_of(s->lay.level[l], 4)) {
        st = launch_tables_bwd(s, l, c, level_dT(s, l));
        if (st != GF_OK) return st;
    }
    return GF_OK;
}

// df_l is given in d.df, or as one vector per node (node_df: the readout's broadcast), or -- a tower's level below the top, rows_too --
// both.  Accumulates dK_l and db_l; leaves dT for the consumer gather (smp_fused_gather_backward), or dP in s->P for the promotion backward.
gf_status smp_fused_backward_level(gf_smp *s, int l, float *dKl, float *dbl, const float *node_df, bool rows_too) {
    const gf_smp::DevLevel &d = s->lv[l];
    const FusedRoute r = fused_route(s, l);
    const BigPart big = big_part(s->lay.level[l]);
    gf_status st = bwd_refusals(s, l, r);
    if (st != GF_OK) return st;
    if (r.skip_empty) ++s->empty_row_calls;
    const float *dfrows = (node_df && !rows_too) ? nullptr : d.df;
    st = bwd_combine(s, l, r, big, dfrows, node_df);
    if (st != GF_OK) return st;
    // the top level of a plain model without nodes above 32 positions: dz[row] = node_df[node(row)] * slope(sign words of the row)
    const bool vec_only = r.panel_combine && !dfrows && node_df && big.nodes == 0 && r.sign_mask;
    FoldGroup rowg, small[4];
    bool x_wgrad_done = false;
    st = bwd_reduce_and_diag_gather(s, l, r);
    if (st == GF_OK) st = bwd_small_nt(s, l, r);
    if (st == GF_OK && r.drop) st = dropout_scale(s, l, d.dVt, d.dSt);
    if (st == GF_OK) st = bwd_weight_grads(s, l, r, &rowg, &x_wgrad_done);
    if (st == GF_OK) st = bwd_small_tn(s, l, r.panels ? (size_t)rowg.splits * rowg.n : 0, small);
    if (st == GF_OK) st = bwd_fold(s, l, rowg, small, dKl, dbl);
    if (st == GF_OK) st = smp_dp_level_done(s, l);  // data-parallel: dK_l and db_l are final -- their all-reduce runs beside what follows
    if (st == GF_OK) st = bwd_table_grads(s, l, r, vec_only ? node_df : nullptr);
    if (st == GF_OK && s->n_extra) st = bwd_extra_products(s, l, r, x_wgrad_done);
    if (st == GF_OK && !r.gather) st = bwd_tables(s, l);   // (else dP is evaluated inside the consumer gather)
    return st;
}

}  // namespace gf
