// smp_fused_combine.hip -- the workgroup-per-(node, four x) combine kernels of the fused SMP level (smp_fused.hip): every node of a level the
// row-panel kernels do not serve, and the nodes above 32 positions of one they do.
#include "smp_fused_internal.h"

using namespace gf::dev;

namespace gf {
namespace {

constexpr float kAlphaF = 0.01f;
__device__ __forceinline__ float lreluf(float z) { return z > 0.f ? z : kAlphaF * z; }

// ---------------------------------------------------------------------------------------------------------------
// combine-forward.  Workgroup per (node, four consecutive x) -- the quads of tables-forward: f_l[x, y, :] for all y.
// A workgroup lives for little more than its memory latencies (one barrier between the gather of U = Z + Z'^T + compact
// terms and the A-products), so four x per workgroup put four times the loads in flight per latency and read the
// adjacency once instead of four times.  Items = (x, e) / (x, y) pairs dealt to the sixteen row groups.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCombX = 4;
constexpr int kFusedMaxN = 32;  // receptive-field cap of the fused levels (smp_fused_supported)
struct QuadWhere {
    int N, x0, cnt, node, win;
    size_t rowbase, pairbase;
};
__device__ __forceinline__ QuadWhere locate_quad(const int *quad_node, const int *quad_b0, const int *node_s,
                                                 const long long *node_row, const long long *node_pair, int nwin) {
    QuadWhere w;
    const int q = (int)(blockIdx.x / nwin);
    w.win = (int)(blockIdx.x % nwin);
    w.node = quad_node[q];
    w.x0 = quad_b0[q];
    w.N = node_s[w.node];
    w.cnt = (w.N - w.x0 < kCombX) ? w.N - w.x0 : kCombX;
    w.rowbase = (size_t)node_row[w.node];
    w.pairbase = (size_t)node_pair[w.node];
    return w;
}

template <int LPC, int MAXN = kFusedMaxN>   // MAXN: largest receptive field of the launch (64: the nodes above 32 positions, round 6)
__global__ __launch_bounds__(kThreads) void smp_combine_fwd(const float *__restrict__ O, const float *__restrict__ A,
                                                            const float *__restrict__ Vout, const float *__restrict__ Sout,
                                                            const float *__restrict__ bias, float *__restrict__ F,
                                                            const int *__restrict__ quad_node, const int *__restrict__ quad_b0,
                                                            const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                            const long long *__restrict__ node_pair, int C, int nwin,
                                                            const float *__restrict__ Gc, const long long *__restrict__ pair_src_pair,
                                                            const short *__restrict__ pi, const float *__restrict__ rsum,
                                                            int ocols,  // 3: O = [O_loc | Z | Z']; 2: O = [O_loc | U], U = Z + Z'^T
                                                            const float *__restrict__ nodefac = nullptr) {  // (or null) slice dropout: [nodes][18]
    // factors; the compact products G15 / G16 take theirs here (as smp_combine_fwd_panels)
    constexpr int CW = 4 * LPC;
    const size_t ldo = (size_t)ocols * C;
    constexpr int NGRP = kThreads / LPC;
    const int tid = threadIdx.x;
    const int grp = tid / LPC, fl = tid % LPC;
    const QuadWhere W = locate_quad(quad_node, quad_b0, node_s, node_row, node_pair, nwin);
    const int N = W.N, items = W.cnt * N;
    const size_t rowbase = W.rowbase, pairbase = W.pairbase;
    const int f = W.win * CW + 4 * fl;
    const bool fok = f < C;
    const int fc = fok ? f : 0;

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AdjLds L = load_adjacency_lite<false>(smem, A + rowbase, rsum + pairbase, N);  // (published by the barrier below)
    float *sU = smem + adj_lds_floats(N);  // [kCombX][N][CW]  Z[x,e] + Z'[e,x] (+ compact terms)
    // Phase-2 item `it` = (xi, y) reads the O_loc block of the row whose U block phase-1 item `it` = (xi, e = y) reads:
    // both are fetched here, so a workgroup pays one HBM round trip instead of one either side of the barrier.
    constexpr int MAXIT = (kCombX * MAXN + NGRP - 1) / NGRP;  // fused levels: N <= 32 (64 for the launch over the big nodes, smp_fused_supported)
    f4 oloc[MAXIT];
#pragma unroll
    for (int k = 0; k < MAXIT; ++k) {
        const int it = grp + k * NGRP;
        if (it >= items) break;
        const int xi = it / N, e = it - xi * N, x = W.x0 + xi;
        const float *orow = O + (rowbase + (size_t)x * N + e) * ldo + fc;
        f4 u = ld4(orow + O_Z * C);
        oloc[k] = ld4(orow + O_LOC * C);
        if (ocols == 3) u += ld4(O + (rowbase + (size_t)e * N + x) * ldo + O_ZP * C + fc);
        {  // + D_bb[x,e] K15 + D_ac[e,x] K16, gathered from the compact products of the level below
            const int pxe = pi[rowbase + (size_t)x * N + e], pex = pi[rowbase + (size_t)e * N + x];
            const f4 g15 = ld4(Gc + (size_t)(pair_src_pair[pairbase + x] + (pxe >= 0 ? pxe : 0)) * 2 * C + fc);
            const f4 g16 = ld4(Gc + (size_t)(pair_src_pair[pairbase + e] + (pex >= 0 ? pex : 0)) * 2 * C + C + fc);
            const float c15 = nodefac ? nodefac[(size_t)W.node * 18 + 15] : 1.f, c16 = nodefac ? nodefac[(size_t)W.node * 18 + 16] : 1.f;
            if (pxe >= 0) u += c15 * g15;
            if (pex >= 0) u += c16 * g16;
        }
        st4(sU + (size_t)it * CW + 4 * fl, fok ? u : splat(0.f));
    }
    float *sV = sU + (size_t)kCombX * N * CW;  // [kCombX][CW]  Vout rows of the quad's x
    if (grp < W.cnt) st4(sV + grp * CW + 4 * fl, ld4(Vout + (pairbase + W.x0 + grp) * (size_t)C + fc));
    const f4 sout = ld4(Sout + (size_t)W.node * C + fc);
    const f4 bb = ld4(bias + fc);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MAXIT; ++k) {
        const int it = grp + k * NGRP;
        if (it >= items) break;
        const int xi = it / N, y = it - xi * N, x = W.x0 + xi;
        const float *const Tt[1] = {sU + (size_t)xi * N * CW};
        f4 m[1];
        small_matvec<1, CW>(L, N, y, fl, Tt, m);
        const f4 vout = ld4(sV + xi * CW + 4 * fl);
        const f4 z = bb + oloc[k] + m[0] + L.r[y] * vout + L.at(x, y, N) * sout;
        if (fok) {
            f4 out;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = lreluf(z[j]);
            st4(F + (rowbase + (size_t)x * N + y) * (size_t)C + f, out);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// combine-backward.  Workgroup per (node, four consecutive x): from dF[x,:,:] produce dO[(x,y)] (the O_loc block), dZ[(x,e)],
// dZ'[(e,x)] and the per-(node,x) partials dVout, dS-part, db-part.
// ---------------------------------------------------------------------------------------------------------------
template <int LPC, int UB = 4>   // UB: rows whose loads a thread issues together, ahead of their stores (measured at cfg3: 2 -> 0.72, 4 -> 0.70, 8 -> 0.81 ms)
__global__ __launch_bounds__(kThreads) void smp_combine_bwd(const float *__restrict__ F, const float *__restrict__ dF,
                                                            const float *__restrict__ node_dF,  // [nodes][C] or null: (dF null) dF is
                                                            // the same C-vector at every (x,y) of a node (readout broadcast)
                                                            const float *__restrict__ A, float *__restrict__ dO,
                                                            float *__restrict__ dVout, float *__restrict__ dSpart,
                                                            float *__restrict__ dbpart, const int *__restrict__ quad_node,
                                                            const int *__restrict__ quad_b0, const int *__restrict__ node_s,
                                                            const long long *__restrict__ node_row,
                                                            const long long *__restrict__ node_pair, int C, int nwin,
                                                            const float *__restrict__ rsum, int ocols,
                                                            float *__restrict__ dzmax) {  // or null: [workgroups][CW] largest |dz| per column
    // of this workgroup's rows (C = 64: the weight gradients' column exponents, WgradScales::chan)
    constexpr int CW = 4 * LPC;
    constexpr int NGRP = kThreads / LPC;
    const int tid = threadIdx.x;
    const int grp = tid / LPC, fl = tid % LPC;
    const QuadWhere W = locate_quad(quad_node, quad_b0, node_s, node_row, node_pair, nwin);
    const int N = W.N, items = W.cnt * N;
    const size_t rowbase = W.rowbase, pairbase = W.pairbase;
    const int f = W.win * CW + 4 * fl;
    const bool fok = f < C;
    const int fc = fok ? f : 0;
    const size_t ldo = (size_t)ocols * C;
    f4 dzm = splat(0.f);

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const AdjLds L = load_adjacency_lite<true>(smem, A + rowbase, rsum + pairbase, N);  // L.A[e][y] = A+[y][e]; see the barrier below
    float *sDz = smem + adj_lds_floats(N);  // [kCombX][N][CW]
    const f4 gnode = node_dF ? ld4(node_dF + (size_t)W.node * C + fc) : splat(0.f);
    for (int it0 = grp; it0 < items; it0 += UB * NGRP) {
        f4 fv[UB], g[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int it = it0 + u * NGRP;
            if (it < items) {
                const int xi = it / N, y = it - xi * N;
                const size_t row = rowbase + (size_t)(W.x0 + xi) * N + y;
                fv[u] = ld4(F + row * C + fc);
                g[u] = !node_dF ? ld4(dF + row * C + fc) : dF ? gnode + ld4(dF + row * C + fc) : gnode;   // (a tower's level below the top: both)
            }
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int it = it0 + u * NGRP;
            if (it < items) {
                const int xi = it / N, y = it - xi * N;
                const size_t row = rowbase + (size_t)(W.x0 + xi) * N + y;
                f4 dz;
#pragma unroll
                for (int j = 0; j < 4; ++j) dz[j] = fok ? g[u][j] * (fv[u][j] > 0.f ? 1.f : kAlphaF) : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) dzm[j] = fmaxf(dzm[j], fabsf(dz[j]));
                st4(sDz + (size_t)it * CW + 4 * fl, dz);
                if (fok) st4(dO + row * ldo + O_LOC * C + f, dz);
            }
        }
    }
    __syncthreads();
    for (int it = grp; it < items; it += NGRP) {
        const int xi = it / N, e = it - xi * N, x = W.x0 + xi;
        const float *const Tt[1] = {sDz + (size_t)xi * N * CW};
        f4 m[1];
        small_matvec<1, CW>(L, N, e, fl, Tt, m);  // dU[e] = sum_y A+[y][e] dz[y]
        if (fok) {
            st4(dO + (rowbase + (size_t)x * N + e) * ldo + O_Z * C + f, m[0]);
            if (ocols == 3) st4(dO + (rowbase + (size_t)e * N + x) * ldo + O_ZP * C + f, m[0]);
        }
    }
    if (fok) {
        for (int it = grp; it < W.cnt * 3; it += NGRP) {  // (x, which) : r[y] | A+[x][y] | 1 weighted sums over y
            const int xi = it / 3, k = it - xi * 3, x = W.x0 + xi;
            const float *dz = sDz + (size_t)xi * N * CW + 4 * fl;
            f4 acc = splat(0.f);
            for (int y = 0; y < N; ++y) {
                const float w = (k == 0) ? L.r[y] : (k == 1) ? L.A[y * (N + 1) + x] : 1.f;
                acc += w * ld4(dz + y * CW);
            }
            float *dst = (k == 0) ? dVout : (k == 1) ? dSpart : dbpart;
            st4(dst + (pairbase + x) * (size_t)C + f, acc);
        }
    }
    if (dzmax) {  // (uniform) the sixteen row groups' maxima through the image of dz, which nobody reads any more
        __syncthreads();
        st4(sDz + (size_t)grp * CW + 4 * fl, dzm);
        __syncthreads();
        if (grp == 0) {
            f4 m = dzm;
            for (int g = 1; g < NGRP; ++g) {
                const f4 v = ld4(sDz + (size_t)g * CW + 4 * fl);
#pragma unroll
                for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], v[j]);
            }
            st4(dzmax + (size_t)blockIdx.x * CW + 4 * fl, m);
        }
    }
}

template <int LPC>
size_t combine_lds(int N) {
    constexpr int CW = 4 * LPC;
    return sizeof(float) * ((size_t)adj_lds_floats(N) + (size_t)kCombX * (N + 1) * CW);  // + the forward's Vout rows
}

template <int LPC, int MAXN>
gf_status launch_combine_fwd_t(gf_smp *s, int l, const QuadRange &q, const char *name, const float *O, const float *bias, int ocols,
                               const float *nodefac) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, nwin = (C + 63) / 64;
    const size_t lds = combine_lds<LPC>(q.smax);
    gf_status st = opt_in_lds(ctx, smp_combine_fwd<LPC, MAXN>, lds);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, name, (smp_combine_fwd<LPC, MAXN>), dim3((unsigned)((size_t)q.quads * nwin)), dim3(kThreads), lds, O, d.adj, d.Vout, d.Sout, bias, d.f,
              d.quad_node + q.quad0, d.quad_b0 + q.quad0, d.node_s, d.node_row, d.node_pair, C, nwin, d.Gc, d.pair_src_pair, d.pi, d.rsum, ocols, nodefac);
    return GF_OK;
}

template <int LPC>
gf_status launch_combine_bwd_t(gf_smp *s, int l, const QuadRange &q, const char *name, const float *dfrows, const float *node_df, float *dO, int ocols,
                               float *dzmax) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, nwin = (C + 4 * LPC - 1) / (4 * LPC);   // (eight lanes: whole 32-channel windows)
    // (the column maxima go through kThreads / LPC x 4 LPC floats of the dz image: room for them whatever the field size)
    const size_t lds = std::max(combine_lds<LPC>(q.smax), sizeof(float) * ((size_t)adj_lds_floats(q.smax) + 1024));
    gf_status st = opt_in_lds(ctx, smp_combine_bwd<LPC>, lds);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, name, (smp_combine_bwd<LPC>), dim3((unsigned)((size_t)q.quads * nwin)), dim3(kThreads), lds, d.f, dfrows, node_df, d.adj, dO, d.dVout,
              d.dSpart, d.dbpart, d.quad_node + q.quad0, d.quad_b0 + q.quad0, d.node_s, d.node_row, d.node_pair, C, nwin, d.rsum, ocols, dzmax);
    return GF_OK;
}

}  // namespace

gf_status launch_combine_fwd(gf_smp *s, int l, const QuadRange &q, const char *name, bool wide, const float *O, const float *bias, int ocols,
                             const float *nodefac) {
    return wide ? launch_combine_fwd_t<16, kFusedMaxField>(s, l, q, name, O, bias, ocols, nodefac)
                : launch_combine_fwd_t<16, kFusedMaxN>(s, l, q, name, O, bias, ocols, nodefac);
}

gf_status launch_combine_bwd(gf_smp *s, int l, const QuadRange &q, const char *name, const float *dfrows, const float *node_df, float *dO, int ocols,
                             float *dzmax) {
    return smp_half_window(s->cfg.nChanels) ? launch_combine_bwd_t<8>(s, l, q, name, dfrows, node_df, dO, ocols, dzmax)
                                            : launch_combine_bwd_t<16>(s, l, q, name, dfrows, node_df, dO, ocols, dzmax);
}

}  // namespace gf
