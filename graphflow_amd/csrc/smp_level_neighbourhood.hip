// smp_level_neighbourhood.hip -- NeuralFingerprint, GCN_1D and GCN_2D (cfg.neighbourhood = 1, 2, 3; GraphFlow/NeuralFingerprint.h, GCN_1D.h,
// GCN_2D.h): the seventh LevelKind and, because level 0 and the read-out are these models' own (softmax, a plain sum), both sweeps of such a
// handle.  One vector h_l[v] [H] per vertex and level:
//   h_0[v] = softmax(W1_0 x[v]);   n_l[v] = aggregate of h_{l-1}[u] over N_l(v);   h_l[v] = softmax(W1_l x[v] + W2_l n_l[v])
//   predict = <W, sum_v h_L[v]>, loss = 0.5 (predict - target)^2
// N_l(v) is a neighbour list of the batch (gfsmp::BatchLayout::nb_lists, members ascending), the aggregate a sum (forms 1, 2) or RisiLayer2D
// (form 3) in closed form: with T_u = sum_k a_u[k], A = sum_u a_u, Tt = sum_u T_u,  n[i] = A[i] Tt - sum_u a_u[i] T_u  and
// da_w[j] = g[j] (Tt - T_w) + <g, A - a_w>.  Summed over the consumers v of a source w that is
//   dh_{l-1}[w][j] = sum_v g_v[j] Tt_v  -  T_w sum_v g_v[j]  +  sum_v <g_v, A_v>  -  <sum_v g_v, a_w>:
// two vector gathers, one scalar gather and one dot product per source.  Softmax::backward is the class's diagonal rule dz = dh h (1 - h).
//   nbh_level_fwd    one launch per level (level 0: no aggregate): W1_l^T and W2_l^T in LDS once per workgroup, a group of G lanes
//                    (G = 8 .. 64, the power of two at or above H; two channels per lane above 64) per vertex: gather, the two products,
//                    max / exp / sum across the group's lanes; stores h_l, n_l and in form 3 A, Tt and T = sum_k h_l[k]
//   nbh_node_bwd     dz in place of dh_l (the top level takes dy[mol] W instead), dn = W2_l^T dz; form 3: dn Tt and <dn, A> beside it
//   nbh_gather_bwd   dh_{l-1} over the transposed list
//   nbh_readout      the sum over a molecule's vertices, prediction, loss, dy; dW is smp_vertex_level.hip's vertex_readout_dW
// dW1_l = dz^T X and dW2_l = dz^T N are the library's deterministic TN products.  Every sum runs in a fixed order; no atomics; an operand
// of a lane without a channel is loaded from a clamped address and never stored (NOTES.md: no guard around an operand load).
// The four kernels and the read-out are also operators of the C ABI on caller-supplied operands (gf_smp_neighbourhood_fwd_ex_f32,
// _node_bwd_ex_f32, _gather_bwd_ex_f32, _readout_ex_f32 at the end of the file), through the launchers the level uses.
// The three level kernels take TWO operand sets by value (gf_nbh_fwd_set / _node_set / _gather_set of include/gf_hip.h) and blockIdx.y
// picks one: a distance handle (smp_level_distance.hip) runs its vertex and its distance channel in one launch each (nsets = 2 of
// smp_neighbourhood_fwd / _node / _gather, gf_smp_neighbourhood_*2_ex_f32).  Everybody else launches grid.y = 1 with the one set given
// twice.  The lane helpers, the list checks and the sweep's tail are smp_vertex_level.h's.
#include <cmath>

#include "smp_vertex_level.h"

namespace gf {
using namespace vertex_level;
namespace {

template <int NK, bool PAIRS>
__device__ __forceinline__ void level_fwd_body(const float *__restrict__ W1, const float *__restrict__ W2, const float *__restrict__ x,
                                               const float *__restrict__ hprev, const float *__restrict__ Tprev,
                                               const long long *__restrict__ ptr, const int *__restrict__ idx, float *__restrict__ h,
                                               float *__restrict__ n, float *__restrict__ A, float *__restrict__ T, float *__restrict__ Tt, int nV,
                                               int H, int FD, int G, int vpg) {
    extern __shared__ __align__(16) float lds[];
    const int Hp = row_stride(H);
    float *W1t = lds;                            // [FD][Hp]: W1t[f][c] = W1[c][f]
    float *W2t = W1t + (size_t)FD * Hp;          // [H][Hp]:  W2t[k][c] = W2[c][k]
    float *nbuf = W2t + (size_t)H * Hp;          // [slots][H]
    for (int i = threadIdx.x; i < H * FD; i += kBlock) {
        const int c = i / FD, f = i - c * FD;
        W1t[f * Hp + c] = W1[i];
    }
    if (W2)
        for (int i = threadIdx.x; i < H * H; i += kBlock) {
            const int c = i / H, k = i - c * H;
            W2t[k * Hp + c] = W2[i];
        }
    __syncthreads();
    const Slot sl = slot_of(G);
    float *nb = nbuf + sl.slot * H;
    int cc[NK];
    bool ok[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        ok[k] = sl.c0 + 64 * k < H;
        cc[k] = ok[k] ? sl.c0 + 64 * k : H - 1;
    }
    const int vbase = blockIdx.x * vpg;
    for (int it = 0; it < vpg; it += sl.slots) {   // (the same trip count in every wave: the barriers below are the workgroup's)
        const int v = vbase + it + sl.slot;
        const bool live = v < nV;
        const size_t vv = live ? v : nV - 1;
        if (W2) {
            float a[NK], sacc[NK], tt = 0.f;
#pragma unroll
            for (int k = 0; k < NK; ++k) a[k] = sacc[k] = 0.f;
            const long long e1 = ptr[vv + 1];
            for (long long e = ptr[vv]; e < e1; ++e) {
                const size_t u = (size_t)idx[e];
                const float tu = PAIRS ? Tprev[u] : 0.f;
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const float hv = hprev[u * H + cc[k]];
                    a[k] += hv;
                    if (PAIRS) sacc[k] = fmaf(hv, tu, sacc[k]);
                }
                tt += tu;
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                // (one member: A Tt and the sum are the same rounded product, n = 0 exactly as in the class)
                const float nk = PAIRS ? mul_rounded(a[k], tt) - sacc[k] : a[k];
                if (ok[k]) nb[cc[k]] = nk;
                if (live && ok[k]) {
                    n[vv * H + cc[k]] = nk;
                    if (PAIRS) A[vv * H + cc[k]] = a[k];
                }
            }
            if (PAIRS && live && sl.c0 == 0) Tt[vv] = tt;
            __syncthreads();
        }
        float z[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) z[k] = 0.f;
        for (int f = 0; f < FD; ++f) {
            const float xf = x[vv * FD + f];
#pragma unroll
            for (int k = 0; k < NK; ++k) z[k] = fmaf(W1t[f * Hp + cc[k]], xf, z[k]);
        }
        if (W2) {
            for (int j = 0; j < H; ++j) {
                const float nj = nb[j];
#pragma unroll
                for (int k = 0; k < NK; ++k) z[k] = fmaf(W2t[j * Hp + cc[k]], nj, z[k]);
            }
            __syncthreads();   // (nb is rewritten by the next vertex of the slot)
        }
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NK; ++k) m = fmaxf(m, ok[k] ? z[k] : -INFINITY);
        m = group_max(m, G);
        float ex[NK], sum = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            ex[k] = ok[k] ? expf(z[k] - m) : 0.f;
            sum += ex[k];
        }
        sum = group_sum(sum, G);
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float hv = ex[k] / sum;
            if (live && ok[k]) h[vv * H + cc[k]] = hv;
            t += ok[k] ? hv : 0.f;
        }
        if (PAIRS) {
            t = group_sum(t, G);
            if (live && sl.c0 == 0) T[vv] = t;
        }
    }
}
// The launch: blockIdx.y picks one of two operand sets passed by value (a distance handle's vertex and distance channel; grid.y = 1: the
// one set of every other caller, given twice).  The pick is uniform for the workgroup; the dynamic LDS is sized for the wider operand.
template <int NK, bool PAIRS>
__global__ __launch_bounds__(kBlock) void nbh_level_fwd(const gf_nbh_fwd_set s0, const gf_nbh_fwd_set s1, const long long *__restrict__ ptr,
                                                        const int *__restrict__ idx, int nV, int H, int G, int vpg) {
    const bool second = blockIdx.y != 0;
    level_fwd_body<NK, PAIRS>(second ? s1.W1 : s0.W1, second ? s1.W2 : s0.W2, second ? s1.x : s0.x, second ? s1.hprev : s0.hprev,
                              second ? s1.Tprev : s0.Tprev, ptr, idx, second ? s1.h : s0.h, second ? s1.n : s0.n, second ? s1.A : s0.A,
                              second ? s1.T : s0.T, second ? s1.Tt : s0.Tt, nV, H, second ? s1.FD : s0.FD, G, vpg);
}

// dz = dh h (1 - h) in place of dh (top: dh = dy[mol] W), and below level 0's: dn = W2^T dz; PAIRS: dn Tt and <dn, A>
template <int NK, bool PAIRS>
__device__ __forceinline__ void node_bwd_body(const float *__restrict__ W2, const float *__restrict__ h, float *__restrict__ dh,
                                              const float *__restrict__ dy, const float *__restrict__ Wout, const int *__restrict__ vmol,
                                              const float *__restrict__ A, const float *__restrict__ Tt, float *__restrict__ dn,
                                              float *__restrict__ gTt, float *__restrict__ sA, int nV, int H, int G, int vpg) {
    extern __shared__ __align__(16) float lds[];
    float *W2s = lds;                                  // [H][H] as it is: lanes run along a row
    float *dzbuf = W2s + (W2 ? (size_t)H * H : 0);     // [slots][H]
    if (W2)
        for (int i = threadIdx.x; i < H * H; i += kBlock) W2s[i] = W2[i];
    __syncthreads();
    const Slot sl = slot_of(G);
    float *dzb = dzbuf + sl.slot * H;
    int cc[NK];
    bool ok[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        ok[k] = sl.c0 + 64 * k < H;
        cc[k] = ok[k] ? sl.c0 + 64 * k : H - 1;
    }
    const int vbase = blockIdx.x * vpg;
    for (int it = 0; it < vpg; it += sl.slots) {
        const int v = vbase + it + sl.slot;
        const bool live = v < nV;
        const size_t vv = live ? v : nV - 1;
        const float top = dy ? dy[vmol[vv]] : 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float hv = h[vv * H + cc[k]];
            const float d = dy ? top * Wout[cc[k]] : dh[vv * H + cc[k]];
            const float dz = d * hv * (1.f - hv);
            if (ok[k]) dzb[cc[k]] = dz;
            if (live && ok[k]) dh[vv * H + cc[k]] = dz;
        }
        if (!W2) continue;   // (level 0: uniform for the launch)
        __syncthreads();
        float g[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) g[k] = 0.f;
        for (int c = 0; c < H; ++c) {
            const float dzc = dzb[c];
#pragma unroll
            for (int k = 0; k < NK; ++k) g[k] = fmaf(W2s[c * H + cc[k]], dzc, g[k]);
        }
        __syncthreads();
        float dot = 0.f;
        const float ttv = PAIRS ? Tt[vv] : 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (PAIRS) dot += ok[k] ? g[k] * A[vv * H + cc[k]] : 0.f;
            if (live && ok[k]) {
                dn[vv * H + cc[k]] = g[k];
                if (PAIRS) gTt[vv * H + cc[k]] = g[k] * ttv;
            }
        }
        if (PAIRS) {
            dot = group_sum(dot, G);
            if (live && sl.c0 == 0) sA[vv] = dot;
        }
    }
}
template <int NK, bool PAIRS>
__global__ __launch_bounds__(kBlock) void nbh_node_bwd(const gf_nbh_node_set s0, const gf_nbh_node_set s1, const float *__restrict__ dy,
                                                       const int *__restrict__ vmol, int nV, int H, int G, int vpg) {
    const bool second = blockIdx.y != 0;
    node_bwd_body<NK, PAIRS>(second ? s1.W2 : s0.W2, second ? s1.h : s0.h, second ? s1.dh : s0.dh, dy, second ? s1.Wout : s0.Wout, vmol,
                             second ? s1.A : s0.A, second ? s1.Tt : s0.Tt, second ? s1.dn : s0.dn, second ? s1.gTt : s0.gTt,
                             second ? s1.sA : s0.sA, nV, H, G, vpg);
}

// dh_{l-1}[w] over the consumers of w (the transposed list, ascending): the sum of dn, or form 3's closed form (see the head of the file)
template <int NK, bool PAIRS>
__device__ __forceinline__ void gather_bwd_body(const long long *__restrict__ tptr, const int *__restrict__ tidx, const float *__restrict__ dn,
                                                const float *__restrict__ gTt, const float *__restrict__ sA, const float *__restrict__ hprev,
                                                const float *__restrict__ Tprev, float *__restrict__ dhprev, int nV, int H, int G) {
    const Slot sl = slot_of(G);
    const long long w = (long long)blockIdx.x * sl.slots + sl.slot;
    const bool live = w < nV;
    const size_t ww = live ? (size_t)w : (size_t)nV - 1;
    int cc[NK];
    bool ok[NK];
    float gs[NK], ps[NK], sa = 0.f;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        ok[k] = sl.c0 + 64 * k < H;
        cc[k] = ok[k] ? sl.c0 + 64 * k : H - 1;
        gs[k] = ps[k] = 0.f;
    }
    const long long e1 = tptr[ww + 1];
    for (long long e = tptr[ww]; e < e1; ++e) {
        const size_t v = (size_t)tidx[e];
        if (PAIRS) sa += sA[v];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            gs[k] += dn[v * H + cc[k]];
            if (PAIRS) ps[k] += gTt[v * H + cc[k]];
        }
    }
    if (PAIRS) {
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) dot += ok[k] ? gs[k] * hprev[ww * H + cc[k]] : 0.f;
        dot = group_sum(dot, G);
        const float tw = Tprev[ww];
#pragma unroll
        for (int k = 0; k < NK; ++k) gs[k] = (ps[k] - tw * gs[k]) + (sa - dot);
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (live && ok[k]) dhprev[ww * H + cc[k]] = gs[k];
}
template <int NK, bool PAIRS>
__global__ __launch_bounds__(kBlock) void nbh_gather_bwd(const long long *__restrict__ tptr, const int *__restrict__ tidx, const gf_nbh_gather_set s0,
                                                         const gf_nbh_gather_set s1, int nV, int H, int G) {
    const bool second = blockIdx.y != 0;
    gather_bwd_body<NK, PAIRS>(tptr, tidx, second ? s1.dn : s0.dn, second ? s1.gTt : s0.gTt, second ? s1.sA : s0.sA, second ? s1.hprev : s0.hprev,
                               second ? s1.Tprev : s0.Tprev, second ? s1.dhprev : s0.dhprev, nV, H, G);
}

// one wave per molecule: g = sum over its vertices (ascending) of h_L, predict = <W, g>, the squared loss and dy = predict - target
__global__ __launch_bounds__(64) void nbh_readout(const float *__restrict__ hL, const int *__restrict__ mol_ptr, const float *__restrict__ W,
                                                  const float *__restrict__ target, float *__restrict__ g, float *__restrict__ yhat,
                                                  float *__restrict__ loss, float *__restrict__ dy, int H) {
    const int m = blockIdx.x;
    float part = 0.f;
    for (int c = threadIdx.x; c < H; c += 64) {
        float acc = 0.f;
        for (int v = mol_ptr[m]; v < mol_ptr[m + 1]; ++v) acc += hL[(size_t)v * H + c];
        g[(size_t)m * H + c] = acc;
        part = fmaf(acc, W[c], part);
    }
    part = wave_sum(part);
    GF_STORE_PREDICTION(m, part, target, yhat, loss, dy);
}

// W1_0; (W1_l, W2_l) l = 1..L; W
template <typename P>
struct View {
    std::vector<P *> W1, W2;
    P *W;
    View(const gfsmp::Config &c, P *p) {   // (view_params: the matrix block of level l is W1_l then W2_l)
        view_params<P>(c, p, &p, &W1, &W2, &W);
        W1[0] = p;
        for (int l = 1; l <= c.nLevels; ++l) W2[l] = W1[l] + c.level_blocks(l).mat[0].n;
    }
};

// vertices per workgroup: whole rounds of its slots, at most GF_NBH_MAX_ROUNDS of them (an A/B build may set another: NOTES.md has what
// was measured).  A workgroup stages W1_l^T and W2_l^T once however many vertices it takes, but its vertices run one after the other
// between two barriers each: more workgroups hide that latency, and the staging comes out of L2.
#ifndef GF_NBH_MAX_ROUNDS
#define GF_NBH_MAX_ROUNDS 2
#endif
inline int vertices_per_group(int nV, int slots) {
    int rounds = nV / (slots * 256);
    rounds = rounds < 1 ? 1 : rounds > GF_NBH_MAX_ROUNDS ? GF_NBH_MAX_ROUNDS : rounds;
    return slots * rounds;
}

// rounds = 0: vertices_per_group; > 0: that many rounds of a workgroup's slots.
inline int group_vertices(int nV, int slots, int rounds) { return rounds > 0 ? slots * rounds : vertices_per_group(nV, slots); }

// the one place the run-time (channels per lane, aggregate) picks an instantiation: f(channels per lane, pairs) as integral constants
template <typename F>
gf_status with_instantiation(int H, bool pairs, F &&f) {
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    if (H > 64) return pairs ? f(two{}, std::true_type{}) : f(two{}, std::false_type{});
    return pairs ? f(one{}, std::true_type{}) : f(one{}, std::false_type{});
}

}  // namespace

// The three launches of a level on `nsets` operand sets (1 or 2): grid.y = nsets, one set is given to the kernel twice.  The level below,
// the gated and the distance level and the stand-alone operators at the end of the file share them.
gf_status smp_neighbourhood_fwd(gf_ctx *ctx, bool pairs, int H, int nV, int rounds, const gf_nbh_fwd_set *sets, int nsets, const long long *ptr,
                                const int *idx) {
    const gf_nbh_fwd_set &s0 = sets[0], &s1 = sets[nsets - 1];
    const int G = smp_neighbourhood_group_width(H), vpg = group_vertices(nV, kBlock / G, rounds);
    const size_t bytes = smp_neighbourhood_lds_bytes(H, s1.FD > s0.FD ? s1.FD : s0.FD);   // (the wider operand; level 0 leaves W2's part unused: one grant per kernel)
    return with_instantiation(H, pairs, [&](auto nk, auto pr) -> gf_status {
        constexpr int NK = decltype(nk)::value;
        constexpr bool PAIRS = decltype(pr)::value;
        const gf_status st = opt_in_lds(ctx, nbh_level_fwd<NK, PAIRS>, bytes);
        if (st != GF_OK) return st;
        GF_LAUNCH(ctx, "nbh_level_fwd", (nbh_level_fwd<NK, PAIRS>), dim3((unsigned)((nV + vpg - 1) / vpg), (unsigned)nsets), dim3(kBlock), bytes, s0,
                  s1, ptr, idx, nV, H, G, vpg);
        return GF_OK;
    });
}

gf_status smp_neighbourhood_node(gf_ctx *ctx, bool pairs, int H, int nV, int rounds, const gf_nbh_node_set *sets, int nsets, const float *dy,
                                 const int *vmol) {
    const gf_nbh_node_set &s0 = sets[0], &s1 = sets[nsets - 1];
    const int G = smp_neighbourhood_group_width(H), slots = kBlock / G, vpg = group_vertices(nV, slots, rounds);
    const size_t bytes = sizeof(float) * ((s0.W2 ? (size_t)H * H : 0) + (size_t)slots * H);
    return with_instantiation(H, pairs, [&](auto nk, auto pr) -> gf_status {
        constexpr int NK = decltype(nk)::value;
        constexpr bool PAIRS = decltype(pr)::value;
        const gf_status st = opt_in_lds(ctx, nbh_node_bwd<NK, PAIRS>, bytes);
        if (st != GF_OK) return st;
        GF_LAUNCH(ctx, "nbh_node_bwd", (nbh_node_bwd<NK, PAIRS>), dim3((unsigned)((nV + vpg - 1) / vpg), (unsigned)nsets), dim3(kBlock), bytes, s0,
                  s1, dy, vmol, nV, H, G, vpg);
        return GF_OK;
    });
}

gf_status smp_neighbourhood_gather(gf_ctx *ctx, bool pairs, int H, int nV, const long long *tptr, const int *tidx, const gf_nbh_gather_set *sets,
                                   int nsets) {
    const gf_nbh_gather_set &s0 = sets[0], &s1 = sets[nsets - 1];
    const int G = smp_neighbourhood_group_width(H), slots = kBlock / G;
    return with_instantiation(H, pairs, [&](auto nk, auto pr) -> gf_status {
        constexpr int NK = decltype(nk)::value;
        constexpr bool PAIRS = decltype(pr)::value;
        GF_LAUNCH(ctx, "nbh_gather_bwd", (nbh_gather_bwd<NK, PAIRS>), dim3((unsigned)((nV + slots - 1) / slots), (unsigned)nsets), dim3(kBlock), 0,
                  tptr, tidx, s0, s1, nV, H, G);
        return GF_OK;
    });
}

namespace {

gf_status level(gf_smp *s, int l, const float *W1, const float *W2, bool forward, bool top = false, const float *Wout = nullptr) {
    gf_ctx *ctx = s->ctx;
    const int H = s->cfg.nChanels, nV = s->lay.level[0].nNodes;
    const bool pairs = s->cfg.neighbourhood == 3;
    gf_smp::DevLevel &d = s->lv[l];
    const gf_smp::DevLevel *pv = l ? &s->lv[l - 1] : nullptr;
    const bool third = l && s->cfg.third_order();   // GCN_3D: n_l is smp_level_third.hip's, handed on as a sum of one term over N(v) = {v}
    if (forward) {
        gf_nbh_fwd_set set = {s->cfg.fdim(), W1, s->x, W2, /*hprev=*/pv ? pv->f : nullptr, /*Tprev=*/pv ? pv->nb_T : nullptr,
                              /*h=*/d.f, /*n=*/d.th_A, /*A=*/d.th_B, /*T=*/d.nb_T, /*Tt=*/d.nb_Tt};
        if (!third) return smp_neighbourhood_fwd(ctx, pairs, H, nV, 0, &set, 1, d.nb_ptr, d.nb_idx);
        const gf_status pooled = smp_third_pool_fwd_launch(ctx, H, nV, d.nb_max_members, pv->f, d.nb_ptr, d.nb_idx, d.nb_pool, d.nb_sel);
        if (pooled != GF_OK) return pooled;
        set.hprev = d.nb_pool, set.Tprev = nullptr;
        return smp_neighbourhood_fwd(ctx, pairs, H, nV, 0, &set, 1, s->nb_id_ptr, s->nb_id_idx);
    }
    const gf_nbh_node_set node = {W2, /*h=*/d.f, /*dh=*/d.df, Wout, /*A=*/d.th_B, /*Tt=*/d.nb_Tt, /*dn=*/d.Q, /*gTt=*/d.th_node, /*sA=*/d.nb_sA};
    const gf_status st = smp_neighbourhood_node(ctx, pairs, H, nV, 0, &node, 1, top ? s->dy : nullptr, s->top_node_mol);
    if (st != GF_OK || !l) return st;
    if (third) return smp_third_pool_bwd_launch(ctx, H, nV, d.nb_ptr, d.nb_idx, d.nb_tptr, d.nb_tidx, pv->f, d.nb_sel, d.Q, pv->df);
    const gf_nbh_gather_set gat = {/*dn=*/d.Q, /*gTt=*/d.th_node, /*sA=*/d.nb_sA, /*hprev=*/pv->f, /*Tprev=*/pv->nb_T, /*dhprev=*/pv->df};
    return smp_neighbourhood_gather(ctx, pairs, H, nV, d.nb_tptr, d.nb_tidx, &gat, 1);
}

}  // namespace

gf_status smp_neighbourhood_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, nMol = s->lay.nMol;
    const View<const float> p(s->cfg, params);
    for (int l = 0; l <= L; ++l) {
        const gf_status st = level(s, l, p.W1[l], p.W2[l], /*forward=*/true);
        if (st != GF_OK) return st;
    }
    const bool has_targets = targets != nullptr || s->cfg.readout == 2;   // (a Gram handle's target is the batch itself)
    if (s->cfg.readout) {   // GCN_*D_Kernel, GCA_1D: the pair and the Gram read-out (smp_level_readouts.hip), which copy out what they have
        const gf_status st = smp_readout_forward(s, p.W, targets, predict, loss, graph_feature);
        return st == GF_OK ? finish_forward(s, has_targets, nullptr, nullptr, 0) : st;
    }
    GF_LAUNCH(ctx, "nbh_readout", nbh_readout, dim3(nMol), dim3(64), 0, s->lv[L].f, s->mol_ptr, p.W, targets, s->g, s->yhat, loss, s->dy, H);
    return finish_forward(s, has_targets, predict, graph_feature, H);
}

// The reverse sweep from the loss of the last forward; every level keeps what a second sweep needs (dz is rebuilt from dy downwards).
gf_status smp_neighbourhood_backward(gf_smp *s, const float *params, float *grads, int accumulate) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, FD = s->cfg.fdim(), nMol = s->lay.nMol, nV = s->lay.level[0].nNodes;
    const View<const float> p(s->cfg, params);
    const View<float> d(s->cfg, grads);
    if (!accumulate) GF_HIP_TRY(ctx, hipMemsetAsync(grads, 0, sizeof(float) * param_count(s->cfg), ctx->stream));
    const bool own_readout = s->cfg.readout != 0;   // (smp_level_readouts.hip: its reverse leaves dh_L in lv[L].df, the top level is then a level like the others)
    const gf_status wst = own_readout ? smp_readout_dW(s, p.W, d.W) : smp_vertex_readout_dW(ctx, "nbh_readout_dW", H, nMol, s->dy, s->g, d.W);
    if (wst != GF_OK) return wst;
    for (int l = L; l >= 0; --l) {
        gf_status st = level(s, l, nullptr, p.W2[l], /*forward=*/false, /*top=*/l == L && !own_readout, p.W);   // dz_l in lv[l].df, dh_{l-1} in lv[l - 1].df
        // dW1_l [H][F'] += dz^T X,  dW2_l [H][H] += dz^T N: tall-skinny TN products over the vertices of the batch
        if (st == GF_OK) st = gemm(ctx, true, false, H, FD, nV, s->lv[l].df, H, 0, s->x, FD, 0, d.W1[l], FD, 0, 1, 1);
        if (st == GF_OK && l) st = gemm(ctx, true, false, H, H, nV, s->lv[l].df, H, 0, s->lv[l].th_A, H, 0, d.W2[l], H, 0, 1, 1);
        if (st != GF_OK) return st;
    }
    mark_used(s);
    return GF_OK;
}

}  // namespace gf

// ---- the level's kernels as stand-alone operators (include/gf_hip.h; tests/test_smp_neighbourhood_ops_gpu.py), on one operand set built
// from positional arguments or on the caller's two (a level of a distance handle): one validation and one launcher for both ----
namespace {

// a refusal of operand set c of a two-set call, or of the one set of a one-set call (c = -1)
gf_status refuse(gf_ctx *ctx, const char *who, const char *what, int c) {
    return c < 0 ? gf::fail(ctx, GF_ERR_INVALID, "%s: %s", who, what) : gf::fail(ctx, GF_ERR_INVALID, "%s: %s (set %d)", who, what, c);
}

gf_status check_fwd_set(gf_ctx *ctx, const char *who, int pairs, int H, const gf_nbh_fwd_set &o, const long long *ptr, const int *idx, int c) {
    if (o.FD < 1 || !o.W1 || !o.x || !o.h) return refuse(ctx, who, "bad argument", c);
    if (o.W2 && (!o.hprev || !ptr || !idx || !o.n)) return refuse(ctx, who, "a level with W2 needs hprev, ptr, idx and n", c);
    if (pairs && (!o.T || (o.W2 && (!o.Tprev || !o.A || !o.Tt)))) return refuse(ctx, who, "the pair form needs T, and with W2 Tprev, A and Tt", c);
    if (gf::smp_neighbourhood_lds_bytes(H, o.FD) > 160 * 1024)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: H = %d, F' = %d need %zu bytes of LDS (160 KiB)", who, H, o.FD, gf::smp_neighbourhood_lds_bytes(H, o.FD));
    return GF_OK;
}
gf_status check_node_set(gf_ctx *ctx, const char *who, int pairs, const gf_nbh_node_set &o, const float *dy, const int *vmol, int nMol, int c) {
    if (!o.h || !o.dh) return refuse(ctx, who, "bad argument", c);
    if (dy && (!o.Wout || !vmol || nMol < 1)) return refuse(ctx, who, "the top level needs Wout, vmol and nMol >= 1", c);
    if (o.W2 && (!o.dn || (pairs && (!o.A || !o.Tt || !o.gTt || !o.sA)))) return refuse(ctx, who, "a level with W2 needs dn, the pair form A, Tt, gTt, sA", c);
    return GF_OK;
}
gf_status check_gather_set(gf_ctx *ctx, const char *who, int pairs, const gf_nbh_gather_set &o, int c) {
    if (!o.dn || !o.dhprev) return refuse(ctx, who, "bad argument", c);
    if (pairs && (!o.gTt || !o.sA || !o.hprev || !o.Tprev)) return refuse(ctx, who, "the pair form needs gTt, sA, hprev and Tprev", c);
    return GF_OK;
}

// what the one-set and the two-set entry of a kernel share, from the shape to the launch (W2 is in both sets of two or in neither)
gf_status fwd_op(gf_ctx *ctx, const char *who, int pairs, int H, int nV, int rounds, const gf_nbh_fwd_set *sets, int nsets, const long long *ptr,
                 const int *idx) {
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kNeighbourhoodMaxChanels, nV, rounds);
    if (st != GF_OK) return st;
    if (!sets) return refuse(ctx, who, "bad argument", -1);
    if ((sets[0].W2 != nullptr) != (sets[nsets - 1].W2 != nullptr)) return refuse(ctx, who, "W2 in one set only", -1);
    for (int c = 0; c < nsets && st == GF_OK; ++c) st = check_fwd_set(ctx, who, pairs, H, sets[c], ptr, idx, nsets > 1 ? c : -1);
    if (st != GF_OK) return st;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (sets[0].W2) st = gf::check_list(ctx, who, "ptr", ptr, idx, nV, nV);
    if (st != GF_OK) return st;
    return gf::smp_neighbourhood_fwd(ctx, pairs != 0, H, nV, rounds, sets, nsets, ptr, idx);
}

gf_status node_op(gf_ctx *ctx, const char *who, int pairs, int H, int nV, int rounds, const gf_nbh_node_set *sets, int nsets, const float *dy,
                  const int *vmol, int nMol) {
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kNeighbourhoodMaxChanels, nV, rounds);
    if (st != GF_OK) return st;
    if (!sets) return refuse(ctx, who, "bad argument", -1);
    if ((sets[0].W2 != nullptr) != (sets[nsets - 1].W2 != nullptr)) return refuse(ctx, who, "W2 in one set only", -1);
    for (int c = 0; c < nsets && st == GF_OK; ++c) st = check_node_set(ctx, who, pairs, sets[c], dy, vmol, nMol, nsets > 1 ? c : -1);
    if (st != GF_OK) return st;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (dy) st = gf::check_members(ctx, who, "vmol", vmol, (size_t)nV, nMol);
    if (st != GF_OK) return st;
    return gf::smp_neighbourhood_node(ctx, pairs != 0, H, nV, rounds, sets, nsets, dy, vmol);
}

gf_status gather_op(gf_ctx *ctx, const char *who, int pairs, int H, int nV, const long long *tptr, const int *tidx, const gf_nbh_gather_set *sets,
                    int nsets) {
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kNeighbourhoodMaxChanels, nV, 0);
    if (st != GF_OK) return st;
    if (!tptr || !tidx || !sets) return refuse(ctx, who, "bad argument", -1);
    for (int c = 0; c < nsets && st == GF_OK; ++c) st = check_gather_set(ctx, who, pairs, sets[c], nsets > 1 ? c : -1);
    if (st != GF_OK) return st;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = gf::check_list(ctx, who, "tptr", tptr, tidx, nV, nV);
    if (st != GF_OK) return st;
    return gf::smp_neighbourhood_gather(ctx, pairs != 0, H, nV, tptr, tidx, sets, nsets);
}

}  // namespace

extern "C" {

gf_status gf_smp_neighbourhood_fwd_ex_f32(gf_ctx *ctx, int pairs, int H, int FD, int nV, int rounds, const float *W1, const float *x, const float *W2,
                                          const float *hprev, const float *Tprev, const long long *ptr, const int *idx, float *h, float *n, float *A,
                                          float *T, float *Tt) {
    const gf_nbh_fwd_set set = {FD, W1, x, W2, hprev, Tprev, h, n, A, T, Tt};
    return fwd_op(ctx, "gf_smp_neighbourhood_fwd_ex_f32", pairs, H, nV, rounds, &set, 1, ptr, idx);
}
gf_status gf_smp_neighbourhood_fwd2_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const gf_nbh_fwd_set *sets, const long long *ptr,
                                           const int *idx) {
    return fwd_op(ctx, "gf_smp_neighbourhood_fwd2_ex_f32", pairs, H, nV, rounds, sets, 2, ptr, idx);
}

gf_status gf_smp_neighbourhood_node_bwd_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const float *W2, const float *h, float *dh,
                                               const float *dy, const float *Wout, const int *vmol, int nMol, const float *A, const float *Tt,
                                               float *dn, float *gTt, float *sA) {
    const gf_nbh_node_set set = {W2, h, dh, Wout, A, Tt, dn, gTt, sA};
    return node_op(ctx, "gf_smp_neighbourhood_node_bwd_ex_f32", pairs, H, nV, rounds, &set, 1, dy, vmol, nMol);
}
gf_status gf_smp_neighbourhood_node_bwd2_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const gf_nbh_node_set *sets, const float *dy,
                                                const int *vmol, int nMol) {
    return node_op(ctx, "gf_smp_neighbourhood_node_bwd2_ex_f32", pairs, H, nV, rounds, sets, 2, dy, vmol, nMol);
}

gf_status gf_smp_neighbourhood_gather_bwd_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, const long long *tptr, const int *tidx, const float *dn,
                                                 const float *gTt, const float *sA, const float *hprev, const float *Tprev, float *dhprev) {
    const gf_nbh_gather_set set = {dn, gTt, sA, hprev, Tprev, dhprev};
    return gather_op(ctx, "gf_smp_neighbourhood_gather_bwd_ex_f32", pairs, H, nV, tptr, tidx, &set, 1);
}
gf_status gf_smp_neighbourhood_gather_bwd2_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, const long long *tptr, const int *tidx,
                                                  const gf_nbh_gather_set *sets) {
    return gather_op(ctx, "gf_smp_neighbourhood_gather_bwd2_ex_f32", pairs, H, nV, tptr, tidx, sets, 2);
}

gf_status gf_smp_neighbourhood_readout_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, const float *hL, const int *mol_ptr, const float *W,
                                              const float *target, float *g, float *yhat, float *loss, float *dy, float *dW) {
    static const char *who = "gf_smp_neighbourhood_readout_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kNeighbourhoodMaxChanels, nV, 0);
    if (st != GF_OK) return st;
    if (nMol < 1 || !hL || !mol_ptr || !W || !g || !yhat || !dy || !dW) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = gf::check_ptr(ctx, who, "mol_ptr", mol_ptr, nMol, nV);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "nbh_readout", gf::nbh_readout, dim3(nMol), dim3(64), 0, hL, mol_ptr, W, target, g, yhat, loss, dy, H);
    return gf::smp_vertex_readout_dW(ctx, "nbh_readout_dW", H, nMol, dy, g, dW);
}

}  // extern "C"
