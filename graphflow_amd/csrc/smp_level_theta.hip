// smp_level_theta.hip -- the first-order level of SMP_theta / SMP_theta_physics / SMP_theta_pairgraphs (GraphFlow/SMP_theta.h:573-613).
//
// Node v with field phi_l(v) = (x_1 .. x_s); its children are the vertices w at hop distance <= 1 (NOT the members of the field, :577-583),
// pi_w(i) = the position of x_i in phi_{l-1}(w) or none.  f_l[v] is a MATRIX [s][Cc]:
//   S[i]   = sum over the children of f_{l-1}[w][pi_w(i)]                       (X[v][w] f_{l-1}[w], SumMatrices; :579-586)
//   z[i]   = lambda1_s S[i] K_top + lambda2_s (sum_i' S[i']) K_bot + b_s        (ScalarMatMul eye / one, MatrixConcat, MatMul K; :590-609)
//   f_l[i] = LeakyReLU(z[i])
// with K_l = [K_top; K_bot] ([2 Cp][Cc], Cp = C_{l-1}, Cc = C_l: equal for SMP_theta, halving in a tower) and lambda1, lambda2, b PER FIELD
// SIZE s.  K acts on the channel axis only, so it commutes with the gathers: with G = f_{l-1} [K_top | K_bot] -- one GEMM over the rows of
// level l - 1, [rows_{l-1}][2 Cc] --
//   A[i] = sum_w G_top[w][pi_w(i)],   B = sum_i sum_w G_bot[w][pi_w(i)],   z[i] = lambda1_s A[i] + lambda2_s B + b_s.
// A ([rows][Cc]) and B ([nodes][Cc]) are kept: they are what dlambda1 / dlambda2 need.  Backward, dz = df_l * lrelu'(z), dzs = sum_i dz[i]:
//   db_s = sum dz,  dlambda1_s = sum k_v dz . A,  dlambda2_s = sum k_v dzs . B   over the nodes of size s (contiguous: nodes are numbered by size)
//   (k_v: the reference hands a vertex's gradient to lambda_s once per appearance of the shared ScalarMatMul ops in its graph -- the j-th
//    vertex of size s of a molecule counts j times, gfsmp::LevelLayout::th_weight; the parity target is the class, not the calculus)
//   dG_top[w][j] = sum over the consumers v of w, i = the position of phi_{l-1}(w)[j] in phi_l(v), of lambda1_{s_v} dz_v[i]
//   dG_bot[w][j] = the same sum of lambda2_{s_v} dzs_v                         (nothing from a consumer whose field misses the vertex)
//   dK_l = f_{l-1}^T dG,   df_{l-1} = dG [K_top | K_bot]^T
// -- again products on the rows of level l - 1.  A field holds 1 - 30 positions of a few channels, so the two gathers pack runs of consecutive
// nodes into a workgroup (about 256 (position, channel vector) items, offsets from a wave scan in LDS), the vector 4 / 2 / 1 floats as Cc
// allows.  Every sum runs in a fixed order (positions, children, consumers ascending; the segment reductions fold fixed trees), the GEMMs
// are the deterministic ones of mixers.hip: two runs give the same bits, no atomics.  Every output element is written by its kernel.
#include "smp_first_order.h"

namespace gf {
using namespace first_order;
namespace {

constexpr float kThetaAlpha = 0.01f;   // LeakyReLU2D.h:31, LeakyReLU.h default

__device__ __forceinline__ float lrelu(float z) { return z > 0.f ? z : kThetaAlpha * z; }
// Forward: nodes [blockIdx.x * npw, + npw); items (node j, position i, vector q) over sum_j s_j * Cc / V.  G rows are 2 Cc floats.
template <int V>
__global__ __launch_bounds__(256) void theta_level_fwd(const float *__restrict__ G, const float *__restrict__ sizes, float *__restrict__ f,
                                                       float *__restrict__ A, float *__restrict__ B, const int *__restrict__ node_s,
                                                       const long long *__restrict__ node_row, const long long *__restrict__ child_ptr,
                                                       const long long *__restrict__ src_row, const long long *__restrict__ pi_off,
                                                       const short *__restrict__ pi, int Cc, int nodes, int npw) {
    __shared__ int off[kThetaMaxPack + 1];
    const int nb = blockIdx.x * npw;
    const int np = nodes - nb < npw ? nodes - nb : npw, Qc = Cc / V, C2 = 2 * Cc;
    int cnt = 0;
    if ((int)threadIdx.x < np) cnt = node_s[nb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int j = pack_find(off, np, it);
        const int n = nb + j, s = node_s[n];
        const int r = it - off[j], i = r / Qc, q = r - i * Qc, cq = q * V;
        const long long e0 = child_ptr[n], e1 = child_ptr[n + 1];
        Vf<V> a = vzero<V>(), b = vzero<V>();
        for (long long e = e0; e < e1; ++e) {
            const int p = pi[pi_off[e] + i];
            if (p >= 0) vadd(a, vld<V>(G + (src_row[e] + p) * C2 + cq));
        }
        for (int i2 = 0; i2 < s; ++i2) {
            Vf<V> t = vzero<V>();
            for (long long e = e0; e < e1; ++e) {
                const int p = pi[pi_off[e] + i2];
                if (p >= 0) vadd(t, vld<V>(G + (src_row[e] + p) * C2 + Cc + cq));
            }
            vadd(b, t);
        }
        const float *se = size_entry(sizes, s, Cc);
        const float l1 = se[0], l2 = se[1];
        Vf<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = lrelu((l1 * a.v[k] + l2 * b.v[k]) + se[2 + cq + k]);
        const long long row = node_row[n] + i;
        vst<V>(f + row * Cc + cq, o);
        vst<V>(A + row * Cc + cq, a);
        if (i == 0) vst<V>(B + (long long)n * Cc + cq, b);
    }
}

// Reverse, per node: one item per (node, vector q).  dz[i] = (df_l[i] (has_df) + dvec[n] (optional: the read-out's gradient, one vector
// per node)) * lrelu'(f_l[i]) is left in df; acc[n] = [ sum_i dz[i] | k_n sum_i dz[i] A[i] | k_n (sum_i dz[i]) B[n] ]  ([nodes][3 Cc]),
// k_n = weight[n] (th_weight).
template <int V>
__global__ __launch_bounds__(256) void theta_node_bwd(const float *__restrict__ f, float *__restrict__ df, const float *__restrict__ dvec,
                                                      const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ acc,
                                                      const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                      const int *__restrict__ weight, int Cc, int nodes, int has_df) {
    const int Qc = Cc / V;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nodes * Qc) return;
    const int n = (int)(t / Qc), cq = (int)(t - (long long)n * Qc) * V;
    const int s = node_s[n];
    const long long r0 = node_row[n];
    Vf<V> dv = vzero<V>(), zs = vzero<V>(), pa = vzero<V>();
    if (dvec) dv = vld<V>(dvec + (long long)n * Cc + cq);
    for (int i = 0; i < s; ++i) {
        const long long o = (r0 + i) * Cc + cq;
        const Vf<V> fv = vld<V>(f + o), av = vld<V>(A + o);
        Vf<V> d = dv;
        if (has_df) vadd(d, vld<V>(df + o));
#pragma unroll
        for (int k = 0; k < V; ++k) {
            d.v[k] *= fv.v[k] > 0.f ? 1.f : kThetaAlpha;
            zs.v[k] += d.v[k];
            pa.v[k] += d.v[k] * av.v[k];
        }
        vst<V>(df + o, d);
    }
    const Vf<V> bv = vld<V>(B + (long long)n * Cc + cq);
    const float kn = (float)weight[n];
    Vf<V> pb;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        pa.v[k] *= kn;
        pb.v[k] = kn * (zs.v[k] * bv.v[k]);
    }
    float *a = acc + (long long)n * 3 * Cc + cq;
    vst<V>(a, zs);
    vst<V>(a + Cc, pa);
    vst<V>(a + 2 * Cc, pb);
}

// The per-size gradients: one workgroup per size bucket (s, first node, count) -- the bucket's nodes are contiguous.  Thread (rr, c) sums
// the nodes rr, rr + rl, .. of channel c, the rl partials are folded in order, the lambda partials through one fixed tree.  `+=` into dsizes.
__global__ __launch_bounds__(256) void theta_size_grads(const float *__restrict__ acc, const int *__restrict__ bucket, float *__restrict__ dsizes,
                                                        int Cc) {
    __shared__ float red[256];
    const int s = bucket[3 * blockIdx.x], n0 = bucket[3 * blockIdx.x + 1], cnt = bucket[3 * blockIdx.x + 2];
    float *out = dsizes + (size_t)(s - 1) * (2 + Cc);
    const int lanes = Cc < 256 ? Cc : 256, rl = 256 / lanes;
    const int f0 = threadIdx.x % lanes, rr = threadIdx.x / lanes;
    float l1 = 0.f, l2 = 0.f;
    for (int fb = 0; fb < Cc; fb += lanes) {
        const int c = fb + f0;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (c < Cc && rr < rl)
            for (int n = n0 + rr; n < n0 + cnt; n += rl) {
                const float *a = acc + (size_t)n * 3 * Cc + c;
                a0 += a[0];
                a1 += a[Cc];
                a2 += a[2 * Cc];
            }
        l1 += a1;
        l2 += a2;
        red[threadIdx.x] = a0;
        __syncthreads();
        if (rr == 0 && c < Cc) {
            float t = 0.f;
            for (int k = 0; k < rl; ++k) t += red[k * lanes + f0];
            out[2 + c] += t;
        }
        __syncthreads();
    }
    for (int pass = 0; pass < 2; ++pass) {
        red[threadIdx.x] = pass ? l2 : l1;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[pass] += red[0];
        __syncthreads();
    }
}

// Reverse gather: source nodes [blockIdx.x * npw, + npw) of level l - 1; items (node j, position p, vector q) over sum_j s_j Cc / V.
// dz rows are Cc floats, acc rows 3 Cc (the first Cc: sum_i dz[i]), dG rows 2 Cc.
template <int V>
__global__ __launch_bounds__(256) void theta_gather_bwd(const float *__restrict__ dz, const float *__restrict__ acc, const float *__restrict__ sizes,
                                                        float *__restrict__ dG, const int *__restrict__ prev_s, const long long *__restrict__ prev_row,
                                                        const long long *__restrict__ cons_ptr, const long long *__restrict__ cons_row,
                                                        const int *__restrict__ cons_s, const int *__restrict__ cons_node,
                                                        const long long *__restrict__ inv_off, const short *__restrict__ inv, int Cc, int nodes,
                                                        int npw) {
    __shared__ int off[kThetaMaxPack + 1];
    const int wb = blockIdx.x * npw;
    const int np = nodes - wb < npw ? nodes - wb : npw, Qc = Cc / V;
    int cnt = 0;
    if ((int)threadIdx.x < np) cnt = prev_s[wb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int j = pack_find(off, np, it);
        const int w = wb + j;
        const int r = it - off[j], p = r / Qc, q = r - p * Qc, cq = q * V;
        Vf<V> gt = vzero<V>(), gb = vzero<V>();
        for (long long c = cons_ptr[w]; c < cons_ptr[w + 1]; ++c) {
            const int i = inv[inv_off[c] + p];
            if (i < 0) continue;
            const float *se = size_entry(sizes, cons_s[c], Cc);
            const float l1 = se[0], l2 = se[1];
            const Vf<V> z = vld<V>(dz + (cons_row[c] + i) * Cc + cq), zs = vld<V>(acc + (long long)cons_node[c] * 3 * Cc + cq);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                gt.v[k] += l1 * z.v[k];
                gb.v[k] += l2 * zs.v[k];
            }
        }
        float *o = dG + (prev_row[w] + p) * 2 * (long long)Cc + cq;
        vst<V>(o, gt);
        vst<V>(o + Cc, gb);
    }
}

// K [2Cp][Cc] (rows k Cp + ci) -> Kh [Cp][2Cc] (Kh[ci][k Cc + co] = K[k Cp + ci][co]) and Kt [2Cc][Cp] (Kt[k Cc + co][ci] = K[k Cp + ci][co])
__global__ void theta_weight_views(const float *__restrict__ K, float *__restrict__ Kh, float *__restrict__ Kt, int Cp, int Cc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * Cp * Cc) return;
    const int k = i / (Cp * Cc), r = i - k * Cp * Cc, ci = r / Cc, co = r - ci * Cc;
    const float v = K[i];
    Kh[(size_t)ci * 2 * Cc + k * Cc + co] = v;
    Kt[((size_t)k * Cc + co) * Cp + ci] = v;
}
// dK [2Cp][Cc] += dKh [Cp][2Cc] rearranged; one thread per element of dK
__global__ void theta_wgrad_fold(const float *__restrict__ dKh, float *__restrict__ dK, int Cp, int Cc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * Cp * Cc) return;
    const int k = i / (Cp * Cc), r = i - k * Cp * Cc, ci = r / Cc, co = r - ci * Cc;
    dK[i] += dKh[(size_t)ci * 2 * Cc + k * Cc + co];
}

// read-out of a level: sh[n][:] = sum over the node's s rows of f_l (ShrinkMatrix(f, 0), ShrinkMatrix.h:43-50), vf = LeakyReLU(sh)
__global__ void theta_readout_nodes(const float *__restrict__ f, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                    float *__restrict__ sh, float *__restrict__ vf, int C, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t n = i / C;
        const int s = node_s[n];
        const float *src = f + node_row[n] * C + c;
        float acc = 0.f;
        for (int r = 0; r < s; ++r) acc += src[(size_t)r * C];
        sh[i] = acc;
        vf[i] = lrelu(acc);
    }
}
// its reverse: df_l[n][r][:] (+)= dvec[n][:] at every row of the node (ShrinkMatrix::backward broadcasts)
__global__ void theta_readout_bwd(const float *__restrict__ dvec, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                  float *__restrict__ df, int C, size_t total, int accumulate) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t n = i / C;
        const int s = node_s[n];
        float *dst = df + node_row[n] * C + c;
        const float v = dvec[i];
        for (int r = 0; r < s; ++r) dst[(size_t)r * C] = accumulate ? dst[(size_t)r * C] + v : v;
    }
}

}  // namespace

// G = f_{l-1} [K_top | K_bot] into the level's Q buffer, then the gather with the per-size factors, bias and LeakyReLU into f_l
gf_status smp_theta_forward_level(gf_smp *s, int l, const float *Kl, const float *sizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);   // (equal unless a tower)
    const long long rows_p = s->lay.level[l - 1].rows, rows = s->lay.level[l].rows;
    const int nodes = s->lay.level[l].nNodes;
    float *Kh = d.Wst, *Kt = d.Wst + (size_t)2 * Cp * Cc;
    GF_LAUNCH(ctx, "smpt_weight_views", theta_weight_views, dim3((2 * Cp * Cc + 255) / 256), dim3(256), 0, Kl, Kh, Kt, Cp, Cc);
    gf_status st = gemm(ctx, false, false, (int)rows_p, 2 * Cc, Cp, pv.f, Cp, 0, Kh, 2 * Cc, 0, d.Q, 2 * Cc, 0, 1, 0);
    if (st != GF_OK || nodes == 0) return st;
    const int npw = theta_pack((double)rows / (double)nodes * (Cc / theta_vec(Cc)));
    const dim3 grid((unsigned)((nodes + npw - 1) / npw));
#define GF_THETA_FWD(V) GF_LAUNCH(ctx, "smpt_level_fwd", theta_level_fwd<V>, grid, dim3(256), 0, d.Q, sizes, d.f, d.th_A, d.th_B, d.node_s, d.node_row, \
                                  d.th_child_ptr, d.th_src_row, d.th_pi_off, d.th_pi, Cc, nodes, npw)
    switch (theta_vec(Cc)) {
        case 4: GF_THETA_FWD(4); break;
        case 2: GF_THETA_FWD(2); break;
        default: GF_THETA_FWD(1); break;
    }
#undef GF_THETA_FWD
    return GF_OK;
}

// node_df: the read-out's gradient as one vector per node ([nodes][Cc]) or null; rows_too: d.df holds a gradient per row as well (what
// the level above sent down).  The weight gradients are final before df_{l-1} is formed; *wgrad_done is called in between.
gf_status smp_theta_backward_level(gf_smp *s, int l, const float *Kl, const float *sizes, float *dKl, float *dsizes, const float *node_df,
                                   bool rows_too, gf_status (*wgrad_done)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);
    const long long rows_p = s->lay.level[l - 1].rows;
    const int nodes = s->lay.level[l].nNodes, np = s->lay.level[l - 1].nNodes, V = theta_vec(Cc);
    const int nbuckets = (int)(s->lay.level[l].th_bucket.size() / 3);
    if (!node_df && !rows_too) return fail(ctx, GF_ERR_INVALID, "first-order level %d: no gradient to back-propagate", l);
    // (the views again: this sweep's parameters need not be the forward's)
    GF_LAUNCH(ctx, "smpt_weight_views", theta_weight_views, dim3((2 * Cp * Cc + 255) / 256), dim3(256), 0, Kl, d.Wst, d.Wst + (size_t)2 * Cp * Cc, Cp, Cc);
    if (nodes > 0) {
        const dim3 grid(grid_for((size_t)nodes * (Cc / V)));
#define GF_THETA_NODE(V) GF_LAUNCH(ctx, "smpt_node_bwd", theta_node_bwd<V>, grid, dim3(256), 0, d.f, d.df, node_df, d.th_A, d.th_B, d.th_node, d.node_s, \
                                   d.node_row, d.th_weight, Cc, nodes, rows_too ? 1 : 0)
        switch (V) {
            case 4: GF_THETA_NODE(4); break;
            case 2: GF_THETA_NODE(2); break;
            default: GF_THETA_NODE(1); break;
        }
#undef GF_THETA_NODE
        GF_LAUNCH(ctx, "smpt_size_grads", theta_size_grads, dim3(nbuckets), dim3(256), 0, d.th_node, d.th_bucket, dsizes, Cc);
    }
    if (np > 0) {
        const int npw = theta_pack((double)rows_p / (double)np * (Cc / V));
        const dim3 grid((unsigned)((np + npw - 1) / npw));
#define GF_THETA_BWD(V) GF_LAUNCH(ctx, "smpt_gather_bwd", theta_gather_bwd<V>, grid, dim3(256), 0, d.df, d.th_node, sizes, d.Q, pv.node_s, pv.node_row, \
                                  d.th_cons_ptr, d.th_cons_row, d.th_cons_s, d.th_cons_node, d.th_inv_off, d.th_inv, Cc, np, npw)
        switch (V) {
            case 4: GF_THETA_BWD(4); break;
            case 2: GF_THETA_BWD(2); break;
            default: GF_THETA_BWD(1); break;
        }
#undef GF_THETA_BWD
    }
    gf_status st = gemm(ctx, true, false, Cp, 2 * Cc, (int)rows_p, pv.f, Cp, 0, d.Q, 2 * Cc, 0, d.dWst, 2 * Cc, 0, 1, 0);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "smpt_wgrad_fold", theta_wgrad_fold, dim3((2 * Cp * Cc + 255) / 256), dim3(256), 0, d.dWst, dKl, Cp, Cc);
    st = wgrad_done(s, l);
    if (st != GF_OK) return st;
    return gemm(ctx, false, false, (int)rows_p, Cp, 2 * Cc, d.Q, 2 * Cc, 0, d.Wst + (size_t)2 * Cp * Cc, Cp, 0, pv.df, Cp, 0, 1, 0);
}

// pieces the other first-order levels share (smp_level_1d.hip): the per-size reduction as it is, and the [2 Cp][Cc] matrix's two views
gf_status smp_theta_size_grads(gf_ctx *ctx, const float *acc, const int *bucket, int nbuckets, float *dsizes, int Cc) {
    GF_LAUNCH(ctx, "smpt_size_grads", theta_size_grads, dim3(nbuckets), dim3(256), 0, acc, bucket, dsizes, Cc);
    return GF_OK;
}
gf_status smp_theta_weight_views(gf_ctx *ctx, const float *K, float *Kh, float *Kt, int Cp, int Cc) {
    GF_LAUNCH(ctx, "smpt_weight_views", theta_weight_views, dim3((2 * Cp * Cc + 255) / 256), dim3(256), 0, K, Kh, Kt, Cp, Cc);
    return GF_OK;
}
gf_status smp_theta_wgrad_fold(gf_ctx *ctx, const float *dKh, float *dK, int Cp, int Cc) {
    GF_LAUNCH(ctx, "smpt_wgrad_fold", theta_wgrad_fold, dim3((2 * Cp * Cc + 255) / 256), dim3(256), 0, dKh, dK, Cp, Cc);
    return GF_OK;
}

gf_status smp_theta_readout(gf_smp *s, int l, float *sh, float *vf) {
    const gf_smp::DevLevel &d = s->lv[l];
    const size_t n = (size_t)s->lay.level[l].nNodes * s->cfg.level_channels(l);
    GF_LAUNCH(s->ctx, "smpt_readout_nodes", theta_readout_nodes, dim3(grid_for(n)), dim3(256), 0, d.f, d.node_s, d.node_row, sh, vf,
              s->cfg.level_channels(l), n);
    return GF_OK;
}

gf_status smp_theta_readout_backward(gf_smp *s, int l, const float *dvec, int accumulate) {
    const gf_smp::DevLevel &d = s->lv[l];
    const size_t n = (size_t)s->lay.level[l].nNodes * s->cfg.level_channels(l);
    GF_LAUNCH(s->ctx, "smpt_readout_bwd", theta_readout_bwd, dim3(grid_for(n)), dim3(256), 0, dvec, d.node_s, d.node_row, d.df,
              s->cfg.level_channels(l), n, accumulate);
    return GF_OK;
}

}  // namespace gf
