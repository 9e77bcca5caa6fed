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
#include "smp_field_level.h"

namespace gf {
using namespace field_level;
namespace {

constexpr float kThetaAlpha = 0.01f;   // LeakyReLU2D.h:31, LeakyReLU.h default

// Forward: nodes [blockIdx.x * npw, + npw); items (node j, position i, vector q) over sum_j s_j * Cc / V.  G rows are 2 Cc floats.
template <int V>
__global__ __launch_bounds__(256) void theta_level_fwd(const float *__restrict__ G, const float *__restrict__ sizes, float *__restrict__ f,
                                                       float *__restrict__ A, float *__restrict__ B, const int *__restrict__ node_s,
                                                       const long long *__restrict__ node_row, const long long *__restrict__ child_ptr,
                                                       const long long *__restrict__ src_row, const long long *__restrict__ pi_off,
                                                       const short *__restrict__ pi, int Cc, int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const Run run = pack_run(off, node_s, nodes, npw, Cc / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cc / V);
        const int n = run.nb + x.j, s = node_s[n], i = x.pos, cq = x.cq;
        const long long e0 = child_ptr[n], e1 = child_ptr[n + 1];
        const Vf<V> a = gather_row<V>(G, 2 * Cc, cq, e0, e1, src_row, pi_off, pi, i);
        Vf<V> b = vzero<V>();
        for (int i2 = 0; i2 < s; ++i2) vadd(b, gather_row<V>(G, 2 * Cc, Cc + cq, e0, e1, src_row, pi_off, pi, i2));
        const float *se = size_entry(sizes, s, Cc);
        const float l1 = se[0], l2 = se[1];
        Vf<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = lrelu((l1 * a.v[k] + l2 * b.v[k]) + se[2 + cq + k], kThetaAlpha);
        const long long row = node_row[n] + i;
        vst<V>(f + row * Cc + cq, o);
        vst<V>(A + row * Cc + cq, a);
        if (i == 0) vst<V>(B + (long long)n * Cc + cq, b);
    }
}

// Reverse, per node: one item per (node, vector q).  dz[i] = (df_l[i] (has_df) + dvec[n] (optional: the read-out's gradient, one vector
// per node)) * lrelu'(f_l[i]) is left in df; acc[n] = [ sum_i dz[i] | k_n sum_i dz[i] A[i] | k_n (sum_i dz[i]) B[n] ]  ([nodes][3 Cc]),
// k_n = weight[n] (th_weight).  (level1d_node_bwd at concat = 0 computes the same sums but contracts dz into them differently with a
// run-time slope: other bits, and 0.12 against 0.08 ms on the cfg3 batch -- NOTES.md)
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
        const Vf<V> av = vld<V>(A + o), d = dz_of<V>(f, df, o, dv, has_df, kThetaAlpha);
#pragma unroll
        for (int k = 0; k < V; ++k) {
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

}  // namespace

// G = f_{l-1} [K_top | K_bot] into the level's Q buffer, then the gather with the per-size factors, bias and LeakyReLU into f_l
gf_status smp_theta_forward_level(gf_smp *s, int l, const float *Kl, const float *sizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);   // (equal unless a tower)
    const long long rows_p = s->lay.level[l - 1].rows;
    const int nodes = s->lay.level[l].nNodes, V = lane_vector(Cc);
    float *Kh = d.Wst, *Kt = d.Wst + (size_t)2 * Cp * Cc;
    gf_status st = smp_field_weight_views(ctx, Kl, Kh, Kt, Cp, Cc);
    if (st == GF_OK) st = gemm(ctx, false, false, (int)rows_p, 2 * Cc, Cp, pv.f, Cp, 0, Kh, 2 * Cc, 0, d.Q, 2 * Cc, 0, 1, 0);
    if (st != GF_OK || nodes == 0) return st;
    const RunGrid g = run_grid(s->lay.level[l], false, Cc / V);
    return with_lane_vector(V, [&](auto v) -> gf_status {
        GF_LAUNCH(ctx, "smpt_level_fwd", theta_level_fwd<v>, g.grid, dim3(256), 0, d.Q, sizes, d.f, d.th_A, d.th_B, d.node_s, d.node_row,
                  d.th_child_ptr, d.th_src_row, d.th_pi_off, d.th_pi, Cc, nodes, g.npw);
        return GF_OK;
    });
}

// node_df: the read-out's gradient as one vector per node ([nodes][Cc]) or null; rows_too: d.df holds a gradient per row as well (what
// the level above sent down).  The weight gradients are final before df_{l-1} is formed; *wgrad_done is called in between.
gf_status smp_theta_backward_level(gf_smp *s, int l, const float *Kl, const float *sizes, float *dKl, float *dsizes, const float *node_df,
                                   bool rows_too, gf_status (*wgrad_done)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);
    const long long rows_p = s->lay.level[l - 1].rows;
    const int nodes = s->lay.level[l].nNodes, np = s->lay.level[l - 1].nNodes;
    const int nbuckets = (int)(s->lay.level[l].th_bucket.size() / 3);
    if (!node_df && !rows_too) return fail(ctx, GF_ERR_INVALID, "first-order level %d: no gradient to back-propagate", l);
    // (the views again: this sweep's parameters need not be the forward's)
    gf_status st = smp_field_weight_views(ctx, Kl, d.Wst, d.Wst + (size_t)2 * Cp * Cc, Cp, Cc);
    if (st == GF_OK && nodes > 0) {
        const int V = lane_vector(Cc);
        st = with_lane_vector(V, [&](auto v) -> gf_status {
            GF_LAUNCH(ctx, "smpt_node_bwd", theta_node_bwd<v>, dim3(grid_for((size_t)nodes * (Cc / V))), dim3(256), 0, d.f, d.df, node_df, d.th_A,
                      d.th_B, d.th_node, d.node_s, d.node_row, d.th_weight, Cc, nodes, rows_too ? 1 : 0);
            return GF_OK;
        });
        if (st == GF_OK) st = smp_field_size_grads(ctx, d.th_node, d.th_bucket, nbuckets, dsizes, Cc);
    }
    // the reverse gather is the SMP_1D level's (smp_level_1d.hip) at Cp := Cc, no concatenation, the two halves of dG kept apart
    if (st == GF_OK && np > 0) st = smp_1d_gather_bwd(s, l, "smpt_gather_bwd", sizes, Cc, 0, /*split=*/true, d.Q);
    if (st == GF_OK) st = gemm(ctx, true, false, Cp, 2 * Cc, (int)rows_p, pv.f, Cp, 0, d.Q, 2 * Cc, 0, d.dWst, 2 * Cc, 0, 1, 0);
    if (st == GF_OK) st = smp_field_wgrad_fold(ctx, d.dWst, dKl, Cp, Cc);
    if (st == GF_OK) st = wgrad_done(s, l);
    if (st != GF_OK) return st;
    return gemm(ctx, false, false, (int)rows_p, Cp, 2 * Cc, d.Q, 2 * Cc, 0, d.Wst + (size_t)2 * Cp * Cc, Cp, 0, pv.df, Cp, 0, 1, 0);
}

}  // namespace gf
