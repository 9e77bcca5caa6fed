// smp_level_1d.hip -- the first-order level of SMP_1D, SMP_1D_ver2 and SMP_1D_ver3 (GraphFlow/SMP_1D.h:480-510, SMP_1D_ver2.h:497-535,
// SMP_1D_ver3.h:511-557; gfsmp::Config::first_order = 2, 3, 4) and of their classifiers.
//
// Fields, children, pi and the per-size (lambda1_s, lambda2_s, b_s) blocks are SMP_theta's (smp_level_theta.hip, tables th_* of smp_prep.h)
// without a cap.  With S[i] = sum over the children w of f_{l-1}[w][pi_w(i)] ([s][Cp], Cp = C_{l-1}) and sumS = sum_i S[i]:
//   SMP_1D       z[i] = lambda1_s S[i] + lambda2_s sumS + b_s                          Cc = Cp,   slope 0.01     (W[s] = lambda1 I + lambda2 1 1^T)
//   SMP_1D_ver2  z[i] = [lambda1_s S[i] | lambda2_s sumS] + b_s                        Cc = 2 Cp, slope 0
//   SMP_1D_ver3  z[i] = [lambda1_s S[i] K_eye | lambda2_s sumS K_one] + b_s            Cc = 2 Cp, slope 0        (K_eye, K_one [Cp][Cp])
//   f_l[i] = LeakyReLU2D(z[i], slope)
// The first two have no matrix: the gathers read f_{l-1} and write df_{l-1} directly, no GEMM in either direction.  In ver3 the matrices
// act on the channel axis and commute with the gathers: G = f_{l-1} [K_eye | K_one] is one GEMM on the rows of level l - 1 (the theta
// level's, with Cc = Cp), the gathers read G and write dG, and dK = f_{l-1}^T dG, df_{l-1} = dG [K_eye | K_one]^T are two more.
// Kept: A[i] = the gathered top half ([rows][Cp]) and B = the bottom half summed over the positions ([nodes][Cp]).  Backward,
// dz = df_l * lrelu'(f_l), dzs = sum_i dz[i]:
//   db_s = sum dzs (all Cc columns),  dlambda1_s = sum k_v dz[:, :Cp] . A,  dlambda2_s = sum k_v dzs[bottom] . B  over the nodes of size s,
//   bottom = the same Cp columns in SMP_1D, columns [Cp, 2 Cp) in the concatenating forms; k_v = th_weight (smp_prep.h: the reference's
//   count of a vertex's contribution, j or j (j + 1) (j + 2) / 6 -- the class is the parity target, not the calculus)
//   dtop[w][j] = sum over the consumers v of w, i = the position of phi_{l-1}(w)[j] in phi_l(v), of lambda1_{s_v} dz_v[i][:Cp]
//   dbot[w][j] = the same sum of lambda2_{s_v} dzs_v[bottom];   df_{l-1} = dtop + dbot  (ver3: dG = [dtop | dbot])
// The lane vector (4 / 2 / 1 floats) divides Cp, NOT Cc: with Cp = 3 a float2 at columns 2, 3 of a [.][6] row would straddle the halves.
// Rows of Cp and of 2 Cp floats are then both multiples of the vector.  Every sum runs in a fixed order (children, positions, consumers
// ascending), no atomics: two runs give the same bits.  Every element of f_l, A, B, acc and df_{l-1} / dG is written by its kernel.
#include "smp_field_level.h"

namespace gf {
using namespace field_level;
namespace {

// Forward: nodes [blockIdx.x * npw, + npw).  Pass 1, items (node j, position i, vector q) over sum_j s_j * Cp / V: the two gathered
// halves -- one and the same gather where there is no matrix (gs == Cp) -- A, the top half of f_l (concatenating forms) and the bottom
// gather into `stash` (A itself without a matrix, else the bottom half of f_l's row).  Pass 2, items (node j, vector q): B = the stash
// summed over the node's positions, then what depends on it: all of f_l (additive) or its bottom half, the same at every position.
// The stash is read back by other lanes of the workgroup after the barrier: f and A are not __restrict__.
template <int V>
__global__ __launch_bounds__(256) void level1d_fwd(const float *__restrict__ G, int gs, const float *__restrict__ sizes, float *f, float *A,
                                                   float *__restrict__ B, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                   const long long *__restrict__ child_ptr, const long long *__restrict__ src_row,
                                                   const long long *__restrict__ pi_off, const short *__restrict__ pi, int Cp, int concat,
                                                   float alpha, int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const int Qc = Cp / V, Cc = concat ? 2 * Cp : Cp;
    const bool matrix = gs != Cp;
    const Run run = pack_run(off, node_s, nodes, npw, Qc);
    const int nb = run.nb, np = run.np;
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, np, it, Qc);
        const int n = nb + x.j, s = node_s[n], i = x.pos, cq = x.cq;
        Vf<V> a = vzero<V>(), t = vzero<V>();   // (both halves of a matrix form's G in one walk over the children)
        for (long long e = child_ptr[n]; e < child_ptr[n + 1]; ++e) {
            const int p = pi[pi_off[e] + i];
            if (p < 0) continue;
            const float *g = G + (src_row[e] + p) * gs + cq;
            vadd(a, vld<V>(g));
            if (matrix) vadd(t, vld<V>(g + Cp));
        }
        const long long row = node_row[n] + i;
        vst<V>(A + row * Cp + cq, a);
        if (!concat) continue;
        const float *se = size_entry(sizes, s, Cc);
        const float l1 = se[0];
        Vf<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = lrelu(l1 * a.v[k] + se[2 + cq + k], alpha);
        vst<V>(f + row * Cc + cq, o);
        if (matrix) vst<V>(f + row * Cc + Cp + cq, t);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < np * Qc; it += blockDim.x) {
        const int j = it / Qc, cq = (it - j * Qc) * V;
        const int n = nb + j, s = node_s[n];
        const long long r0 = node_row[n];
        const float *stash = matrix ? f + r0 * Cc + Cp + cq : A + r0 * Cp + cq;
        const int ss = matrix ? Cc : Cp;
        Vf<V> b = vzero<V>();
        for (int i = 0; i < s; ++i) vadd(b, vld<V>(stash + (long long)i * ss));
        vst<V>(B + (long long)n * Cp + cq, b);
        const float *se = size_entry(sizes, s, Cc);
        const float l1 = se[0], l2 = se[1];
        if (concat) {
            Vf<V> o;
#pragma unroll
            for (int k = 0; k < V; ++k) o.v[k] = lrelu(l2 * b.v[k] + se[2 + Cp + cq + k], alpha);
            for (int i = 0; i < s; ++i) vst<V>(f + (r0 + i) * Cc + Cp + cq, o);
        } else {
            for (int i = 0; i < s; ++i) {
                const Vf<V> a = vld<V>(A + (r0 + i) * Cp + cq);
                Vf<V> o;
#pragma unroll
                for (int k = 0; k < V; ++k) o.v[k] = lrelu((l1 * a.v[k] + l2 * b.v[k]) + se[2 + cq + k], alpha);
                vst<V>(f + (r0 + i) * Cc + cq, o);
            }
        }
    }
}

// Reverse, per node: one item per (node, vector q of Cp).  dz[i] = (df_l[i] (has_df) + dvec[n] (optional: the read-out's gradient, one
// vector per node)) * lrelu'(f_l[i]) is left in df; acc[n] = [ dzs | k_n sum_i dz[i][:Cp] A[i], 0 | 0, k_n dzs[bottom] B ] ([nodes][3 Cc];
// additive: [ dzs | k_n sum_i dz[i] A[i] | k_n dzs B ]) -- the layout the per-size reduction of the theta level sums; the zero halves
// add nothing to its lambda sums.  lrelu'(f) = 1 where f > 0, else alpha: at slope 0 the kept f is 0 where z <= 0.
template <int V>
__global__ __launch_bounds__(256) void level1d_node_bwd(const float *__restrict__ f, float *__restrict__ df, const float *__restrict__ dvec,
                                                        const float *__restrict__ A, const float *__restrict__ B, float *__restrict__ acc,
                                                        const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                        const int *__restrict__ weight, int Cp, int concat, float alpha, int nodes, int has_df) {
    const int Qc = Cp / V, Cc = concat ? 2 * Cp : Cp, halves = concat ? 2 : 1;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nodes * Qc) return;
    const int n = (int)(t / Qc), cq = (int)(t - (long long)n * Qc) * V;
    const int s = node_s[n];
    const long long r0 = node_row[n];
    const float kn = (float)weight[n];
    float *a = acc + (long long)n * 3 * Cc;
    Vf<V> zs[2];
    for (int h = 0; h < halves; ++h) {
        const int c0 = h * Cp + cq;
        Vf<V> dv = vzero<V>(), pa = vzero<V>();
        zs[h] = vzero<V>();
        if (dvec) dv = vld<V>(dvec + (long long)n * Cc + c0);
        for (int i = 0; i < s; ++i) {
            const long long o = (r0 + i) * Cc + c0;
            const Vf<V> d = dz_of<V>(f, df, o, dv, has_df, alpha);
            vadd(zs[h], d);
            if (h == 0) {
                const Vf<V> av = vld<V>(A + (r0 + i) * Cp + cq);
#pragma unroll
                for (int k = 0; k < V; ++k) pa.v[k] += d.v[k] * av.v[k];
            }
            vst<V>(df + o, d);
        }
        vst<V>(a + c0, zs[h]);
        if (h == 0) {
#pragma unroll
            for (int k = 0; k < V; ++k) pa.v[k] *= kn;
            vst<V>(a + Cc + cq, pa);
            if (concat) vst<V>(a + 2 * Cc + cq, vzero<V>());
        } else {
            vst<V>(a + Cc + c0, vzero<V>());
        }
    }
    const Vf<V> bv = vld<V>(B + (long long)n * Cp + cq);
    Vf<V> pb;
#pragma unroll
    for (int k = 0; k < V; ++k) pb.v[k] = kn * (zs[halves - 1].v[k] * bv.v[k]);
    vst<V>(a + 2 * Cc + (halves - 1) * Cp + cq, pb);
}

// Reverse gather: source nodes [blockIdx.x * npw, + npw) of level l - 1; items (node j, position p, vector q) over sum_j s_j Cp / V.
// dz rows are Cc floats, acc rows 3 Cc (the first Cc: dzs).  split = 0: out = df_{l-1} [rows][Cp] <- dtop + dbot; 1: out = dG [rows][2 Cp].
template <int V>
__global__ __launch_bounds__(256) void level1d_gather_bwd(const float *__restrict__ dz, const float *__restrict__ acc, const float *__restrict__ sizes,
                                                          float *__restrict__ out, const int *__restrict__ prev_s,
                                                          const long long *__restrict__ prev_row, const long long *__restrict__ cons_ptr,
                                                          const long long *__restrict__ cons_row, const int *__restrict__ cons_s,
                                                          const int *__restrict__ cons_node, const long long *__restrict__ inv_off,
                                                          const short *__restrict__ inv, int Cp, int concat, int split, int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const int Cc = concat ? 2 * Cp : Cp, bot = concat ? Cp : 0;
    const Run run = pack_run(off, prev_s, nodes, npw, Cp / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int w = run.nb + x.j, p = x.pos, cq = x.cq;
        Vf<V> gt = vzero<V>(), gb = vzero<V>();
        for (long long c = cons_ptr[w]; c < cons_ptr[w + 1]; ++c) {
            const int i = inv[inv_off[c] + p];
            if (i < 0) continue;
            const float *se = size_entry(sizes, cons_s[c], Cc);
            const float l1 = se[0], l2 = se[1];
            const Vf<V> z = vld<V>(dz + (cons_row[c] + i) * Cc + cq), zs = vld<V>(acc + (long long)cons_node[c] * 3 * Cc + bot + cq);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                gt.v[k] += l1 * z.v[k];
                gb.v[k] += l2 * zs.v[k];
            }
        }
        const long long row = prev_row[w] + p;
        if (split) {
            vst<V>(out + row * 2 * Cp + cq, gt);
            vst<V>(out + row * 2 * Cp + Cp + cq, gb);
        } else {
            vadd(gt, gb);
            vst<V>(out + row * Cp + cq, gt);
        }
    }
}

}  // namespace

// f_l from f_{l-1}: SMP_1D / ver2 gather the rows of f_{l-1} themselves; ver3 gathers G = f_{l-1} [K_eye | K_one] (the level's Q buffer)
gf_status smp_1d_forward_level(gf_smp *s, int l, const float *Kl, const float *sizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), concat = s->cfg.concat() ? 1 : 0;
    const bool matrix = s->cfg.first_order == 4;
    const long long rows_p = s->lay.level[l - 1].rows;
    const int nodes = s->lay.level[l].nNodes, V = lane_vector(Cp);
    if (matrix) {
        gf_status st = smp_field_weight_views(ctx, Kl, d.Wst, d.Wst + (size_t)2 * Cp * Cp, Cp, Cp);
        if (st == GF_OK) st = gemm(ctx, false, false, (int)rows_p, 2 * Cp, Cp, pv.f, Cp, 0, d.Wst, 2 * Cp, 0, d.Q, 2 * Cp, 0, 1, 0);
        if (st != GF_OK) return st;
    }
    if (nodes == 0) return GF_OK;
    const RunGrid g = run_grid(s->lay.level[l], false, Cp / V);
    return with_lane_vector(V, [&](auto v) -> gf_status {
        GF_LAUNCH(ctx, "smp1d_level_fwd", level1d_fwd<v>, g.grid, dim3(256), 0, matrix ? d.Q : pv.f, matrix ? 2 * Cp : Cp, sizes, d.f, d.th_A, d.th_B,
                  d.node_s, d.node_row, d.th_child_ptr, d.th_src_row, d.th_pi_off, d.th_pi, Cp, concat, s->cfg.level_slope(), nodes, g.npw);
        return GF_OK;
    });
}

// The reverse gather of level l at Cp channels per half under the caller's timer name: out = df_{l-1} [rows][Cp], or split: dG
// [rows][2 Cp].  smp_level_theta.hip launches it too (Cp := its Cc, concat = 0, split).
gf_status smp_1d_gather_bwd(gf_smp *s, int l, const char *timer, const float *sizes, int Cp, int concat, bool split, float *out) {
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int np = s->lay.level[l - 1].nNodes, V = lane_vector(Cp);
    const RunGrid g = run_grid(s->lay.level[l - 1], false, Cp / V);
    return with_lane_vector(V, [&](auto v) -> gf_status {
        GF_LAUNCH(s->ctx, timer, level1d_gather_bwd<v>, g.grid, dim3(256), 0, d.df, d.th_node, sizes, out, pv.node_s, pv.node_row, d.th_cons_ptr,
                  d.th_cons_row, d.th_cons_s, d.th_cons_node, d.th_inv_off, d.th_inv, Cp, concat, split ? 1 : 0, np, g.npw);
        return GF_OK;
    });
}

// node_df / rows_too / wgrad_done as smp_theta_backward_level.  The per-size gradients are final after the reduction, ver3's dK after
// its product; df_{l-1} comes last.
gf_status smp_1d_backward_level(gf_smp *s, int l, const float *Kl, const float *sizes, float *dKl, float *dsizes, const float *node_df,
                                bool rows_too, gf_status (*wgrad_done)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l), concat = s->cfg.concat() ? 1 : 0;
    const bool matrix = s->cfg.first_order == 4;
    const long long rows_p = s->lay.level[l - 1].rows;
    const int nbuckets = (int)(s->lay.level[l].th_bucket.size() / 3);
    if (!node_df && !rows_too) return fail(ctx, GF_ERR_INVALID, "first-order level %d: no gradient to back-propagate", l);
    gf_status st = GF_OK;
    if (s->lay.level[l].nNodes > 0) {
        const int nodes = s->lay.level[l].nNodes, V = lane_vector(Cp);
        st = with_lane_vector(V, [&](auto v) -> gf_status {
            GF_LAUNCH(ctx, "smp1d_node_bwd", level1d_node_bwd<v>, dim3(grid_for((size_t)nodes * (Cp / V))), dim3(256), 0, d.f, d.df, node_df, d.th_A,
                      d.th_B, d.th_node, d.node_s, d.node_row, d.th_weight, Cp, concat, s->cfg.level_slope(), nodes, rows_too ? 1 : 0);
            return GF_OK;
        });
        if (st == GF_OK) st = smp_field_size_grads(ctx, d.th_node, d.th_bucket, nbuckets, dsizes, Cc);
    }
    if (st == GF_OK && s->lay.level[l - 1].nNodes > 0) st = smp_1d_gather_bwd(s, l, "smp1d_gather_bwd", sizes, Cp, concat, matrix, matrix ? d.Q : pv.df);
    if (st != GF_OK) return st;
    if (!matrix) return wgrad_done(s, l);
    // (the views again: this sweep's parameters need not be the forward's)
    st = smp_field_weight_views(ctx, Kl, d.Wst, d.Wst + (size_t)2 * Cp * Cp, Cp, Cp);
    if (st == GF_OK) st = gemm(ctx, true, false, Cp, 2 * Cp, (int)rows_p, pv.f, Cp, 0, d.Q, 2 * Cp, 0, d.dWst, 2 * Cp, 0, 1, 0);
    if (st == GF_OK) st = smp_field_wgrad_fold(ctx, d.dWst, dKl, Cp, Cp);
    if (st == GF_OK) st = wgrad_done(s, l);
    if (st != GF_OK) return st;
    return gemm(ctx, false, false, (int)rows_p, Cp, 2 * Cp, d.Q, 2 * Cp, 0, d.Wst + (size_t)2 * Cp * Cp, Cp, 0, pv.df, Cp, 0, 1, 0);
}

}  // namespace gf
