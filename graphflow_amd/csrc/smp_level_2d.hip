// smp_level_2d.hip -- the level of the second-order steerable models SMP_2D and SMP_2D_ver4 (GraphFlow/SMP_2D.h:523-581,
// SMP_2D_ver4.h:560-620; gfsmp::Config::steerable_2d = 1, 2) and of their classifiers.
//
// f_l[v] is [s][s][C_l] on the field phi_l(v), s = |phi_l(v)|.  Fields, children (hop distance <= 1) and the position maps pi / inv are the
// first-order levels' (tables th_* of smp_prep.h), applied to BOTH indices.  With Cp = C_{l-1}, per channel:
//   S[i][j]  = sum over the children w of f_{l-1}[w][pi_w(i)][pi_w(j)]  +  scalar_l adj_v[i][j]      (a missing position: no term)
//   col[j]   = sum_k S[k][j]                                  (W[s] = lambda1_s I + lambda2_s 1 1^T, TensorMul along the first index)
//   SMP_2D       z[i][j] = lambda1_s S[i][j] + lambda2_s col[j] + b_s                  Cc = Cp
//   SMP_2D_ver4  z[i][j] = [lambda1_s S[i][j] | lambda2_s col[j]] + b_s                Cc = 2 Cp
//   f_l = LeakyReLU3D(z), slope 0.01
// The per-size entry s of a level is (lambda1_s[Cp], lambda2_s[Cp], b_s[Cc]).  No matrix anywhere: a memory-bound gather, column sum and
// scatter on the sum s^2 rows of the level, no GEMM in either direction.
// Lanes sit on (column j, channel vector) and walk the rows i: col[j] stays in registers, every lane reads back only what it wrote.
// Kept for the reverse sweep: S ([rows][Cp]) and col ([sum s][Cp]) -- DESIGN.md section 4.9 counts the bytes against re-gathering.
// Backward, dz = df_l * lrelu'(f_l), cz[j] = sum_i dz[i][j] (ver4: of the bottom half):
//   dS[i][j]     = lambda1_s dz[i][j] (top half) + lambda2_s cz[j]                     left in the first Cp columns of df_l
//   db_s         = sum_ij dz;  dlambda1_s = sum k_v sum_ij dz[i][j] S[i][j];  dlambda2_s = sum k_v sum_j cz[j] col[j]  over the nodes of size s
//   dscalar_l    = sum over the level of adj_v[i][j] dS[i][j]
//   df_{l-1}[w][p][q] = sum over the consumers v of w of dS_v[inv(p)][inv(q)]
// k_v = th_weight (smp_prep.h): the reference's count of a vertex's contribution, j (j + 1) / 2 or j -- the class is the parity target.
// The lane vector (4 / 2 / 1 floats) divides Cp.  Every sum runs in a fixed order (children, rows, consumers ascending; the reductions
// fold fixed chunks in order), no atomics: two runs give the same bits.  Every element of f_l, S, col, the partials and df_{l-1} is
// written by its kernel before anything reads it.
#include "smp_field_level.h"

namespace gf {
using namespace field_level;
namespace {

constexpr int kSplit2d = 16;   // row chunks per size bucket in the reduction of the column partials

// Forward: nodes [blockIdx.x * npw, + npw); items (node, column j, vector q) over sum s * Cp / V.  Pass 1 over the rows i: S[i][j] gathered,
// stored, summed into col[j]; the top half of f_l in the concatenating form.  Pass 2: what needs col[j].  S is read back by the lane
// that wrote it: not __restrict__.
template <int V>
__global__ __launch_bounds__(256) void level2d_fwd(const float *__restrict__ fp, const float *__restrict__ sizes, const float *__restrict__ scalar,
                                                   const float *__restrict__ adj, float *__restrict__ f, float *S, float *__restrict__ col,
                                                   const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                   const long long *__restrict__ node_pair, const long long *__restrict__ child_ptr,
                                                   const long long *__restrict__ src_row, const int *__restrict__ src_s,
                                                   const long long *__restrict__ pi_off, const short *__restrict__ pi, int Cp, int concat,
                                                   float alpha, int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const int Cc = concat ? 2 * Cp : Cp;
    const Run run = pack_run(off, node_s, nodes, npw, Cp / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int n = run.nb + x.j, s = node_s[n], j = x.pos, cq = x.cq;
        const long long r0 = node_row[n], e0 = child_ptr[n], e1 = child_ptr[n + 1];
        const float *se = size_entry_2d(sizes, s, Cp, Cc);
        const Vf<V> l1 = vld<V>(se + cq), l2 = vld<V>(se + Cp + cq), bt = vld<V>(se + 2 * Cp + cq), sc = vld<V>(scalar + cq);
        Vf<V> cs = vzero<V>();
        for (int i = 0; i < s; ++i) {
            Vf<V> a = gather_pair<V>(fp, Cp, cq, e0, e1, src_row, src_s, pi_off, pi, i, j);
            const long long row = r0 + (long long)i * s + j;
            const float av = adj[row];
#pragma unroll
            for (int c = 0; c < V; ++c) a.v[c] += sc.v[c] * av;
            vst<V>(S + row * Cp + cq, a);
            vadd(cs, a);
            if (concat) {
                Vf<V> o;
#pragma unroll
                for (int c = 0; c < V; ++c) o.v[c] = lrelu(l1.v[c] * a.v[c] + bt.v[c], alpha);
                vst<V>(f + row * Cc + cq, o);
            }
        }
        vst<V>(col + (node_pair[n] + j) * Cp + cq, cs);
        if (concat) {
            const Vf<V> bb = vld<V>(se + 3 * Cp + cq);
            Vf<V> o;
#pragma unroll
            for (int c = 0; c < V; ++c) o.v[c] = lrelu(l2.v[c] * cs.v[c] + bb.v[c], alpha);
            for (int i = 0; i < s; ++i) vst<V>(f + (r0 + (long long)i * s + j) * Cc + Cp + cq, o);
        } else {
            for (int i = 0; i < s; ++i) {
                const long long row = r0 + (long long)i * s + j;
                const Vf<V> a = vld<V>(S + row * Cp + cq);
                Vf<V> o;
#pragma unroll
                for (int c = 0; c < V; ++c) o.v[c] = lrelu((l1.v[c] * a.v[c] + l2.v[c] * cs.v[c]) + bt.v[c], alpha);
                vst<V>(f + row * Cc + cq, o);
            }
        }
    }
}

// Reverse, per (node, column j, vector q), packed as the forward.  dz = (df_l (has_df) + dvec[n] (optional: the read-out's gradient, one
// vector per node)) * lrelu'(f_l); dS is left in the first Cp columns of df_l's rows.  part[node_pair[n] + j] = [ sum_i dz[i][j] (Cc) |
// k_n sum_i dz[i][j] S[i][j] (Cp) | k_n cz[j] col[j] (Cp) | sum_i adj[i][j] dS[i][j] (Cp) ], Wd = Cc + 3 Cp floats.  df is read back by the
// lane that wrote it: not __restrict__.
template <int V>
__global__ __launch_bounds__(256) void level2d_node_bwd(const float *__restrict__ f, float *df, const float *__restrict__ dvec,
                                                        const float *__restrict__ S, const float *__restrict__ col, const float *__restrict__ sizes,
                                                        const float *__restrict__ adj, float *__restrict__ part, const int *__restrict__ node_s,
                                                        const long long *__restrict__ node_row, const long long *__restrict__ node_pair,
                                                        const int *__restrict__ weight, int Cp, int concat, float alpha, int nodes, int npw,
                                                        int has_df) {
    __shared__ int off[kMaxPack + 1];
    const int Cc = concat ? 2 * Cp : Cp, Wd = Cc + 3 * Cp;
    const Run run = pack_run(off, node_s, nodes, npw, Cp / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int n = run.nb + x.j, s = node_s[n], j = x.pos, cq = x.cq;
        const long long r0 = node_row[n];
        const float *se = size_entry_2d(sizes, s, Cp, Cc);
        const Vf<V> l1 = vld<V>(se + cq), l2 = vld<V>(se + Cp + cq);
        const float kn = (float)weight[n];
        float *pr = part + (node_pair[n] + j) * Wd;
        Vf<V> cz = vzero<V>();   // sum_i dz[i][j] of the half that feeds col: all of dz (additive), the bottom half (concatenating)
        if (concat) {
            Vf<V> dv = vzero<V>();
            if (dvec) dv = vld<V>(dvec + (long long)n * Cc + Cp + cq);
            for (int i = 0; i < s; ++i) {
                const long long o = (r0 + (long long)i * s + j) * Cc + Cp + cq;
                vadd(cz, dz_of<V>(f, df, o, dv, has_df, alpha));
            }
            vst<V>(pr + Cp + cq, cz);
        }
        Vf<V> dv = vzero<V>(), zs = vzero<V>(), pa = vzero<V>(), ps = vzero<V>();
        if (dvec) dv = vld<V>(dvec + (long long)n * Cc + cq);
        for (int i = 0; i < s; ++i) {
            const long long row = r0 + (long long)i * s + j, o = row * Cc + cq;
            const Vf<V> sv = vld<V>(S + row * Cp + cq);
            Vf<V> d = dz_of<V>(f, df, o, dv, has_df, alpha);
#pragma unroll
            for (int c = 0; c < V; ++c) {
                zs.v[c] += d.v[c];
                pa.v[c] += d.v[c] * sv.v[c];
            }
            if (concat) {   // (cz is complete: dS in one pass)
                const float av = adj[row];
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    d.v[c] = l1.v[c] * d.v[c] + l2.v[c] * cz.v[c];
                    ps.v[c] += av * d.v[c];
                }
            }
            vst<V>(df + o, d);
        }
        if (!concat) {
            cz = zs;
            for (int i = 0; i < s; ++i) {
                const long long row = r0 + (long long)i * s + j, o = row * Cc + cq;
                Vf<V> d = vld<V>(df + o);
                const float av = adj[row];
#pragma unroll
                for (int c = 0; c < V; ++c) {
                    d.v[c] = l1.v[c] * d.v[c] + l2.v[c] * cz.v[c];
                    ps.v[c] += av * d.v[c];
                }
                vst<V>(df + o, d);
            }
        }
        const Vf<V> cv = vld<V>(col + (node_pair[n] + j) * Cp + cq);
        Vf<V> pb;
#pragma unroll
        for (int c = 0; c < V; ++c) {
            pa.v[c] *= kn;
            pb.v[c] = kn * (cz.v[c] * cv.v[c]);
        }
        vst<V>(pr + cq, zs);
        vst<V>(pr + Cc + cq, pa);
        vst<V>(pr + Cc + Cp + cq, pb);
        vst<V>(pr + Cc + 2 * Cp + cq, ps);
    }
}

// The column partials of one size bucket (s, first node, count: its nodes and so its sum-s rows of `part` are contiguous) in kSplit2d row
// chunks: workgroup (bucket, chunk), thread (rr, c) sums the chunk's rows rr, rr + rl, .. of column c, the rl partials are folded in order.
// out[bucket][chunk][Wd]; an empty chunk writes zeros.
__global__ __launch_bounds__(256) void level2d_bucket_partials(const float *__restrict__ part, const int *__restrict__ bucket,
                                                               const long long *__restrict__ node_pair, float *__restrict__ out, int Wd) {
    __shared__ float red[256];
    const int s = bucket[3 * blockIdx.x], n0 = bucket[3 * blockIdx.x + 1], cnt = bucket[3 * blockIdx.x + 2];
    const long long nrows = (long long)cnt * s, chunk = (nrows + kSplit2d - 1) / kSplit2d;
    const long long b0 = node_pair[n0] + chunk * blockIdx.y;
    long long len = nrows - chunk * blockIdx.y;
    len = len < 0 ? 0 : len > chunk ? chunk : len;
    float *o = out + ((size_t)blockIdx.x * kSplit2d + blockIdx.y) * Wd;
    const int lanes = Wd < 256 ? Wd : 256, rl = 256 / lanes;
    const int f0 = threadIdx.x % lanes, rr = threadIdx.x / lanes;
    for (int fb = 0; fb < Wd; fb += lanes) {
        const int c = fb + f0;
        float a = 0.f;
        if (c < Wd && rr < rl)
            for (long long r = rr; r < len; r += rl) a += part[(b0 + r) * Wd + c];
        red[threadIdx.x] = a;
        __syncthreads();
        if (rr == 0 && c < Wd) {
            float t = 0.f;
            for (int k = 0; k < rl; ++k) t += red[k * lanes + f0];
            o[c] = t;
        }
        __syncthreads();
    }
}

// Workgroup b < nbuckets: the bucket's chunks in order, `+=` into its per-size entry (db | dlambda1 | dlambda2 sit at 2 Cp | 0 | Cp of the
// entry).  Workgroup nbuckets: dscalar += the last Cp columns over the buckets and chunks in order.
__global__ __launch_bounds__(256) void level2d_grads_finish(const float *__restrict__ bp, const int *__restrict__ bucket, float *__restrict__ dsizes,
                                                            float *__restrict__ dscalar, int Cp, int Cc, int nbuckets) {
    const int Wd = Cc + 3 * Cp;
    if ((int)blockIdx.x < nbuckets) {
        float *out = dsizes + (size_t)(bucket[3 * blockIdx.x] - 1) * (2 * Cp + Cc);
        for (int c = threadIdx.x; c < Cc + 2 * Cp; c += blockDim.x) {
            float t = 0.f;
            for (int k = 0; k < kSplit2d; ++k) t += bp[((size_t)blockIdx.x * kSplit2d + k) * Wd + c];
            out[c < Cc ? 2 * Cp + c : c - Cc] += t;
        }
        return;
    }
    for (int c = threadIdx.x; c < Cp; c += blockDim.x) {
        float t = 0.f;
        for (int k = 0; k < nbuckets * kSplit2d; ++k) t += bp[(size_t)k * Wd + Cc + 2 * Cp + c];
        dscalar[c] += t;
    }
}

}  // namespace

// f_l from f_{l-1}: one launch
gf_status smp_2d_forward_level(gf_smp *s, int l, const float *scalar, const float *sizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), concat = s->cfg.concat() ? 1 : 0;
    const int nodes = s->lay.level[l].nNodes, V = lane_vector(Cp);
    if (nodes == 0) return GF_OK;
    const RunGrid g = run_grid(s->lay.level[l], true, Cp / V);
    return with_lane_vector(V, [&](auto v) -> gf_status {
        GF_LAUNCH(ctx, "smp2d_level_fwd", level2d_fwd<v>, g.grid, dim3(256), 0, pv.f, sizes, scalar, d.adj, d.f, d.th_A, d.th_B, d.node_s, d.node_row,
                  d.node_pair, d.th_child_ptr, d.th_src_row, d.th_src_s, d.th_pi_off, d.th_pi, Cp, concat, s->cfg.level_slope(), nodes, g.npw);
        return GF_OK;
    });
}

// dz and dS per node, the per-size gradients and dscalar_l over the buckets, then df_{l-1}.  (scalar_l itself and wgrad_done: not needed)
gf_status smp_2d_backward_level(gf_smp *s, int l, const float *, const float *sizes, float *dscalar, float *dsizes, const float *node_df,
                                bool rows_too, gf_status (*)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int Cp = s->cfg.level_channels(l - 1), concat = s->cfg.concat() ? 1 : 0;
    const int nodes = s->lay.level[l].nNodes, V = lane_vector(Cp);
    if (!node_df && !rows_too) return fail(ctx, GF_ERR_INVALID, "steerable level %d: no gradient to back-propagate", l);
    if (nodes > 0) {
        const RunGrid g = run_grid(s->lay.level[l], true, Cp / V);
        gf_status st = with_lane_vector(V, [&](auto v) -> gf_status {
            GF_LAUNCH(ctx, "smp2d_node_bwd", level2d_node_bwd<v>, g.grid, dim3(256), 0, d.f, d.df, node_df, d.th_A, d.th_B, sizes, d.adj, d.th_node,
                      d.node_s, d.node_row, d.node_pair, d.th_weight, Cp, concat, s->cfg.level_slope(), nodes, g.npw, rows_too ? 1 : 0);
            return GF_OK;
        });
        if (st == GF_OK) st = smp_2d_size_grads(s, l, dscalar, dsizes);
        if (st != GF_OK) return st;
    }
    return smp_field_gather_down(s, l, d.df, s->cfg.level_channels(l), true, "smp2d_gather_bwd");
}

// The column partials in d.th_node ([sum s][Cc + 3 Cp]) over the size buckets: `+=` into the per-size entries and dscalar_l
gf_status smp_2d_size_grads(gf_smp *s, int l, float *dscalar, float *dsizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);
    const int nbuckets = (int)(s->lay.level[l].th_bucket.size() / 3);
    GF_LAUNCH(ctx, "smp2d_bucket_partials", level2d_bucket_partials, dim3((unsigned)nbuckets, kSplit2d), dim3(256), 0, d.th_node, d.th_bucket,
              d.node_pair, d.part2d, Cc + 3 * Cp);
    GF_LAUNCH(ctx, "smp2d_grads_finish", level2d_grads_finish, dim3((unsigned)nbuckets + 1), dim3(256), 0, d.part2d, d.th_bucket, dsizes, dscalar, Cp,
              Cc, nbuckets);
    return GF_OK;
}

}  // namespace gf
