// smp_level_unrestricted.hip -- the level of Unrestricted_SMP_1D, Unrestricted_SMP_1D_ver2 and Unrestricted_SMP_2D
// (GraphFlow/Unrestricted_SMP_1D.h:440-470, Unrestricted_SMP_1D_ver2.h:462-500, Unrestricted_SMP_2D.h:480-525;
// gfsmp::Config::unrestricted = 1, 2, 3): the steerable models with a DENSE learned filter per field size.
//
// Fields, children (hop distance <= 1), pi / inv and the size buckets are the first-order tables th_* of smp_prep.h; forms 1 and 2 sit on
// the rows of SMP_1D / SMP_1D_ver2 (f_l[v] is [s][C_l]), form 3 on those of SMP_2D (f_l[v] is [s][s][C], the plain reduced adjacency).
// With Cp = C_{l-1}, S = the gather-sum over the children (form 3: both indices, plus scalar_l adj_v):
//   1  z[i][c]    = sum_k W_s[i][k] S[k][c] + b_s[c]                          Cc = Cp,   slope 0.01
//   2  z[i]       = [ (W1_s S)[i] | (W2_s S)[i] ] + b_s                       Cc = 2 Cp, slope 0
//   3  z[i][j][c] = sum_k W_s[i][k][c] S[k][j][c] + b_s[c]                    Cc = Cp,   slope 0.01       (one filter per channel)
// The per-size block of a level: for s = 1 .. max_nVertices the filter (s^2, 2 s^2 or s^2 Cp floats, row-major, the channel innermost
// in form 3) then b_s[Cc]; entry s starts at fl (s - 1) s (2 s - 1) / 6 + (s - 1) Cc with fl = 1, 2, Cp.  Form 3: scalar_l[Cp] behind it.
// Forward, one kernel per level.  Forms 1 / 2: lanes on (node, row, channel vector) of a packed run of nodes; pass 1 gathers S, stores it
// (dW needs it) and keeps the run's S in LDS, pass 2 walks k.  A run whose S is above kUnLds floats (one node of s Cp > kUnLds, or a run
// of nodes above the level's average) reads the stored S back instead: the same arithmetic in the same order.  W_s is a broadcast read
// (every lane of a (node, row) reads the same word).  Form 3: lanes on (node, column j, channel vector); W_s at s = 29, C = 64 is 215 KB,
// more than the LDS, so it is streamed: the nodes come in bucket order, the workgroups that share a W_s run together and it stays in L2.
// Plain FMAs with the lanes on the channels: the product is element-wise in c.
// Backward, dz = df_l * lrelu'(f_l) in place:
//   dS = W_s^T dz (per channel in form 3) into its own buffer [rows][Cp];  db_s = sum dz;  dscalar_l = sum adj dS
//   1, 2  dW_s[i][k] = sum over the nodes of size s, sum_c dz[i][c] S[k][c]        (per half in form 2)
//   3     dW_s[i][k][c] = sum over the nodes, sum_j dz[i][j][c] S[k][j][c]
//   df_{l-1} = the consumer-side gather of dS
// The classes register W_s / b_s once per graph (Unrestricted_SMP_1D.h:420-421): every gradient is the plain derivative, no th_weight.
// The filter gradients never leave a per-node copy behind: workgroup (bucket, node chunk, tile of the entry) sums its elements over the
// chunk's nodes in order -- forms 1 / 2 with kUnGroup lanes per element on the channels, folded by a fixed shuffle tree -- and a finish
// kernel folds the kUnSplit chunks in order.  No atomics, fixed orders: two runs give the same bits.  Every element of f_l, S, dS, the
// column partials, the chunk partials and df_{l-1} is written by its kernel before anything reads it.
#include "smp_field_level.h"

namespace gf {
using namespace field_level;
namespace {

constexpr int kUnSplit = gfsmp::kUnrestrictedSplit;   // node chunks per size bucket in the reduction of the filter gradients
constexpr int kUnLds = 2048;                          // floats of S a workgroup of the first-order forward keeps in LDS
constexpr int kUnGroup = 16;                          // lanes on one element of a first-order filter gradient

// z[i][cq ..] of one half: b + sum_k Wrow[k] src[k * Cp]
template <int V>
__device__ __forceinline__ Vf<V> filter_row(const float *__restrict__ Wrow, const float *src, const float *__restrict__ b, int s, int Cp, float alpha) {
    Vf<V> z = vld<V>(b);
    for (int k = 0; k < s; ++k) {
        const float w = Wrow[k];
        const Vf<V> a = vld<V>(src + (size_t)k * Cp);
#pragma unroll
        for (int c = 0; c < V; ++c) z.v[c] += w * a.v[c];
    }
#pragma unroll
    for (int c = 0; c < V; ++c) z.v[c] = lrelu(z.v[c], alpha);
    return z;
}

// Forms 1 / 2, forward: nodes [blockIdx.x * npw, + npw); items (node, row, vector q) over sum s Cp / V.  Item `it` of pass 1 owns
// S[row][cq ..]: the float offset of that element inside the run is it * V, which is where the LDS copy goes.  S is read back by other
// lanes of the workgroup after the barrier: not __restrict__.
template <int V>
__global__ __launch_bounds__(256) void unres1d_fwd(const float *__restrict__ fp, const float *__restrict__ sizes, float *__restrict__ f, float *S,
                                                   const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                   const long long *__restrict__ child_ptr, const long long *__restrict__ src_row,
                                                   const long long *__restrict__ pi_off, const short *__restrict__ pi, int Cp, int halves,
                                                   float alpha, int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    __shared__ __align__(16) float lds[kUnLds];
    const int Cc = halves * Cp;
    const Run run = pack_run(off, node_s, nodes, npw, Cp / V);
    const bool in_lds = (long long)run.total * V <= kUnLds;
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int n = run.nb + x.j, k = x.pos, cq = x.cq;
        const Vf<V> a = gather_row<V>(fp, Cp, cq, child_ptr[n], child_ptr[n + 1], src_row, pi_off, pi, k);
        vst<V>(S + (node_row[n] + k) * Cp + cq, a);
        if (in_lds) vst<V>(lds + (size_t)it * V, a);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int j = x.j, n = run.nb + j, s = node_s[n], i = x.pos, cq = x.cq;
        const long long r0 = node_row[n];
        const float *se = sizes + entry_off(s, halves, Cc);
        const float *b = se + (size_t)halves * s * s;
        for (int h = 0; h < halves; ++h) {
            const float *Wrow = se + ((size_t)h * s + i) * s;
            const Vf<V> o = in_lds ? filter_row<V>(Wrow, lds + (size_t)off[j] * V + cq, b + h * Cp + cq, s, Cp, alpha)
                                   : filter_row<V>(Wrow, S + r0 * Cp + cq, b + h * Cp + cq, s, Cp, alpha);
            vst<V>(f + (r0 + i) * Cc + h * Cp + cq, o);
        }
    }
}

// Forms 1 / 2, reverse, packed as the forward.  Pass 1: dz = (df_l (has_df) + dvec[n] (optional: the read-out's gradient, one vector per
// node)) * lrelu'(f_l), left in df.  Pass 2, item (node, k, vector): dS[k] = sum_i W1[i][k] dz[i][:Cp] (+ W2[i][k] dz[i][Cp:]).
// df is read back by other lanes after the barrier: not __restrict__.
template <int V>
__global__ __launch_bounds__(256) void unres1d_node_bwd(const float *__restrict__ f, float *df, const float *__restrict__ dvec,
                                                        const float *__restrict__ sizes, float *__restrict__ dS, const int *__restrict__ node_s,
                                                        const long long *__restrict__ node_row, int Cp, int halves, float alpha, int nodes,
                                                        int npw, int has_df) {
    __shared__ int off[kMaxPack + 1];
    const int Cc = halves * Cp;
    const Run run = pack_run(off, node_s, nodes, npw, Cp / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int n = run.nb + x.j, i = x.pos, cq = x.cq;
        for (int h = 0; h < halves; ++h) {
            const long long o = (node_row[n] + i) * Cc + h * Cp + cq;
            Vf<V> dv = vzero<V>();
            if (dvec) dv = vld<V>(dvec + (long long)n * Cc + h * Cp + cq);
            vst<V>(df + o, dz_of<V>(f, df, o, dv, has_df, alpha));
        }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int n = run.nb + x.j, s = node_s[n], k = x.pos, cq = x.cq;
        const long long r0 = node_row[n];
        const float *se = sizes + entry_off(s, halves, Cc);
        Vf<V> g = vzero<V>();
        for (int h = 0; h < halves; ++h) {
            const float *Wc = se + (size_t)h * s * s + k;
            for (int i = 0; i < s; ++i) {
                const float w = Wc[(size_t)i * s];
                const Vf<V> d = vld<V>(df + (r0 + i) * Cc + h * Cp + cq);
#pragma unroll
                for (int c = 0; c < V; ++c) g.v[c] += w * d.v[c];
            }
        }
        vst<V>(dS + (r0 + k) * Cp + cq, g);
    }
}

// Forms 1 / 2: the entry of one size bucket (s, first node, count: its nodes, and so its rows, are contiguous) over the nodes of chunk
// blockIdx.y; out[part_off[bucket] + chunk * Wd + e], Wd = halves s^2 + Cc, e in the entry's own order (W1, W2, b).  kUnGroup lanes per
// element: on the channels c = g, g + kUnGroup, .. of a filter element, on the chunk's rows of a bias element; folded by a fixed tree.
// The loop runs the same number of times in every lane (the shuffles need them all); an empty chunk writes zeros.
__global__ __launch_bounds__(256) void unres1d_bucket_partials(const float *__restrict__ dz, const float *__restrict__ S,
                                                               const int *__restrict__ bucket, const long long *__restrict__ node_row,
                                                               const long long *__restrict__ part_off, float *__restrict__ out, int Cp,
                                                               int halves) {
    const BucketChunk bc = bucket_chunk(bucket, blockIdx.x, blockIdx.y, kUnSplit);
    const int s = bc.s, len = bc.len, Cc = halves * Cp, ss = s * s, Wd = halves * ss + Cc;
    const long long r0 = len > 0 ? node_row[bc.n0] : 0;
    float *o = out + part_off[blockIdx.x] + (size_t)blockIdx.y * Wd;
    const int g = threadIdx.x % kUnGroup, slot = threadIdx.x / kUnGroup;
    constexpr int per = 256 / kUnGroup;
    for (int base = blockIdx.z * per; base < Wd; base += gridDim.z * per) {
        const int e = base + slot;
        float acc = 0.f;
        if (e < halves * ss) {
            const int h = e / ss, rem = e - h * ss, i = rem / s, k = rem - i * s;
            for (int nn = 0; nn < len; ++nn) {
                const long long row = r0 + (long long)nn * s;
                const float *zp = dz + (row + i) * Cc + h * Cp, *sp = S + (row + k) * Cp;
                for (int c = g; c < Cp; c += kUnGroup) acc += zp[c] * sp[c];
            }
        } else if (e < Wd) {
            const int c = e - halves * ss;
            for (long long r = g; r < (long long)len * s; r += kUnGroup) acc += dz[(r0 + r) * Cc + c];
        }
        for (int d = kUnGroup / 2; d >= 1; d >>= 1) acc += __shfl_down(acc, d, kUnGroup);
        if (g == 0 && e < Wd) o[e] = acc;
    }
}

// Form 3, forward: items (node, column j, vector q) over sum s C / V, packed as above.  Pass 1 over the rows i: S[i][j] gathered, plus
// scalar adj, stored.  Pass 2: z[i][j] = b + sum_k W[i][k] S[k][j], element-wise in the channel.  S is read back by the lane that
// wrote it: not __restrict__.
template <int V>
__global__ __launch_bounds__(256) void unres2d_fwd(const float *__restrict__ fp, const float *__restrict__ sizes, const float *__restrict__ scalar,
                                                   const float *__restrict__ adj, float *__restrict__ f, float *S, const int *__restrict__ node_s,
                                                   const long long *__restrict__ node_row, const long long *__restrict__ child_ptr,
                                                   const long long *__restrict__ src_row, const int *__restrict__ src_s,
                                                   const long long *__restrict__ pi_off, const short *__restrict__ pi, int C, float alpha,
                                                   int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const Run run = pack_run(off, node_s, nodes, npw, C / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, C / V);
        const int n = run.nb + x.j, s = node_s[n], j = x.pos, cq = x.cq;
        const long long r0 = node_row[n], e0 = child_ptr[n], e1 = child_ptr[n + 1];
        const float *W = sizes + entry_off(s, C, C);
        const Vf<V> bt = vld<V>(W + (size_t)s * s * C + cq), sc = vld<V>(scalar + cq);
        for (int i = 0; i < s; ++i) {
            Vf<V> a = gather_pair<V>(fp, C, cq, e0, e1, src_row, src_s, pi_off, pi, i, j);
            const long long row = r0 + (long long)i * s + j;
            const float av = adj[row];
#pragma unroll
            for (int c = 0; c < V; ++c) a.v[c] += sc.v[c] * av;
            vst<V>(S + row * C + cq, a);
        }
        for (int i = 0; i < s; ++i) {
            Vf<V> z = bt;
            for (int k = 0; k < s; ++k) {
                const Vf<V> w = vld<V>(W + ((size_t)i * s + k) * C + cq), a = vld<V>(S + (r0 + (long long)k * s + j) * C + cq);
#pragma unroll
                for (int c = 0; c < V; ++c) z.v[c] += w.v[c] * a.v[c];
            }
#pragma unroll
            for (int c = 0; c < V; ++c) z.v[c] = lrelu(z.v[c], alpha);
            vst<V>(f + (r0 + (long long)i * s + j) * C + cq, z);
        }
    }
}

// Form 3, reverse, per (node, column j, vector q).  dz left in df; dS[k][j] = sum_i W[i][k] dz[i][j] into its own buffer;
// colpart[node_pair[n] + j] = [ sum_i dz[i][j] | sum_k adj[k][j] dS[k][j] ] ([sum s][2 C]).  df is read back by the lane that wrote it.
template <int V>
__global__ __launch_bounds__(256) void unres2d_node_bwd(const float *__restrict__ f, float *df, const float *__restrict__ dvec,
                                                        const float *__restrict__ sizes, const float *__restrict__ adj, float *__restrict__ dS,
                                                        float *__restrict__ colpart, const int *__restrict__ node_s,
                                                        const long long *__restrict__ node_row, const long long *__restrict__ node_pair, int C,
                                                        float alpha, int nodes, int npw, int has_df) {
    __shared__ int off[kMaxPack + 1];
    const Run run = pack_run(off, node_s, nodes, npw, C / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, C / V);
        const int n = run.nb + x.j, s = node_s[n], j = x.pos, cq = x.cq;
        const long long r0 = node_row[n];
        const float *W = sizes + entry_off(s, C, C);
        Vf<V> dv = vzero<V>(), zs = vzero<V>(), ps = vzero<V>();
        if (dvec) dv = vld<V>(dvec + (long long)n * C + cq);
        for (int i = 0; i < s; ++i) {
            const long long o = (r0 + (long long)i * s + j) * C + cq;
            const Vf<V> d = dz_of<V>(f, df, o, dv, has_df, alpha);
            vadd(zs, d);
            vst<V>(df + o, d);
        }
        for (int k = 0; k < s; ++k) {
            Vf<V> g = vzero<V>();
            for (int i = 0; i < s; ++i) {
                const Vf<V> w = vld<V>(W + ((size_t)i * s + k) * C + cq), d = vld<V>(df + (r0 + (long long)i * s + j) * C + cq);
#pragma unroll
                for (int c = 0; c < V; ++c) g.v[c] += w.v[c] * d.v[c];
            }
            const long long row = r0 + (long long)k * s + j;
            const float av = adj[row];
#pragma unroll
            for (int c = 0; c < V; ++c) ps.v[c] += av * g.v[c];
            vst<V>(dS + row * C + cq, g);
        }
        float *cp = colpart + (node_pair[n] + j) * 2 * C;
        vst<V>(cp + cq, zs);
        vst<V>(cp + C + cq, ps);
    }
}

// Form 3: the entry of one size bucket over the nodes of chunk blockIdx.y, thread per element e of [ dW s^2 C | db C | dscalar C ]
// (Wp = s^2 C + 2 C floats per chunk): a filter element sums dz[i][j][c] S[k][j][c] over the chunk's nodes and j in order, the two
// vectors sum their column partials.  Lanes on c: coalesced.
__global__ __launch_bounds__(256) void unres2d_bucket_partials(const float *__restrict__ dz, const float *__restrict__ S,
                                                               const float *__restrict__ colpart, const int *__restrict__ bucket,
                                                               const long long *__restrict__ node_row, const long long *__restrict__ node_pair,
                                                               const long long *__restrict__ part_off, float *__restrict__ out, int C) {
    const BucketChunk bc = bucket_chunk(bucket, blockIdx.x, blockIdx.y, kUnSplit);
    const int s = bc.s, len = bc.len;
    const long long ss = (long long)s * s, Wf = ss * C, Wp = Wf + 2 * C;
    const long long r0 = len > 0 ? node_row[bc.n0] : 0, p0 = len > 0 ? node_pair[bc.n0] : 0;
    float *o = out + part_off[blockIdx.x] + (size_t)blockIdx.y * Wp;
    for (long long e = (long long)blockIdx.z * 256 + threadIdx.x; e < Wp; e += (long long)gridDim.z * 256) {
        float acc = 0.f;
        if (e < Wf) {
            const int pair = (int)(e / C), c = (int)(e - (long long)pair * C), i = pair / s, k = pair - i * s;
            for (int nn = 0; nn < len; ++nn) {
                const long long base = r0 + nn * ss;
                const float *zp = dz + (base + (long long)i * s) * C + c, *sp = S + (base + (long long)k * s) * C + c;
                for (int j = 0; j < s; ++j) acc += zp[(size_t)j * C] * sp[(size_t)j * C];
            }
        } else {
            const int cc = (int)(e - Wf);
            for (long long r = 0; r < (long long)len * s; ++r) acc += colpart[(p0 + r) * 2 * C + cc];
        }
        o[e] = acc;
    }
}

// Workgroup b < nbuckets: the bucket's chunks in order, `+=` into its per-size entry (the first Wd = fl s^2 + Cc floats of a chunk's
// partial are in the entry's order).  Workgroup nbuckets (form 3 only): dscalar += the last Cp floats over the buckets and chunks in order.
__global__ __launch_bounds__(256) void unres_grads_finish(const float *__restrict__ bp, const int *__restrict__ bucket,
                                                          const long long *__restrict__ part_off, float *__restrict__ dsizes,
                                                          float *__restrict__ dscalar, int fl, int Cc, int tail, int nbuckets) {
    if ((int)blockIdx.x < nbuckets) {
        const int s = bucket[3 * blockIdx.x];
        const long long Wd = (long long)fl * s * s + Cc, Wp = Wd + tail;
        float *out = dsizes + entry_off(s, fl, Cc);
        const float *in = bp + part_off[blockIdx.x];
        for (long long e = threadIdx.x; e < Wd; e += blockDim.x) {
            float t = 0.f;
            for (int k = 0; k < kUnSplit; ++k) t += in[k * Wp + e];
            out[e] += t;
        }
        return;
    }
    for (int c = threadIdx.x; c < tail; c += blockDim.x) {
        float t = 0.f;
        for (int b = 0; b < nbuckets; ++b) {
            const int s = bucket[3 * b];
            const long long Wd = (long long)fl * s * s + Cc, Wp = Wd + tail;
            for (int k = 0; k < kUnSplit; ++k) t += bp[part_off[b] + k * Wp + Wd + c];
        }
        dscalar[c] += t;
    }
}

}  // namespace

// f_l from f_{l-1}: one launch
gf_status smp_unrestricted_forward_level(gf_smp *s, int l, const float *scalar, const float *sizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int form = s->cfg.unrestricted, Cp = s->cfg.level_channels(l - 1);
    const int nodes = s->lay.level[l].nNodes, V = lane_vector(Cp);
    if (nodes == 0) return GF_OK;
    const RunGrid g = run_grid(s->lay.level[l], form == 3, Cp / V);
    const float alpha = s->cfg.level_slope();
    return with_lane_vector(V, [&](auto v) -> gf_status {
        if (form == 3)
            GF_LAUNCH(ctx, "unres2d_level_fwd", unres2d_fwd<v>, g.grid, dim3(256), 0, pv.f, sizes, scalar, d.adj, d.f, d.th_A, d.node_s, d.node_row,
                      d.th_child_ptr, d.th_src_row, d.th_src_s, d.th_pi_off, d.th_pi, Cp, alpha, nodes, g.npw);
        else
            GF_LAUNCH(ctx, "unres1d_level_fwd", unres1d_fwd<v>, g.grid, dim3(256), 0, pv.f, sizes, d.f, d.th_A, d.node_s, d.node_row, d.th_child_ptr,
                      d.th_src_row, d.th_pi_off, d.th_pi, Cp, form, alpha, nodes, g.npw);
        return GF_OK;
    });
}

// dz and dS per node, the per-size gradients (and dscalar_l) over the buckets, then df_{l-1}.  (scalar_l itself and wgrad_done: not needed)
gf_status smp_unrestricted_backward_level(gf_smp *s, int l, const float *, const float *sizes, float *dscalar, float *dsizes, const float *node_df,
                                          bool rows_too, gf_status (*)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const int form = s->cfg.unrestricted, Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);
    const int nodes = h.nNodes, V = lane_vector(Cp);
    const int nbuckets = (int)(h.th_bucket.size() / 3);
    const float alpha = s->cfg.level_slope();
    if (!node_df && !rows_too) return fail(ctx, GF_ERR_INVALID, "unrestricted level %d: no gradient to back-propagate", l);
    if (nodes > 0) {
        const RunGrid g = run_grid(h, form == 3, Cp / V);
        const gf_status st = with_lane_vector(V, [&](auto v) -> gf_status {
            if (form == 3)
                GF_LAUNCH(ctx, "unres2d_node_bwd", unres2d_node_bwd<v>, g.grid, dim3(256), 0, d.f, d.df, node_df, sizes, d.adj, d.Q, d.th_node, d.node_s,
                          d.node_row, d.node_pair, Cp, alpha, nodes, g.npw, rows_too ? 1 : 0);
            else
                GF_LAUNCH(ctx, "unres1d_node_bwd", unres1d_node_bwd<v>, g.grid, dim3(256), 0, d.f, d.df, node_df, sizes, d.Q, d.node_s, d.node_row, Cp,
                          form, alpha, nodes, g.npw, rows_too ? 1 : 0);
            return GF_OK;
        });
        if (st != GF_OK) return st;
        const long long smax = h.buckets.back().s;   // (buckets ascend by size) tiles of the largest entry, at most 64
        if (form == 3) {
            const long long tiles = (smax * smax * Cp + 2 * Cp + 255) / 256;
            GF_LAUNCH(ctx, "unres2d_bucket_partials", unres2d_bucket_partials, dim3((unsigned)nbuckets, kUnSplit, (unsigned)(tiles > 64 ? 64 : tiles)),
                      dim3(256), 0, d.df, d.th_A, d.th_node, d.th_bucket, d.node_row, d.node_pair, d.un_part_off, d.part2d, Cp);
        } else {
            const long long tiles = (form * smax * smax + Cc + 15) / 16;
            GF_LAUNCH(ctx, "unres1d_bucket_partials", unres1d_bucket_partials, dim3((unsigned)nbuckets, kUnSplit, (unsigned)(tiles > 64 ? 64 : tiles)),
                      dim3(256), 0, d.df, d.th_A, d.th_bucket, d.node_row, d.un_part_off, d.part2d, Cp, form);
        }
        GF_LAUNCH(ctx, "unres_grads_finish", unres_grads_finish, dim3((unsigned)nbuckets + (form == 3 ? 1 : 0)), dim3(256), 0, d.part2d, d.th_bucket,
                  d.un_part_off, dsizes, dscalar, form == 3 ? Cp : form, Cc, form == 3 ? Cp : 0, nbuckets);
    }
    return smp_field_gather_down(s, l, d.Q, Cp, form == 3, "unres_gather_bwd");
}

}  // namespace gf
