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
#include "smp_first_order.h"

namespace gf {
using namespace first_order;
namespace {

constexpr int kUnSplit = gfsmp::kUnrestrictedSplit;   // node chunks per size bucket in the reduction of the filter gradients
constexpr int kUnLds = 2048;                          // floats of S a workgroup of the first-order forward keeps in LDS
constexpr int kUnGroup = 16;                          // lanes on one element of a first-order filter gradient

// floats in front of entry s of a per-size block: sum over t < s of (fl t^2 + Cc)
__device__ __forceinline__ size_t entry_off(int s, int fl, int Cc) {
    const size_t t = (size_t)(s - 1);
    return (size_t)fl * (t * (t + 1) * (2 * t + 1) / 6) + t * (size_t)Cc;
}

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
    for (int c = 0; c < V; ++c) z.v[c] = z.v[c] > 0.f ? z.v[c] : alpha * z.v[c];
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
    __shared__ int off[kThetaMaxPack + 1];
    __shared__ __align__(16) float lds[kUnLds];
    const int nb = blockIdx.x * npw;
    const int np = nodes - nb < npw ? nodes - nb : npw, Qc = Cp / V, Cc = halves * Cp;
    int cnt = 0;
    if ((int)threadIdx.x < np) cnt = node_s[nb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, np);
    const int total = off[np];
    const bool in_lds = (long long)total * V <= kUnLds;
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int j = pack_find(off, np, it);
        const int n = nb + j;
        const int r = it - off[j], k = r / Qc, cq = (r - k * Qc) * V;
        Vf<V> a = vzero<V>();
        for (long long e = child_ptr[n]; e < child_ptr[n + 1]; ++e) {
            const int p = pi[pi_off[e] + k];
            if (p < 0) continue;
            vadd(a, vld<V>(fp + (src_row[e] + p) * Cp + cq));
        }
        vst<V>(S + (node_row[n] + k) * Cp + cq, a);
        if (in_lds) vst<V>(lds + (size_t)it * V, a);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int j = pack_find(off, np, it);
        const int n = nb + j, s = node_s[n];
        const int r = it - off[j], i = r / Qc, cq = (r - i * Qc) * V;
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
    __shared__ int off[kThetaMaxPack + 1];
    const int nb = blockIdx.x * npw;
    const int np = nodes - nb < npw ? nodes - nb : npw, Qc = Cp / V, Cc = halves * Cp;
    int cnt = 0;
    if ((int)threadIdx.x < np) cnt = node_s[nb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int j = pack_find(off, np, it);
        const int n = nb + j;
        const int r = it - off[j], i = r / Qc, cq = (r - i * Qc) * V;
        for (int h = 0; h < halves; ++h) {
            const long long o = (node_row[n] + i) * Cc + h * Cp + cq;
            const Vf<V> fv = vld<V>(f + o);
            Vf<V> d = vzero<V>();
            if (dvec) d = vld<V>(dvec + (long long)n * Cc + h * Cp + cq);
            if (has_df) vadd(d, vld<V>(df + o));
#pragma unroll
            for (int c = 0; c < V; ++c) d.v[c] *= fv.v[c] > 0.f ? 1.f : alpha;
            vst<V>(df + o, d);
        }
    }
    __syncthreads();
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int j = pack_find(off, np, it);
        const int n = nb + j, s = node_s[n];
        const int r = it - off[j], k = r / Qc, cq = (r - k * Qc) * V;
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
    const int s = bucket[3 * blockIdx.x], n0 = bucket[3 * blockIdx.x + 1], cnt = bucket[3 * blockIdx.x + 2];
    const int chunk = (cnt + kUnSplit - 1) / kUnSplit;
    int len = cnt - chunk * (int)blockIdx.y;
    len = len < 0 ? 0 : len > chunk ? chunk : len;
    const int Cc = halves * Cp, ss = s * s, Wd = halves * ss + Cc;
    const long long r0 = len > 0 ? node_row[n0 + chunk * (int)blockIdx.y] : 0;
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
    __shared__ int off[kThetaMaxPack + 1];
    const int nb = blockIdx.x * npw;
    const int np = nodes - nb < npw ? nodes - nb : npw, Qc = C / V;
    int cnt = 0;
    if ((int)threadIdx.x < np) cnt = node_s[nb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int kk = pack_find(off, np, it);
        const int n = nb + kk, s = node_s[n];
        const int r = it - off[kk], j = r / Qc, cq = (r - j * Qc) * V;
        const long long r0 = node_row[n], e0 = child_ptr[n], e1 = child_ptr[n + 1];
        const float *W = sizes + entry_off(s, C, C);
        const Vf<V> bt = vld<V>(W + (size_t)s * s * C + cq), sc = vld<V>(scalar + cq);
        for (int i = 0; i < s; ++i) {
            Vf<V> a = vzero<V>();
            for (long long e = e0; e < e1; ++e) {
                const short *pe = pi + pi_off[e];
                const int p = pe[i], q = pe[j];
                if (p < 0 || q < 0) continue;
                vadd(a, vld<V>(fp + (src_row[e] + (long long)p * src_s[e] + q) * C + cq));
            }
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
            for (int c = 0; c < V; ++c) z.v[c] = z.v[c] > 0.f ? z.v[c] : alpha * z.v[c];
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
    __shared__ int off[kThetaMaxPack + 1];
    const int nb = blockIdx.x * npw;
    const int np = nodes - nb < npw ? nodes - nb : npw, Qc = C / V;
    int cnt = 0;
    if ((int)threadIdx.x < np) cnt = node_s[nb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int kk = pack_find(off, np, it);
        const int n = nb + kk, s = node_s[n];
        const int r = it - off[kk], j = r / Qc, cq = (r - j * Qc) * V;
        const long long r0 = node_row[n];
        const float *W = sizes + entry_off(s, C, C);
        Vf<V> dv = vzero<V>(), zs = vzero<V>(), ps = vzero<V>();
        if (dvec) dv = vld<V>(dvec + (long long)n * C + cq);
        for (int i = 0; i < s; ++i) {
            const long long o = (r0 + (long long)i * s + j) * C + cq;
            const Vf<V> fv = vld<V>(f + o);
            Vf<V> d = dv;
            if (has_df) vadd(d, vld<V>(df + o));
#pragma unroll
            for (int c = 0; c < V; ++c) {
                d.v[c] *= fv.v[c] > 0.f ? 1.f : alpha;
                zs.v[c] += d.v[c];
            }
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
    const int s = bucket[3 * blockIdx.x], n0 = bucket[3 * blockIdx.x + 1], cnt = bucket[3 * blockIdx.x + 2];
    const int chunk = (cnt + kUnSplit - 1) / kUnSplit;
    int len = cnt - chunk * (int)blockIdx.y;
    len = len < 0 ? 0 : len > chunk ? chunk : len;
    const long long ss = (long long)s * s, Wf = ss * C, Wp = Wf + 2 * C;
    const long long r0 = len > 0 ? node_row[n0 + chunk * (int)blockIdx.y] : 0, p0 = len > 0 ? node_pair[n0 + chunk * (int)blockIdx.y] : 0;
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

// Reverse gather of dS ([rows of level l][Cp]) into df_{l-1}: source nodes [blockIdx.x * npw, + npw) of level l - 1.  SQ = false: items
// (node, position p, vector); SQ = true: items (node, column q, vector) walking the source's rows p, inv applied to both indices.
template <int V, bool SQ>
__global__ __launch_bounds__(256) void unres_gather_bwd(const float *__restrict__ dS, float *__restrict__ out, const int *__restrict__ prev_s,
                                                        const long long *__restrict__ prev_row, const long long *__restrict__ cons_ptr,
                                                        const long long *__restrict__ cons_row, const int *__restrict__ cons_s,
                                                        const long long *__restrict__ inv_off, const short *__restrict__ inv, int Cp, int nodes,
                                                        int npw) {
    __shared__ int off[kThetaMaxPack + 1];
    const int wb = blockIdx.x * npw;
    const int np = nodes - wb < npw ? nodes - wb : npw, Qc = Cp / V;
    int cnt = 0;
    if ((int)threadIdx.x < np) cnt = prev_s[wb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int k = pack_find(off, np, it);
        const int w = wb + k, sw = prev_s[w];
        const int r = it - off[k], q = r / Qc, cq = (r - q * Qc) * V;
        const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1], r0 = prev_row[w];
        if (!SQ) {
            Vf<V> g = vzero<V>();
            for (long long c = c0; c < c1; ++c) {
                const int i = inv[inv_off[c] + q];
                if (i < 0) continue;
                vadd(g, vld<V>(dS + (cons_row[c] + i) * Cp + cq));
            }
            vst<V>(out + (r0 + q) * Cp + cq, g);
            continue;
        }
        for (int p = 0; p < sw; ++p) {
            Vf<V> g = vzero<V>();
            for (long long c = c0; c < c1; ++c) {
                const short *ie = inv + inv_off[c];
                const int i = ie[p], j = ie[q];
                if (i < 0 || j < 0) continue;
                vadd(g, vld<V>(dS + (cons_row[c] + (long long)i * cons_s[c] + j) * Cp + cq));
            }
            vst<V>(out + (r0 + (long long)p * sw + q) * Cp + cq, g);
        }
    }
}

// items (position or column, vector) of an average node of level h: sum s / nodes * Cp / V
inline double items_per_node(const gfsmp::LevelLayout &h, bool sq, int Qc) {
    if (h.nNodes == 0) return 1.0;
    const double cols = sq ? (double)(h.node_pair.back() + h.node_s.back()) : (double)h.rows;
    return cols / (double)h.nNodes * Qc;
}

}  // namespace

// f_l from f_{l-1}: one launch
gf_status smp_unrestricted_forward_level(gf_smp *s, int l, const float *scalar, const float *sizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int form = s->cfg.unrestricted, Cp = s->cfg.level_channels(l - 1);
    const int nodes = s->lay.level[l].nNodes, V = theta_vec(Cp);
    if (nodes == 0) return GF_OK;
    const int npw = theta_pack(items_per_node(s->lay.level[l], form == 3, Cp / V));
    const dim3 grid((unsigned)((nodes + npw - 1) / npw));
    const float alpha = s->cfg.level_slope();
#define GF_UN_FWD(V)                                                                                                                                  \
    if (form == 3)                                                                                                                                    \
        GF_LAUNCH(ctx, "unres2d_level_fwd", unres2d_fwd<V>, grid, dim3(256), 0, pv.f, sizes, scalar, d.adj, d.f, d.th_A, d.node_s, d.node_row,        \
                  d.th_child_ptr, d.th_src_row, d.th_src_s, d.th_pi_off, d.th_pi, Cp, alpha, nodes, npw);                                             \
    else                                                                                                                                              \
        GF_LAUNCH(ctx, "unres1d_level_fwd", unres1d_fwd<V>, grid, dim3(256), 0, pv.f, sizes, d.f, d.th_A, d.node_s, d.node_row, d.th_child_ptr,       \
                  d.th_src_row, d.th_pi_off, d.th_pi, Cp, form, alpha, nodes, npw)
    switch (V) {
        case 4: GF_UN_FWD(4); break;
        case 2: GF_UN_FWD(2); break;
        default: GF_UN_FWD(1); break;
    }
#undef GF_UN_FWD
    return GF_OK;
}

// dz and dS per node, the per-size gradients (and dscalar_l) over the buckets, then df_{l-1}
gf_status smp_unrestricted_backward_level(gf_smp *s, int l, const float *sizes, float *dscalar, float *dsizes, const float *node_df, bool rows_too) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const int form = s->cfg.unrestricted, Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);
    const int nodes = h.nNodes, np = s->lay.level[l - 1].nNodes, V = theta_vec(Cp);
    const int nbuckets = (int)(h.th_bucket.size() / 3);
    const float alpha = s->cfg.level_slope();
    if (!node_df && !rows_too) return fail(ctx, GF_ERR_INVALID, "unrestricted level %d: no gradient to back-propagate", l);
    if (nodes > 0) {
        const int npw = theta_pack(items_per_node(h, form == 3, Cp / V));
        const dim3 grid((unsigned)((nodes + npw - 1) / npw));
#define GF_UN_NODE(V)                                                                                                                                 \
    if (form == 3)                                                                                                                                    \
        GF_LAUNCH(ctx, "unres2d_node_bwd", unres2d_node_bwd<V>, grid, dim3(256), 0, d.f, d.df, node_df, sizes, d.adj, d.Q, d.th_node, d.node_s,       \
                  d.node_row, d.node_pair, Cp, alpha, nodes, npw, rows_too ? 1 : 0);                                                                  \
    else                                                                                                                                              \
        GF_LAUNCH(ctx, "unres1d_node_bwd", unres1d_node_bwd<V>, grid, dim3(256), 0, d.f, d.df, node_df, sizes, d.Q, d.node_s, d.node_row, Cp, form,   \
                  alpha, nodes, npw, rows_too ? 1 : 0)
        switch (V) {
            case 4: GF_UN_NODE(4); break;
            case 2: GF_UN_NODE(2); break;
            default: GF_UN_NODE(1); break;
        }
#undef GF_UN_NODE
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
    if (np > 0) {
        const int npw = theta_pack(items_per_node(s->lay.level[l - 1], form == 3, Cp / V));
        const dim3 grid((unsigned)((np + npw - 1) / npw));
#define GF_UN_BWD(V)                                                                                                                                  \
    if (form == 3)                                                                                                                                    \
        GF_LAUNCH(ctx, "unres_gather_bwd", (unres_gather_bwd<V, true>), grid, dim3(256), 0, d.Q, pv.df, pv.node_s, pv.node_row, d.th_cons_ptr,        \
                  d.th_cons_row, d.th_cons_s, d.th_inv_off, d.th_inv, Cp, np, npw);                                                                   \
    else                                                                                                                                              \
        GF_LAUNCH(ctx, "unres_gather_bwd", (unres_gather_bwd<V, false>), grid, dim3(256), 0, d.Q, pv.df, pv.node_s, pv.node_row, d.th_cons_ptr,       \
                  d.th_cons_row, d.th_cons_s, d.th_inv_off, d.th_inv, Cp, np, npw)
        switch (V) {
            case 4: GF_UN_BWD(4); break;
            case 2: GF_UN_BWD(2); break;
            default: GF_UN_BWD(1); break;
        }
#undef GF_UN_BWD
    }
    return GF_OK;
}

}  // namespace gf
