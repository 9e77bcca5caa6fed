// smp_field_level.h -- what the field levels share: the levels on the th_* tables of smp_prep.h with lanes on (node, position or column,
// channel vector) -- smp_level_theta.hip, smp_level_1d.hip, smp_level_2d.hip, smp_level_2d_ver5.hip, smp_level_unrestricted.hip, and
// smp_field_level.hip with the kernels more than one of them launches.  Device side: the 4 / 2 / 1-float lane vector, the packing of runs
// of consecutive nodes into a workgroup, the child gathers, LeakyReLU and dz, the per-size entries, the chunk of a size bucket.  Host
// side: the lane-vector dispatch and the grid of a packed run.
#ifndef GF_SMP_FIELD_LEVEL_H_INCLUDED
#define GF_SMP_FIELD_LEVEL_H_INCLUDED

#include <type_traits>

#include "smp_internal.h"

namespace gf {
namespace field_level {

constexpr int kMaxPack = 64;      // nodes per workgroup: one wave builds their item offsets

template <int V>
struct Vf {
    float v[V];
};
template <int V>
__device__ __forceinline__ Vf<V> vzero() {
    Vf<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = 0.f;
    return r;
}
template <int V>
__device__ __forceinline__ Vf<V> vld(const float *p) {   // (p is V-float aligned: rows are multiples of Cc, V | Cc)
    Vf<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        r.v[0] = t.x, r.v[1] = t.y;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V>
__device__ __forceinline__ void vst(float *p, const Vf<V> &r) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else if constexpr (V == 2) *reinterpret_cast<float2 *>(p) = make_float2(r.v[0], r.v[1]);
    else *p = r.v[0];
}
template <int V>
__device__ __forceinline__ void vadd(Vf<V> &a, const Vf<V> &b) {
#pragma unroll
    for (int k = 0; k < V; ++k) a.v[k] += b.v[k];
}

// off[0 .. np] = exclusive prefix of cnt over the workgroup's np <= 64 nodes (wave 0), then a barrier
__device__ __forceinline__ void pack_offsets(int *off, int cnt, int np) {
    if (threadIdx.x < 64) {
        int v = (int)threadIdx.x < np ? cnt : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d, 64);
            if ((int)threadIdx.x >= d) v += u;
        }
        off[threadIdx.x + 1] = v;
        if (threadIdx.x == 0) off[0] = 0;
    }
    __syncthreads();
}
__device__ __forceinline__ int pack_find(const int *off, int np, int i) {   // the j with off[j] <= i < off[j + 1]
    int lo = 0, hi = np - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// The packed run of a workgroup: nodes [nb, nb + np) of the level, node j's items (position or column, vector q) at [off[j], off[j + 1])
// of the run's `total`, Qc = channels / V vectors per position.  off: kMaxPack + 1 ints of LDS.  Ends in a barrier.
struct Run {
    int nb, np, total;
};
__device__ __forceinline__ Run pack_run(int *off, const int *__restrict__ node_s, int nodes, int npw, int Qc) {
    Run r;
    r.nb = blockIdx.x * npw;
    r.np = nodes - r.nb < npw ? nodes - r.nb : npw;
    int cnt = 0;
    if ((int)threadIdx.x < r.np) cnt = node_s[r.nb + threadIdx.x] * Qc;
    pack_offsets(off, cnt, r.np);
    r.total = off[r.np];
    return r;
}
struct Item {
    int j, pos, cq;   // node nb + j of the run, its position (or column), the first channel of the vector
};
template <int V>
__device__ __forceinline__ Item pack_item(const int *off, int np, int it, int Qc) {
    Item x;
    x.j = pack_find(off, np, it);
    const int r = it - off[x.j];
    x.pos = r / Qc;
    x.cq = (r - x.pos * Qc) * V;
    return x;
}

// The child gathers over the edges [e0, e1) of a node, children ascending; a child whose field misses the position adds nothing.
// First order: sum of src[src_row[e] + pi_e(i)][col ..], src rows `stride` floats apart.
template <int V>
__device__ __forceinline__ Vf<V> gather_row(const float *__restrict__ src, int stride, int col, long long e0, long long e1,
                                            const long long *__restrict__ src_row, const long long *__restrict__ pi_off,
                                            const short *__restrict__ pi, int i) {
    Vf<V> a = vzero<V>();
    for (long long e = e0; e < e1; ++e) {
        const int p = pi[pi_off[e] + i];
        if (p >= 0) vadd(a, vld<V>(src + (src_row[e] + p) * stride + col));
    }
    return a;
}
// Second order: sum of src[src_row[e] + pi_e(i) s_e + pi_e(j)][cq ..], rows C floats apart (the caller adds scalar * adj)
template <int V>
__device__ __forceinline__ Vf<V> gather_pair(const float *__restrict__ src, int C, int cq, long long e0, long long e1,
                                             const long long *__restrict__ src_row, const int *__restrict__ src_s,
                                             const long long *__restrict__ pi_off, const short *__restrict__ pi, int i, int j) {
    Vf<V> a = vzero<V>();
    for (long long e = e0; e < e1; ++e) {
        const short *pe = pi + pi_off[e];
        const int p = pe[i], q = pe[j];
        if (p < 0 || q < 0) continue;
        vadd(a, vld<V>(src + (src_row[e] + (long long)p * src_s[e] + q) * C + cq));
    }
    return a;
}

__device__ __forceinline__ float lrelu(float z, float alpha) { return z > 0.f ? z : alpha * z; }
__device__ __forceinline__ float lrelu_slope(float f, float alpha) { return f > 0.f ? 1.f : alpha; }   // lrelu'(z) from the kept f = lrelu(z)
// dz = (df (has_df) + dv) * lrelu'(f) of the vector at float offset o of f and df, dv = the read-out's gradient of the node (or zero)
template <int V>
__device__ __forceinline__ Vf<V> dz_of(const float *f, const float *df, long long o, Vf<V> d, int has_df, float alpha) {
    const Vf<V> fv = vld<V>(f + o);
    if (has_df) vadd(d, vld<V>(df + o));
#pragma unroll
    for (int k = 0; k < V; ++k) d.v[k] *= lrelu_slope(fv.v[k], alpha);
    return d;
}

// The per-size entries of a level's block, side by side.  First order: (lambda1_s, lambda2_s, b_s[Cc]); steerable: (lambda1_s[Cp],
// lambda2_s[Cp], b_s[Cc]); SMP_2D_ver5: the same at Cp = Cc = C; unrestricted: the floats in front of entry s = sum over t < s of
// (fl t^2 + Cc), fl = 1, 2, Cp floats per filter element.
__device__ __forceinline__ const float *size_entry(const float *sizes, int s, int Cc) { return sizes + (size_t)(s - 1) * (2 + Cc); }
__device__ __forceinline__ const float *size_entry_2d(const float *sizes, int s, int Cp, int Cc) { return sizes + (size_t)(s - 1) * (2 * Cp + Cc); }
__device__ __forceinline__ const float *size_entry_v5(const float *sizes, int s, int C) { return sizes + (size_t)(s - 1) * (3 * C); }
__device__ __forceinline__ size_t entry_off(int s, int fl, int Cc) {
    const size_t t = (size_t)(s - 1);
    return (size_t)fl * (t * (t + 1) * (2 * t + 1) / 6) + t * (size_t)Cc;
}

// Chunk `chunk` of `split` of size bucket b (s, first node, count: its nodes are contiguous): size, first node and node count (0: empty)
struct BucketChunk {
    int s, n0, len;
};
__device__ __forceinline__ BucketChunk bucket_chunk(const int *__restrict__ bucket, int b, int chunk, int split) {
    const int cnt = bucket[3 * b + 2], per = (cnt + split - 1) / split, len = cnt - per * chunk;
    return {bucket[3 * b], bucket[3 * b + 1] + per * chunk, len < 0 ? 0 : len > per ? per : len};
}

inline int lane_vector(int C) { return C % 4 == 0 ? 4 : C % 2 == 0 ? 2 : 1; }
// f(std::integral_constant<int, V>) for the lane vector V = 4 / 2 / 1: the one place a run-time V picks a kernel instantiation
template <typename F>
inline gf_status with_lane_vector(int V, F &&f) {
    switch (V) {
        case 4: return f(std::integral_constant<int, 4>());
        case 2: return f(std::integral_constant<int, 2>());
        default: return f(std::integral_constant<int, 1>());
    }
}
// nodes per workgroup: ~256 lanes' worth of (position, vector) items, at most kMaxPack nodes
inline int nodes_per_group(double items_per_node) {
    const int k = (int)(256.0 / (items_per_node > 1.0 ? items_per_node : 1.0));
    return k < 1 ? 1 : k > kMaxPack ? kMaxPack : k;
}
// the packed runs of level h: items (position -- square: column --, vector) of Qc vectors each; npw nodes per workgroup, `grid` workgroups
struct RunGrid {
    int npw;
    dim3 grid;
};
inline RunGrid run_grid(const gfsmp::LevelLayout &h, bool square, int Qc) {
    if (h.nNodes == 0) return {1, dim3(0)};
    const double cols = square ? (double)(h.node_pair.back() + h.node_s.back()) : (double)h.rows;   // sum s
    const int npw = nodes_per_group(cols / (double)h.nNodes * Qc);
    return {npw, dim3((unsigned)((h.nNodes + npw - 1) / npw))};
}
inline unsigned grid_for(size_t total) {
    const size_t blocks = (total + 255) / 256;
    return (unsigned)(blocks > 1048576 ? 1048576 : (blocks == 0 ? 1 : blocks));
}

}  // namespace field_level

// smp_field_level.hip: the per-size gradients from acc [nodes][3 Cc] (sum_i dz[i] | the dlambda1 terms | the dlambda2 terms) over the size
// buckets, `+=` into dsizes; K [2 Cp][Cc] -> Kh [Cp][2 Cc] and Kt [2 Cc][Cp]; dK += dKh rearranged
gf_status smp_field_size_grads(gf_ctx *ctx, const float *acc, const int *bucket, int nbuckets, float *dsizes, int Cc);
gf_status smp_field_weight_views(gf_ctx *ctx, const float *K, float *Kh, float *Kt, int Cp, int Cc);
gf_status smp_field_wgrad_fold(gf_ctx *ctx, const float *dKh, float *dK, int Cp, int Cc);
// df_{l-1} gathered from dS of level l (rows `stride` floats apart, the first C_{l-1} columns); square: both indices through inv
gf_status smp_field_gather_down(gf_smp *s, int l, const float *dS, int stride, bool square, const char *timer);
// smp_level_1d.hip: the reverse gather of a first-order level at Cp channels per half, under the caller's timer name (SMP_theta's level
// launches it too).  out = df_{l-1} [rows][Cp], or split: dG [rows][2 Cp]
gf_status smp_1d_gather_bwd(gf_smp *s, int l, const char *timer, const float *sizes, int Cp, int concat, bool split, float *out);
}  // namespace gf
#endif
