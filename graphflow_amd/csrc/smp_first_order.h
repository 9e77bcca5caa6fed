// smp_first_order.h -- what the first-order levels share (smp_level_theta.hip: SMP_theta; smp_level_1d.hip: SMP_1D, SMP_1D_ver2,
// SMP_1D_ver3): the 4 / 2 / 1-float lane vector, the packing of runs of consecutive nodes into a workgroup, the per-size entry.
#ifndef GF_SMP_FIRST_ORDER_H_INCLUDED
#define GF_SMP_FIRST_ORDER_H_INCLUDED

#include "smp_internal.h"

namespace gf {
namespace first_order {

constexpr int kThetaMaxPack = 64;      // nodes per workgroup: one wave builds their item offsets

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

// the per-size block of a level: entry s at (s - 1) * (2 + Cc) = lambda1_s, lambda2_s, b_s[Cc]
__device__ __forceinline__ const float *size_entry(const float *sizes, int s, int Cc) { return sizes + (size_t)(s - 1) * (2 + Cc); }

inline int theta_vec(int Cc) { return Cc % 4 == 0 ? 4 : Cc % 2 == 0 ? 2 : 1; }
// nodes per workgroup: ~256 lanes' worth of (position, vector) items, at most kThetaMaxPack nodes
inline int theta_pack(double items_per_node) {
    const int k = (int)(256.0 / (items_per_node > 1.0 ? items_per_node : 1.0));
    return k < 1 ? 1 : k > kThetaMaxPack ? kThetaMaxPack : k;
}
inline unsigned grid_for(size_t total) {
    const size_t blocks = (total + 255) / 256;
    return (unsigned)(blocks > 1048576 ? 1048576 : (blocks == 0 ? 1 : blocks));
}

}  // namespace first_order

// smp_level_theta.hip: the per-size gradients from acc [nodes][3 Cc] (sum_i dz[i] | the dlambda1 terms | the dlambda2 terms) over the size
// buckets, `+=` into dsizes; K [2 Cp][Cc] -> Kh [Cp][2 Cc] and Kt [2 Cc][Cp]; dK += dKh rearranged
gf_status smp_theta_size_grads(gf_ctx *ctx, const float *acc, const int *bucket, int nbuckets, float *dsizes, int Cc);
gf_status smp_theta_weight_views(gf_ctx *ctx, const float *K, float *Kh, float *Kt, int Cp, int Cc);
gf_status smp_theta_wgrad_fold(gf_ctx *ctx, const float *dKh, float *dK, int Cp, int Cc);
}  // namespace gf
#endif
