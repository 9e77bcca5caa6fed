// smp_vertex_level.h -- what the vertex levels share: the levels that keep one vector per vertex and level, lanes in groups of G on a
// vertex's channels -- smp_level_neighbourhood.hip, smp_level_gru.hip, smp_level_distance.hip, smp_level_third.hip,
// smp_level_readouts.hip, smp_level_rowlist.hip, smp_level_covariant.hip, and smp_vertex_level.hip with the kernel and the host checks more
// than one of them uses.  Device side: the workgroup of four waves, the odd row stride of the LDS images, the sums and the maximum across
// a lane group, the product rounded on its own, a workgroup's vertex slots, the lane-0 tail of a read-out.  Host side: the shape and list
// checks of the stand-alone operators, the tail of a forward sweep, the read-outs' dW, and the neighbourhood level's three launches on
// operand sets (the gated and the distance level launch them too).
#ifndef GF_SMP_VERTEX_LEVEL_H_INCLUDED
#define GF_SMP_VERTEX_LEVEL_H_INCLUDED

#include <type_traits>

#include "smp_internal.h"

namespace gf {
namespace vertex_level {

constexpr int kBlock = 256;   // four waves

// the row stride of the transposed LDS images (smp_neighbourhood_lds_bytes): odd, so their transposing stores hit 32 different banks
__host__ __device__ inline int row_stride(int H) { return H | 1; }

__device__ __forceinline__ float group_sum(float v, int G) {   // every lane of the group gets the same bits (a + b == b + a)
    for (int d = G >> 1; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float group_max(float v, int G) {
    for (int d = G >> 1; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return group_sum(v, 64); }

// a * b rounded on its own: the subtraction that follows must not fuse it into an fma (one member: A Tt - a T has to be exactly 0)
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// a workgroup's vertex slots: slot = one group of G lanes, kBlock / G of them; it takes vertices vbase + it + slot, it = 0, slots, .. < vpg
struct Slot {
    int slot, slots, c0;
};
__device__ __forceinline__ Slot slot_of(int G) {
    const int lane = threadIdx.x & 63, per_wave = 64 / G;
    return {(int)(threadIdx.x >> 6) * per_wave + lane / G, kBlock / G, lane % G};
}

// The tail of a read-out of one wave per molecule (or pair) m: lane 0 stores the prediction `part` (a variable: read more than once), the
// squared loss and dy.  A macro on purpose.  As a __forceinline__ function its null tests of `target` and `loss` reach the kernel only
// when the inliner runs, after the kernel's own code has been through its first clean-up, and nbh_readout and pair_readout then come
// out with another block order and one register move more or less than the text written out gives (NOTES.md).
#define GF_STORE_PREDICTION(m, part, target, yhat, loss, dy)                        \
    do {                                                                            \
        if (threadIdx.x == 0) {                                                     \
            const float t__ = (target) ? (target)[m] : 0.f;                         \
            (yhat)[m] = (part);                                                     \
            if (loss) (loss)[m] = 0.5f * ((part) - t__) * ((part) - t__);           \
            (dy)[m] = (part) - t__; /* SquaredLoss::backward */                     \
        }                                                                           \
    } while (0)

// H, nV and the largest accepted rounds of a stand-alone call (an operator without rounds passes 0)
inline gf_status check_shape(gf_ctx *ctx, const char *who, int H, int max_channels, int nV, int rounds) {
    if (H < 1 || H > max_channels) return fail(ctx, GF_ERR_INVALID, "%s: %d channels (1 .. %d)", who, H, max_channels);
    if (nV < 1 || rounds < 0 || rounds > 65536) return fail(ctx, GF_ERR_INVALID, "%s: %d vertices, %d rounds", who, nV, rounds);
    return GF_OK;
}

// The lists of a stand-alone call, checked on the host (smp_vertex_level.hip; one blocking copy each: these are test operators).
// check_list: ptr [n + 1] starts at 0 and never decreases, every member lies in [0, bound); *longest (optional) = its longest entry.
// check_ptr: a 32-bit prefix-sum table (mol_ptr, graph_ptr): from 0, never decreasing, its last entry at most `bound` rows.
// check_members: every one of the n device ints lies in [0, bound).
gf_status check_list(gf_ctx *ctx, const char *who, const char *what, const long long *ptr, const int *idx, int n, int bound,
                     long long *longest = nullptr);
gf_status check_ptr(gf_ctx *ctx, const char *who, const char *what, const int *ptr, int n, int bound);
gf_status check_members(gf_ctx *ctx, const char *who, const char *what, const int *idx, size_t n, int bound);

// The tail of a forward sweep: s->yhat [nMol] and s->g [nMol][feature_width] to the caller's buffers where given, and the handle's marks
inline gf_status finish_forward(gf_smp *s, bool has_targets, float *predict, float *graph_feature, size_t feature_width) {
    gf_ctx *ctx = s->ctx;
    const size_t nMol = (size_t)s->lay.nMol;
    if (predict) GF_HIP_TRY(ctx, hipMemcpyAsync(predict, s->yhat, sizeof(float) * nMol, hipMemcpyDeviceToDevice, ctx->stream));
    if (graph_feature)
        GF_HIP_TRY(ctx, hipMemcpyAsync(graph_feature, s->g, sizeof(float) * nMol * feature_width, hipMemcpyDeviceToDevice, ctx->stream));
    s->bwd_consumed = false;
    s->forwarded = true;
    s->has_targets = has_targets;
    mark_used(s);
    return GF_OK;
}

}  // namespace vertex_level

// smp_vertex_level.hip: dW[c] += sum_m dy[m] g[m][c], c < width, over the n molecules (or pairs) under the caller's timer name
gf_status smp_vertex_readout_dW(gf_ctx *ctx, const char *timer, int width, int n, const float *dy, const float *g, float *dW);
// smp_level_neighbourhood.hip: the launches of its three level kernels on `nsets` operand sets (1 or 2; the sets of include/gf_hip.h;
// blockIdx.y picks the set, one set is given to the kernel twice).  pairs: the RisiLayer2D instantiation; rounds = 0: the level's own
// vertices per workgroup.  The gated level's level 0 and reverse gather and a distance handle's two channels are these launches.
gf_status smp_neighbourhood_fwd(gf_ctx *ctx, bool pairs, int H, int nV, int rounds, const gf_nbh_fwd_set *sets, int nsets, const long long *ptr,
                                const int *idx);
gf_status smp_neighbourhood_node(gf_ctx *ctx, bool pairs, int H, int nV, int rounds, const gf_nbh_node_set *sets, int nsets, const float *dy,
                                 const int *vmol);
gf_status smp_neighbourhood_gather(gf_ctx *ctx, bool pairs, int H, int nV, const long long *tptr, const int *tidx, const gf_nbh_gather_set *sets,
                                   int nsets);
}  // namespace gf
#endif
