// smp_optimisers.hip -- the reference's remaining optimisers and its regularisers on flat fp32 device buffers:
//   SGD::Learn(lr, nBatch)          GraphFlow/SGD.h:44-50               no state
//   AdaMax::Learn(alpha, nBatch)    GraphFlow/AdaMax.h:97-122           first_order [n] fp32, infinity_norm [nBlocks] double, beta1_t (host)
//   AdaDelta::Learn(alpha, nBatch)  GraphFlow/AdaDelta.h:90-112         E[g^2], E[dx^2] [n] fp32; alpha is not read
//   L1Regularization                GraphFlow/L1Regularization.h:39-67  value = lambda sum |p|, grads += times lambda sign(p)
//   L2Regularization                GraphFlow/L2Regularization.h:39-58  value = lambda sum p^2, grads += times 2 lambda p
// Storage is fp32, the arithmetic double: every load widens, every expression is the reference's, operation for operation in its order (g =
// gradient / nBatch is a division), every store rounds once, and a state the reference reads back after writing it is read back as stored.
// Contraction is off for the whole file: a product fused into the addition that follows would round once where the reference rounds twice.
// Nothing here needs LDS but the regulariser's sum; the flat passes are grid-stride loops of 256-thread workgroups, one coalesced element
// per lane.
#include <cstdint>
#include <vector>

#include "smp_optimisers.h"

#pragma clang fp contract(off)

namespace gf {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int kSumGroups = 256;   // workgroups of the regulariser's first stage: the shape of the sum, whatever n is

unsigned grid_for(size_t n) {
    const size_t blocks = (n + kBlock - 1) / kBlock;
    return (unsigned)(blocks > 65536 ? 65536 : (blocks == 0 ? 1 : blocks));
}

__global__ void __launch_bounds__(kBlock) sgd_step(float *__restrict__ p, const float *__restrict__ grad, size_t n, double lr, double nBatch) {
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
        p[i] = (float)((double)p[i] - lr * (double)grad[i] / nBatch);
}

__global__ void __launch_bounds__(kBlock) adadelta_step(float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ eg,
                                                        float *__restrict__ edx, size_t n, double nBatch, double rho, double epsilon) {
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const double g = (double)grad[i] / nBatch;
        const float eg_new = (float)(rho * (double)eg[i] + (1.0 - rho) * g * g);
        eg[i] = eg_new;
        const double old = (double)edx[i];
        const double deltax = -sqrt(old + epsilon) / sqrt((double)eg_new + epsilon) * g;
        edx[i] = (float)(rho * old + (1.0 - rho) * deltax * deltax);
        p[i] = (float)((double)p[i] + deltax);
    }
}

// the block of element i: offsets [nBlocks + 1] ascending, offsets[0] = 0 <= i < offsets[nBlocks]
__device__ __forceinline__ int block_of(const size_t *__restrict__ offsets, int nBlocks, size_t i) {
    int lo = 0, hi = nBlocks;   // offsets[lo] <= i < offsets[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// AdaMax, phase 1: maxima[b] = max over the block of |grad| as a float's bit pattern -- the values are non-negative, so the unsigned order is
// the numeric one and the result does not depend on who arrives first.  A wave whose lanes share one block folds to one atomic.  Every
// lane of a workgroup runs the same number of rounds (the shuffles want whole waves); a lane past the end carries 0 and no block.
__global__ void __launch_bounds__(kBlock) adamax_block_max(const float *__restrict__ grad, size_t n, const size_t *__restrict__ offsets, int nBlocks,
                                                           unsigned *__restrict__ maxima) {
    for (size_t base = blockIdx.x * (size_t)kBlock; base < n; base += (size_t)gridDim.x * kBlock) {
        const size_t i = base + threadIdx.x;
        const bool live = i < n;
        unsigned v = live ? __float_as_uint(fabsf(grad[i])) : 0u;
        const int b = live ? block_of(offsets, nBlocks, i) : -1;
        const int b0 = __shfl(b, 0, kWave);   // (lane 0 of a wave is live whenever any of its lanes is)
        if (__all(b == b0 || b < 0)) {
            for (int d = kWave / 2; d > 0; d >>= 1) {
                const unsigned o = (unsigned)__shfl_xor((int)v, d, kWave);
                v = o > v ? o : v;
            }
            if ((threadIdx.x & (kWave - 1)) == 0 && b0 >= 0) atomicMax(&maxima[b0], v);
        } else if (live) {
            atomicMax(&maxima[b], v);
        }
    }
}

// phase 2: infinity_norm[b] = max(beta2 infinity_norm[b], g_norm[b]) with g_norm = (max |grad|) / nBatch = max |grad / nBatch| (rounding is
// monotone); std::max(a, b) is b where a < b, else a.  The maxima go back to zero for the next call.
__global__ void __launch_bounds__(kBlock) adamax_commit(double *__restrict__ norms, unsigned *__restrict__ maxima, int nBlocks, double beta2,
                                                        double nBatch) {
    for (int b = blockIdx.x * kBlock + threadIdx.x; b < nBlocks; b += gridDim.x * kBlock) {
        const double g_norm = (double)__uint_as_float(maxima[b]) / nBatch;
        const double decayed = beta2 * norms[b];
        norms[b] = decayed < g_norm ? g_norm : decayed;
        maxima[b] = 0u;
    }
}

// phase 3: first_order = beta1 first_order + (1 - beta1) g;  p -= alpha / (1 - beta1_t) * first_order / infinity_norm[block]
// (scale = alpha / (1 - beta1_t), one double division on the host).  A block whose norm is 0 had no gradient yet: 0 / 0, as in the class.
__global__ void __launch_bounds__(kBlock) adamax_update(float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ first, size_t n,
                                                        const size_t *__restrict__ offsets, int nBlocks, const double *__restrict__ norms,
                                                        double nBatch, double beta1, double scale) {
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const double g = (double)grad[i] / nBatch;
        const float f = (float)(beta1 * (double)first[i] + (1.0 - beta1) * g);
        first[i] = f;
        const double norm = norms[block_of(offsets, nBlocks, i)];
        p[i] = (float)((double)p[i] - scale * (double)f / norm);
    }
}

// a workgroup's sum in a fixed shape: xor-shuffles inside each wave, then the four wave sums in ascending order by lane 0
__device__ __forceinline__ double group_sum(double v, double *wave_sums) {
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) wave_sums[threadIdx.x / kWave] = v;
    __syncthreads();
    double total = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBlock / kWave; ++w) total += wave_sums[w];
    return total;   // (lane 0's)
}

// The regularisers, stage 1: grads[i] += times * term_i, and partial[group] = the group's share of sum |p| (L1) or sum p^2 (L2) in double.
// L1's sign() is 0 for |p| < 1e-8 (L1Regularization.h:51-59); L2's term is 2.0 * lambda * gradient[0] * p with gradient[0] = 1.0.
template <int NORM>
__global__ void __launch_bounds__(kBlock) regularise_terms(const float *__restrict__ p, float *__restrict__ grads, size_t n, double lambda,
                                                           double times, double *__restrict__ partial) {
    __shared__ double wave_sums[kBlock / kWave];
    double sum = 0.0;
    for (size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const double x = (double)p[i];
        double term;
        if (NORM == 1) {
            sum += fabs(x);
            term = lambda * (fabs(x) < 1e-8 ? 0.0 : (x > 0.0 ? 1.0 : -1.0));
        } else {
            sum += x * x;
            term = 2.0 * lambda * 1.0 * x;
        }
        grads[i] = (float)((double)grads[i] + times * term);
    }
    const double total = group_sum(sum, wave_sums);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// stage 2: one workgroup adds the kSumGroups partials in the same fixed shape;  value = sum * lambda (value[0] *= lambda)
__global__ void __launch_bounds__(kBlock) regularise_value(const double *__restrict__ partial, int groups, double lambda, double *__restrict__ value) {
    __shared__ double wave_sums[kBlock / kWave];
    double sum = 0.0;
    for (int i = threadIdx.x; i < groups; i += kBlock) sum += partial[i];
    const double total = group_sum(sum, wave_sums);
    if (threadIdx.x == 0) *value = total * lambda;
}

gf_status sgd_launch(gf_ctx *ctx, float *params, const float *grads, size_t n, double lr, int nBatch) {
    if (n) GF_LAUNCH(ctx, "smp_sgd", sgd_step, dim3(grid_for(n)), dim3(kBlock), 0, params, grads, n, lr, (double)nBatch);
    return GF_OK;
}

gf_status adadelta_launch(gf_ctx *ctx, float *params, const float *grads, float *eg, float *edx, size_t n, int nBatch, const OptimConstants &k) {
    if (n) GF_LAUNCH(ctx, "smp_adadelta", adadelta_step, dim3(grid_for(n)), dim3(kBlock), 0, params, grads, eg, edx, n, (double)nBatch, k.rho, k.epsilon);
    return GF_OK;
}

// offsets, norms, maxima: device; the maxima are zero on entry and on return.  *beta1_t (host) is advanced first, as the class does.
gf_status adamax_launch(gf_ctx *ctx, float *params, const float *grads, float *first, size_t n, const size_t *offsets, int nBlocks, double *norms,
                        unsigned *maxima, double alpha, int nBatch, const OptimConstants &k, double *beta1_t) {
    *beta1_t *= k.beta1;
    if (!n || nBlocks < 1) return GF_OK;
    const double scale = alpha / (1.0 - *beta1_t);
    GF_LAUNCH(ctx, "smp_adamax_max", adamax_block_max, dim3(grid_for(n)), dim3(kBlock), 0, grads, n, offsets, nBlocks, maxima);
    GF_LAUNCH(ctx, "smp_adamax_commit", adamax_commit, dim3(grid_for((size_t)nBlocks)), dim3(kBlock), 0, norms, maxima, nBlocks, k.beta2, (double)nBatch);
    GF_LAUNCH(ctx, "smp_adamax_update", adamax_update, dim3(grid_for(n)), dim3(kBlock), 0, params, grads, first, n, offsets, nBlocks, norms,
              (double)nBatch, k.beta1, scale);
    return GF_OK;
}

// ascending, from 0 to n, no empty block
bool offsets_valid(const size_t *offsets, int nBlocks, size_t n) {
    if (!offsets || nBlocks < 1 || offsets[0] != 0 || offsets[nBlocks] != n) return false;
    for (int b = 0; b < nBlocks; ++b)
        if (offsets[b + 1] <= offsets[b]) return false;
    return true;
}

size_t block_bytes(int nBlocks) { return sizeof(size_t) * ((size_t)nBlocks + 1) + (sizeof(double) + sizeof(unsigned)) * (size_t)nBlocks; }

}  // namespace

OptimConstants optim_constants(const gf_optim_config *cfg) {
    OptimConstants k = {cfg->beta1, cfg->beta2, cfg->rho, cfg->epsilon};
    if (cfg->beta1 == 0.0 && cfg->beta2 == 0.0) k.beta1 = 0.9, k.beta2 = 0.999;
    if (cfg->rho == 0.0 && cfg->epsilon == 0.0) k.rho = 0.95, k.epsilon = 1e-6;
    return k;
}

gf_status optim_check(gf_ctx *ctx, const OptimState *st, const gf_optim_config *cfg, const char *who) {
    if (!cfg) return fail(ctx, GF_ERR_INVALID, "%s: null configuration", who);
    if (cfg->kind < kOptimAdam || cfg->kind > kOptimAdaDelta)
        return fail(ctx, GF_ERR_INVALID, "%s: kind %d (0: Adam, 1: Momentum, 2: SGD, 3: AdaMax, 4: AdaDelta)", who, cfg->kind);
    if (cfg->nBatch <= 0) return fail(ctx, GF_ERR_INVALID, "%s: nBatch %d", who, cfg->nBatch);
    if (st->kind != kOptimNone && st->kind != cfg->kind)
        return fail(ctx, GF_ERR_INVALID, "%s: kind %d after steps of kind %d: the handle's state is the other optimiser's (gf_smp_adam_reset first)", who,
                    cfg->kind, st->kind);
    return GF_OK;
}

gf_status optim_step(gf_ctx *ctx, OptimState *st, const std::vector<size_t> &block_sizes, float *params, const float *grads, size_t n, float *s0,
                     float *s1, const gf_optim_config *cfg, const char *who) {
    const OptimConstants k = optim_constants(cfg);
    gf_status rc = GF_OK;
    if (cfg->kind == kOptimSGD) {
        rc = sgd_launch(ctx, params, grads, n, cfg->learning_rate, cfg->nBatch);
    } else if (cfg->kind == kOptimAdaDelta) {
        rc = adadelta_launch(ctx, params, grads, s0, s1, n, cfg->nBatch, k);
    } else if (cfg->kind == kOptimAdaMax) {
        if (!st->blocks) {   // the block table, once per handle
            const int nBlocks = (int)block_sizes.size();
            std::vector<size_t> offsets((size_t)nBlocks + 1, 0);
            for (int b = 0; b < nBlocks; ++b) offsets[b + 1] = offsets[b] + block_sizes[b];
            if (!offsets_valid(offsets.data(), nBlocks, n)) return fail(ctx, GF_ERR_INVALID, "%s: the handle's block table does not cover its %zu parameters", who, n);
            GF_HIP_TRY(ctx, hipMalloc(&st->blocks, block_bytes(nBlocks)));
            st->nBlocks = nBlocks;
            GF_HIP_TRY(ctx, hipMemsetAsync(st->blocks, 0, block_bytes(nBlocks), ctx->stream));
            GF_HIP_TRY(ctx, hipMemcpyAsync(st->blocks, offsets.data(), sizeof(size_t) * offsets.size(), hipMemcpyHostToDevice, ctx->stream));
            GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (offsets goes away)
        }
        rc = adamax_launch(ctx, params, grads, s0, n, st->offsets(), st->nBlocks, st->norms(), st->maxima(), cfg->learning_rate, cfg->nBatch, k, &st->beta1_t);
    } else {
        return fail(ctx, GF_ERR_INVALID, "%s: kind %d is not one of this file's", who, cfg->kind);
    }
    if (rc == GF_OK) st->kind = cfg->kind;
    return rc;
}

gf_status optim_reset(gf_ctx *ctx, OptimState *st) {
    st->kind = kOptimNone;
    st->beta1_t = 1.0;
    if (st->blocks)   // (the offsets stay)
        GF_HIP_TRY(ctx, hipMemsetAsync(st->norms(), 0, (sizeof(double) + sizeof(unsigned)) * (size_t)st->nBlocks, ctx->stream));
    return GF_OK;
}

void optim_free(OptimState *st) {
    if (st->blocks) (void)hipFree(st->blocks);
    st->blocks = nullptr;
}

}  // namespace gf

using gf::fail;

extern "C" {

gf_status gf_optimiser_step_f32(gf_ctx *ctx, const gf_optim_config *cfg, float *params, const float *grads, size_t n, const size_t *block_offsets_host,
                                int nBlocks, float *state0, float *state1, double *block_norms, double *beta1_t_inout) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (!cfg || !params || !grads || cfg->nBatch <= 0) return fail(ctx, GF_ERR_INVALID, "gf_optimiser_step_f32: bad argument");
    if (cfg->kind < gf::kOptimSGD || cfg->kind > gf::kOptimAdaDelta)
        return fail(ctx, GF_ERR_INVALID, "gf_optimiser_step_f32: kind %d (2: SGD, 3: AdaMax, 4: AdaDelta; gf_adam_step_f32 is Adam's)", cfg->kind);
    const gf::OptimConstants k = gf::optim_constants(cfg);
    if (cfg->kind == gf::kOptimSGD) return gf::sgd_launch(ctx, params, grads, n, cfg->learning_rate, cfg->nBatch);
    if (cfg->kind == gf::kOptimAdaDelta) {
        if (!state0 || !state1) return fail(ctx, GF_ERR_INVALID, "gf_optimiser_step_f32: AdaDelta needs state0 (E[g^2]) and state1 (E[dx^2])");
        return gf::adadelta_launch(ctx, params, grads, state0, state1, n, cfg->nBatch, k);
    }
    if (!state0 || !block_norms || !beta1_t_inout)
        return fail(ctx, GF_ERR_INVALID, "gf_optimiser_step_f32: AdaMax needs state0 (first_order), block_norms and beta1_t_inout");
    if (n == 0) {
        *beta1_t_inout *= k.beta1;
        return GF_OK;
    }
    if (!gf::offsets_valid(block_offsets_host, nBlocks, n))
        return fail(ctx, GF_ERR_INVALID, "gf_optimiser_step_f32: block_offsets_host must hold nBlocks + 1 strictly ascending offsets from 0 to n");
    // offsets and the per-block maxima in the context's scratch
    const size_t off_bytes = sizeof(size_t) * ((size_t)nBlocks + 1);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gf_status st = gf::ensure_ws(ctx, off_bytes + sizeof(unsigned) * (size_t)nBlocks);
    if (st != GF_OK) return st;
    size_t *offsets = static_cast<size_t *>(ctx->ws);
    unsigned *maxima = reinterpret_cast<unsigned *>(static_cast<char *>(ctx->ws) + off_bytes);
    GF_HIP_TRY(ctx, hipMemcpyAsync(offsets, block_offsets_host, off_bytes, hipMemcpyHostToDevice, ctx->stream));
    GF_HIP_TRY(ctx, hipMemsetAsync(maxima, 0, sizeof(unsigned) * (size_t)nBlocks, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the caller's table may go away)
    return gf::adamax_launch(ctx, params, grads, state0, n, offsets, nBlocks, block_norms, maxima, cfg->learning_rate, cfg->nBatch, k, beta1_t_inout);
}

gf_status gf_regularise_f32(gf_ctx *ctx, const float *params, float *grads, size_t n, int norm, double lambda, int times, double *value_host) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (!params || !grads || !value_host || (norm != 1 && norm != 2) || times < 0)
        return fail(ctx, GF_ERR_INVALID, "gf_regularise_f32: bad argument (norm 1 | 2, times >= 0)");
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gf_status st = gf::ensure_ws(ctx, sizeof(double) * (gf::kSumGroups + 1));
    if (st != GF_OK) return st;
    double *partial = static_cast<double *>(ctx->ws), *value = partial + gf::kSumGroups;
    if (norm == 1)
        GF_LAUNCH(ctx, "smp_regularise_l1", gf::regularise_terms<1>, dim3(gf::kSumGroups), dim3(gf::kBlock), 0, params, grads, n, lambda, (double)times, partial);
    else
        GF_LAUNCH(ctx, "smp_regularise_l2", gf::regularise_terms<2>, dim3(gf::kSumGroups), dim3(gf::kBlock), 0, params, grads, n, lambda, (double)times, partial);
    GF_LAUNCH(ctx, "smp_regularise_value", gf::regularise_value, dim3(1), dim3(gf::kBlock), 0, partial, gf::kSumGroups, lambda, value);
    GF_HIP_TRY(ctx, hipMemcpyAsync(value_host, value, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GF_OK;
}

}  // extern "C"
