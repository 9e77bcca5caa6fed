// smp_optimisers.h -- what a handle keeps for the optimisers beyond Adam and Momentum (SGD, AdaMax, AdaDelta; smp_optimisers.hip) and the
// calls gf_smp / gf_smp_model share.  The two fp32 state buffers are the handle's adam_m / adam_v; this struct has the rest.
#ifndef GF_SMP_OPTIMISERS_H_INCLUDED
#define GF_SMP_OPTIMISERS_H_INCLUDED

#include <vector>

#include "gf_internal.h"

namespace gf {

enum OptimKind { kOptimNone = -1, kOptimAdam = 0, kOptimMomentum = 1, kOptimSGD = 2, kOptimAdaMax = 3, kOptimAdaDelta = 4 };

struct OptimState {
    int kind = kOptimNone;    // gf_optim_config.kind of the last step on the handle; kOptimNone after create and after a reset
    double beta1_t = 1.0;     // AdaMax::beta1_t (AdaMax.h:30), advanced on the host once per call
    int nBlocks = 0;          // the blocks the class registers with sgd->add (gf_smp_config_param_blocks)
    // one device allocation, taken by the first AdaMax step: offsets [nBlocks + 1] (size_t), infinity_norm [nBlocks] (double), the
    // per-block maxima of |grad| as float bit patterns [nBlocks] (unsigned; zero between calls)
    void *blocks = nullptr;
    size_t *offsets() const { return static_cast<size_t *>(blocks); }
    double *norms() const { return reinterpret_cast<double *>(offsets() + nBlocks + 1); }
    unsigned *maxima() const { return reinterpret_cast<unsigned *>(norms() + nBlocks); }
};

// the constants of a gf_optim_config with the classes' defaults filled in (AdaMax.h:26-29, AdaDelta.h:26-28)
struct OptimConstants {
    double beta1, beta2, rho, epsilon;
};
OptimConstants optim_constants(const gf_optim_config *cfg);

// kind, nBatch and the recorded kind of the handle: GF_ERR_INVALID with a message, or GF_OK
gf_status optim_check(gf_ctx *ctx, const OptimState *st, const gf_optim_config *cfg, const char *who);
// One step of kind 2, 3 or 4 on a handle's flat vector: s0 / s1 = the handle's two fp32 state buffers, block_sizes = the registered blocks
// (read by the first AdaMax step only).  Records the kind.
gf_status optim_step(gf_ctx *ctx, OptimState *st, const std::vector<size_t> &block_sizes, float *params, const float *grads, size_t n, float *s0,
                     float *s1, const gf_optim_config *cfg, const char *who);
gf_status optim_reset(gf_ctx *ctx, OptimState *st);   // gf_smp_adam_reset's share: no kind, beta1_t = 1, norms and maxima zero
void optim_free(OptimState *st);
// Momentum::Learn(lr, nBatch) on any flat buffer (smp_optim.hip: the kernel of gf_smp_momentum_step)
gf_status momentum_step_on(gf_ctx *ctx, float *params, const float *grads, float *m, size_t n, double learning_rate, int nBatch, double gamma);

}  // namespace gf
#endif
