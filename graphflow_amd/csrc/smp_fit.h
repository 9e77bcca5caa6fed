// smp_fit.h -- the iterative training calls of the reference's model classes (BatchLearn with nIterations, Learn) as one loop over a
// handle's existing passes; shared by gf_smp_fit (smp_fit.hip) and gf_smp_model_fit (smp_model.hip).  The decisions are
// smp_fit_policy.h's; the device side is the parameter cache (two device-to-device copies) and the sum of the per-sample losses.
#ifndef GF_SMP_FIT_H_INCLUDED
#define GF_SMP_FIT_H_INCLUDED

#include <functional>

#include "gf_internal.h"

namespace gf {

// What the loop needs of a handle.  forward evaluates the per-sample losses into `loss` (with targets); backward is the reverse sweep
// from the last forward; step(lr, nBatch, per_call) the optimiser: per_call = the reference's Learn(lr) overload (kind 1).
struct FitDriver {
    gf_ctx *ctx = nullptr;
    const char *who = "gf_smp_fit";
    float *params = nullptr;   // device, [n_params]
    size_t n_params = 0;
    int nSamples = 0;
    const float *loss = nullptr;   // device, [nSamples], written by forward
    float **cache = nullptr;       // the handle's parameter cache (allocated on first snapshot)
    double **sum = nullptr;        // the handle's 8 bytes for the loss sum
    std::function<gf_status()> forward, backward;
    std::function<gf_status(double, int, bool)> step;
};

// device-to-device copies of the flat parameter buffer into / out of *cache on the context's stream; values only
gf_status fit_snapshot(gf_ctx *ctx, float **cache, const float *params, size_t n);
gf_status fit_rollback(gf_ctx *ctx, float *const *cache, float *params, size_t n, const char *who);
// *host = sum over i < n of (double)loss[i], added in ascending order (the bits of the classes' host loop).  One small blocking readback.
gf_status fit_loss_sum(gf_ctx *ctx, const float *loss, int n, double **dev_sum, double *host);
// Adam::Learn(alpha) (GraphFlow/Adam.h:77-105): ONE advance of the bias-correction powers per call, shared by every element -- unlike
// Learn(alpha, nBatch), which advances them per element (gf_adam_step_f32).  *elements is the handle's running exponent.
gf_status fit_adam_step_per_call(gf_ctx *ctx, float *params, const float *grads, float *m, float *v, size_t n, double learning_rate,
                                 unsigned long long *elements);
gf_status fit_check_config(gf_ctx *ctx, const gf_smp_fit_config *cfg, gf_smp_fit_report *report, int nSamples, const char *who);
gf_status fit_run(const FitDriver &d, const gf_smp_fit_config *cfg, gf_smp_fit_report *report, unsigned char *decisions);

}  // namespace gf
#endif
