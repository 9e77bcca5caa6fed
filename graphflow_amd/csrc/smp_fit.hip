// smp_fit.hip -- the iterative training calls of the reference's model classes on a gf_smp handle (gf_smp_fit, gf_smp_fit_host), the
// parameter cache behind them (gf_smp_parameters_snapshot / _rollback) and the host-pointer forward of every handle kind
// (gf_smp_forward_host_samples, gf_smp_gram_host).  The levels' passes are the existing ones; the device code of this file is the sum of
// the per-sample losses and the optimiser step of the reference's Learn(alpha) overload.
#include <vector>

#include "smp_fit.h"
#include "smp_fit_policy.h"
#include "smp_internal.h"

namespace gf {
namespace {

constexpr int kSumChunk = 2048;   // losses one workgroup stages in LDS at a time (16 KiB of doubles)

// sum over i < n of (double)loss[i], ADDED IN ASCENDING ORDER by one lane: the classes' host loop `total += loss[i]` adds that way, and a
// tree over the same doubles rounds differently once the losses spread over more than 29 binary orders.  The workgroup's lanes only
// fetch; n is a batch's sample count.
__global__ void __launch_bounds__(256) loss_sum_ordered(const float *__restrict__ loss, int n, double *__restrict__ out) {
    __shared__ double stage[kSumChunk];
    double total = 0.0;
    for (int base = 0; base < n; base += kSumChunk) {
        const int m = n - base < kSumChunk ? n - base : kSumChunk;
        for (int i = threadIdx.x; i < m; i += blockDim.x) stage[i] = (double)loss[base + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < m; ++i) total += stage[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = total;
}

// Adam::Learn(alpha) (GraphFlow/Adam.h:77-105): every element uses the powers beta^t of the call
__global__ void adam_step_per_call(float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ m, float *__restrict__ v, size_t n,
                                   double alpha, double t, double beta1, double beta2, double eps) {
    const double c1 = 1.0 - exp(t * log(beta1)), c2 = 1.0 - exp(t * log(beta2));
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double g = (double)grad[i];
        const double mi = beta1 * (double)m[i] + (1.0 - beta1) * g;
        const double vi = beta2 * (double)v[i] + (1.0 - beta2) * g * g;
        m[i] = (float)mi;
        v[i] = (float)vi;
        p[i] = (float)((double)p[i] - alpha * (mi / c1) / (sqrt(vi / c2) + eps));
    }
}

int sample_count(const gf_smp *s) { return s->cfg.readout == 1 ? s->lay.nMol / 2 : s->lay.nMol; }

// the per-sample device arrays of the host-pointer calls of this file (from the pool: the batch's)
gf_status sample_buffers(gf_smp *s) {
    if (s->fit_loss) return GF_OK;
    const size_t n = (size_t)sample_count(s);
    gf_status st = upload(s, &s->fit_t, nullptr, n);
    if (st == GF_OK) st = upload(s, &s->fit_y, nullptr, n);
    if (st == GF_OK) st = upload(s, &s->fit_feat, nullptr, n * gf_smp_feature_width(s));
    if (st == GF_OK) st = upload(s, &s->fit_loss, nullptr, n);
    return st;
}

gf_status moment_buffers(gf_smp *s) {   // (as the optimiser steps of smp_optim.hip take them on first use)
    if (s->adam_m) return GF_OK;
    gf_ctx *ctx = s->ctx;
    const size_t bytes = param_count(s->ucfg) * sizeof(float);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&s->adam_m), bytes));
    GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&s->adam_v), bytes));
    GF_HIP_TRY(ctx, hipMemsetAsync(s->adam_m, 0, bytes, ctx->stream));
    GF_HIP_TRY(ctx, hipMemsetAsync(s->adam_v, 0, bytes, ctx->stream));
    s->adam_n = 0;
    return GF_OK;
}

gf_status host_targets(gf_smp *s, const double *targets, int n) {
    std::vector<float> tmp((size_t)n);
    for (int i = 0; i < n; ++i) tmp[i] = (float)targets[i];
    GF_HIP_TRY(s->ctx, hipMemcpyAsync(s->fit_t, tmp.data(), sizeof(float) * n, hipMemcpyHostToDevice, s->ctx->stream));
    GF_HIP_TRY(s->ctx, hipStreamSynchronize(s->ctx->stream));   // (tmp goes away)
    return GF_OK;
}

gf_status floats_to_host(gf_ctx *ctx, double *dst, const float *src, size_t n) {
    if (!dst || !n) return GF_OK;
    std::vector<float> tmp(n);
    GF_HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), src, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) dst[i] = (double)tmp[i];
    return GF_OK;
}

}  // namespace

gf_status fit_snapshot(gf_ctx *ctx, float **cache, const float *params, size_t n) {
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!*cache) GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(cache), (n ? n : 1) * sizeof(float)));
    if (n) GF_HIP_TRY(ctx, hipMemcpyAsync(*cache, params, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return GF_OK;
}

gf_status fit_rollback(gf_ctx *ctx, float *const *cache, float *params, size_t n, const char *who) {
    if (!*cache) return fail(ctx, GF_ERR_INVALID, "%s: nothing to roll back to (no snapshot of this handle yet)", who);
    if (n) GF_HIP_TRY(ctx, hipMemcpyAsync(params, *cache, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return GF_OK;
}

gf_status fit_loss_sum(gf_ctx *ctx, const float *loss, int n, double **dev_sum, double *host) {
    if (!*dev_sum) GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(dev_sum), sizeof(double)));
    GF_LAUNCH(ctx, "smp_fit_loss_sum", loss_sum_ordered, dim3(1), dim3(256), 0, loss, n, *dev_sum);
    GF_HIP_TRY(ctx, hipMemcpyAsync(host, *dev_sum, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GF_OK;
}

gf_status fit_adam_step_per_call(gf_ctx *ctx, float *params, const float *grads, float *m, float *v, size_t n, double learning_rate,
                                 unsigned long long *elements) {
    *elements += 1;   // beta1_t *= beta1, beta2_t *= beta2: once, before the element loop
    if (!n) return GF_OK;
    const size_t blocks = (n + 255) / 256;
    GF_LAUNCH(ctx, "smp_adam", adam_step_per_call, dim3((unsigned)(blocks > 1048576 ? 1048576 : blocks)), dim3(256), 0, params, grads, m, v, n,
              learning_rate, (double)*elements, 0.9, 0.999, 1e-8);
    return GF_OK;
}

gf_status fit_check_config(gf_ctx *ctx, const gf_smp_fit_config *cfg, gf_smp_fit_report *report, int nSamples, const char *who) {
    if (!cfg || !report) return fail(ctx, GF_ERR_INVALID, "%s: null configuration or report", who);
    if (cfg->kind < 0 || cfg->kind > 1 || cfg->optimiser < kOptimAdam || cfg->optimiser > kOptimAdaDelta || cfg->nIterations < 0)
        return fail(ctx, GF_ERR_INVALID, "%s: kind %d (0: BatchLearn, 1: Learn), optimiser %d (0: Adam, 1: Momentum, 2: SGD, 3: AdaMax, 4: AdaDelta), nIterations %d",
                    who, cfg->kind, cfg->optimiser, cfg->nIterations);
    if (nSamples < 1) return fail(ctx, GF_ERR_INVALID, "%s: no prepared batch", who);
    if (cfg->kind == gf_fit::kLearn && nSamples != 1)
        return fail(ctx, GF_ERR_INVALID, "%s: kind 1 (Learn) trains on one sample, the prepared batch holds %d", who, nSamples);
    return GF_OK;
}

gf_status fit_run(const FitDriver &d, const gf_smp_fit_config *cfg, gf_smp_fit_report *report, unsigned char *decisions) {
    gf_ctx *ctx = d.ctx;
    gf_fit::State state;
    double loss = 0.0;
    gf_status st = fit_snapshot(ctx, d.cache, d.params, d.n_params);   // cache_parameters()
    if (st == GF_OK) st = d.forward();
    if (st == GF_OK) st = fit_loss_sum(ctx, d.loss, d.nSamples, d.sum, &loss);
    if (st != GF_OK) return st;
    bool stale = false;   // a rollback has put back parameters the activations on the device were not computed from
    if (gf_fit::begin(&state, cfg->kind, cfg->learning_rate, cfg->epsilon, loss))
        for (int iter = 0; iter < cfg->nIterations; ++iter) {
            if (stale) st = d.forward();
            stale = false;
            if (st == GF_OK) st = d.backward();
            if (st == GF_OK) st = d.step(state.learning_rate, cfg->kind == gf_fit::kLearn ? 1 : d.nSamples, cfg->kind == gf_fit::kLearn);
            if (st == GF_OK) st = d.forward();
            if (st == GF_OK) st = fit_loss_sum(ctx, d.loss, d.nSamples, d.sum, &loss);
            if (st != GF_OK) return st;
            const gf_fit::Decision dec = gf_fit::step(&state, loss);
            if (decisions) decisions[iter] = (unsigned char)dec;
            if (dec == gf_fit::kAccept) st = fit_snapshot(ctx, d.cache, d.params, d.n_params);
            if (dec == gf_fit::kReject || dec == gf_fit::kRejectLeave) {
                st = fit_rollback(ctx, d.cache, d.params, d.n_params, d.who);
                stale = true;
            }
            if (st != GF_OK) return st;
            if (dec == gf_fit::kRejectLeave || dec == gf_fit::kLeave) break;
        }
    if (stale) st = d.forward();   // the handle is left forwarded at the parameters it is left with
    if (st != GF_OK) return st;
    report->first = state.first;
    report->second = state.second;
    report->iterations = state.iterations;
    report->accepted = state.accepted;
    report->rejected = state.rejected;
    report->left_early = state.left_early ? 1 : 0;
    report->learning_rate = state.learning_rate;
    return GF_OK;
}

}  // namespace gf

using gf::fail;

extern "C" {

gf_status gf_smp_parameters_snapshot(gf_smp *s, const float *params) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (!params) params = s->own_p;
    if (!params) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_parameters_snapshot: null params and no handle-owned model");
    return gf::fit_snapshot(s->ctx, &s->fit_cache, params, gf::param_count(s->ucfg));
}

gf_status gf_smp_parameters_rollback(gf_smp *s, float *params) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (!params) params = s->own_p;
    if (!params) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_parameters_rollback: null params and no handle-owned model");
    return gf::fit_rollback(s->ctx, &s->fit_cache, params, gf::param_count(s->ucfg), "gf_smp_parameters_rollback");
}

gf_status gf_smp_forward_host_samples(gf_smp *s, const double *targets, double *predict, double *loss, double *graph_feature) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!s->prepared) return fail(ctx, GF_ERR_INVALID, "gf_smp_forward_host_samples before gf_smp_prepare");
    if (!s->own_p) return fail(ctx, GF_ERR_INVALID, "gf_smp_forward_host_samples: no handle-owned model (gf_smp_parameters_upload)");
    if (s->cfg.physics) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_forward_host_samples: a physics tower has no samples of its own (gf_smp_model_forward_host)");
    const bool gram = s->cfg.readout == 2;
    if (gram && (targets || predict || graph_feature))
        return fail(ctx, GF_ERR_INVALID, "gf_smp_forward_host_samples: a Gram handle (readout = 2) takes NULL targets, predict and graph_feature");
    const int n = gf::sample_count(s);
    gf_status st = gf::sample_buffers(s);
    if (st == GF_OK && targets) st = gf::host_targets(s, targets, n);
    if (st != GF_OK) return st;
    st = gram ? gf_smp_forward(s, s->own_p, nullptr, nullptr, s->fit_loss, nullptr)
              : gf_smp_forward(s, s->own_p, targets ? s->fit_t : nullptr, s->fit_y, s->fit_loss, s->fit_feat);
    if (st == GF_OK && !gram) st = gf::floats_to_host(ctx, predict, s->fit_y, (size_t)n);
    if (st == GF_OK && (targets || gram)) st = gf::floats_to_host(ctx, loss, s->fit_loss, (size_t)n);
    if (st == GF_OK && !gram) st = gf::floats_to_host(ctx, graph_feature, s->fit_feat, (size_t)n * gf_smp_feature_width(s));
    return st;
}

gf_status gf_smp_gram_host(gf_smp *s, double *out) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!out) return fail(ctx, GF_ERR_INVALID, "gf_smp_gram_host: null argument");
    if (s->cfg.readout != 2) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_gram_host: not a Gram handle (readout = 2)");
    if (!s->prepared || !s->forwarded) return fail(ctx, GF_ERR_INVALID, "gf_smp_gram_host before a forward");
    const size_t total = s->gram_count;
    gf_status st = s->fit_gram ? GF_OK : gf::upload(s, &s->fit_gram, nullptr, total);   // (the batch's: one block, back in the pool with it)
    if (st == GF_OK) st = gf_smp_gram(s, s->fit_gram);
    if (st == GF_OK) st = gf::floats_to_host(ctx, out, s->fit_gram, total);
    return st;
}

gf_status gf_smp_loss_sum_f32(gf_ctx *ctx, const float *loss, size_t n, double *sum) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (!loss || !sum || n < 1 || n > 0x7fffffffu) return fail(ctx, GF_ERR_INVALID, "gf_smp_loss_sum_f32: bad argument");
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gf_status st = gf::ensure_ws(ctx, sizeof(double));
    if (st != GF_OK) return st;
    double *dev = static_cast<double *>(ctx->ws);
    return gf::fit_loss_sum(ctx, loss, (int)n, &dev, sum);
}

gf_status gf_smp_fit(gf_smp *s, float *params, float *grads, const float *targets, const gf_smp_fit_config *cfg, gf_smp_fit_report *report,
                     unsigned char *decisions) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!s->prepared) return fail(ctx, GF_ERR_INVALID, "gf_smp_fit before gf_smp_prepare");
    if (s->cfg.physics) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_fit: a physics tower has no loss of its own (gf_smp_model_fit)");
    if (!params && !grads && s->own_p) {
        params = s->own_p;
        grads = s->own_g;
    }
    if (!params || !grads) return fail(ctx, GF_ERR_INVALID, "gf_smp_fit: null params / grads and no handle-owned model");
    const bool gram = s->cfg.readout == 2;
    if (gram ? targets != nullptr : targets == nullptr)
        return fail(ctx, GF_ERR_INVALID, gram ? "gf_smp_fit: a Gram handle (readout = 2) takes NULL targets" : "gf_smp_fit: null targets");
    gf_status st = gf::fit_check_config(ctx, cfg, report, gf::sample_count(s), "gf_smp_fit");
    if (st == GF_OK) st = gf::sample_buffers(s);
    if (st == GF_OK) st = gf::moment_buffers(s);
    if (st != GF_OK) return st;
    gf::FitDriver d;
    d.ctx = ctx;
    d.params = params;
    const size_t n_params = gf::param_count(s->ucfg);
    d.n_params = n_params;
    d.nSamples = gf::sample_count(s);
    d.loss = s->fit_loss;
    d.cache = &s->fit_cache;
    d.sum = &s->fit_sum;
    d.forward = [=]() { return gf_smp_forward(s, params, targets, nullptr, s->fit_loss, nullptr); };
    d.backward = [=]() { return gf_smp_backward(s, params, grads, 0); };
    const gf_smp_fit_config c = *cfg;
    d.step = [=](double lr, int nBatch, bool per_call) {
        if (c.optimiser == 1) return gf_smp_momentum_step(s, params, grads, lr, nBatch, c.gamma);   // (Learn(lr) is Learn(lr, 1) there)
        if (c.optimiser >= gf::kOptimSGD) {   // SGD, AdaMax, AdaDelta at the classes' default constants; Learn(lr) is Learn(lr, 1) there too
            const gf_optim_config oc = {c.optimiser, nBatch, lr, 0.0, 0.0, 0.0, 0.0, 0.0};
            return gf_smp_optimiser_step(s, params, grads, &oc);
        }
        s->optim.kind = gf::kOptimAdam;
        if (per_call) return gf::fit_adam_step_per_call(ctx, params, grads, s->adam_m, s->adam_v, n_params, lr, &s->adam_n);
        return gf_smp_adam_step(s, params, grads, lr, nBatch);
    };
    return gf::fit_run(d, cfg, report, decisions);
}

gf_status gf_smp_fit_host(gf_smp *s, const double *targets, const gf_smp_fit_config *cfg, gf_smp_fit_report *report, unsigned char *decisions) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!s->prepared) return fail(ctx, GF_ERR_INVALID, "gf_smp_fit_host before gf_smp_prepare");
    if (!s->own_p) return fail(ctx, GF_ERR_INVALID, "gf_smp_fit_host: no handle-owned model (gf_smp_parameters_upload)");
    gf_status st = gf::sample_buffers(s);
    if (st == GF_OK && targets) st = gf::host_targets(s, targets, gf::sample_count(s));
    if (st != GF_OK) return st;
    return gf_smp_fit(s, nullptr, nullptr, targets ? s->fit_t : nullptr, cfg, report, decisions);
}

}  // extern "C"
