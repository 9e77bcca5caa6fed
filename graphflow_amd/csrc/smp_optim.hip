// smp_optim.hip -- the host-pointer mode of the batched SMP driver (the handle owns the model; batches and results cross as host arrays),
// the optimisers of the reference's training loops (Adam, Momentum), its weight initialisation and its text checkpoints.
#include <cstdio>
#include <cstdlib>

#include "smp_internal.h"

namespace gf {
namespace {

#define GRID_STRIDE(idx, total) \
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < (total); idx += (size_t)gridDim.x * blockDim.x)
unsigned grid_for(size_t total, int per_block = 256) {
    size_t blocks = (total + per_block - 1) / per_block;
    return (unsigned)(blocks > 1048576 ? 1048576 : (blocks == 0 ? 1 : blocks));
}

// Adam::Learn(alpha, nBatch) (GraphFlow/Adam.h:106-133) on the flat parameter buffer.  The reference advances its
// bias-correction powers INSIDE the element loop (beta1_t *= beta1 per element, :121,:125), so element i of the call that
// starts after n0 processed elements uses beta^(n0 + i + 1); restated in closed form, in double like the reference.
__global__ void adam_step(float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ m, float *__restrict__ v,
                          size_t n, double alpha, double inv_batch, unsigned long long n0, double beta1, double beta2,
                          double eps) {
    const double l1 = log(beta1), l2 = log(beta2);
    GRID_STRIDE(i, n) {
        const double g = (double)grad[i] * inv_batch;
        const double mi = beta1 * (double)m[i] + (1.0 - beta1) * g;
        const double vi = beta2 * (double)v[i] + (1.0 - beta2) * g * g;
        const double t = (double)(n0 + i + 1);
        const double mh = mi / (1.0 - exp(t * l1)), vh = vi / (1.0 - exp(t * l2));
        m[i] = (float)mi;
        v[i] = (float)vi;
        p[i] = (float)((double)p[i] - alpha * mh / (sqrt(vh) + eps));
    }
}

// Momentum::Learn(learning_rate, nBatch) (GraphFlow/Momentum.h:64-71): m = gamma m + lr g / nBatch;  p -= m
__global__ void momentum_step(float *__restrict__ p, const float *__restrict__ grad, float *__restrict__ m, size_t n, double lr,
                              double inv_batch, double gamma) {
    GRID_STRIDE(i, n) {
        const double mi = gamma * (double)m[i] + lr * (double)grad[i] * inv_batch;
        m[i] = (float)mi;
        p[i] = (float)((double)p[i] - mi);
    }
}

// what the handle's two optimisers share: the handle's own model for null arguments, the argument check, the moment buffers
gf_status optimiser_begin(gf_smp *s, float **params, const float **grads, int nBatch, const char *who) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!*params && !*grads && s->own_p) {
        *params = s->own_p;
        *grads = s->own_g;
    }
    if (!*params || !*grads || nBatch <= 0) return fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (s->adam_m) return GF_OK;
    const size_t bytes = param_count(s->ucfg) * sizeof(float);
    GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&s->adam_m), bytes));
    GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&s->adam_v), bytes));
    GF_HIP_TRY(ctx, hipMemsetAsync(s->adam_m, 0, bytes, ctx->stream));
    GF_HIP_TRY(ctx, hipMemsetAsync(s->adam_v, 0, bytes, ctx->stream));
    s->adam_n = 0;
    return GF_OK;
}
}  // namespace

gf_status momentum_step_on(gf_ctx *ctx, float *params, const float *grads, float *m, size_t n, double learning_rate, int nBatch, double gamma) {
    GF_LAUNCH(ctx, "smp_momentum", momentum_step, dim3(grid_for(n)), dim3(256), 0, params, grads, m, n, learning_rate, 1.0 / (double)nBatch, gamma);
    return GF_OK;
}

// the handle-owned parameter / gradient buffers (host-pointer mode), created on first use
gf_status own_model(gf_smp *s) {
    if (s->own_p) return GF_OK;
    GF_HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    const size_t n = param_count(s->ucfg);
    GF_HIP_TRY(s->ctx, hipMalloc(reinterpret_cast<void **>(&s->own_p), n * sizeof(float)));
    GF_HIP_TRY(s->ctx, hipMalloc(reinterpret_cast<void **>(&s->own_g), n * sizeof(float)));
    GF_HIP_TRY(s->ctx, hipMemsetAsync(s->own_p, 0, n * sizeof(float), s->ctx->stream));
    GF_HIP_TRY(s->ctx, hipMemsetAsync(s->own_g, 0, n * sizeof(float), s->ctx->stream));
    return GF_OK;
}
}  // namespace gf

using gf::fail;

extern "C" {

// ---- host-pointer mode of the driver: the handle owns the model, batches and results cross as host arrays -------------
gf_status gf_smp_parameters_upload(gf_smp *s, const float *host) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (!host) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_parameters_upload: null argument");
    gf_status st = gf::own_model(s);
    if (st != GF_OK) return st;
    GF_HIP_TRY(s->ctx, hipMemcpyAsync(s->own_p, host, gf::param_count(s->ucfg) * sizeof(float), hipMemcpyHostToDevice, s->ctx->stream));
    GF_HIP_TRY(s->ctx, hipStreamSynchronize(s->ctx->stream));
    return GF_OK;
}

gf_status gf_smp_parameters_download(gf_smp *s, float *host_params, float *host_grads) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (!s->own_p) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_parameters_download: no handle-owned model");
    const size_t bytes = gf::param_count(s->ucfg) * sizeof(float);
    if (host_params) GF_HIP_TRY(s->ctx, hipMemcpyAsync(host_params, s->own_p, bytes, hipMemcpyDeviceToHost, s->ctx->stream));
    if (host_grads) GF_HIP_TRY(s->ctx, hipMemcpyAsync(host_grads, s->own_g, bytes, hipMemcpyDeviceToHost, s->ctx->stream));
    GF_HIP_TRY(s->ctx, hipStreamSynchronize(s->ctx->stream));
    return GF_OK;
}

gf_status gf_smp_forward_host(gf_smp *s, const double *targets, double *predict, double *loss, double *graph_feature) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (s->cfg.readout)   // (in every state of the handle: its outputs are per pair, or a Gram matrix: not this call's per-molecule arrays)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_forward_host: the %s read-out (readout = %d) has no host-pointer forward: gf_smp_forward",
                    s->cfg.readout == 1 ? "pair" : "Gram", s->cfg.readout);
    if (s->cfg.covariant)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_forward_host: a covariant handle (CGCN_1D, CGCN_2D) has no host-pointer forward: gf_smp_forward");
    if (!s->prepared) return fail(ctx, GF_ERR_INVALID, "gf_smp_forward_host before gf_smp_prepare");
    if (!s->own_p) return fail(ctx, GF_ERR_INVALID, "gf_smp_forward_host: no handle-owned model (gf_smp_parameters_upload)");
    const int nMol = s->lay.nMol, C = s->ucfg.top_channels();
    gf_status st = GF_OK;
    if (!s->own_y) {
        st = gf::upload(s, &s->own_t, nullptr, (size_t)nMol);
        if (st == GF_OK) st = gf::upload(s, &s->own_y, nullptr, (size_t)nMol);
        if (st == GF_OK) st = gf::upload(s, &s->own_loss, nullptr, (size_t)nMol);
        if (st == GF_OK) st = gf::upload(s, &s->own_feat, nullptr, (size_t)nMol * C);
        if (st != GF_OK) return st;
    }
    std::vector<float> tmp((size_t)nMol * (C > 1 ? C : 1));
    if (targets) {
        for (int m = 0; m < nMol; ++m) tmp[m] = (float)targets[m];
        GF_HIP_TRY(ctx, hipMemcpyAsync(s->own_t, tmp.data(), sizeof(float) * nMol, hipMemcpyHostToDevice, ctx->stream));
        GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // tmp is reused below
    }
    st = gf_smp_forward(s, s->own_p, targets ? s->own_t : nullptr, s->own_y, s->own_loss, s->own_feat);
    if (st != GF_OK) return st;
    struct Out { double *dst; const float *src; size_t n; } outs[3] = {
        {predict, s->own_y, (size_t)nMol}, {targets ? loss : nullptr, s->own_loss, (size_t)nMol}, {graph_feature, s->own_feat, (size_t)nMol * C}};
    for (const Out &o : outs) {
        if (!o.dst) continue;
        GF_HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), o.src, sizeof(float) * o.n, hipMemcpyDeviceToHost, ctx->stream));
        GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < o.n; ++i) o.dst[i] = (double)tmp[i];
    }
    return GF_OK;
}

// One optimiser step of SMP_omega::BatchLearn (SMP_omega.h:820-821): grads hold the SUM over the batch (gf_smp_backward),
// Adam::Learn(learning_rate, nBatch) divides by nBatch.  Defaults of Adam.h:26-29: beta1 0.9, beta2 0.999, epsilon 1e-8.
gf_status gf_smp_adam_step(gf_smp *s, float *params, const float *grads, double learning_rate, int nBatch) {
    gf_status st = gf::optimiser_begin(s, &params, &grads, nBatch, "gf_smp_adam_step");
    if (st != GF_OK) return st;
    gf_ctx *ctx = s->ctx;
    const size_t n = gf::param_count(s->ucfg);
    GF_LAUNCH(ctx, "smp_adam", gf::adam_step, dim3(gf::grid_for(n)), dim3(256), 0, params, grads, s->adam_m, s->adam_v, n,
              learning_rate, 1.0 / (double)nBatch, s->adam_n, 0.9, 0.999, 1e-8);
    s->adam_n += n;   // (touches the moment buffers only, not the batch's: the handle's next gf_smp_prepare need not wait for it)
    s->optim.kind = gf::kOptimAdam;
    return GF_OK;
}

// The optimiser of the SMP_2D_ver6-8 models (sgd = new Momentum(momentum_param), SMP_2D_ver6.h:204).  Shares the handle's
// first moment buffer with Adam: a model uses one optimiser or the other.
gf_status gf_smp_momentum_step(gf_smp *s, float *params, const float *grads, double learning_rate, int nBatch, double gamma) {
    gf_status st = gf::optimiser_begin(s, &params, &grads, nBatch, "gf_smp_momentum_step");
    if (st != GF_OK) return st;
    gf_ctx *ctx = s->ctx;
    const size_t n = gf::param_count(s->ucfg);
    GF_LAUNCH(ctx, "smp_momentum", gf::momentum_step, dim3(gf::grid_for(n)), dim3(256), 0, params, grads, s->adam_m, n,
              learning_rate, 1.0 / (double)nBatch, gamma);
    s->optim.kind = gf::kOptimMomentum;
    return GF_OK;
}

// sgd->Learn(learning_rate, nBatch) for whichever of the reference's five optimisers `sgd` is (gf_optim_config.kind).  Kinds 0 and 1 are
// the two calls above, launch for launch; 2 .. 4 are smp_optimisers.hip's, over the handle's block table.  A kind other than the one the
// handle last stepped with is refused until gf_smp_adam_reset: the state buffers are shared.
gf_status gf_smp_optimiser_step(gf_smp *s, float *params, const float *grads, const gf_optim_config *cfg) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_status st = gf::optim_check(s->ctx, &s->optim, cfg, "gf_smp_optimiser_step");
    if (st != GF_OK) return st;
    if (cfg->kind == gf::kOptimAdam) return gf_smp_adam_step(s, params, grads, cfg->learning_rate, cfg->nBatch);
    if (cfg->kind == gf::kOptimMomentum) return gf_smp_momentum_step(s, params, grads, cfg->learning_rate, cfg->nBatch, cfg->gamma);
    st = gf::optimiser_begin(s, &params, &grads, cfg->nBatch, "gf_smp_optimiser_step");
    if (st != GF_OK) return st;
    std::vector<size_t> blocks;
    if (cfg->kind == gf::kOptimAdaMax && !s->optim.blocks) s->ucfg.each_registered([&blocks](size_t n) { blocks.push_back(n); });
    return gf::optim_step(s->ctx, &s->optim, blocks, params, grads, gf::param_count(s->ucfg), s->adam_m, s->adam_v, cfg, "gf_smp_optimiser_step");
}

// L1Regularization / L2Regularization over every registered parameter: the value to the host, grads += times * the term of backward()
gf_status gf_smp_regularise(gf_smp *s, const float *params, float *grads, int norm, double lambda, int times, double *value_host) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (!params && !grads && s->own_p) {
        params = s->own_p;
        grads = s->own_g;
    }
    return gf_regularise_f32(s->ctx, params, grads, gf::param_count(s->ucfg), norm, lambda, times, value_host);
}

// Adam::Learn(learning_rate, nBatch) (GraphFlow/Adam.h:106-133) on any flat parameter buffer with caller-owned moments:
// element i uses the bias-correction powers beta^(elements_before + i + 1) (the reference advances them per element).
gf_status gf_adam_step_f32(gf_ctx *ctx, float *params, const float *grads, float *m, float *v, size_t n, double learning_rate,
                           int nBatch, unsigned long long elements_before) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (!params || !grads || !m || !v || nBatch <= 0) return fail(ctx, GF_ERR_INVALID, "gf_adam_step_f32: bad argument");
    if (n == 0) return GF_OK;
    GF_LAUNCH(ctx, "smp_adam", gf::adam_step, dim3(gf::grid_for(n)), dim3(256), 0, params, grads, m, v, n, learning_rate,
              1.0 / (double)nBatch, elements_before, 0.9, 0.999, 1e-8);
    return GF_OK;
}

gf_status gf_smp_adam_reset(gf_smp *s) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (s->adam_m) {
        const size_t n = gf::param_count(s->ucfg);
        GF_HIP_TRY(s->ctx, hipMemsetAsync(s->adam_m, 0, n * sizeof(float), s->ctx->stream));
        GF_HIP_TRY(s->ctx, hipMemsetAsync(s->adam_v, 0, n * sizeof(float), s->ctx->stream));
    }
    s->adam_n = 0;
    return gf::optim_reset(s->ctx, &s->optim);   // no recorded kind, AdaMax's beta1_t and norms
}

// SMP_omega::weights_initialization (SMP_omega.h:334-338) = GraphFlow::uniform_init (GraphFlow.h:1297-1306) over the
// parameters in registration order, drawn from the C library's rand() exactly as the reference draws them: after the
// same srand() a model built here starts from the same weights as one built by the reference.  Host buffer, host only:
// gfsmp::resolve_config says what gf_smp_create / gf_smp_create_classifier would build, Config::level_blocks what it holds.
static gf_status uniform_init_host(const gf_smp_config *cfg, const gfsmp::ConfigEntry &entry, float *params) {
    gfsmp::Config c;
    char why[640];
    if (!params || gfsmp::resolve_config(cfg, entry, &c, why, sizeof why) != GF_OK) return GF_ERR_INVALID;
    const auto draw = [&params](const gfsmp::Config::Block &b) { gfsmp::uniform_draw(b, &params); };
    draw(c.first_block());
    c.shared_blocks().each_draw(draw);
    for (int l = 1; l <= c.nLevels; ++l) c.level_blocks(l).each_draw(draw);
    draw(c.readout_block());
    return GF_OK;
}
static size_t config_param_count(const gf_smp_config *cfg, const gfsmp::ConfigEntry &entry) {
    gfsmp::Config c;
    char why[640];
    return gfsmp::resolve_config(cfg, entry, &c, why, sizeof why) == GF_OK ? gf::param_count(c) : 0;
}
gf_status gf_smp_uniform_init_host(const gf_smp_config *cfg, float *params) { return uniform_init_host(cfg, gfsmp::kHandleEntry, params); }
size_t gf_smp_config_param_count(const gf_smp_config *cfg) { return config_param_count(cfg, gfsmp::kHandleEntry); }
size_t gf_smp_classifier_config_param_count(const gf_smp_config *cfg, int nClass) {
    return config_param_count(cfg, {gfsmp::ConfigEntry::Classifier, nClass, 0.0});
}
// ... of the `_classification` models (SMP_2D_ver6_classification.h:256-259): sgd->params holds Vector*, so W [nClass][C] is drawn by
// uniform_init(Vector*) like the rest, with the divisor 10 * nClass * C
gf_status gf_smp_classifier_uniform_init_host(const gf_smp_config *cfg, int nClass, float *params) {
    return uniform_init_host(cfg, {gfsmp::ConfigEntry::Classifier, nClass, 0.0}, params);
}

// Text checkpoints in the reference's format (SMP_omega.h:1033-1042 / :1044-1055): every parameter value in
// registration order, printed with the default ostream format (= "%g", 6 significant digits) followed by one blank.
gf_status gf_smp_save_model(const gf_smp *s, const float *params, const char *path) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp");
    if (!params) params = s->own_p;
    if (!params || !path) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_save_model: null argument");
    const size_t n = gf::param_count(s->ucfg);
    std::vector<float> host(n);
    GF_HIP_TRY(s->ctx, hipMemcpyAsync(host.data(), params, n * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream));
    GF_HIP_TRY(s->ctx, hipStreamSynchronize(s->ctx->stream));
    FILE *f = std::fopen(path, "w");
    if (!f) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_save_model: cannot open %s", path);
    bool ok = true;
    std::vector<size_t> order;   // (a distance handle: the classes write channel by channel, not in registration order)
    if (s->ucfg.distance_channel) gf::smp_distance_checkpoint_order(s->ucfg, &order);
    for (size_t i = 0; i < n && ok; ++i) ok = std::fprintf(f, "%g ", (double)host[order.empty() ? i : order[i]]) > 0;
    ok = (std::fclose(f) == 0) && ok;
    return ok ? GF_OK : fail(s->ctx, GF_ERR_INVALID, "gf_smp_save_model: write to %s failed", path);
}

gf_status gf_smp_load_model(gf_smp *s, float *params, const char *path) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp");
    if (!params) {
        gf_status st0 = gf::own_model(s);
        if (st0 != GF_OK) return st0;
        params = s->own_p;
    }
    if (!params || !path) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_load_model: null argument");
    const size_t n = gf::param_count(s->ucfg);
    FILE *f = std::fopen(path, "r");
    if (!f) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_load_model: cannot open %s", path);
    std::vector<float> host(n);
    size_t got = 0;
    double v;
    std::vector<size_t> order;   // (a distance handle: the classes' files go channel by channel)
    if (s->ucfg.distance_channel) gf::smp_distance_checkpoint_order(s->ucfg, &order);
    while (got < n && std::fscanf(f, "%lf", &v) == 1) {
        host[order.empty() ? got : order[got]] = (float)v;
        ++got;
    }
    std::fclose(f);
    // the reference would silently keep reading garbage; a short file is an error here
    if (got != n) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_load_model: %s holds %zu values, the model has %zu", path, got, n);
    GF_HIP_TRY(s->ctx, hipMemcpyAsync(params, host.data(), n * sizeof(float), hipMemcpyHostToDevice, s->ctx->stream));
    GF_HIP_TRY(s->ctx, hipStreamSynchronize(s->ctx->stream));
    return GF_OK;
}

}  // extern "C"
