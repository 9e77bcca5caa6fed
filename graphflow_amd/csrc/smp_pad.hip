// smp_pad.hip -- the caller's layout (gf_smp::ucfg: what crosses the C ABI) against the device's (gf_smp::cfg, smp.hip: smp_derive_plan): channels
// padded to 16 / 32 / 64, or SMP_2D_ver6 / ver7 embedded in the 18-slice level on [f | f^T] channels.  Parameters are padded, gradients cropped.
#include "smp_internal.h"

namespace gf {
// The two parameter layouts.  Order H [C_0][FD], (K_l, b_l)..., W [C] ([nClass][C] on a classifier handle; no W in a physics tower); K_l is [18][C_{l-1}][C_l] as (k, ci, co)
// (SMP_omega.h:289-295; C_l = C, or halving per level in a tower) or, custom_matmul, [C][18 C] as (co, k, ci) (CustomMatMulTensor,
// SMP_2D_ver8).  The padded layout has Cc channels at every level.
struct PadMap {
    int L, nK, custom, FD, Cc, hasW, nW;   // nW: rows of W (Config::readout_rows)
    int cu[kPadMaxLevels + 1];          // the caller's channels of level l
    long long uoff[kPadMaxLevels + 2];  // the caller's offset of H (0), K_1, ..., K_L, W
};
static PadMap pad_map(const gfsmp::Config &u, const gfsmp::Config &c) {
    PadMap m = {};
    m.L = u.nLevels, m.nK = u.nContractions, m.custom = u.custom_matmul, m.FD = u.fdim(), m.Cc = c.nChanels, m.hasW = u.physics ? 0 : 1, m.nW = u.readout_rows();
    for (int l = 0; l <= m.L; ++l) m.cu[l] = u.level_channels(l);
    m.uoff[0] = 0;
    m.uoff[1] = (long long)m.cu[0] * m.FD;
    for (int l = 1; l <= m.L; ++l) m.uoff[l + 1] = m.uoff[l] + (long long)m.nK * m.cu[l - 1] * m.cu[l] + m.cu[l];
    return m;
}
// element i of the PADDED parameter vector -> its place in the caller's, or -1 (a padded weight: zero)
__device__ __forceinline__ long long padded_to_user(long long i, const PadMap &m) {
    const int Cc = m.Cc;
    const long long hpad = (long long)Cc * m.FD;
    if (i < hpad) {
        const int c = (int)(i / m.FD);
        return c < m.cu[0] ? i : -1;   // (same index: rows c < C_0 come first in both layouts)
    }
    i -= hpad;
    const long long lvl_pad = (long long)m.nK * Cc * Cc + Cc;
    const long long lq = i / lvl_pad;
    if (lq < m.L) {
        const int l = (int)lq + 1, Ci = m.cu[l - 1], Co = m.cu[l];
        const long long j = i - lq * lvl_pad, base = m.uoff[l];
        if (j >= (long long)m.nK * Cc * Cc) {   // bias
            const long long c = j - (long long)m.nK * Cc * Cc;
            return c < Co ? base + (long long)m.nK * Ci * Co + c : -1;
        }
        int k, ci, co;
        if (m.custom) {
            co = (int)(j / ((long long)m.nK * Cc));
            const long long r = j % ((long long)m.nK * Cc);
            k = (int)(r / Cc), ci = (int)(r % Cc);
            return (co < Co && ci < Ci) ? base + (long long)co * m.nK * Ci + (long long)k * Ci + ci : -1;
        }
        k = (int)(j / ((long long)Cc * Cc));
        const long long r = j % ((long long)Cc * Cc);
        ci = (int)(r / Cc), co = (int)(r % Cc);
        return (ci < Ci && co < Co) ? base + ((long long)k * Ci + ci) * Co + co : -1;
    }
    const long long c = i - (long long)m.L * lvl_pad;   // W [nW][Cc]
    const long long r = c / Cc, f = c % Cc;
    return (m.hasW && r < m.nW && f < m.cu[m.L]) ? m.uoff[m.L + 1] + r * m.cu[m.L] + f : -1;
}
__global__ void pad_parameters(const float *__restrict__ user, float *__restrict__ padded, long long n_padded, PadMap m) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_padded) return;
    const long long u = padded_to_user(i, m);
    padded[i] = u >= 0 ? user[u] : 0.f;
}
__global__ void crop_gradients(const float *__restrict__ padded, float *__restrict__ user, long long n_padded, PadMap m, int accumulate) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_padded) return;
    const long long u = padded_to_user(i, m);
    if (u >= 0) user[u] = accumulate ? user[u] + padded[i] : padded[i];
}
// ---- SMP_2D_ver6 on the 18-slice level (gf_smp::dup_channels) --------------------------------------------------------------------
// RisiContraction_10's slice k (RisiContraction_10.h:94-142 = cases 1..10 of RisiContraction_50.h) as (slot of RisiContraction_18, input
// group 0 = f, 1 = f^T), for a SYMMETRIC reduced adjacency (row sums = column sums; checked numerically against the oracle, all 18 slots
// on P and on P with b and c swapped):
//   1 (a,b) -> slot 0 on f        2 (a,c) -> slot 0 on f^T      3 (a,d), 4 (a,e) -> slot 1 on f       5 (b,c) -> slot 2 on f
//   6 (b,d), 7 (b,e) -> slot 3 on f          8 (c,d), 9 (c,e) -> slot 3 on f^T          10 (d,e) -> slot 4 on f
// Two slices that share a slot share its padded weight block: the block holds their SUM (the level is linear in K), and both receive
// the block's gradient.
__device__ __forceinline__ void v6_slot(int k, int *slot, int *grp) {
    const int sl[10] = {0, 0, 1, 1, 2, 3, 3, 3, 3, 4}, gr[10] = {0, 1, 0, 0, 0, 0, 0, 1, 1, 0};
    *slot = sl[k];
    *grp = gr[k];
}
// RisiContraction_50's cases 1..50 (RisiContraction_50.h:94-430) the same way; slots 18, 19, 20 = the extra products (S_ab, 1), (S_bc, 1),
// (S_bc, tr) of gf_smp::n_extra (cases 41 / 42, 45, 25 with the reduced adjacency's unit diagonal).  At most two cases share a block.
__device__ __forceinline__ void v7_slot(int k, int *slot, int *grp) {
    const signed char sl[50] = {0, 0, 1, 1, 2, 3, 3, 3, 3, 4,   5, 5, 6, 5, 5, 6, 7, 8, 8, 7,   8, 8, 9, 9, 20, 10, 11, 12, 10, 11,
                                12, 10, 11, 12, 10, 11, 12, 13, 13, 14,   18, 18, 15, 15, 19, 16, 16, 16, 16, 17};
    const signed char gr[50] = {0, 1, 0, 0, 0, 0, 0, 1, 1, 0,   0, 0, 0, 1, 1, 1, 0, 0, 1, 0,   0, 1, 0, 0, 0, 0, 0, 0, 0, 0,
                                0, 1, 1, 1, 1, 1, 1, 0, 1, 0,   0, 1, 0, 0, 0, 0, 0, 1, 1, 0};
    *slot = sl[k];
    *grp = gr[k];
}
// the caller's parameter u -> its (only) place in the padded [H | (K_l [18 Cc][Cc], b_l [Cc]) x L | W [nW][Cc] | X_1 .. X_L] vector
__device__ __forceinline__ long long v6_user_to_padded(long long u, const PadMap &m) {
    const int C = m.cu[0], Cc = m.Cc, nK = m.nK;
    if (u < m.uoff[1]) return u;   // H: rows c < C first in both layouts
    const long long hpad = (long long)Cc * m.FD, lvl_pad = 18ll * Cc * Cc + Cc;
    for (int l = 1; l <= m.L; ++l) {
        if (u >= m.uoff[l + 1]) continue;
        const long long j = u - m.uoff[l], base = hpad + (l - 1) * lvl_pad;
        if (j >= (long long)nK * C * C) return base + 18ll * Cc * Cc + (j - (long long)nK * C * C);   // bias
        int k, ci, co;
        if (m.custom) {   // [C][nK C]
            co = (int)(j / (nK * C));
            const int r = (int)(j % (nK * C));
            k = r / C, ci = r % C;
        } else {          // [nK C][C]
            k = (int)(j / ((long long)C * C));
            const int r = (int)(j % ((long long)C * C));
            ci = r / C, co = r % C;
        }
        int slot, grp;
        if (nK == 10) v6_slot(k, &slot, &grp);
        else v7_slot(k, &slot, &grp);
        if (slot >= 18)   // an extra product's block
            return hpad + m.L * lvl_pad + (long long)m.nW * Cc + ((long long)(l - 1) * 3 + (slot - 18)) * Cc * Cc + (long long)(grp * C + ci) * Cc + co;
        return base + ((long long)slot * Cc + grp * C + ci) * Cc + co;
    }
    const long long w = u - m.uoff[m.L + 1];   // W [nW][C] -> [nW][Cc]
    return hpad + m.L * lvl_pad + (w / C) * Cc + w % C;
}
__global__ void v6_pad_parameters(const float *__restrict__ user, float *__restrict__ padded, long long n_user, PadMap m) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_user) return;
    atomicAdd(padded + v6_user_to_padded(u, m), user[u]);   // (padded starts at zero; at most two terms per entry: the order cannot matter)
}
__global__ void v6_crop_gradients(const float *__restrict__ padded, float *__restrict__ user, long long n_user, PadMap m, int accumulate) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_user) return;
    const float g = padded[v6_user_to_padded(u, m)];
    user[u] = accumulate ? user[u] + g : g;
}
// f [rows][Cc]: channels [C, 2C) of row (x, y) <- channels [0, C) of row (y, x) of the same node (trow; null: level 0, one row per node);
// pmax [panels][Cc] (or null): the per-panel channel maxima combine-forward left, copied likewise (a level-wide maximum is all they serve)
__global__ void dup_transposed_channels(float *__restrict__ f, const int *__restrict__ trow, long long rows, int C, int Cc, float *__restrict__ pmax,
                                        long long panels) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * C) {
        const long long r = i / C;
        const int c = (int)(i % C);
        const long long t = trow ? trow[r] : r;
        f[r * Cc + C + c] = f[t * Cc + c];
    } else if (pmax && i < rows * C + panels * C) {
        const long long j = i - rows * C;
        pmax[(j / C) * Cc + C + j % C] = pmax[(j / C) * Cc + j % C];
    }
}
// the reverse: df[(x, y)][c] += df[(y, x)][C + c], and the upper channels (read exactly once, by this thread) are cleared
__global__ void fold_transposed_channels(float *__restrict__ df, const int *__restrict__ trow, long long rows, int C, int Cc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * C) return;
    const long long r = i / C;
    const int c = (int)(i % C);
    const long long t = trow ? trow[r] : r;
    df[r * Cc + c] += df[t * Cc + C + c];
    df[t * Cc + C + c] = 0.f;
}
gf_status dup_level(gf_smp *s, int l) {
    if (!s->dup_channels) return GF_OK;
    const gf_smp::DevLevel &d = s->lv[l];
    const long long rows = l == 0 ? s->lay.level[0].nNodes : s->lay.level[l].rows;
    if (l > 0 && !d.trow) return fail(s->ctx, GF_ERR_UNSUPPORTED, "SMP_2D_ver6 on the fused level: level %d has no transposed-row table", l);
    const bool pm = l > 0 && d.pmax && d.pmax_ready;
    const long long panels = pm ? d.fwd_npanels : 0, n = (rows + panels) * s->dup_channels;
    GF_LAUNCH(s->ctx, "smp_dup_transposed", dup_transposed_channels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d.f, l == 0 ? (const int *)nullptr : d.trow,
              rows, s->dup_channels, s->cfg.nChanels, pm ? d.pmax : (float *)nullptr, panels);
    return GF_OK;
}
gf_status fold_level(gf_smp *s, int l) {
    if (!s->dup_channels) return GF_OK;
    const gf_smp::DevLevel &d = s->lv[l];
    const long long rows = l == 0 ? s->lay.level[0].nNodes : s->lay.level[l].rows, n = rows * s->dup_channels;
    GF_LAUNCH(s->ctx, "smp_fold_transposed", fold_transposed_channels, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d.df,
              l == 0 ? (const int *)nullptr : d.trow, rows, s->dup_channels, s->cfg.nChanels);
    return GF_OK;
}
// ---- the extra products of SMP_2D_ver7 (gf_smp::n_extra) on an OP-BY-OP level: the tables are slices of Q -- slice 0 = tot S_ab, slice 2 =
// tot S_bc (RisiContraction_18's cases 1 and 5) -- so the products take the row factors (1 / tot, tr / tot)
__global__ void invert_rowscale(const float2 *__restrict__ rowscale, float2 *__restrict__ inv, long long rows) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const float2 v = rowscale[i];
    inv[i] = make_float2(1.f / v.x, v.y / v.x);   // (tot >= the trace >= 1: a reduced adjacency has a unit diagonal)
}
static gf_status extra_rs_inv(gf_smp *s, int l) {
    const long long rows = s->lay.level[l].rows;
    if (s->rs_inv_rows < (size_t)rows) {
        if (s->rs_inv) (void)hipFree(s->rs_inv);
        s->rs_inv = nullptr;
        s->rs_inv_rows = 0;
        GF_HIP_TRY(s->ctx, hipMalloc(reinterpret_cast<void **>(&s->rs_inv), sizeof(float) * 2 * (size_t)rows));
        s->rs_inv_rows = (size_t)rows;
    }
    GF_LAUNCH(s->ctx, "smp_extra_rowscale", invert_rowscale, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0,
              reinterpret_cast<const float2 *>(s->lv[l].rowscale), reinterpret_cast<float2 *>(s->rs_inv), rows);
    return GF_OK;
}
// forward: f_l (before bias and LeakyReLU) += (Q_0 / tot) X_a + (Q_2 / tot) X_b + (tr Q_2 / tot) X_c
gf_status extra_products_forward(gf_smp *s, int l) {
    if (!s->n_extra) return GF_OK;
    gf_ctx *ctx = s->ctx;
    if (!s->extra_w) return fail(ctx, GF_ERR_INVALID, "level %d: the extra products' weights are not bound", l);
    gf_status st = extra_rs_inv(s, l);
    if (st != GF_OK) return st;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, KC = 18 * C, rows = (int)s->lay.level[l].rows;
    const float *X = s->extra_w + (size_t)(l - 1) * 3 * C * C;
    st = gemm_rs(ctx, false, false, rows, C, C, d.Q, KC, 0, X, C, 0, d.f, C, 0, 1, 1, s->rs_inv, 2, 0);
    if (st == GF_OK) st = gemm_rs(ctx, false, false, rows, C, C, d.Q + 2 * C, KC, 0, X + (size_t)C * C, C, 0, d.f, C, 0, 1, 1, s->rs_inv, 2, 0);
    if (st == GF_OK) st = gemm_rs(ctx, false, false, rows, C, C, d.Q + 2 * C, KC, 0, X + 2 * (size_t)C * C, C, 0, d.f, C, 0, 1, 1, s->rs_inv, 2, 1);
    return st;
}
// backward, first half (Q still holds the forward's slices, d.df = dZ): dX
gf_status extra_products_wgrad(gf_smp *s, int l) {
    if (!s->n_extra) return GF_OK;
    gf_ctx *ctx = s->ctx;
    if (!s->extra_w || !s->extra_g) return fail(ctx, GF_ERR_INVALID, "level %d: the extra products' weights are not bound", l);
    gf_status st = extra_rs_inv(s, l);
    if (st != GF_OK) return st;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, KC = 18 * C, rows = (int)s->lay.level[l].rows;
    float *dX = s->extra_g + (size_t)(l - 1) * 3 * C * C;
    st = gemm_rs(ctx, true, false, C, C, rows, d.Q, KC, 0, d.df, C, 0, dX, C, 0, 1, 0, s->rs_inv, 2, 0);
    if (st == GF_OK) st = gemm_rs(ctx, true, false, C, C, rows, d.Q + 2 * C, KC, 0, d.df, C, 0, dX + (size_t)C * C, C, 0, 1, 0, s->rs_inv, 2, 0);
    if (st == GF_OK) st = gemm_rs(ctx, true, false, C, C, rows, d.Q + 2 * C, KC, 0, d.df, C, 0, dX + 2 * (size_t)C * C, C, 0, 1, 0, s->rs_inv, 2, 1);
    return st;
}
// ... second half (Q now holds dQ): dQ_0 += (dZ / tot) X_a^T, dQ_2 += (dZ / tot) X_b^T + (tr dZ / tot) X_c^T
gf_status extra_products_backward(gf_smp *s, int l) {
    if (!s->n_extra) return GF_OK;
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.nChanels, KC = 18 * C, rows = (int)s->lay.level[l].rows;
    const float *X = s->extra_w + (size_t)(l - 1) * 3 * C * C;
    gf_status st = gemm_rs(ctx, false, true, rows, C, C, d.df, C, 0, X, C, 0, d.Q, KC, 0, 1, 1, s->rs_inv, 2, 0);
    if (st == GF_OK) st = gemm_rs(ctx, false, true, rows, C, C, d.df, C, 0, X + (size_t)C * C, C, 0, d.Q + 2 * C, KC, 0, 1, 1, s->rs_inv, 2, 0);
    if (st == GF_OK) st = gemm_rs(ctx, false, true, rows, C, C, d.df, C, 0, X + 2 * (size_t)C * C, C, 0, d.Q + 2 * C, KC, 0, 1, 1, s->rs_inv, 2, 1);
    return st;
}
// floats of the device's parameter / gradient vector (the extra products' blocks behind the padded layout: gf_smp::n_extra)
static size_t padded_param_count(const gf_smp *s) {
    return param_count(s->cfg) + (size_t)s->cfg.nLevels * s->n_extra * s->cfg.nChanels * s->cfg.nChanels;
}
// the handle's padded copies of the caller's parameters / of the gradients of the running step
static gf_status pad_buffers(gf_smp *s) {
    if (s->pad_p && s->pad_g) return GF_OK;
    const size_t n = padded_param_count(s);
    if (!s->pad_p) GF_HIP_TRY(s->ctx, hipMalloc(reinterpret_cast<void **>(&s->pad_p), n * sizeof(float)));
    if (!s->pad_g && hipMalloc(reinterpret_cast<void **>(&s->pad_g), n * sizeof(float)) != hipSuccess) {
        // (both or neither: a later call must not find pad_p set and skip the gradient buffer)
        (void)hipGetLastError();
        s->pad_g = nullptr;
        (void)hipFree(s->pad_p);
        s->pad_p = nullptr;
        return fail(s->ctx, GF_ERR_NOMEM, "padded gradient buffer: %zu bytes", n * sizeof(float));
    }
    return GF_OK;
}
gf_status pad_params_now(gf_smp *s, const float *params) {
    gf_status st = pad_buffers(s);
    if (st != GF_OK) return st;
    const long long n = (long long)padded_param_count(s), nu = (long long)param_count(s->ucfg);
    if (s->dup_channels) {
        GF_HIP_TRY(s->ctx, hipMemsetAsync(s->pad_p, 0, (size_t)n * sizeof(float), s->ctx->stream));
        GF_LAUNCH(s->ctx, "smp_pad_params", v6_pad_parameters, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, params, s->pad_p, nu, pad_map(s->ucfg, s->cfg));
    } else {
        GF_LAUNCH(s->ctx, "smp_pad_params", pad_parameters, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, params, s->pad_p, n, pad_map(s->ucfg, s->cfg));
    }
    return GF_OK;
}
gf_status crop_grads_now(gf_smp *s, float *grads, int accumulate) {
    const long long n = (long long)param_count(s->cfg), nu = (long long)param_count(s->ucfg);
    const PadMap m = pad_map(s->ucfg, s->cfg);
    if (s->dup_channels)
        GF_LAUNCH(s->ctx, "smp_crop_grads", v6_crop_gradients, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, s->pad_g, grads, nu, m, accumulate ? 1 : 0);
    else
        GF_LAUNCH(s->ctx, "smp_crop_grads", crop_gradients, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->pad_g, grads, n, m, accumulate ? 1 : 0);
    return GF_OK;
}
// the handle's padded feature rows ([nMol][feature width of cfg]): the device's graph features, or the caller's feature gradient padded
gf_status pad_feature_buffer(gf_smp *s) {
    const size_t n = (size_t)s->lay.nMol * (s->cfg.physics ? feature_width(s->cfg) : (size_t)s->cfg.nChanels);
    if (s->pad_feat_n >= n) return GF_OK;
    if (s->pad_feat) (void)hipFree(s->pad_feat);
    s->pad_feat = nullptr;
    s->pad_feat_n = 0;
    GF_HIP_TRY(s->ctx, hipMalloc(reinterpret_cast<void **>(&s->pad_feat), n * sizeof(float)));
    s->pad_feat_n = n;
    return GF_OK;
}
// feature rows between the two layouts, level block by level block (one block outside the towers): to_user crops, else pads (the
// caller's columns into a zeroed padded row)
gf_status copy_feature_blocks(gf_smp *s, float *user, float *padded, bool to_user) {
    gf_ctx *ctx = s->ctx;
    const int nMol = s->lay.nMol, Cc = s->cfg.nChanels;
    const int nblk = s->cfg.physics ? s->cfg.nLevels + 1 : 1;
    const size_t wu = s->cfg.physics ? feature_width(s->ucfg) : (size_t)s->ucfg.nChanels, wp = (size_t)nblk * Cc;
    if (!to_user) GF_HIP_TRY(ctx, hipMemsetAsync(padded, 0, (size_t)nMol * wp * sizeof(float), ctx->stream));
    size_t uo = 0;
    for (int l = 0; l < nblk; ++l) {
        const size_t cu = s->cfg.physics ? (size_t)s->ucfg.level_channels(l) : (size_t)s->ucfg.nChanels;
        float *pu = user + uo, *pp = padded + (size_t)l * Cc;
        if (to_user)
            GF_HIP_TRY(ctx, hipMemcpy2DAsync(pu, wu * sizeof(float), pp, wp * sizeof(float), cu * sizeof(float), (size_t)nMol, hipMemcpyDeviceToDevice,
                                             ctx->stream));
        else
            GF_HIP_TRY(ctx, hipMemcpy2DAsync(pp, wp * sizeof(float), pu, wu * sizeof(float), cu * sizeof(float), (size_t)nMol, hipMemcpyDeviceToDevice,
                                             ctx->stream));
        uo += cu;
    }
    return GF_OK;
}
}  // namespace gf
