// smp_field_level.hip -- the kernels more than one field level launches (smp_field_level.h names the levels), and the two functions a
// sweep calls for a level of a first-order, steerable or unrestricted handle.
//   size_grads, weight_views, wgrad_fold   SMP_theta and SMP_1D*: the per-size reduction of acc [nodes][3 Cc], the two views of a
//                                          [2 Cp][Cc] matrix and the fold of its gradient
//   readout_nodes, readout_bwd             the first-order read-out of a level (f_l[v] is [s][C]) and its reverse
//   gather_bwd                             df_{l-1} from dS: SMP_2D, _ver4, _ver5 (dS in the first Cp columns of df_l's rows) and the
//                                          unrestricted forms (dS in a buffer of its own)
// Every sum runs in a fixed order, no atomics; every output element is written by its kernel.
#include "smp_field_level.h"

namespace gf {
using namespace field_level;
namespace {

// The per-size gradients: one workgroup per size bucket (s, first node, count) -- the bucket's nodes are contiguous.  Thread (rr, c) sums
// the nodes rr, rr + rl, .. of channel c, the rl partials are folded in order, the lambda partials through one fixed tree.  `+=` into dsizes.
__global__ __launch_bounds__(256) void theta_size_grads(const float *__restrict__ acc, const int *__restrict__ bucket, float *__restrict__ dsizes,
                                                        int Cc) {
    __shared__ float red[256];
    const int s = bucket[3 * blockIdx.x], n0 = bucket[3 * blockIdx.x + 1], cnt = bucket[3 * blockIdx.x + 2];
    float *out = dsizes + (size_t)(s - 1) * (2 + Cc);
    const int lanes = Cc < 256 ? Cc : 256, rl = 256 / lanes;
    const int f0 = threadIdx.x % lanes, rr = threadIdx.x / lanes;
    float l1 = 0.f, l2 = 0.f;
    for (int fb = 0; fb < Cc; fb += lanes) {
        const int c = fb + f0;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (c < Cc && rr < rl)
            for (int n = n0 + rr; n < n0 + cnt; n += rl) {
                const float *a = acc + (size_t)n * 3 * Cc + c;
                a0 += a[0];
                a1 += a[Cc];
                a2 += a[2 * Cc];
            }
        l1 += a1;
        l2 += a2;
        red[threadIdx.x] = a0;
        __syncthreads();
        if (rr == 0 && c < Cc) {
            float t = 0.f;
            for (int k = 0; k < rl; ++k) t += red[k * lanes + f0];
            out[2 + c] += t;
        }
        __syncthreads();
    }
    for (int pass = 0; pass < 2; ++pass) {
        red[threadIdx.x] = pass ? l2 : l1;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[pass] += red[0];
        __syncthreads();
    }
}

// K [2Cp][Cc] (rows k Cp + ci) -> Kh [Cp][2Cc] (Kh[ci][k Cc + co] = K[k Cp + ci][co]) and Kt [2Cc][Cp] (Kt[k Cc + co][ci] = K[k Cp + ci][co])
__global__ void theta_weight_views(const float *__restrict__ K, float *__restrict__ Kh, float *__restrict__ Kt, int Cp, int Cc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * Cp * Cc) return;
    const int k = i / (Cp * Cc), r = i - k * Cp * Cc, ci = r / Cc, co = r - ci * Cc;
    const float v = K[i];
    Kh[(size_t)ci * 2 * Cc + k * Cc + co] = v;
    Kt[((size_t)k * Cc + co) * Cp + ci] = v;
}
// dK [2Cp][Cc] += dKh [Cp][2Cc] rearranged; one thread per element of dK
__global__ void theta_wgrad_fold(const float *__restrict__ dKh, float *__restrict__ dK, int Cp, int Cc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * Cp * Cc) return;
    const int k = i / (Cp * Cc), r = i - k * Cp * Cc, ci = r / Cc, co = r - ci * Cc;
    dK[i] += dKh[(size_t)ci * 2 * Cc + k * Cc + co];
}

// read-out of a level: sh[n][:] = sum over the node's s rows of f_l (ShrinkMatrix(f, 0), ShrinkMatrix.h:43-50), vf = LeakyReLU(sh) at the
// slope of LeakyReLU2D.h:31 (the LeakyReLU.h default)
__global__ void theta_readout_nodes(const float *__restrict__ f, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                    float *__restrict__ sh, float *__restrict__ vf, int C, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t n = i / C;
        const int s = node_s[n];
        const float *src = f + node_row[n] * C + c;
        float acc = 0.f;
        for (int r = 0; r < s; ++r) acc += src[(size_t)r * C];
        sh[i] = acc;
        vf[i] = lrelu(acc, 0.01f);
    }
}
// its reverse: df_l[n][r][:] (+)= dvec[n][:] at every row of the node (ShrinkMatrix::backward broadcasts)
__global__ void theta_readout_bwd(const float *__restrict__ dvec, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                  float *__restrict__ df, int C, size_t total, int accumulate) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t n = i / C;
        const int s = node_s[n];
        float *dst = df + node_row[n] * C + c;
        const float v = dvec[i];
        for (int r = 0; r < s; ++r) dst[(size_t)r * C] = accumulate ? dst[(size_t)r * C] + v : v;
    }
}

// Reverse gather of dS (rows of level l, `stride` floats apart, Cp columns read) into df_{l-1} [.][Cp]: source nodes [blockIdx.x * npw,
// + npw) of level l - 1.  SQ = false: items (node, position p, vector); SQ = true: items (node, column q, vector) walking the source's
// rows p, inv applied to both indices.
template <int V, bool SQ>
__global__ __launch_bounds__(256) void field_gather_bwd(const float *__restrict__ dS, float *__restrict__ out, const int *__restrict__ prev_s,
                                                        const long long *__restrict__ prev_row, const long long *__restrict__ cons_ptr,
                                                        const long long *__restrict__ cons_row, const int *__restrict__ cons_s,
                                                        const long long *__restrict__ inv_off, const short *__restrict__ inv, int Cp, int stride,
                                                        int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const Run run = pack_run(off, prev_s, nodes, npw, Cp / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, Cp / V);
        const int w = run.nb + x.j, sw = prev_s[w], q = x.pos, cq = x.cq;
        const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1], r0 = prev_row[w];
        if (!SQ) {
            Vf<V> g = vzero<V>();
            for (long long c = c0; c < c1; ++c) {
                const int i = inv[inv_off[c] + q];
                if (i < 0) continue;
                vadd(g, vld<V>(dS + (cons_row[c] + i) * stride + cq));
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
                vadd(g, vld<V>(dS + (cons_row[c] + (long long)i * cons_s[c] + j) * stride + cq));
            }
            vst<V>(out + (r0 + (long long)p * sw + q) * Cp + cq, g);
        }
    }
}

}  // namespace

gf_status smp_field_size_grads(gf_ctx *ctx, const float *acc, const int *bucket, int nbuckets, float *dsizes, int Cc) {
    GF_LAUNCH(ctx, "smpt_size_grads", theta_size_grads, dim3(nbuckets), dim3(256), 0, acc, bucket, dsizes, Cc);
    return GF_OK;
}
gf_status smp_field_weight_views(gf_ctx *ctx, const float *K, float *Kh, float *Kt, int Cp, int Cc) {
    GF_LAUNCH(ctx, "smpt_weight_views", theta_weight_views, dim3((2 * Cp * Cc + 255) / 256), dim3(256), 0, K, Kh, Kt, Cp, Cc);
    return GF_OK;
}
gf_status smp_field_wgrad_fold(gf_ctx *ctx, const float *dKh, float *dK, int Cp, int Cc) {
    GF_LAUNCH(ctx, "smpt_wgrad_fold", theta_wgrad_fold, dim3((2 * Cp * Cc + 255) / 256), dim3(256), 0, dKh, dK, Cp, Cc);
    return GF_OK;
}

gf_status smp_theta_readout(gf_smp *s, int l, float *sh, float *vf) {
    const gf_smp::DevLevel &d = s->lv[l];
    const size_t n = (size_t)s->lay.level[l].nNodes * s->cfg.level_channels(l);
    GF_LAUNCH(s->ctx, "smpt_readout_nodes", theta_readout_nodes, dim3(grid_for(n)), dim3(256), 0, d.f, d.node_s, d.node_row, sh, vf,
              s->cfg.level_channels(l), n);
    return GF_OK;
}

gf_status smp_theta_readout_backward(gf_smp *s, int l, const float *dvec, int accumulate) {
    const gf_smp::DevLevel &d = s->lv[l];
    const size_t n = (size_t)s->lay.level[l].nNodes * s->cfg.level_channels(l);
    GF_LAUNCH(s->ctx, "smpt_readout_bwd", theta_readout_bwd, dim3(grid_for(n)), dim3(256), 0, dvec, d.node_s, d.node_row, d.df,
              s->cfg.level_channels(l), n, accumulate);
    return GF_OK;
}

gf_status smp_field_gather_down(gf_smp *s, int l, const float *dS, int stride, bool square, const char *timer) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), np = s->lay.level[l - 1].nNodes, V = lane_vector(Cp);
    if (np == 0) return GF_OK;
    const RunGrid g = run_grid(s->lay.level[l - 1], square, Cp / V);
    return with_lane_vector(V, [&](auto v) -> gf_status {
        if (square)
            GF_LAUNCH(ctx, timer, (field_gather_bwd<v, true>), g.grid, dim3(256), 0, dS, pv.df, pv.node_s, pv.node_row, d.th_cons_ptr, d.th_cons_row,
                      d.th_cons_s, d.th_inv_off, d.th_inv, Cp, stride, np, g.npw);
        else
            GF_LAUNCH(ctx, timer, (field_gather_bwd<v, false>), g.grid, dim3(256), 0, dS, pv.df, pv.node_s, pv.node_row, d.th_cons_ptr, d.th_cons_row,
                      d.th_cons_s, d.th_inv_off, d.th_inv, Cp, stride, np, g.npw);
        return GF_OK;
    });
}

// The level of a handle whose levels are field levels (is_field_level(LevelKind)): cfg picks the file, in smp_level_kind's order
gf_status smp_field_forward_level(gf_smp *s, int l, const float *K, const float *sizes) {
    const gfsmp::Config &c = s->cfg;
    return (c.unrestricted ? smp_unrestricted_forward_level : c.first_order == 1 ? smp_theta_forward_level : c.first_order ? smp_1d_forward_level
            : c.steerable_2d == 5 ? smp_2d_ver5_forward_level : smp_2d_forward_level)(s, l, K, sizes);
}
gf_status smp_field_backward_level(gf_smp *s, int l, const float *K, const float *sizes, float *dK, float *dsizes, const float *node_df,
                                   bool rows_too, gf_status (*wgrad_done)(gf_smp *, int)) {
    const gfsmp::Config &c = s->cfg;
    return (c.unrestricted ? smp_unrestricted_backward_level : c.first_order == 1 ? smp_theta_backward_level : c.first_order ? smp_1d_backward_level
            : c.steerable_2d == 5 ? smp_2d_ver5_backward_level : smp_2d_backward_level)(s, l, K, sizes, dK, dsizes, node_df, rows_too, wgrad_done);
}

}  // namespace gf
