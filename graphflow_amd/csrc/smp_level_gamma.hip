// smp_level_gamma.hip -- the SMP_gamma level (GraphFlow/SMP_gamma.h: RisiContraction_4, no receptive-field cap, no reduced adjacency)
// without the promoted stack and with its block products on the rows of the level BELOW.
//
// Node v with field (x_1 .. x_s), child w_a = x_a with positions pi_a(.), P[a][i][j] = f_{l-1}[w_a][pi_a(i), pi_a(j)] (0 outside w_a's
// field).  RisiContraction_4.h cases 1-4 and the K-projection (Reshape2D + MatMul, SMP_gamma.h:206-211, K_l = [K0; K1; K2; K3]) give
//   z[x,y] = b + S_ab[x,y] K0 + S_bc[x,y] K1 + Pc[x,y] K2 + Pd[x,y] K3,   f_l = LeakyReLU(z)
//   S_ab[x,y] = sum_c P[x,y,c]   S_bc[x,y] = sum_a P[a,x,y]   Pc[x,y] = P[x,x,y]   Pd[x,y] = P[x,y,y].
// Every block is a sum of entries of f_{l-1} picked by the selection maps, and K acts on the channel axis only, so the products commute
// with the gathers: with G_k = f_{l-1} K_k (one GEMM over the rows of level l - 1, [rows_{l-1}][4C])
//   z[x,y] = b + sum_c G0[w_x][pi_x(y), pi_x(c)] + sum_a G1[w_a][pi_a(x), pi_a(y)] + G2[w_x][pi_x(x), pi_x(y)] + G3[w_x][pi_x(y), pi_x(y)].
// The product runs on sum s_{l-1}^2 rows instead of sum s_l^2 (a third of them at cfg3's top level), the four-block table T of level l
// is never formed, and the gather applies bias + LeakyReLU and stores f_l directly.  Backward, with dz = df_l * lrelu'(z):
//   dG[w][p,q] = sum over the consumers (n, a) of w, b / c the positions of p / q in n's field, of
//                [ dz_n[a,b] | dz_n[b,c] | [b=a] dz_n[a,c] | [b=c] dz_n[a,b] ]
//   dK_k = f_{l-1}^T dG_k,   df_{l-1} = sum_k dG_k K_k^T
// -- again products over the rows of level l - 1.  P, dP, T and dT never exist.  Every sum runs in a fixed order (positions, children,
// consumers ascending), the GEMMs are the deterministic ones of mixers.hip: bit-reproducible, no atomics.  Both gathers write every
// element of their outputs, so nothing downstream reads memory that nobody wrote.
#include "smp_internal.h"

namespace gf {
namespace {

constexpr float kGammaAlpha = 0.01f;  // LeakyReLU3D.h:41

__device__ __forceinline__ void add4(float4 &a, const float4 &b) {
    a.x += b.x;
    a.y += b.y;
    a.z += b.z;
    a.w += b.w;
}
__device__ __forceinline__ float lrelu(float z) { return z > 0.f ? z : kGammaAlpha * z; }

// One workgroup per (node n, child x) pair; items (y, channel quad) over s * C / 4, the quad fastest.  G rows are 4C floats = C float4.
__global__ __launch_bounds__(128) void gamma_level_fwd(const float *__restrict__ G, const float *__restrict__ bias, float *__restrict__ f,
                                                       const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                       const long long *__restrict__ node_pair, const int *__restrict__ pair_node,
                                                       const long long *__restrict__ pair_src_row, const int *__restrict__ pair_src_s,
                                                       const short *__restrict__ pi, int C) {
    const long long e = blockIdx.x;
    const int n = pair_node[e];
    const int s = node_s[n], x = (int)(e - node_pair[n]), swx = pair_src_s[e];
    const long long r0 = node_row[n], e0 = node_pair[n];
    const short *mx = pi + r0 + (long long)x * s;
    const int Q = C >> 2, px = mx[x];   // (px >= 0: w_x's field holds w_x)
    const float4 *G4 = reinterpret_cast<const float4 *>(G);
    const float4 *gx = G4 + pair_src_row[e] * C;   // first row of w_x
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x; i < s * Q; i += blockDim.x) {
        const int y = i / Q, q = i - y * Q;
        const int py = mx[y];
        float4 sab = z4, sbc = z4, pc = z4, pd = z4;
        if (py >= 0) {
            const float4 *row = gx + (size_t)py * swx * C + q;   // G[w_x][pi_x(y), .]
            for (int c = 0; c < s; ++c) {
                const int pcc = mx[c];
                if (pcc >= 0) add4(sab, row[(size_t)pcc * C]);
            }
            pd = row[(size_t)py * C + 3 * Q];
            if (px >= 0) pc = gx[((size_t)px * swx + py) * C + 2 * Q + q];
        }
        for (int a = 0; a < s; ++a) {
            const short *ma = pi + r0 + (long long)a * s;
            const int pa = ma[x], pb = ma[y];
            if (pa >= 0 && pb >= 0) add4(sbc, G4[(pair_src_row[e0 + a] + (long long)pa * pair_src_s[e0 + a] + pb) * C + Q + q]);
        }
        const float4 bb = reinterpret_cast<const float4 *>(bias)[q];
        float4 o;
        o.x = lrelu(((sab.x + sbc.x) + (pc.x + pd.x)) + bb.x);
        o.y = lrelu(((sab.y + sbc.y) + (pc.y + pd.y)) + bb.y);
        o.z = lrelu(((sab.z + sbc.z) + (pc.z + pd.z)) + bb.z);
        o.w = lrelu(((sab.w + sbc.w) + (pc.w + pd.w)) + bb.w);
        reinterpret_cast<float4 *>(f)[(r0 + (long long)x * s + y) * Q + q] = o;
    }
}

// One workgroup per source node w of level l - 1; items (p, q, channel quad) over s_w^2 C / 4.  dz rows are C floats (Q float4), dG
// rows 4C floats (C float4).
__global__ __launch_bounds__(256) void gamma_level_bwd(const float *__restrict__ dz, float *__restrict__ dG, const int *__restrict__ prev_s,
                                                       const long long *__restrict__ prev_row, const long long *__restrict__ cons_ptr,
                                                       const long long *__restrict__ cons_row, const int *__restrict__ cons_s,
                                                       const int *__restrict__ cons_a, const long long *__restrict__ cons_inv_off,
                                                       const short *__restrict__ inv, int C) {
    const int w = blockIdx.x;
    const int sw = prev_s[w], Q = C >> 2;
    const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1];
    const float4 *d4 = reinterpret_cast<const float4 *>(dz);
    float4 *dst = reinterpret_cast<float4 *>(dG) + prev_row[w] * C;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x; i < sw * sw * Q; i += blockDim.x) {
        const int q4 = i % Q, pq = i / Q;
        const int p = pq / sw, q = pq - p * sw;
        float4 g0 = z4, g1 = z4, g2 = z4, g3 = z4;
        for (long long e = c0; e < c1; ++e) {
            const short *iv = inv + cons_inv_off[e];
            const int b = iv[p], c = iv[q];
            if (b < 0 || c < 0) continue;
            const int s = cons_s[e], a = cons_a[e];
            const long long R = cons_row[e];
            const float4 zab = d4[(R + (long long)a * s + b) * Q + q4];
            add4(g0, zab);                                               // S_ab:  z[a, b] for every c
            add4(g1, d4[(R + (long long)b * s + c) * Q + q4]);           // S_bc:  z[b, c]
            if (b == a) add4(g2, d4[(R + (long long)a * s + c) * Q + q4]);   // Pc: z[a, c]
            if (b == c) add4(g3, zab);                                   // Pd:    z[a, b]
        }
        float4 *o = dst + (size_t)pq * C + q4;
        o[0] = g0;
        o[Q] = g1;
        o[2 * Q] = g2;
        o[3 * Q] = g3;
    }
}

// K [4C][C] (rows k C + ci) -> Kh [C][4C] (Kh[ci][k C + co] = K[k C + ci][co]) and Kt [4C][C] (Kt[k C + co][ci] = K[k C + ci][co])
__global__ void gamma_weight_views(const float *__restrict__ K, float *__restrict__ Kh, float *__restrict__ Kt, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * C * C) return;
    const int k = i / (C * C), r = i - k * C * C, ci = r / C, co = r - ci * C;
    const float v = K[i];
    Kh[(size_t)ci * 4 * C + k * C + co] = v;
    Kt[((size_t)k * C + co) * C + ci] = v;
}
// dK [4C][C] += dKh [C][4C] rearranged (dK[k C + ci][co] += dKh[ci][k C + co]); one thread per element of dK
__global__ void gamma_wgrad_fold(const float *__restrict__ dKh, float *__restrict__ dK, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * C * C) return;
    const int k = i / (C * C), r = i - k * C * C, ci = r / C, co = r - ci * C;
    dK[i] += dKh[(size_t)ci * 4 * C + k * C + co];
}

}  // namespace

bool smp_gamma_fused(const gf_smp *s, int l) {
    const int C = s->cfg.nChanels;
    if (!s->fused || s->cfg.nContractions != 4 || !s->cfg.square()) return false;
    if (C % 4 != 0 || C > 64) return false;   // (wider models, or C % 4 != 0 unpadded: the op-by-op level on the batched `_4` kernels)
    const gfsmp::LevelLayout &h = s->lay.level[l];
    return !h.buckets.empty() && h.buckets.back().s <= kFusedMaxField && s->lv[l].Wst && s->lv[l].dWst;
}

// G = f_{l-1} [K0 | K1 | K2 | K3] into the level's Q buffer, then the gather with bias + LeakyReLU into f_l
gf_status smp_gamma_forward_level(gf_smp *s, int l, const float *Kl, const float *bl) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int C = s->cfg.nChanels;
    const long long rows_p = s->lay.level[l - 1].rows, pairs = s->lay.level[l].pairs;
    float *Kh = d.Wst, *Kt = d.Wst + (size_t)4 * C * C;
    GF_LAUNCH(ctx, "smpg_weight_views", gamma_weight_views, dim3((4 * C * C + 255) / 256), dim3(256), 0, Kl, Kh, Kt, C);
    gf_status st = gemm(ctx, false, false, (int)rows_p, 4 * C, C, pv.f, C, 0, Kh, 4 * C, 0, d.Q, 4 * C, 0, 1, 0);
    if (st != GF_OK || pairs == 0) return st;
    GF_LAUNCH(ctx, "smpg_level_fwd", gamma_level_fwd, dim3((unsigned)pairs), dim3(128), 0, d.Q, bl, d.f, d.node_s, d.node_row, d.node_pair,
              d.pair_node, d.pair_src_row, d.pair_src_s, d.pi, C);
    return GF_OK;
}

// d.df holds dz (lrelu_backward_colsum ran): dG into the level's Q buffer, dK_l += f_{l-1}^T dG (rearranged), df_{l-1} = dG Kt.
// The weight gradient is final before df_{l-1} is formed; *wgrad_done is called in between (the data-parallel all-reduce of the level).
gf_status smp_gamma_backward_level(gf_smp *s, int l, const float *Kl, float *dKl, gf_status (*wgrad_done)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int C = s->cfg.nChanels;
    const long long rows_p = s->lay.level[l - 1].rows;
    const int np = s->lay.level[l - 1].nNodes;
    // (the views again: this sweep's parameters need not be the forward's)
    GF_LAUNCH(ctx, "smpg_weight_views", gamma_weight_views, dim3((4 * C * C + 255) / 256), dim3(256), 0, Kl, d.Wst, d.Wst + (size_t)4 * C * C, C);
    if (np > 0)
        GF_LAUNCH(ctx, "smpg_level_bwd", gamma_level_bwd, dim3((unsigned)np), dim3(256), 0, d.df, d.Q, pv.node_s, pv.node_row, d.cons_ptr, d.cons_row,
                  d.cons_s, d.cons_a, d.cons_inv_off, d.inv, C);
    gf_status st = gemm(ctx, true, false, C, 4 * C, (int)rows_p, pv.f, C, 0, d.Q, 4 * C, 0, d.dWst, 4 * C, 0, 1, 0);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "smpg_wgrad_fold", gamma_wgrad_fold, dim3((4 * C * C + 255) / 256), dim3(256), 0, d.dWst, dKl, C);
    st = wgrad_done(s, l);
    if (st != GF_OK) return st;
    return gemm(ctx, false, false, (int)rows_p, C, 4 * C, d.Q, 4 * C, 0, d.Wst + (size_t)4 * C * C, C, 0, pv.df, C, 0, 1, 0);
}

}  // namespace gf
