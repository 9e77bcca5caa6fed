// smp_level_gru.hip -- GRU_GCN_1D and GRU_GCN_2D (cfg.neighbourhood = 4, 5; GraphFlow/GRU_GCN_1D.h, GRU_GCN_2D.h): the neighbourhood kind's
// second set of sweeps.  The lists, x, the lane groups and level 0 are smp_level_neighbourhood.hip's; the level's update
// is a GRU cell and the read-out is gated.  With hp = h_{l-1}[v] and n = the aggregate of h_{l-1} over N_l(v) (a sum, or RisiLayer2D in
// the closed form of that file):
//   z = sigmoid(W_z n + U_z hp),  r = sigmoid(W_r n + U_r hp),  q = r hp,  c = tanh(W_h n + U_h q),  h_l[v] = (1 - z) hp + z c
//   g_v = sigmoid(W_g h_L[v]) tanh(U_g h_L[v]),  graph_feature = tanh(sum_v g_v),  predict = <U, graph_feature>, loss = 0.5 (predict - target)^2
// The eight matrices are shared by all levels: their gradients accumulate across them, levels from the top down.
//   nbh_level_fwd / nbh_node_bwd (W2 = nullptr)   level 0, through smp_neighbourhood_fwd / _node on one operand set
//   gru_cell_fwd     one launch per level: the six matrices transposed in LDS once per workgroup, a group of G lanes per vertex; the
//                    gather, n and hp staged per slot, five products, q through LDS, the sixth product, gates and blend
//   gru_cell_bwd     the six matrices as they are (lanes along a row): dz', dc', dq = U_h^T dc', dr', dn and the direct part of dh_{l-1}
//   nbh_gather_bwd   dh_{l-1} over the transposed list (smp_neighbourhood_gather), then gru_add: gather + direct
//   gru_readout_fwd, gru_readout_mol, gru_readout_bwd   the gates per vertex, the sum per molecule, their reverse; dU is
//                    smp_vertex_level.hip's vertex_readout_dW under the timer name gru_readout_dU
// The eight weight gradients are the library's deterministic TN products.  Every sum runs in a fixed order; no atomics; every wave of a
// workgroup makes the same trips around the barriers; an operand of a lane without a channel is loaded from a clamped address and never
// stored (NOTES.md: no guard around an operand load).
// The cell, its reverse and the read-out are also operators of the C ABI on caller-supplied operands (gf_smp_gru_cell_fwd_ex_f32,
// gf_smp_gru_cell_bwd_ex_f32, gf_smp_gru_readout_fwd_ex_f32, gf_smp_gru_readout_bwd_ex_f32, at the end of this file): the launchers
// below, for tests/test_smp_gru_ops_gpu.py.
#include <cmath>

#include "smp_vertex_level.h"

namespace gf {
using namespace vertex_level;
namespace {

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// M6 = W_z, U_z, W_r, U_r, W_h, U_h back to back, [H][H] each.  GIVEN: n holds the aggregate already (GRU_GCN_3D: smp_level_third.hip)
template <bool PAIRS, bool GIVEN = false>
__global__ __launch_bounds__(kBlock) void gru_cell_fwd(const float *__restrict__ M6, const float *__restrict__ hprev, const float *__restrict__ Tprev,
                                                       const long long *__restrict__ ptr, const int *__restrict__ idx, float *__restrict__ h,
                                                       float *__restrict__ n, float *__restrict__ z, float *__restrict__ r, float *__restrict__ c,
                                                       float *__restrict__ A, float *__restrict__ T, float *__restrict__ Tt, int nV, int H, int G,
                                                       int vpg) {
    extern __shared__ __align__(16) float lds[];
    const int Hp = row_stride(H);
    const size_t img = (size_t)H * Hp;
    float *Mt = lds;   // [6][H][Hp]: Mt[m][k][ch] = M_m[ch][k]
    const Slot sl = slot_of(G);
    float *nb = Mt + 6 * img + (size_t)sl.slot * H;   // [slots][H] each: n, hp, q
    float *hb = nb + (size_t)sl.slots * H;
    float *qb = hb + (size_t)sl.slots * H;
    for (int i = threadIdx.x; i < 6 * H * H; i += kBlock) {
        const int m = i / (H * H), e = i - m * H * H, ch = e / H, k = e - ch * H;
        Mt[m * img + (size_t)k * Hp + ch] = M6[i];
    }
    __syncthreads();
    const bool ok = sl.c0 < H;
    const int cc = ok ? sl.c0 : H - 1;
    const float *Wz = Mt + cc, *Uz = Wz + img, *Wr = Uz + img, *Ur = Wr + img, *Wh = Ur + img, *Uh = Wh + img;
    const int vbase = blockIdx.x * vpg;
    for (int it = 0; it < vpg; it += sl.slots) {   // (the same trip count in every wave: the barriers below are the workgroup's)
        const int v = vbase + it + sl.slot;
        const bool live = v < nV;
        const size_t vv = live ? v : nV - 1;
        float a = 0.f, sacc = 0.f, tt = 0.f;
        const long long e1 = GIVEN ? 0 : ptr[vv + 1];
        for (long long e = GIVEN ? 0 : ptr[vv]; e < e1; ++e) {
            const size_t u = (size_t)idx[e];
            const float hv = hprev[u * H + cc];
            a += hv;
            if (PAIRS) {
                const float tu = Tprev[u];
                sacc = fmaf(hv, tu, sacc);
                tt += tu;
            }
        }
        const float nk = GIVEN ? n[vv * H + cc] : PAIRS ? mul_rounded(a, tt) - sacc : a;
        const float hp = hprev[vv * H + cc];
        if (ok) nb[cc] = nk, hb[cc] = hp;
        if (live && ok) {
            if (!GIVEN) n[vv * H + cc] = nk;
            if (PAIRS) A[vv * H + cc] = a;
        }
        if (PAIRS && live && sl.c0 == 0) Tt[vv] = tt;
        __syncthreads();
        float az = 0.f, ar = 0.f, ac = 0.f;
        for (int j = 0; j < H; ++j) {
            const float nj = nb[j], hj = hb[j];
            const int o = j * Hp;
            az = fmaf(Wz[o], nj, az);
            ar = fmaf(Wr[o], nj, ar);
            ac = fmaf(Wh[o], nj, ac);
            az = fmaf(Uz[o], hj, az);
            ar = fmaf(Ur[o], hj, ar);
        }
        const float zz = sigmoidf(az), rr = sigmoidf(ar);
        if (ok) qb[cc] = rr * hp;
        __syncthreads();
        for (int j = 0; j < H; ++j) ac = fmaf(Uh[j * Hp], qb[j], ac);
        const float cv = tanhf(ac), hn = (1.f - zz) * hp + zz * cv;
        if (live && ok) {
            h[vv * H + cc] = hn;
            z[vv * H + cc] = zz;
            r[vv * H + cc] = rr;
            c[vv * H + cc] = cv;
        }
        if (PAIRS) {   // (h_l is no softmax vector: its sum is an arbitrary number the next level reads)
            const float t = group_sum(ok ? hn : 0.f, G);
            if (live && sl.c0 == 0) T[vv] = t;
        }
        __syncthreads();   // (nb, hb, qb are rewritten by the next vertex of the slot)
    }
}

// From dh_l: dz' = dh (c - hp) z (1 - z), dc' = dh z (1 - c^2), dq = U_h^T dc', dr' = dq hp r (1 - r), q = r hp,
// dn = W_z^T dz' + W_r^T dr' + W_h^T dc' (PAIRS: dn Tt and <dn, A> beside it), direct = dh (1 - z) + dq r + U_z^T dz' + U_r^T dr'
template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void gru_cell_bwd(const float *__restrict__ M6, const float *__restrict__ hprev, const float *__restrict__ dh,
                                                       const float *__restrict__ z, const float *__restrict__ r, const float *__restrict__ c,
                                                       const float *__restrict__ A, const float *__restrict__ Tt, float *__restrict__ dzp,
                                                       float *__restrict__ drp, float *__restrict__ dcp, float *__restrict__ q,
                                                       float *__restrict__ dn, float *__restrict__ gTt, float *__restrict__ sA,
                                                       float *__restrict__ direct, int nV, int H, int G, int vpg) {
    extern __shared__ __align__(16) float lds[];
    const size_t img = (size_t)H * H;
    float *Ms = lds;   // [6][H][H] as they are: lanes run along a row
    const Slot sl = slot_of(G);
    float *zb = Ms + 6 * img + (size_t)sl.slot * H;   // [slots][H] each: dz', dr', dc'
    float *rb = zb + (size_t)sl.slots * H;
    float *cb = rb + (size_t)sl.slots * H;
    for (int i = threadIdx.x; i < 6 * H * H; i += kBlock) Ms[i] = M6[i];
    __syncthreads();
    const bool ok = sl.c0 < H;
    const int cc = ok ? sl.c0 : H - 1;
    const float *Wz = Ms + cc, *Uz = Wz + img, *Wr = Uz + img, *Ur = Wr + img, *Wh = Ur + img, *Uh = Wh + img;
    const int vbase = blockIdx.x * vpg;
    for (int it = 0; it < vpg; it += sl.slots) {
        const int v = vbase + it + sl.slot;
        const bool live = v < nV;
        const size_t vv = live ? v : nV - 1, o = vv * H + cc;
        const float d = dh[o], hp = hprev[o], zz = z[o], rr = r[o], cv = c[o];
        const float gz = d * (cv - hp) * zz * (1.f - zz), gc = d * zz * (1.f - cv * cv);
        if (ok) zb[cc] = gz, cb[cc] = gc;
        __syncthreads();
        float dq = 0.f;
        for (int k = 0; k < H; ++k) dq = fmaf(Uh[k * H], cb[k], dq);
        const float gr = dq * hp * rr * (1.f - rr);
        if (ok) rb[cc] = gr;
        __syncthreads();
        float g = 0.f, dir = 0.f;
        for (int k = 0; k < H; ++k) {
            const float a = zb[k], b = rb[k], e = cb[k];
            const int w = k * H;
            g = fmaf(Wz[w], a, g);
            g = fmaf(Wr[w], b, g);
            g = fmaf(Wh[w], e, g);
            dir = fmaf(Uz[w], a, dir);
            dir = fmaf(Ur[w], b, dir);
        }
        dir += d * (1.f - zz) + dq * rr;
        const float ttv = PAIRS ? Tt[vv] : 0.f;
        if (live && ok) {
            dzp[o] = gz;
            drp[o] = gr;
            dcp[o] = gc;
            q[o] = rr * hp;
            dn[o] = g;
            direct[o] = dir;
            if (PAIRS) gTt[o] = g * ttv;
        }
        if (PAIRS) {
            const float dot = group_sum(ok ? g * A[o] : 0.f, G);
            if (live && sl.c0 == 0) sA[vv] = dot;
        }
        __syncthreads();   // (zb, rb, cb are rewritten by the next vertex of the slot)
    }
}

// dst += src: dh_{l-1} = the gather over the transposed list (already there) + the direct part, in that order; and an accumulating sweep
__global__ __launch_bounds__(kBlock) void gru_add(float *__restrict__ dst, const float *__restrict__ src, size_t count) {
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (size_t)gridDim.x * kBlock) dst[i] += src[i];
}

// M2 = W_g, U_g back to back: s = sigmoid(W_g h_L[v]), t = tanh(U_g h_L[v]) per vertex
__global__ __launch_bounds__(kBlock) void gru_readout_fwd(const float *__restrict__ M2, const float *__restrict__ hL, float *__restrict__ s,
                                                          float *__restrict__ t, int nV, int H, int G, int vpg) {
    extern __shared__ __align__(16) float lds[];
    const int Hp = row_stride(H);
    const size_t img = (size_t)H * Hp;
    float *Mt = lds;   // [2][H][Hp] transposed
    const Slot sl = slot_of(G);
    float *hb = Mt + 2 * img + (size_t)sl.slot * H;
    for (int i = threadIdx.x; i < 2 * H * H; i += kBlock) {
        const int m = i / (H * H), e = i - m * H * H, ch = e / H, k = e - ch * H;
        Mt[m * img + (size_t)k * Hp + ch] = M2[i];
    }
    __syncthreads();
    const bool ok = sl.c0 < H;
    const int cc = ok ? sl.c0 : H - 1;
    const float *Wg = Mt + cc, *Ug = Wg + img;
    const int vbase = blockIdx.x * vpg;
    for (int it = 0; it < vpg; it += sl.slots) {
        const int v = vbase + it + sl.slot;
        const bool live = v < nV;
        const size_t vv = live ? v : nV - 1;
        const float hv = hL[vv * H + cc];
        if (ok) hb[cc] = hv;
        __syncthreads();
        float a1 = 0.f, a2 = 0.f;
        for (int j = 0; j < H; ++j) {
            const float hj = hb[j];
            a1 = fmaf(Wg[j * Hp], hj, a1);
            a2 = fmaf(Ug[j * Hp], hj, a2);
        }
        if (live && ok) {
            s[vv * H + cc] = sigmoidf(a1);
            t[vv * H + cc] = tanhf(a2);
        }
        __syncthreads();
    }
}

// one wave per molecule: graph_feature = tanh(sum over its vertices (ascending) of s t), predict = <U, graph_feature>, loss, dy
__global__ __launch_bounds__(64) void gru_readout_mol(const float *__restrict__ s, const float *__restrict__ t, const int *__restrict__ mol_ptr,
                                                      const float *__restrict__ U, const float *__restrict__ target, float *__restrict__ g,
                                                      float *__restrict__ yhat, float *__restrict__ loss, float *__restrict__ dy, int H) {
    const int m = blockIdx.x;
    float part = 0.f;
    for (int c = threadIdx.x; c < H; c += 64) {
        float acc = 0.f;
        for (int v = mol_ptr[m]; v < mol_ptr[m + 1]; ++v) acc = fmaf(s[(size_t)v * H + c], t[(size_t)v * H + c], acc);
        const float gf = tanhf(acc);
        g[(size_t)m * H + c] = gf;
        part = fmaf(gf, U[c], part);
    }
    part = wave_sum(part);
    GF_STORE_PREDICTION(m, part, target, yhat, loss, dy);
}

// dgf = dy[mol] U (1 - gf^2) per vertex; ds = dgf t s (1 - s), dt = dgf s (1 - t^2) (the gradients of the two arguments), and
// dh_L = W_g^T ds + U_g^T dt
__global__ __launch_bounds__(kBlock) void gru_readout_bwd(const float *__restrict__ M2, const float *__restrict__ s, const float *__restrict__ t,
                                                          const float *__restrict__ g, const float *__restrict__ dy, const float *__restrict__ U,
                                                          const int *__restrict__ vmol, float *__restrict__ ds, float *__restrict__ dt,
                                                          float *__restrict__ dh, int nV, int H, int G, int vpg) {
    extern __shared__ __align__(16) float lds[];
    const size_t img = (size_t)H * H;
    float *Ms = lds;   // [2][H][H] as they are
    const Slot sl = slot_of(G);
    float *sb = Ms + 2 * img + (size_t)sl.slot * H;
    float *tb = sb + (size_t)sl.slots * H;
    for (int i = threadIdx.x; i < 2 * H * H; i += kBlock) Ms[i] = M2[i];
    __syncthreads();
    const bool ok = sl.c0 < H;
    const int cc = ok ? sl.c0 : H - 1;
    const float *Wg = Ms + cc, *Ug = Wg + img;
    const int vbase = blockIdx.x * vpg;
    for (int it = 0; it < vpg; it += sl.slots) {
        const int v = vbase + it + sl.slot;
        const bool live = v < nV;
        const size_t vv = live ? v : nV - 1, o = vv * H + cc;
        const int m = vmol[vv];
        const float gf = g[(size_t)m * H + cc], sv = s[o], tv = t[o];
        const float dgf = dy[m] * U[cc] * (1.f - gf * gf);
        const float gs = dgf * tv * sv * (1.f - sv), gt = dgf * sv * (1.f - tv * tv);
        if (ok) sb[cc] = gs, tb[cc] = gt;
        __syncthreads();
        float acc = 0.f;
        for (int k = 0; k < H; ++k) {
            acc = fmaf(Wg[k * H], sb[k], acc);
            acc = fmaf(Ug[k * H], tb[k], acc);
        }
        if (live && ok) {
            ds[o] = gs;
            dt[o] = gt;
            dh[o] = acc;
        }
        __syncthreads();
    }
}

// W; the eight shared matrices; U
template <typename P>
struct View {
    P *W, *M, *U;
    size_t hh;
    View(const gfsmp::Config &c, P *p) : hh((size_t)c.nChanels * c.nChanels) {
        std::vector<P *> K, b;
        view_params<P>(c, p, &W, &K, &b, &U, &M);
    }
    P *mat(int i) const { return M + (size_t)i * hh; }   // 0 .. 7: W_z, U_z, W_r, U_r, W_h, U_h, W_g, U_g
};

// Vertices per workgroup: whole rounds of its slots.  A workgroup stages its images (100 KB at 64 channels: one workgroup per CU) once
// however many vertices it takes, so the grid is about one wave of workgroups over the device -- 256 CUs times the workgroups whose
// images fit one CU's 160 KiB side by side, at most four -- and the rounds follow from the batch.
inline int vertices_per_group(int nV, int slots, size_t lds_bytes) {
    const size_t fit = (size_t)160 * 1024 / (lds_bytes ? lds_bytes : 1);
    const long long groups = 256 * (long long)(fit < 1 ? 1 : fit > 4 ? 4 : fit), per = (long long)slots * groups;
    const long long rounds = ((long long)nV + per - 1) / per;
    return slots * (int)(rounds < 1 ? 1 : rounds);
}

// rounds = 0: the level's own vertices per workgroup; > 0: that many rounds of a workgroup's slots (the stand-alone operators)
inline int group_vertices(int nV, int slots, size_t lds_bytes, int rounds) {
    return rounds > 0 ? slots * rounds : vertices_per_group(nV, slots, lds_bytes);
}

// the launches on raw operands
struct Shape {
    int H, nV, G, slots;
    explicit Shape(int H_, int nV_) : H(H_), nV(nV_), G(smp_neighbourhood_group_width(H_)), slots(kBlock / smp_neighbourhood_group_width(H_)) {}
    dim3 grid(int vpg) const { return dim3((unsigned)((nV + vpg - 1) / vpg)); }
};

template <bool PAIRS, bool GIVEN = false>
gf_status cell_fwd_launch(gf_ctx *ctx, const Shape &sh, int rounds, const float *M6, const float *hprev, const float *Tprev,
                          const long long *ptr, const int *idx, float *h, float *n, float *z, float *r, float *c, float *A, float *T, float *Tt) {
    const size_t bytes = smp_gru_lds_bytes(sh.H);
    const int vpg = group_vertices(sh.nV, sh.slots, bytes, rounds);
    const gf_status st = opt_in_lds(ctx, gru_cell_fwd<PAIRS, GIVEN>, bytes);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "gru_cell_fwd", (gru_cell_fwd<PAIRS, GIVEN>), sh.grid(vpg), dim3(kBlock), bytes, M6, hprev, Tprev, ptr, idx, h, n, z, r, c, A, T, Tt,
              sh.nV, sh.H, sh.G, vpg);
    return GF_OK;
}

template <bool PAIRS>
gf_status cell_bwd_launch(gf_ctx *ctx, const Shape &sh, int rounds, const float *M6, const float *hprev, const float *dh, const float *z,
                          const float *r, const float *c, const float *A, const float *Tt, float *dzp, float *drp, float *dcp, float *q,
                          float *dn, float *gTt, float *sA, float *direct) {
    const size_t bytes = sizeof(float) * (6 * (size_t)sh.H * sh.H + 3 * (size_t)sh.slots * sh.H);
    const int vpg = group_vertices(sh.nV, sh.slots, bytes, rounds);
    const gf_status st = opt_in_lds(ctx, gru_cell_bwd<PAIRS>, bytes);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "gru_cell_bwd", (gru_cell_bwd<PAIRS>), sh.grid(vpg), dim3(kBlock), bytes, M6, hprev, dh, z, r, c, A, Tt, dzp, drp, dcp, q, dn,
              gTt, sA, direct, sh.nV, sh.H, sh.G, vpg);
    return GF_OK;
}

gf_status readout_fwd_launch(gf_ctx *ctx, const Shape &sh, int rounds, int nMol, const float *M2, const float *U, const float *hL,
                             const int *mol_ptr, const float *target, float *s, float *t, float *g, float *yhat, float *loss, float *dy) {
    const size_t bytes = sizeof(float) * (2 * (size_t)sh.H * row_stride(sh.H) + (size_t)sh.slots * sh.H);
    const int vpg = group_vertices(sh.nV, sh.slots, bytes, rounds);
    const gf_status st = opt_in_lds(ctx, gru_readout_fwd, bytes);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "gru_readout_fwd", gru_readout_fwd, sh.grid(vpg), dim3(kBlock), bytes, M2, hL, s, t, sh.nV, sh.H, sh.G, vpg);
    GF_LAUNCH(ctx, "gru_readout_mol", gru_readout_mol, dim3(nMol), dim3(64), 0, s, t, mol_ptr, U, target, g, yhat, loss, dy, sh.H);
    return GF_OK;
}

gf_status readout_bwd_launch(gf_ctx *ctx, const Shape &sh, int rounds, const float *M2, const float *U, const float *s, const float *t,
                             const float *g, const float *dy, const int *vmol, float *ds, float *dt, float *dh) {
    const size_t bytes = sizeof(float) * (2 * (size_t)sh.H * sh.H + 2 * (size_t)sh.slots * sh.H);
    const int vpg = group_vertices(sh.nV, sh.slots, bytes, rounds);
    const gf_status st = opt_in_lds(ctx, gru_readout_bwd, bytes);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "gru_readout_bwd", gru_readout_bwd, sh.grid(vpg), dim3(kBlock), bytes, M2, s, t, g, dy, U, vmol, ds, dt, dh, sh.nV, sh.H, sh.G,
              vpg);
    return GF_OK;
}

// f(pairs as an integral constant): the one place the aggregate picks an instantiation
template <typename F>
gf_status with_aggregate(bool pairs, F &&f) {
    return pairs ? f(std::true_type{}) : f(std::false_type{});
}

// C [H][H] += A^T B over the vertices: a tall-skinny TN product
gf_status wgrad(gf_ctx *ctx, const Shape &sh, const float *A, const float *B, float *C) {
    return gemm(ctx, true, false, sh.H, sh.H, sh.nV, A, sh.H, 0, B, sh.H, 0, C, sh.H, 0, 1, 1);
}

}  // namespace

gf_status smp_gru_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, FD = s->cfg.fdim(), nMol = s->lay.nMol, nV = s->lay.level[0].nNodes;
    const bool pairs = s->cfg.neighbourhood == 5;
    const View<const float> p(s->cfg, params);
    const Shape sh(H, nV);
    gf_nbh_fwd_set level0 = {};   // (no W2: no aggregate, every other operand stays null)
    level0.FD = FD, level0.W1 = p.W, level0.x = s->x, level0.h = s->lv[0].f, level0.T = s->lv[0].nb_T;
    gf_status st = smp_neighbourhood_fwd(ctx, pairs, H, nV, 0, &level0, 1, nullptr, nullptr);
    for (int l = 1; l <= L && st == GF_OK; ++l) {
        gf_smp::DevLevel &d = s->lv[l];
        const gf_smp::DevLevel &pv = s->lv[l - 1];
        if (s->cfg.third_order()) {   // GRU_GCN_3D: the pool leaves n_l in th_A, the cell reads it there
            st = smp_third_pool_fwd_launch(ctx, H, nV, d.nb_max_members, pv.f, d.nb_ptr, d.nb_idx, d.th_A, d.nb_sel);
            if (st == GF_OK)
                st = cell_fwd_launch<false, true>(ctx, sh, 0, p.mat(0), pv.f, nullptr, d.nb_ptr, d.nb_idx, d.f, d.th_A, d.gru_z, d.gru_r, d.gru_c,
                                                  nullptr, nullptr, nullptr);
            continue;
        }
        st = with_aggregate(pairs, [&](auto pr) -> gf_status {
            return cell_fwd_launch<decltype(pr)::value>(ctx, sh, 0, p.mat(0), pv.f, pv.nb_T, d.nb_ptr, d.nb_idx, d.f, d.th_A, d.gru_z, d.gru_r,
                                                        d.gru_c, d.th_B, d.nb_T, d.nb_Tt);
        });
    }
    if (st == GF_OK)
        st = readout_fwd_launch(ctx, sh, 0, nMol, p.mat(6), p.U, s->lv[L].f, s->mol_ptr, targets, s->gru_s, s->gru_t, s->g, s->yhat, loss,
                                s->dy);
    return st == GF_OK ? finish_forward(s, targets != nullptr, predict, graph_feature, H) : st;
}

// The reverse sweep from the loss of the last forward.  Every level keeps what a second sweep needs: dh_l is rebuilt from dy downwards.
gf_status smp_gru_backward(gf_smp *s, const float *params, float *grads, int accumulate) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, FD = s->cfg.fdim(), nMol = s->lay.nMol, nV = s->lay.level[0].nNodes;
    const bool pairs = s->cfg.neighbourhood == 5;
    const View<const float> p(s->cfg, params);
    const Shape sh(H, nV);
    // The shared blocks are summed over the levels, from the top down, into zeros.  accumulate: the sweep is formed on its own, in the
    // same order, and added once -- so that it adds exactly what a sweep without it writes.
    const size_t np = param_count(s->cfg);
    if (accumulate && !s->gru_acc) {
        const gf_status got = upload(s, &s->gru_acc, nullptr, np);
        if (got != GF_OK) return got;
    }
    float *sweep = accumulate ? s->gru_acc : grads;
    const View<float> d(s->cfg, sweep);
    GF_HIP_TRY(ctx, hipMemsetAsync(sweep, 0, sizeof(float) * np, ctx->stream));
    gf_status st = smp_vertex_readout_dW(ctx, "gru_readout_dU", H, nMol, s->dy, s->g, d.U);
    if (st == GF_OK)
        st = readout_bwd_launch(ctx, sh, 0, p.mat(6), p.U, s->gru_s, s->gru_t, s->g, s->dy, s->top_node_mol, s->gru_ds, s->gru_dt, s->lv[L].df);
    if (st == GF_OK) st = wgrad(ctx, sh, s->gru_ds, s->lv[L].f, d.mat(6));   // dW_g += ds^T h_L
    if (st == GF_OK) st = wgrad(ctx, sh, s->gru_dt, s->lv[L].f, d.mat(7));   // dU_g += dt^T h_L
    for (int l = L; l >= 1 && st == GF_OK; --l) {   // dh_l in lv[l].df -> dh_{l-1} in lv[l - 1].df
        gf_smp::DevLevel &v = s->lv[l];
        gf_smp::DevLevel &pv = s->lv[l - 1];
        st = with_aggregate(pairs, [&](auto pr) -> gf_status {
            return cell_bwd_launch<decltype(pr)::value>(ctx, sh, 0, p.mat(0), pv.f, v.df, v.gru_z, v.gru_r, v.gru_c, v.th_B, v.nb_Tt, v.gru_dz,
                                                        v.gru_dr, v.gru_dc, v.gru_q, v.Q, v.th_node, v.nb_sA, v.gru_direct);
        });
        const float *lhs[6] = {v.gru_dz, v.gru_dz, v.gru_dr, v.gru_dr, v.gru_dc, v.gru_dc};
        const float *rhs[6] = {v.th_A, pv.f, v.th_A, pv.f, v.th_A, v.gru_q};   // n, hp, n, hp, n, q
        for (int i = 0; i < 6 && st == GF_OK; ++i) st = wgrad(ctx, sh, lhs[i], rhs[i], d.mat(i));
        if (st == GF_OK && s->cfg.third_order())
            st = smp_third_pool_bwd_launch(ctx, H, nV, v.nb_ptr, v.nb_idx, v.nb_tptr, v.nb_tidx, pv.f, v.nb_sel, v.Q, pv.df);
        else if (st == GF_OK) {
            const gf_nbh_gather_set gat = {/*dn=*/v.Q, /*gTt=*/v.th_node, /*sA=*/v.nb_sA, /*hprev=*/pv.f, /*Tprev=*/pv.nb_T, /*dhprev=*/pv.df};
            st = smp_neighbourhood_gather(ctx, pairs, H, nV, v.nb_tptr, v.nb_tidx, &gat, 1);
        }
        if (st != GF_OK) break;
        const size_t count = (size_t)nV * H, blocks = (count + kBlock - 1) / kBlock;
        GF_LAUNCH(ctx, "gru_add", gru_add, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(kBlock), 0, pv.df, v.gru_direct, count);
    }
    // level 0: dz = dh h (1 - h) in place (the classes' diagonal softmax rule), dW [H][F'] += dz^T X
    gf_nbh_node_set level0 = {};   // (no W2: dz alone)
    level0.h = s->lv[0].f, level0.dh = s->lv[0].df;
    if (st == GF_OK) st = smp_neighbourhood_node(ctx, pairs, H, nV, 0, &level0, 1, nullptr, s->top_node_mol);
    if (st == GF_OK) st = gemm(ctx, true, false, H, FD, nV, s->lv[0].df, H, 0, s->x, FD, 0, d.W, FD, 0, 1, 1);
    if (st != GF_OK) return st;
    if (accumulate) GF_LAUNCH(ctx, "gru_add", gru_add, dim3((unsigned)((np + kBlock - 1) / kBlock)), dim3(kBlock), 0, grads, sweep, np);
    mark_used(s);
    return GF_OK;
}

}  // namespace gf

// ---- the level's kernels as stand-alone operators (include/gf_hip.h; tests/test_smp_gru_ops_gpu.py) ----
extern "C" {

gf_status gf_smp_gru_cell_fwd_ex_f32(gf_ctx *ctx, int aggregate, int H, int nV, int rounds, const float *M6, const float *hprev, const float *Tprev,
                                     const long long *ptr, const int *idx, float *h, float *n, float *z, float *r, float *c, float *A, float *T,
                                     float *Tt) {
    static const char *who = "gf_smp_gru_cell_fwd_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kGruMaxChanels, nV, rounds);
    if (st != GF_OK) return st;
    if (aggregate < 0 || aggregate > 2) return gf::fail(ctx, GF_ERR_INVALID, "%s: aggregate = %d (0: sum, 1: pairs, 2: given)", who, aggregate);
    if (!M6 || !hprev || !h || !n || !z || !r || !c) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    if (aggregate != 2 && (!ptr || !idx)) return gf::fail(ctx, GF_ERR_INVALID, "%s: the sum and the pair form need ptr and idx", who);
    if (aggregate == 1 && (!Tprev || !A || !T || !Tt)) return gf::fail(ctx, GF_ERR_INVALID, "%s: the pair form needs Tprev, A, T and Tt", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (aggregate != 2) st = gf::check_list(ctx, who, "ptr", ptr, idx, nV, nV);
    if (st != GF_OK) return st;
    const gf::Shape sh(H, nV);
    if (aggregate == 2) return gf::cell_fwd_launch<false, true>(ctx, sh, rounds, M6, hprev, Tprev, ptr, idx, h, n, z, r, c, A, T, Tt);
    return gf::with_aggregate(aggregate == 1, [&](auto pr) -> gf_status {
        return gf::cell_fwd_launch<decltype(pr)::value>(ctx, sh, rounds, M6, hprev, Tprev, ptr, idx, h, n, z, r, c, A, T, Tt);
    });
}

gf_status gf_smp_gru_cell_bwd_ex_f32(gf_ctx *ctx, int pairs, int H, int nV, int rounds, const float *M6, const float *hprev, const float *dh,
                                     const float *z, const float *r, const float *c, const float *A, const float *Tt, float *dzp, float *drp,
                                     float *dcp, float *q, float *dn, float *gTt, float *sA, float *direct) {
    static const char *who = "gf_smp_gru_cell_bwd_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    const gf_status st = gf::check_shape(ctx, who, H, gf::kGruMaxChanels, nV, rounds);
    if (st != GF_OK) return st;
    if (!M6 || !hprev || !dh || !z || !r || !c || !dzp || !drp || !dcp || !q || !dn || !direct)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    if (pairs && (!A || !Tt || !gTt || !sA)) return gf::fail(ctx, GF_ERR_INVALID, "%s: the pair form needs A, Tt, gTt and sA", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gf::Shape sh(H, nV);
    return gf::with_aggregate(pairs != 0, [&](auto pr) -> gf_status {
        return gf::cell_bwd_launch<decltype(pr)::value>(ctx, sh, rounds, M6, hprev, dh, z, r, c, A, Tt, dzp, drp, dcp, q, dn, gTt, sA, direct);
    });
}

gf_status gf_smp_gru_readout_fwd_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, int rounds, const float *M2, const float *U, const float *hL,
                                        const int *mol_ptr, const float *target, float *s, float *t, float *g, float *yhat, float *loss,
                                        float *dy) {
    static const char *who = "gf_smp_gru_readout_fwd_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kGruMaxChanels, nV, rounds);
    if (st != GF_OK) return st;
    if (nMol < 1 || !M2 || !U || !hL || !mol_ptr || !s || !t || !g || !yhat || !dy) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = gf::check_ptr(ctx, who, "mol_ptr", mol_ptr, nMol, nV);
    if (st != GF_OK) return st;
    return gf::readout_fwd_launch(ctx, gf::Shape(H, nV), rounds, nMol, M2, U, hL, mol_ptr, target, s, t, g, yhat, loss, dy);
}

gf_status gf_smp_gru_readout_bwd_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, int rounds, const float *M2, const float *U, const float *s,
                                        const float *t, const float *g, const float *dy, const int *vmol, float *ds, float *dt, float *dh,
                                        float *dU) {
    static const char *who = "gf_smp_gru_readout_bwd_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kGruMaxChanels, nV, rounds);
    if (st != GF_OK) return st;
    if (nMol < 1 || !M2 || !U || !s || !t || !g || !dy || !vmol || !ds || !dt || !dh || !dU)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = gf::check_members(ctx, who, "vmol", vmol, (size_t)nV, nMol);
    if (st != GF_OK) return st;
    st = gf::smp_vertex_readout_dW(ctx, "gru_readout_dU", H, nMol, dy, g, dU);
    if (st != GF_OK) return st;
    return gf::readout_bwd_launch(ctx, gf::Shape(H, nV), rounds, M2, U, s, t, g, dy, vmol, ds, dt, dh);
}

}  // extern "C"
