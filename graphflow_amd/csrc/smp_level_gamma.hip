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

// ---- physics towers (SMP_gamma_physics / SMP_gamma_pairgraphs): the level is rectangular, Cp = C_{l-1} -> Cc = C_l (channels halve
// per level, 16 -> 8 -> 4 -> 2 or 10 -> 5 -> 2 -> 1), fields hold 4 - 64 positions.  One (node, child) pair -- or one source node
// backward -- per workgroup would leave most lanes idle, so a workgroup takes a run of consecutive pairs (source nodes) and flattens
// (pair, y, channel vector) over its lanes; the vector is V floats, V = 4 / 2 / 1 as Cc allows.  Sums in the order of the square level.
constexpr int kTowerMaxPack = 64;   // pairs (source nodes) per workgroup: one wave builds their item offsets

template <int V>
struct Vf {
    float v[V];
};
template <int V>
__device__ __forceinline__ Vf<V> vzero() {
    Vf<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.v[k] = 0.f;
    return r;
}
template <int V>
__device__ __forceinline__ Vf<V> vld(const float *p) {   // (p is V-float aligned: rows are multiples of Cc, V | Cc)
    Vf<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4 *>(p);
        r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
    } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        r.v[0] = t.x, r.v[1] = t.y;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V>
__device__ __forceinline__ void vst(float *p, const Vf<V> &r) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else if constexpr (V == 2) *reinterpret_cast<float2 *>(p) = make_float2(r.v[0], r.v[1]);
    else *p = r.v[0];
}
template <int V>
__device__ __forceinline__ void vadd(Vf<V> &a, const Vf<V> &b) {
#pragma unroll
    for (int k = 0; k < V; ++k) a.v[k] += b.v[k];
}

// off[0 .. np] = exclusive prefix of cnt over the workgroup's np <= 64 work items (wave 0), then a barrier
__device__ __forceinline__ void pack_offsets(int *off, int cnt, int np) {
    if (threadIdx.x < 64) {
        int v = threadIdx.x < np ? cnt : 0;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d, 64);
            if ((int)threadIdx.x >= d) v += u;
        }
        off[threadIdx.x + 1] = v;
        if (threadIdx.x == 0) off[0] = 0;
    }
    __syncthreads();
}
__device__ __forceinline__ int pack_find(const int *off, int np, int i) {   // the j with off[j] <= i < off[j + 1]
    int lo = 0, hi = np - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Forward: pairs [blockIdx.x * ppw, + ppw); items (pair j, y, vector q) over sum_j s_j * Cc / V.  G rows are 4 Cc floats.
template <int V>
__global__ __launch_bounds__(256) void gamma_tower_fwd(const float *__restrict__ G, const float *__restrict__ bias, float *__restrict__ f,
                                                       const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                       const long long *__restrict__ node_pair, const int *__restrict__ pair_node,
                                                       const long long *__restrict__ pair_src_row, const int *__restrict__ pair_src_s,
                                                       const short *__restrict__ pi, int Cc, long long pairs, int ppw) {
    __shared__ int off[kTowerMaxPack + 1];
    __shared__ int pnode[kTowerMaxPack];
    const long long eb = (long long)blockIdx.x * ppw;
    const int np = (int)(pairs - eb < ppw ? pairs - eb : ppw), Qc = Cc / V, C4 = 4 * Cc;
    int cnt = 0;
    if ((int)threadIdx.x < np) {
        const int n = pair_node[eb + threadIdx.x];
        pnode[threadIdx.x] = n;
        cnt = node_s[n] * Qc;
    }
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int j = pack_find(off, np, i);
        const long long e = eb + j;
        const int n = pnode[j], s = node_s[n];
        const int r = i - off[j], y = r / Qc, q = r - y * Qc;
        const long long r0 = node_row[n], e0 = node_pair[n];
        const int x = (int)(e - e0), swx = pair_src_s[e];
        const short *mx = pi + r0 + (long long)x * s;
        const int px = mx[x], py = mx[y], cq = q * V;
        const float *gx = G + pair_src_row[e] * C4;   // first row of w_x
        Vf<V> sab = vzero<V>(), sbc = vzero<V>(), pc = vzero<V>(), pd = vzero<V>();
        if (py >= 0) {
            const float *row = gx + (size_t)py * swx * C4 + cq;   // G[w_x][pi_x(y), .]
            for (int c = 0; c < s; ++c) {
                const int pcc = mx[c];
                if (pcc >= 0) vadd(sab, vld<V>(row + (size_t)pcc * C4));
            }
            pd = vld<V>(row + (size_t)py * C4 + 3 * Cc);
            if (px >= 0) pc = vld<V>(gx + ((size_t)px * swx + py) * C4 + 2 * Cc + cq);
        }
        for (int a = 0; a < s; ++a) {
            const short *ma = pi + r0 + (long long)a * s;
            const int pa = ma[x], pb = ma[y];
            if (pa >= 0 && pb >= 0) vadd(sbc, vld<V>(G + (pair_src_row[e0 + a] + (long long)pa * pair_src_s[e0 + a] + pb) * C4 + Cc + cq));
        }
        Vf<V> o;
#pragma unroll
        for (int k = 0; k < V; ++k) o.v[k] = lrelu(((sab.v[k] + sbc.v[k]) + (pc.v[k] + pd.v[k])) + bias[cq + k]);
        vst<V>(f + (r0 + (long long)x * s + y) * Cc + cq, o);
    }
}

// Backward: source nodes [blockIdx.x * npw, + npw) of level l - 1; items (node j, p, q, vector q4) over sum_j s_j^2 Cc / V.  dz rows
// are Cc floats, dG rows 4 Cc.
template <int V>
__global__ __launch_bounds__(256) void gamma_tower_bwd(const float *__restrict__ dz, float *__restrict__ dG, const int *__restrict__ prev_s,
                                                       const long long *__restrict__ prev_row, const long long *__restrict__ cons_ptr,
                                                       const long long *__restrict__ cons_row, const int *__restrict__ cons_s,
                                                       const int *__restrict__ cons_a, const long long *__restrict__ cons_inv_off,
                                                       const short *__restrict__ inv, int Cc, int nodes, int npw) {
    __shared__ int off[kTowerMaxPack + 1];
    const int wb = blockIdx.x * npw;
    const int np = nodes - wb < npw ? nodes - wb : npw, Qc = Cc / V;
    int cnt = 0;
    if ((int)threadIdx.x < np) {
        const int sw = prev_s[wb + threadIdx.x];
        cnt = sw * sw * Qc;
    }
    pack_offsets(off, cnt, np);
    const int total = off[np];
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int j = pack_find(off, np, i);
        const int w = wb + j, sw = prev_s[w];
        const int r = i - off[j], pq = r / Qc, q4 = r - pq * Qc, cq = q4 * V;
        const int p = pq / sw, q = pq - p * sw;
        const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1];
        Vf<V> g0 = vzero<V>(), g1 = vzero<V>(), g2 = vzero<V>(), g3 = vzero<V>();
        for (long long e = c0; e < c1; ++e) {
            const short *iv = inv + cons_inv_off[e];
            const int b = iv[p], c = iv[q];
            if (b < 0 || c < 0) continue;
            const int s = cons_s[e], a = cons_a[e];
            const long long R = cons_row[e];
            const Vf<V> zab = vld<V>(dz + (R + (long long)a * s + b) * Cc + cq);
            vadd(g0, zab);                                                  // S_ab:  z[a, b] for every c
            vadd(g1, vld<V>(dz + (R + (long long)b * s + c) * Cc + cq));    // S_bc:  z[b, c]
            if (b == a) vadd(g2, vld<V>(dz + (R + (long long)a * s + c) * Cc + cq));   // Pc: z[a, c]
            if (b == c) vadd(g3, zab);                                      // Pd:    z[a, b]
        }
        float *o = dG + (prev_row[w] + pq) * 4 * (long long)Cc + cq;
        vst<V>(o, g0);
        vst<V>(o + Cc, g1);
        vst<V>(o + 2 * Cc, g2);
        vst<V>(o + 3 * Cc, g3);
    }
}

// K [4Cp][Cc] (rows k Cp + ci) -> Kh [Cp][4Cc] (Kh[ci][k Cc + co] = K[k Cp + ci][co]) and Kt [4Cc][Cp] (Kt[k Cc + co][ci] = K[k Cp + ci][co])
__global__ void gamma_weight_views(const float *__restrict__ K, float *__restrict__ Kh, float *__restrict__ Kt, int Cp, int Cc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * Cp * Cc) return;
    const int k = i / (Cp * Cc), r = i - k * Cp * Cc, ci = r / Cc, co = r - ci * Cc;
    const float v = K[i];
    Kh[(size_t)ci * 4 * Cc + k * Cc + co] = v;
    Kt[((size_t)k * Cc + co) * Cp + ci] = v;
}
// dK [4Cp][Cc] += dKh [Cp][4Cc] rearranged (dK[k Cp + ci][co] += dKh[ci][k Cc + co]); one thread per element of dK
__global__ void gamma_wgrad_fold(const float *__restrict__ dKh, float *__restrict__ dK, int Cp, int Cc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * Cp * Cc) return;
    const int k = i / (Cp * Cc), r = i - k * Cp * Cc, ci = r / Cc, co = r - ci * Cc;
    dK[i] += dKh[(size_t)ci * 4 * Cc + k * Cc + co];
}

bool gamma_tower(const gf_smp *s) { return s->cfg.physics && !s->cfg.square(); }
int tower_vec(int Cc) { return Cc % 4 == 0 ? 4 : Cc % 2 == 0 ? 2 : 1; }
// work items per workgroup: ~256 lanes' worth of (position, vector) items, at most kTowerMaxPack pairs / source nodes
int tower_pack(double items_per_unit) {
    const int k = (int)(256.0 / (items_per_unit > 1.0 ? items_per_unit : 1.0));
    return k < 1 ? 1 : k > kTowerMaxPack ? kTowerMaxPack : k;
}

}  // namespace

bool smp_gamma_fused(const gf_smp *s, int l) {
    const int C = s->cfg.nChanels;
    if (!s->fused || s->cfg.nContractions != 4) return false;
    if (gamma_tower(s)) {   // (a tower at its own halving widths: Cc <= Cp)
        if (s->cfg.level_channels(l - 1) > 64) return false;
    } else {
        if (!s->cfg.square()) return false;
        if (C % 4 != 0 || C > 64) return false;   // (wider models, or C % 4 != 0 unpadded: the op-by-op level on the batched `_4` kernels)
    }
    const gfsmp::LevelLayout &h = s->lay.level[l];
    return !h.buckets.empty() && h.buckets.back().s <= kFusedMaxField && s->lv[l].Wst && s->lv[l].dWst;
}

// G = f_{l-1} [K0 | K1 | K2 | K3] into the level's Q buffer, then the gather with bias + LeakyReLU into f_l
gf_status smp_gamma_forward_level(gf_smp *s, int l, const float *Kl, const float *bl) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);   // (equal unless a tower)
    const long long rows_p = s->lay.level[l - 1].rows, pairs = s->lay.level[l].pairs;
    float *Kh = d.Wst, *Kt = d.Wst + (size_t)4 * Cp * Cc;
    GF_LAUNCH(ctx, "smpg_weight_views", gamma_weight_views, dim3((4 * Cp * Cc + 255) / 256), dim3(256), 0, Kl, Kh, Kt, Cp, Cc);
    gf_status st = gemm(ctx, false, false, (int)rows_p, 4 * Cc, Cp, pv.f, Cp, 0, Kh, 4 * Cc, 0, d.Q, 4 * Cc, 0, 1, 0);
    if (st != GF_OK || pairs == 0) return st;
    if (gamma_tower(s)) {
        const int ppw = tower_pack((double)s->lay.level[l].rows / (double)pairs * (Cc / tower_vec(Cc)));
        const dim3 grid((unsigned)((pairs + ppw - 1) / ppw));
#define GF_TOWER_FWD(V) GF_LAUNCH(ctx, "smpg_tower_fwd", gamma_tower_fwd<V>, grid, dim3(256), 0, d.Q, bl, d.f, d.node_s, d.node_row, d.node_pair, \
                                  d.pair_node, d.pair_src_row, d.pair_src_s, d.pi, Cc, pairs, ppw)
        switch (tower_vec(Cc)) {
            case 4: GF_TOWER_FWD(4); break;
            case 2: GF_TOWER_FWD(2); break;
            default: GF_TOWER_FWD(1); break;
        }
#undef GF_TOWER_FWD
        return GF_OK;
    }
    GF_LAUNCH(ctx, "smpg_level_fwd", gamma_level_fwd, dim3((unsigned)pairs), dim3(128), 0, d.Q, bl, d.f, d.node_s, d.node_row, d.node_pair,
              d.pair_node, d.pair_src_row, d.pair_src_s, d.pi, Cc);
    return GF_OK;
}

// d.df holds dz (lrelu_backward_colsum ran): dG into the level's Q buffer, dK_l += f_{l-1}^T dG (rearranged), df_{l-1} = dG Kt.
// The weight gradient is final before df_{l-1} is formed; *wgrad_done is called in between (the data-parallel all-reduce of the level).
gf_status smp_gamma_backward_level(gf_smp *s, int l, const float *Kl, float *dKl, gf_status (*wgrad_done)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);
    const long long rows_p = s->lay.level[l - 1].rows;
    const int np = s->lay.level[l - 1].nNodes;
    // (the views again: this sweep's parameters need not be the forward's)
    GF_LAUNCH(ctx, "smpg_weight_views", gamma_weight_views, dim3((4 * Cp * Cc + 255) / 256), dim3(256), 0, Kl, d.Wst, d.Wst + (size_t)4 * Cp * Cc, Cp, Cc);
    if (np > 0 && gamma_tower(s)) {
        const int npw = tower_pack((double)rows_p / (double)np * (Cc / tower_vec(Cc)));
        const dim3 grid((unsigned)((np + npw - 1) / npw));
#define GF_TOWER_BWD(V) GF_LAUNCH(ctx, "smpg_tower_bwd", gamma_tower_bwd<V>, grid, dim3(256), 0, d.df, d.Q, pv.node_s, pv.node_row, d.cons_ptr, \
                                  d.cons_row, d.cons_s, d.cons_a, d.cons_inv_off, d.inv, Cc, np, npw)
        switch (tower_vec(Cc)) {
            case 4: GF_TOWER_BWD(4); break;
            case 2: GF_TOWER_BWD(2); break;
            default: GF_TOWER_BWD(1); break;
        }
#undef GF_TOWER_BWD
    } else if (np > 0) {
        GF_LAUNCH(ctx, "smpg_level_bwd", gamma_level_bwd, dim3((unsigned)np), dim3(256), 0, d.df, d.Q, pv.node_s, pv.node_row, d.cons_ptr, d.cons_row,
                  d.cons_s, d.cons_a, d.cons_inv_off, d.inv, Cc);
    }
    gf_status st = gemm(ctx, true, false, Cp, 4 * Cc, (int)rows_p, pv.f, Cp, 0, d.Q, 4 * Cc, 0, d.dWst, 4 * Cc, 0, 1, 0);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "smpg_wgrad_fold", gamma_wgrad_fold, dim3((4 * Cp * Cc + 255) / 256), dim3(256), 0, d.dWst, dKl, Cp, Cc);
    st = wgrad_done(s, l);
    if (st != GF_OK) return st;
    return gemm(ctx, false, false, (int)rows_p, Cp, 4 * Cc, d.Q, 4 * Cc, 0, d.Wst + (size_t)4 * Cp * Cc, Cp, 0, pv.df, Cp, 0, 1, 0);
}

}  // namespace gf
