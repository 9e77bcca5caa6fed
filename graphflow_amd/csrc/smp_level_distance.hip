// smp_level_distance.hip -- GCN_1D_Distance, GCN_2D_Distance, GCN_3D_Distance (cfg.distance_channel with cfg.neighbourhood = 2, 3, 6;
// GraphFlow/GCN_1D_Distance.h, GCN_2D_Distance.h, GCN_3D_Distance.h): two copies of the softmax neighbourhood level side by side over the same
// neighbour lists -- the vertex channel on the shell sums x_v [F'], the distance channel on x_d [M], M = max_nVertices: column v of the
// molecule's distance matrix, padded with zeros and sorted ascending (the class's Sort op: data, nothing flows back) -- read out over
//   final = [sum_v h^v_L[v] | sum_v h^d_L[v]]  [2 H],   predict = <W, final>,   loss = 0.5 (predict - target)^2.
//   dist_rows_sort_wave / _lds   x_d on the device: the column gathered and converted to fp32 (rounding is monotone: the sorted fp32 values
//                    are the fp32 of the class's sorted doubles), M - V zeros, +inf up to the next power of two P for the network only; a
//                    bitonic network across the P lanes of a group (__shfl_xor) while P <= 64, in LDS with one workgroup per vertex above.
//                    A compare-exchange swaps on a strict `<` only, so the row stays a permutation of its inputs (-0.0 and 0.0 included).
//   the level        smp_level_neighbourhood.hip's three kernels with blockIdx.y = the channel (one forward launch, one node launch and one
//                    gather per level for both channels); GCN_3D_Distance runs third_pool_fwd / third_pool_bwd once per channel
//   dist_readout     final, prediction, loss, dy; dW [2 H] in molecule order is smp_vertex_level.hip's vertex_readout_dW
// The weight gradients are the library's deterministic TN products, 2 (2 L + 1) per step.  No atomics; two runs give the same bits.
// GF_SMP_DISTANCE_LAUNCHES=2 (read per call; tools/distance_time.py): every level kernel once per channel instead -- the same bits.
#include <cmath>

#include "smp_vertex_level.h"

namespace gf {
using namespace vertex_level;
namespace {

// what a vertex's row is gathered from: entry i of column j of molecule m, zeros up to M, +inf beyond (never stored)
struct Column {
    const double *col;
    int V;
};
__device__ __forceinline__ Column column_of(const double *__restrict__ dist, const long long *__restrict__ mat_off, const int *__restrict__ mol_ptr,
                                            const int *__restrict__ vmol, size_t v) {
    const int m = vmol[v], v0 = mol_ptr[m], V = mol_ptr[m + 1] - v0;
    return {dist + mat_off[m] + ((long long)v - v0), V};
}
__device__ __forceinline__ float entry_of(const Column &c, int i, int M) {
    return i < c.V ? (float)c.col[(size_t)i * c.V] : i < M ? 0.f : INFINITY;
}

// P <= 64 (a power of two): a group of P lanes per vertex, 256 / P vertices per workgroup, the network across the lanes
__global__ __launch_bounds__(kBlock) void dist_rows_sort_wave(const double *__restrict__ dist, const long long *__restrict__ mat_off,
                                                              const int *__restrict__ mol_ptr, const int *__restrict__ vmol, float *__restrict__ xd,
                                                              int nV, int M, int P) {
    const int lane = threadIdx.x & 63, i = lane & (P - 1);
    const long long v = (long long)blockIdx.x * (kBlock / P) + (threadIdx.x >> 6) * (64 / P) + lane / P;
    const bool live = v < nV;
    const size_t vv = live ? (size_t)v : (size_t)nV - 1;
    float val = entry_of(column_of(dist, mat_off, mol_ptr, vmol, vv), i, M);
    for (int k = 2; k <= P; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {   // (every lane of the wave takes part: the partner lane ^ d stays inside the group)
            const float other = __shfl_xor(val, d, 64);
            const bool keep_min = ((i & k) == 0) == ((i & d) == 0);
            val = keep_min ? (other < val ? other : val) : (val < other ? other : val);
        }
    if (live && i < M) xd[vv * M + i] = val;
}

// P = 128 .. 4096: one workgroup per vertex, the row in LDS, one barrier per step of the network.  Thread t of a step owns the pair
// (lo, lo | d), lo = t with a zero bit inserted at d: consecutive threads touch consecutive words once d >= 32 (no bank conflict; two-way
// below, where a pair's two words share a 32-word line).
__global__ __launch_bounds__(kBlock) void dist_rows_sort_lds(const double *__restrict__ dist, const long long *__restrict__ mat_off,
                                                             const int *__restrict__ mol_ptr, const int *__restrict__ vmol, float *__restrict__ xd,
                                                             int nV, int M, int P) {
    extern __shared__ __align__(16) float row[];   // [P]
    const size_t v = blockIdx.x;
    const Column c = column_of(dist, mat_off, mol_ptr, vmol, v);
    for (int i = threadIdx.x; i < P; i += kBlock) row[i] = entry_of(c, i, M);
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int d = k >> 1; d > 0; d >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += kBlock) {
                const int lo = ((t & ~(d - 1)) << 1) | (t & (d - 1)), hi = lo | d;
                const float a = row[lo], b = row[hi];
                const bool up = (lo & k) == 0;
                if (up ? b < a : a < b) {
                    row[lo] = b;
                    row[hi] = a;
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < M; i += kBlock) xd[v * M + i] = row[i];
}

// one wave per molecule: g = [sum_v h^v_L | sum_v h^d_L] over its vertices (ascending), predict = <W, g>, the squared loss, dy
__global__ __launch_bounds__(64) void dist_readout(const float *__restrict__ hv, const float *__restrict__ hd, const int *__restrict__ mol_ptr,
                                                   const float *__restrict__ W, const float *__restrict__ target, float *__restrict__ g,
                                                   float *__restrict__ yhat, float *__restrict__ loss, float *__restrict__ dy, int H) {
    const int m = blockIdx.x;
    float part = 0.f;
    for (int c = threadIdx.x; c < 2 * H; c += 64) {
        const float *__restrict__ src = c < H ? hv + c : hd + (c - H);
        float acc = 0.f;
        for (int v = mol_ptr[m]; v < mol_ptr[m + 1]; ++v) acc += src[(size_t)v * H];
        g[(size_t)m * 2 * H + c] = acc;
        part = fmaf(acc, W[c], part);
    }
    part = wave_sum(part);
    GF_STORE_PREDICTION(m, part, target, yhat, loss, dy);
}

// The flat buffer in registration order: per level W1^v_l [H][F'], W1^d_l [H][M] and from level 1 on W2^v_l, W2^d_l [H][H]; W [2 H].
// [0] = the vertex channel, [1] = the distance channel.
struct Layout {   // first float of every block
    std::vector<size_t> W1[2], W2[2];
    size_t W;
    explicit Layout(const gfsmp::Config &c) {
        const size_t H = (size_t)c.nChanels, width[2] = {(size_t)c.fdim(), (size_t)c.max_nVertices};
        size_t p = 0;
        for (int ch = 0; ch < 2; ++ch) {
            W1[ch].assign(c.nLevels + 1, 0);
            W2[ch].assign(c.nLevels + 1, 0);
        }
        for (int l = 0; l <= c.nLevels; ++l) {
            for (int ch = 0; ch < 2; ++ch) {
                W1[ch][l] = p;
                p += H * width[ch];
            }
            for (int ch = 0; ch < 2 && l; ++ch) {
                W2[ch][l] = p;
                p += H * H;
            }
        }
        W = p;
    }
};
template <typename P>
struct View {
    std::vector<P *> W1[2], W2[2];
    P *W;
    View(const gfsmp::Config &c, P *p) {
        const Layout at(c);
        for (int ch = 0; ch < 2; ++ch)
            for (int l = 0; l <= c.nLevels; ++l) {
                W1[ch].push_back(p + at.W1[ch][l]);
                W2[ch].push_back(l ? p + at.W2[ch][l] : nullptr);
            }
        W = p + at.W;
    }
};

bool per_channel_launches() { return env_is("GF_SMP_DISTANCE_LAUNCHES", '2'); }

gf_smp::DevLevel &level_of(gf_smp *s, int ch, int l) { return ch ? s->lvd[l] : s->lv[l]; }

gf_status level_forward(gf_smp *s, int l, const View<const float> &p) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &cfg = s->cfg;
    const int H = cfg.nChanels, nV = s->lay.level[0].nNodes;
    const bool pairs = cfg.neighbourhood == 3, third = l && cfg.third_order();
    const float *x[2] = {s->x, s->xd};
    const int width[2] = {cfg.fdim(), cfg.max_nVertices};
    gf_nbh_fwd_set set[2];
    for (int ch = 0; ch < 2; ++ch) {
        gf_smp::DevLevel &d = level_of(s, ch, l);
        const gf_smp::DevLevel *pv = l ? &level_of(s, ch, l - 1) : nullptr;
        if (third) {   // n_l from smp_level_third.hip, handed on as a sum of one term over N(v) = {v}
            const gf_status st = smp_third_pool_fwd_launch(ctx, H, nV, d.nb_max_members, pv->f, d.nb_ptr, d.nb_idx, d.nb_pool, d.nb_sel);
            if (st != GF_OK) return st;
        }
        set[ch] = {width[ch], p.W1[ch][l], x[ch], p.W2[ch][l], /*hprev=*/third ? d.nb_pool : pv ? pv->f : nullptr, /*Tprev=*/pv ? pv->nb_T : nullptr,
                   /*h=*/d.f, /*n=*/d.th_A, /*A=*/d.th_B, /*T=*/d.nb_T, /*Tt=*/d.nb_Tt};
    }
    const gf_smp::DevLevel &d0 = s->lv[l];
    const long long *ptr = third ? s->nb_id_ptr : d0.nb_ptr;
    const int *idx = third ? s->nb_id_idx : d0.nb_idx;
    if (!per_channel_launches()) return smp_neighbourhood_fwd(ctx, pairs, H, nV, 0, set, 2, ptr, idx);
    gf_status st = GF_OK;
    for (int ch = 0; ch < 2 && st == GF_OK; ++ch) st = smp_neighbourhood_fwd(ctx, pairs, H, nV, 0, &set[ch], 1, ptr, idx);
    return st;
}

// dz_l in place of dh_l (the top level from dy and its half of W) and dh_{l-1}, both channels
gf_status level_backward(gf_smp *s, int l, const View<const float> &p) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &cfg = s->cfg;
    const int H = cfg.nChanels, L = cfg.nLevels, nV = s->lay.level[0].nNodes;
    const bool pairs = cfg.neighbourhood == 3, third = l && cfg.third_order(), top = l == L, split = per_channel_launches();
    const float *dy = top ? s->dy : nullptr;
    gf_nbh_node_set node[2];
    gf_nbh_gather_set gat[2];
    for (int ch = 0; ch < 2; ++ch) {
        gf_smp::DevLevel &d = level_of(s, ch, l);
        gf_smp::DevLevel *pv = l ? &level_of(s, ch, l - 1) : nullptr;
        node[ch] = {p.W2[ch][l], /*h=*/d.f, /*dh=*/d.df, /*Wout=*/top ? p.W + (size_t)ch * H : nullptr, /*A=*/d.th_B, /*Tt=*/d.nb_Tt,
                    /*dn=*/d.Q, /*gTt=*/d.th_node, /*sA=*/d.nb_sA};
        gat[ch] = {/*dn=*/d.Q, /*gTt=*/d.th_node, /*sA=*/d.nb_sA, /*hprev=*/pv ? pv->f : nullptr, /*Tprev=*/pv ? pv->nb_T : nullptr,
                   /*dhprev=*/pv ? pv->df : nullptr};
    }
    gf_status st = GF_OK;
    if (!split) st = smp_neighbourhood_node(ctx, pairs, H, nV, 0, node, 2, dy, s->top_node_mol);
    for (int ch = 0; ch < 2 && split && st == GF_OK; ++ch) st = smp_neighbourhood_node(ctx, pairs, H, nV, 0, &node[ch], 1, dy, s->top_node_mol);
    if (st != GF_OK || !l) return st;
    const gf_smp::DevLevel &d0 = s->lv[l];
    if (third) {
        for (int ch = 0; ch < 2 && st == GF_OK; ++ch) {
            const gf_smp::DevLevel &d = level_of(s, ch, l);
            st = smp_third_pool_bwd_launch(ctx, H, nV, d.nb_ptr, d.nb_idx, d.nb_tptr, d.nb_tidx, gat[ch].hprev, d.nb_sel, d.Q, gat[ch].dhprev);
        }
        return st;
    }
    if (!split) return smp_neighbourhood_gather(ctx, pairs, H, nV, d0.nb_tptr, d0.nb_tidx, gat, 2);
    for (int ch = 0; ch < 2 && st == GF_OK; ++ch) st = smp_neighbourhood_gather(ctx, pairs, H, nV, d0.nb_tptr, d0.nb_tidx, &gat[ch], 1);
    return st;
}

int next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

gf_status smp_distance_rows_launch(gf_ctx *ctx, hipStream_t stream, int nV, int M, const double *dist, const long long *mat_off, const int *mol_ptr,
                                   const int *vmol, float *xd) {
    const int P = next_pow2(M);
    if (P <= 64) {
        const int per_group = kBlock / P;
        hipLaunchKernelGGL(dist_rows_sort_wave, dim3((unsigned)((nV + per_group - 1) / per_group)), dim3(kBlock), 0, stream, dist, mat_off, mol_ptr, vmol,
                           xd, nV, M, P);
    } else {
        hipLaunchKernelGGL(dist_rows_sort_lds, dim3((unsigned)nV), dim3(kBlock), sizeof(float) * (size_t)P, stream, dist, mat_off, mol_ptr, vmol, xd, nV,
                           M, P);
    }
    GF_LAUNCH_CHECK(ctx, "dist_rows_sort");
    return GF_OK;
}

gf_status smp_distance_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, nMol = s->lay.nMol;
    const View<const float> p(s->cfg, params);
    for (int l = 0; l <= L; ++l) {
        const gf_status st = level_forward(s, l, p);
        if (st != GF_OK) return st;
    }
    GF_LAUNCH(ctx, "dist_readout", dist_readout, dim3(nMol), dim3(64), 0, s->lv[L].f, s->lvd[L].f, s->mol_ptr, p.W, targets, s->g, s->yhat, loss, s->dy,
              H);
    return finish_forward(s, targets != nullptr, predict, graph_feature, 2 * (size_t)H);
}

// The reverse sweep from the loss of the last forward; every level keeps what a second sweep needs (dz is rebuilt from dy downwards).
gf_status smp_distance_backward(gf_smp *s, const float *params, float *grads, int accumulate) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, nMol = s->lay.nMol, nV = s->lay.level[0].nNodes;
    const View<const float> p(s->cfg, params);
    const View<float> d(s->cfg, grads);
    const float *x[2] = {s->x, s->xd};
    const int width[2] = {s->cfg.fdim(), s->cfg.max_nVertices};
    if (!accumulate) GF_HIP_TRY(ctx, hipMemsetAsync(grads, 0, sizeof(float) * param_count(s->cfg), ctx->stream));
    const gf_status wst = smp_vertex_readout_dW(ctx, "dist_readout_dW", 2 * H, nMol, s->dy, s->g, d.W);
    if (wst != GF_OK) return wst;
    for (int l = L; l >= 0; --l) {
        gf_status st = level_backward(s, l, p);   // dz_l in lv / lvd[l].df, dh_{l-1} in [l - 1].df
        // per channel dW1_l [H][width] += dz^T X, dW2_l [H][H] += dz^T N: tall-skinny TN products over the vertices of the batch
        for (int ch = 0; ch < 2 && st == GF_OK; ++ch) {
            const gf_smp::DevLevel &dl = level_of(s, ch, l);
            st = gemm(ctx, true, false, H, width[ch], nV, dl.df, H, 0, x[ch], width[ch], 0, d.W1[ch][l], width[ch], 0, 1, 1);
            if (st == GF_OK && l) st = gemm(ctx, true, false, H, H, nV, dl.df, H, 0, dl.th_A, H, 0, d.W2[ch][l], H, 0, 1, 1);
        }
        if (st != GF_OK) return st;
    }
    mark_used(s);
    return GF_OK;
}

void smp_distance_checkpoint_order(const gfsmp::Config &c, std::vector<size_t> *perm) {
    const Layout v(c);
    const size_t H = (size_t)c.nChanels, width[2] = {(size_t)c.fdim(), (size_t)c.max_nVertices};
    perm->clear();
    const auto block = [&](size_t first, size_t n) {
        for (size_t i = 0; i < n; ++i) perm->push_back(first + i);
    };
    for (int ch = 0; ch < 2; ++ch)   // save_model: the vertex channel's blocks by level, then the distance channel's, then W
        for (int l = 0; l <= c.nLevels; ++l) {
            block(v.W1[ch][l], H * width[ch]);
            if (l) block(v.W2[ch][l], H * H);
        }
    block(v.W, 2 * H);
}

}  // namespace gf

// ---- the row builder as a stand-alone operator (include/gf_hip.h; tests/test_smp_distance_ops_gpu.py) ----
extern "C" gf_status gf_smp_distance_rows_ex_f32(gf_ctx *ctx, int nMol, int M, const int *mol_ptr, const int *nVertices, const double *distance,
                                                 float *x_d) {
    static const char *who = "gf_smp_distance_rows_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (nMol < 1 || M < 1 || M > 4096) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d molecules, rows of %d entries (1 .. 4096)", who, nMol, M);
    if (!mol_ptr || !nVertices || !distance || !x_d) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int> mp((size_t)nMol + 1), nv((size_t)nMol);
    GF_HIP_TRY(ctx, hipMemcpyAsync(mp.data(), mol_ptr, sizeof(int) * mp.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipMemcpyAsync(nv.data(), nVertices, sizeof(int) * nv.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (mp[0] != 0) return gf::fail(ctx, GF_ERR_INVALID, "%s: mol_ptr starts at %d, not at 0", who, mp[0]);
    std::vector<long long> off((size_t)nMol);
    long long total = 0;
    for (int m = 0; m < nMol; ++m) {
        const int V = nv[(size_t)m];
        if (V < 1 || V > M) return gf::fail(ctx, GF_ERR_INVALID, "%s: molecule %d has %d vertices (1 .. M = %d)", who, m, V, M);
        if (mp[(size_t)m + 1] - mp[(size_t)m] != V)
            return gf::fail(ctx, GF_ERR_INVALID, "%s: mol_ptr gives molecule %d %d vertices, nVertices %d", who, m, mp[(size_t)m + 1] - mp[(size_t)m], V);
        off[(size_t)m] = total;
        total += (long long)V * V;
    }
    const int nV = mp[(size_t)nMol];
    std::vector<double> h((size_t)total);
    GF_HIP_TRY(ctx, hipMemcpyAsync(h.data(), distance, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int m = 0; m < nMol; ++m) {
        const size_t n = (size_t)nv[(size_t)m] * (size_t)nv[(size_t)m];
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(h[(size_t)off[(size_t)m] + i]))
                return gf::fail(ctx, GF_ERR_INVALID, "%s: molecule %d has a distance entry that is not finite", who, m);
    }
    std::vector<int> vmol((size_t)nV);
    for (int m = 0; m < nMol; ++m)
        for (int v = mp[(size_t)m]; v < mp[(size_t)m + 1]; ++v) vmol[(size_t)v] = m;
    // the two small tables of the launch: one allocation for the length of the call (a test operator: blocking)
    const size_t off_bytes = sizeof(long long) * off.size();
    char *tab = nullptr;
    GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&tab), off_bytes + sizeof(int) * vmol.size()));
    gf_status st = GF_OK;
    hipError_t e = hipMemcpyAsync(tab, off.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tab + off_bytes, vmol.data(), sizeof(int) * vmol.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        st = gf::smp_distance_rows_launch(ctx, ctx->stream, nV, M, distance, reinterpret_cast<const long long *>(tab),
                                          mol_ptr, reinterpret_cast<const int *>(tab + off_bytes), x_d);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    (void)hipFree(tab);
    if (e != hipSuccess || e2 != hipSuccess) return gf::fail(ctx, GF_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2));
    return st;
}
