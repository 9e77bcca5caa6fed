// smp_level_readouts.hip -- the two read-outs of gf_smp_config.readout above the softmax neighbourhood level (smp_level_neighbourhood.hip,
// smp_level_third.hip), whose levels, lists and buffers they share:
//   readout = 1  GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (GraphFlow/GCN_*D_Kernel.h): kernel learning on PAIRS of graphs.  The batch is
//                the 2 nPairs graphs X_0, Y_0, X_1, Y_1, .. (gfsmp::interleave_pairs): graph 2 p + side belongs to pair p.
//                  g[p] = [sum_v h^X_L[v] | sum_v h^Y_L[v]] [2 H],  predict = <W, g[p]>,  loss = 0.5 (predict - target)^2
//   readout = 2  GCA_1D (GraphFlow/GCA_1D.h, LinearGram.h): the graph auto-encoder, no W and no target.
//                  G[x][y] = <h_L[x], h_L[y]>,  loss = 0.5 sum_{x,y} (G[x][y] - adj[x][y])^2,  E = G - adj,
//                  dh_L[x] = sum_y (E[x][y] + E[y][x]) h_L[y]      (LinearGram::backward: the diagonal term counts twice)
//   pair_readout     one wave per pair: the two segment sums in ascending vertex order, predict, loss, dy
//   dW [2 H] += sum_p dy[p] g[p] is smp_vertex_level.hip's vertex_readout_dW under the timer name pair_readout_dW
//   pair_dh          dh_L[v][c] = dy[pair(v)] W[side(v) H + c], one workgroup per graph; the levels' reverse kernels then run with dy = NULL
//   gram_readout     one workgroup per molecule, one launch for G, the loss and dh_L (below)
// Every sum runs in a fixed order; no atomics; two runs give the same bits.  Both read-outs are also operators of the C ABI on
// caller-supplied operands (gf_smp_pair_readout_ex_f32, gf_smp_gram_readout_ex_f32 at the end of the file).
#include <cmath>

#include "smp_vertex_level.h"

namespace gf {
using namespace vertex_level;
namespace {

__global__ __launch_bounds__(64) void pair_readout(const float *__restrict__ hL, const int *__restrict__ graph_ptr, const float *__restrict__ W,
                                                   const float *__restrict__ target, float *__restrict__ g, float *__restrict__ yhat,
                                                   float *__restrict__ loss, float *__restrict__ dy, int H) {
    const int p = blockIdx.x;
    float part = 0.f;
    for (int side = 0; side < 2; ++side) {
        const int v0 = graph_ptr[2 * p + side], v1 = graph_ptr[2 * p + side + 1];
        for (int c = threadIdx.x; c < H; c += 64) {
            float acc = 0.f;
            for (int v = v0; v < v1; ++v) acc += hL[(size_t)v * H + c];
            g[((size_t)2 * p + side) * H + c] = acc;
            part = fmaf(acc, W[side * H + c], part);
        }
    }
    part = wave_sum(part);
    GF_STORE_PREDICTION(p, part, target, yhat, loss, dy);
}

// ConCat::backward and RisiLayer1D::backward: every vertex of graph 2 p + side gets dy[p] W[side H ..]
__global__ __launch_bounds__(kBlock) void pair_dh(const int *__restrict__ graph_ptr, const float *__restrict__ dy, const float *__restrict__ W,
                                                  float *__restrict__ dhL, int H) {
    const int gr = blockIdx.x, v0 = graph_ptr[gr], n = (graph_ptr[gr + 1] - v0) * H;
    const float d = dy[gr >> 1];
    const float *w = W + (size_t)(gr & 1) * H;
    float *out = dhL + (size_t)v0 * H;
    for (int i = threadIdx.x; i < n; i += kBlock) out[i] = d * w[i % H];
}

// The Gram read-out of one molecule per workgroup.  LDS (gf::smp_gram_lds_bytes): hs [V][Hp], Hp = H | 1; E [V][Vp], Vp = V | 1; four floats.
// The row stride of hs is ODD, and that serves both products (ds_read_b32 banks are dword address mod 32, per 32-lane half):
//   G[x][y] = <hs[x], hs[y]>: lanes run along y -- lane addresses y Hp + c are 32 different banks for 32 consecutive y (an odd stride
//             is a unit modulo 32); hs[x][c] is one address for the lanes of a row (a broadcast).  A stride of H = 64 would put all 32
//             lanes on one bank.
//   dh[x][c] = sum_y S[x][y] hs[y][c]: lanes run along c -- consecutive words whatever the stride; S[x][y] = E[x][y] + E[y][x] is one
//             address per row x, and where a half-wave spans several rows (H < 32) their addresses x Vp + y and y Vp + x differ by
//             multiples of the odd Vp or by single words: distinct banks again.
// The loops are strided over the V V entries and the V H outputs (V runs from 1 to the configuration's bound); the loss is each lane's
// partial in its own fixed order, a butterfly across the wave and the four wave partials added in order.  fp32 FMAs; no atomics.
__global__ __launch_bounds__(kBlock) void gram_readout(const float *__restrict__ hL, const int *__restrict__ mol_ptr, const float *__restrict__ adj,
                                                       const long long *__restrict__ mat_off, float *__restrict__ gram, float *__restrict__ loss,
                                                       float *__restrict__ dhL, int H) {
    extern __shared__ __align__(16) float lds[];
    const int m = blockIdx.x, v0 = mol_ptr[m], V = mol_ptr[m + 1] - v0;
    if (V <= 0) {   // (uniform for the workgroup: an empty molecule of a stand-alone call)
        if (loss && threadIdx.x == 0) loss[m] = 0.f;
        return;
    }
    const int Hp = H | 1, Vp = V | 1;
    float *hs = lds;                      // [V][Hp]
    float *E = hs + (size_t)V * Hp;       // [V][Vp]
    float *red = E + (size_t)V * Vp;      // [4]
    const float *src = hL + (size_t)v0 * H;
    for (int i = threadIdx.x; i < V * H; i += kBlock) {
        const int x = i / H, c = i - x * H;
        hs[x * Hp + c] = src[i];
    }
    __syncthreads();
    const long long off = mat_off[m];
    float part = 0.f;
    for (int i = threadIdx.x; i < V * V; i += kBlock) {
        const int x = i / V, y = i - x * V;
        const float *a = hs + x * Hp, *b = hs + y * Hp;
        float gxy = 0.f;
        for (int c = 0; c < H; ++c) gxy = fmaf(a[c], b[c], gxy);
        gram[off + i] = gxy;
        const float e = gxy - adj[off + i];
        E[x * Vp + y] = e;
        part = fmaf(e, e, part);
    }
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();   // (E is complete as well)
    if (loss && threadIdx.x == 0) loss[m] = 0.5f * (((red[0] + red[1]) + red[2]) + red[3]);
    if (!dhL) return;
    float *dst = dhL + (size_t)v0 * H;
    for (int i = threadIdx.x; i < V * H; i += kBlock) {
        const int x = i / H, c = i - x * H;
        float acc = 0.f;
        for (int y = 0; y < V; ++y) acc = fmaf(E[x * Vp + y] + E[y * Vp + x], hs[y * Hp + c], acc);
        dst[i] = acc;
    }
}

gf_status gram_launch(gf_ctx *ctx, int H, int nMol, int maxV, const float *hL, const int *mol_ptr, const float *adj, const long long *mat_off,
                      float *gram, float *loss, float *dhL) {
    const size_t bytes = smp_gram_lds_bytes(maxV, H);
    const gf_status st = opt_in_lds(ctx, gram_readout, bytes);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "gram_readout", gram_readout, dim3((unsigned)nMol), dim3(kBlock), bytes, hL, mol_ptr, adj, mat_off, gram, loss, dhL, H);
    return GF_OK;
}

gf_status pair_dh_launch(gf_ctx *ctx, int H, int nPairs, const int *graph_ptr, const float *dy, const float *W, float *dhL) {
    GF_LAUNCH(ctx, "pair_dh", pair_dh, dim3((unsigned)(2 * nPairs)), dim3(kBlock), 0, graph_ptr, dy, W, dhL, H);
    return GF_OK;
}

}  // namespace

// (called by smp_neighbourhood_forward in place of nbh_readout; the levels are done)
gf_status smp_readout_forward(gf_smp *s, const float *W, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, nMol = s->lay.nMol;
    if (s->cfg.readout == 2)   // (dh_L unconditionally: a gf_smp_backward after this forward needs no second launch)
        return gram_launch(ctx, H, nMol, s->lay.max_vertices, s->lv[L].f, s->mol_ptr, s->gram_adj, s->gram_off, s->gram, loss, s->lv[L].df);
    const int nPairs = nMol / 2;
    GF_LAUNCH(ctx, "pair_readout", pair_readout, dim3((unsigned)nPairs), dim3(64), 0, s->lv[L].f, s->mol_ptr, W, targets, s->g, s->yhat, loss, s->dy, H);
    if (predict) GF_HIP_TRY(ctx, hipMemcpyAsync(predict, s->yhat, sizeof(float) * nPairs, hipMemcpyDeviceToDevice, ctx->stream));
    if (graph_feature)
        GF_HIP_TRY(ctx, hipMemcpyAsync(graph_feature, s->g, sizeof(float) * nPairs * 2 * H, hipMemcpyDeviceToDevice, ctx->stream));
    return GF_OK;
}

// (called by smp_neighbourhood_backward in place of nbh_readout_dW: the read-out's reverse leaves dh_L in lv[L].df.  A Gram handle's
// forward has left it there already, and the top level's nbh_node_bwd replaces it by dz_L: one reverse sweep per forward)
gf_status smp_readout_dW(gf_smp *s, const float *W, float *dW) {
    if (s->cfg.readout == 2) {
        s->bwd_consumed = true;
        return GF_OK;
    }
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, nPairs = s->lay.nMol / 2;
    const gf_status st = smp_vertex_readout_dW(s->ctx, "pair_readout_dW", 2 * H, nPairs, s->dy, s->g, dW);
    return st == GF_OK ? pair_dh_launch(s->ctx, H, nPairs, s->mol_ptr, s->dy, W, s->lv[L].df) : st;
}

}  // namespace gf

extern "C" {

gf_status gf_smp_gram(gf_smp *s, float *out) {
    if (!s) return gf::fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (s->cfg.readout != 2) return gf::fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_gram: the handle has no Gram read-out (gf_smp_config.readout = %d)", s->cfg.readout);
    if (!out) return gf::fail(ctx, GF_ERR_INVALID, "gf_smp_gram: null argument");
    if (!s->prepared || !s->forwarded) return gf::fail(ctx, GF_ERR_INVALID, "gf_smp_gram before gf_smp_forward");
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    GF_HIP_TRY(ctx, hipMemcpyAsync(out, s->gram, sizeof(float) * s->gram_count, hipMemcpyDeviceToDevice, ctx->stream));
    gf::mark_used(s);
    return GF_OK;
}

// ---- the read-outs as stand-alone operators (include/gf_hip.h; tests/test_pair_gram_ops_gpu.py) ----
gf_status gf_smp_pair_readout_ex_f32(gf_ctx *ctx, int H, int nV, int nPairs, const float *hL, const int *graph_ptr, const float *W,
                                     const float *target, float *g, float *yhat, float *loss, float *dy, float *dW, float *dhL) {
    static const char *who = "gf_smp_pair_readout_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (H < 1 || H > gf::kNeighbourhoodMaxChanels) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d channels (1 .. %d)", who, H, gf::kNeighbourhoodMaxChanels);
    if (nV < 1 || nPairs < 1 || nPairs > 0x3fffffff) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d vertices, %d pairs", who, nV, nPairs);
    if (!hL || !graph_ptr || !W || !g || !yhat || !dy || !dW) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gf_status st = gf::check_ptr(ctx, who, "graph_ptr", graph_ptr, 2 * nPairs, nV);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "pair_readout", gf::pair_readout, dim3((unsigned)nPairs), dim3(64), 0, hL, graph_ptr, W, target, g, yhat, loss, dy, H);
    gf_status st2 = gf::smp_vertex_readout_dW(ctx, "pair_readout_dW", 2 * H, nPairs, dy, g, dW);
    if (st2 == GF_OK && dhL) st2 = gf::pair_dh_launch(ctx, H, nPairs, graph_ptr, dy, W, dhL);
    return st2;
}

gf_status gf_smp_gram_readout_ex_f32(gf_ctx *ctx, int H, int nV, int nMol, const float *hL, const int *mol_ptr, const float *adj, float *gram,
                                     float *loss, float *dhL) {
    static const char *who = "gf_smp_gram_readout_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (H < 1 || H > gf::kNeighbourhoodMaxChanels) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d channels (1 .. %d)", who, H, gf::kNeighbourhoodMaxChanels);
    if (nV < 1 || nMol < 1) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d vertices, %d molecules", who, nV, nMol);
    if (!hL || !mol_ptr || !adj || !gram) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gf_status st = gf::check_ptr(ctx, who, "mol_ptr", mol_ptr, nMol, nV);
    if (st != GF_OK) return st;
    std::vector<int> mp((size_t)nMol + 1);   // (checked above: from 0, never decreasing, within the nV rows)
    GF_HIP_TRY(ctx, hipMemcpyAsync(mp.data(), mol_ptr, sizeof(int) * mp.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<long long> off((size_t)nMol);
    long long total = 0;
    int maxV = 1;
    for (int m = 0; m < nMol; ++m) {
        const int V = mp[(size_t)m + 1] - mp[(size_t)m];
        if (gf::smp_gram_lds_bytes(V, H) > 160 * 1024)
            return gf::fail(ctx, GF_ERR_INVALID, "%s: molecule %d has %d vertices: 4 (V (H | 1) + V (V | 1) + 4) = %zu bytes of LDS at %d channels (160 KiB)",
                            who, m, V, gf::smp_gram_lds_bytes(V, H), H);
        off[(size_t)m] = total;
        total += (long long)V * V;
        maxV = V > maxV ? V : maxV;
    }
    // the offsets of the launch: one allocation for the length of the call (a test operator: blocking)
    long long *tab = nullptr;
    GF_HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&tab), sizeof(long long) * off.size()));
    gf_status launched = GF_OK;
    const hipError_t e = hipMemcpyAsync(tab, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) launched = gf::gram_launch(ctx, H, nMol, maxV, hL, mol_ptr, adj, tab, gram, loss, dhL);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    (void)hipFree(tab);
    if (e != hipSuccess || e2 != hipSuccess) return gf::fail(ctx, GF_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : e2));
    return launched;
}

}  // extern "C"
