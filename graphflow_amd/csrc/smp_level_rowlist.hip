// smp_level_rowlist.hip -- the row-list GEMM level: LCNN (PATCHY-SAN, GraphFlow/LCNN.h) and GCN_MW (the Kipf-Welling GCN in matrix form,
// GraphFlow/GCN_MW.h), gf_smp_config.matrix_form = 1, 2.  Neither is a per-vertex softmax over a neighbour list; both are products whose
// A operand is a short list of rows of the level below per output row:
//
//   A[r][slot * Cin + c] = sum over the entries e of row r with that slot of coef_e * X[src_e][c]          (K = slots * Cin columns)
//
//   use                  slots   entries per slot              list
//   LCNN forward         k       one, coefficient 1            row (m, i): the sequence of rank position i
//   LCNN backward-data   k       any number, including none    row (m, u): the (i, j) with seq[i][j] = u, slot j
//   GCN_MW forward       1       weighted (A-hat[v][u])        row v: the non-zero columns of A-hat
//   GCN_MW backward      1       weighted (A-hat[v][u])        row u: the non-zero rows of column u
//
// The lists are CSR (ptr [R + 1], then per entry src, slot, coef), a row's entries in ascending slot order.  A handle's lists also carry
// the first entry of every (row, slot) (sptr [R slots + 1]; one slot: ptr itself), so that its kernels search nothing; a stand-alone
// operator's list comes without it and every element searches its row's entries for its slot.  Kernels:
//   rowlist_gemm<TB>   out = act(A B + bias).  The A tile is assembled from the list straight into the LDS operand image of gemm_lds.h
//                      (it never exists in memory); v_mfma_f32_32x32x2_f32, fp32 accumulation.  TB: B is read as the forward's matrix
//                      transposed slot by slot -- element (slot * Cin + a, n) = B[(slot * N + n) * Cin + a] -- which is what both
//                      backward-data products need (LCNN: F [k][Cprev][Cnext] against dOut [.][Cnext]; one slot: the plain transpose).
//                      LeakyReLU keeps the sign of z, so the stored output is all the reverse sweep needs for the slope; a level without
//                      an activation stores the pre-activation.
//   rowlist_wgrad      dB += A^T dOut: the TN product of the same assembled operand, split over row chunks into partial images that
//                      splitk_fold adds in ascending order (deterministic).
//   colsum_chunks      the column sums of dOut per row chunk, 16 row classes folded in order; splitk_fold adds the chunks to db.
//   mf_dz, mf_rowsum, mf_readout, mf_readout_dW   LeakyReLU', GCN_MW's row-sum read-out, prediction / loss / dy, dW.
// LCNN's dense layer is a [nMol][V C2] x [V C2][nDense] product: the library's tiled GEMM (gf::gemm).  No atomics anywhere: two runs give
// the same bits.  The two products are also operators of the C ABI (gf_smp_rowlist_product_ex_f32, gf_smp_rowlist_wgrad_ex_f32).
#include <vector>

#include "gemm_lds.h"
#include "smp_vertex_level.h"

namespace gf {
using namespace vertex_level;
namespace {

using namespace lds_image;

struct DevList {
    const long long *ptr;
    const int *src, *slot;
    const float *coef;      // null: every coefficient is 1
    const long long *sptr;  // null, or [R slots + 1]: the first entry of every (row, slot) -- then nothing is searched
};

// A[r][slot * Cin + c] of row r: the entries of (r, slot) straight from sptr, or the row's entries (ascending slot order) searched for the slot
__device__ __forceinline__ float assemble(const DevList &L, const float *__restrict__ X, int ldx, int r, int slots, int slot, int c) {
    float acc = 0.f;
    if (L.sptr) {
        const long long e1 = L.sptr[(size_t)r * slots + slot + 1];
        for (long long e = L.sptr[(size_t)r * slots + slot]; e < e1; ++e) acc = fmaf(L.coef ? L.coef[e] : 1.f, X[(size_t)L.src[e] * ldx + c], acc);
        return acc;
    }
    const long long e1 = L.ptr[r + 1];
    for (long long e = L.ptr[r]; e < e1; ++e) {
        const int sl = L.slot[e];
        if (sl > slot) break;
        if (sl == slot) acc = fmaf(L.coef ? L.coef[e] : 1.f, X[(size_t)L.src[e] * ldx + c], acc);
    }
    return acc;
}

// the k-loop over one pair of LDS images: wave (wm, wn) owns rows [64 wm, 64 wm + 64) x columns [32 wn, 32 wn + 32) (mixers.hip)
__device__ __forceinline__ void mfma_tile(const float *As, const float *Bs, int wm, int wn, int li, int lh, f16v &acc0, f16v &acc1) {
    const float *a0p = As + (wm * 64 + li) * LDS_ROW + lh * (BK / 2);
    const float *a1p = a0p + 32 * LDS_ROW;
    const float *bp = Bs + (wn * 32 + li) * LDS_ROW + lh * (BK / 2);
    const int za0 = lds_swz(wm * 64 + li), za1 = lds_swz(wm * 64 + 32 + li), zb = lds_swz(wn * 32 + li);
    f4v fa0[4], fa1[4], fb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        fa0[q] = *reinterpret_cast<const f4v *>(a0p + 4 * (q ^ za0));
        fa1[q] = *reinterpret_cast<const f4v *>(a1p + 4 * (q ^ za1));
        fb[q] = *reinterpret_cast<const f4v *>(bp + 4 * (q ^ zb));
    }
#pragma unroll
    for (int j = 0; j < BK / 2; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0[j >> 2][j & 3], fb[j >> 2][j & 3], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1[j >> 2][j & 3], fb[j >> 2][j & 3], acc1, 0, 0, 0);
    }
}

// out [R][N] = act(A [R][slots Cin] B + bias); one 128 x 64 tile per workgroup, the N tile varying fastest
template <bool TB>
__global__ __launch_bounds__(kThreads) void rowlist_gemm(DevList L, const float *__restrict__ X, int Cin, int slots, const float *__restrict__ B,
                                                         const float *__restrict__ bias, float *__restrict__ out, int R, int N, int act) {
    __shared__ __attribute__((aligned(16))) float smem[(BM + BN) * LDS_ROW];
    float *As = smem, *Bs = smem + BM * LDS_ROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int ntn = (N + BN - 1) / BN;
    const int m0 = (int)(blockIdx.x / ntn) * BM, n0 = (int)(blockIdx.x % ntn) * BN;
    const int K = slots * Cin;
    // a thread assembles column tid % 32 of the step for the rows tid / 32 + 8 e of the tile
    const int ka = tid % BK, ma = tid / BK;
    f16v acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
    for (int k0 = 0; k0 < K; k0 += BK) {
        {
            const int gk = k0 + ka, slot = gk / Cin, c = gk - slot * Cin;
            const int kp = kpos(ka);
#pragma unroll 4
            for (int e = 0; e < BM * BK / kThreads; ++e) {
                const int m = ma + e * (kThreads / BK), gm = m0 + m;
                As[lds_at(m, kp)] = gk < K && gm < R ? assemble(L, X, Cin, gm, slots, slot, c) : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < BN * BK / kThreads; ++e) {
            const int idx = tid + e * kThreads;
            int k, n;
            if (TB) { k = idx % BK; n = idx / BK; } else { n = idx % BN; k = idx / BN; }
            const int gk = k0 + k, gn = n0 + n;
            float v = 0.f;
            if (gk < K && gn < N) {
                if (TB) {
                    const int slot = gk / Cin, a = gk - slot * Cin;
                    v = B[((size_t)slot * N + gn) * Cin + a];
                } else {
                    v = B[(size_t)gk * N + gn];
                }
            }
            Bs[lds_at(n, kpos(k))] = v;
        }
        __syncthreads();
        mfma_tile(As, Bs, wm, wn, li, lh, acc0, acc1);
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int col = n0 + wn * 32 + li;
    if (col >= N) return;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float z0 = acc0[r] + bv, z1 = acc1[r] + bv;
        if (act) {
            z0 = z0 > 0.f ? z0 : 0.01f * z0;
            z1 = z1 > 0.f ? z1 : 0.01f * z1;
        }
        if (row < R) out[(size_t)row * N + col] = z0;
        if (row + 32 < R) out[(size_t)(row + 32) * N + col] = z1;
    }
}

// part [split][K][N] = the rows [split * rchunk, (split + 1) * rchunk) of A^T dOut; tiles of 128 columns of A x 64 columns of dOut.
// blockIdx.x = (split, k tile, n tile), the n tile varying fastest.  rchunk is a multiple of BK.
__global__ __launch_bounds__(kThreads) void rowlist_wgrad(DevList L, const float *__restrict__ X, int Cin, int slots, const float *__restrict__ dOut,
                                                          float *__restrict__ part, int R, int N, int rchunk) {
    __shared__ __attribute__((aligned(16))) float smem[(BM + BN) * LDS_ROW];
    float *As = smem, *Bs = smem + BM * LDS_ROW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int K = slots * Cin;
    const int ntn = (N + BN - 1) / BN, ntk = (K + BM - 1) / BM;
    const int split = (int)(blockIdx.x / (unsigned)(ntn * ntk)), t = (int)(blockIdx.x % (unsigned)(ntn * ntk));
    const int m0 = (t / ntn) * BM, n0 = (t % ntn) * BN;
    const int rbeg = split * rchunk, rend = rbeg + rchunk < R ? rbeg + rchunk : R;
    // a thread assembles one column of A (tid % 128) for the rows tid / 128 + 2 e of the step
    const int gk = m0 + tid % BM, slot = gk / Cin, c = gk - slot * Cin;
    f16v acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
    for (int r0 = rbeg; r0 < rend; r0 += BK) {
#pragma unroll
        for (int e = 0; e < BM * BK / kThreads; ++e) {
            const int rr = tid / BM + e * (kThreads / BM), gr = r0 + rr;
            float v = 0.f;
            if (gk < K && gr < rend) v = assemble(L, X, Cin, gr, slots, slot, c);
            As[lds_at(tid % BM, kpos(rr))] = v;
        }
#pragma unroll
        for (int e = 0; e < BN * BK / kThreads; ++e) {
            const int idx = tid + e * kThreads, n = idx % BN, rr = idx / BN;
            const int gr = r0 + rr, gn = n0 + n;
            Bs[lds_at(n, kpos(rr))] = (gr < rend && gn < N) ? dOut[(size_t)gr * N + gn] : 0.f;
        }
        __syncthreads();
        mfma_tile(As, Bs, wm, wn, li, lh, acc0, acc1);
        __syncthreads();
    }
    const int col = n0 + wn * 32 + li;
    if (col >= N) return;
    float *P = part + (size_t)split * K * N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 64 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < K) P[(size_t)row * N + col] = acc0[r];
        if (row + 32 < K) P[(size_t)(row + 32) * N + col] = acc1[r];
    }
}

// out[chunk][c] = the sum of d[r][c] over the chunk's rows [chunk * rchunk, ..): 64 columns per workgroup, row class q of its 16 sums the
// rows q, q + 16, .. of the chunk, the 16 partials are folded in order; splitk_fold then adds the chunks in ascending order
__global__ __launch_bounds__(1024) void colsum_chunks(const float *__restrict__ d, float *__restrict__ out, int R, int N, int rchunk) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const int cc = c < N ? c : N - 1;
    const int r0 = blockIdx.y * rchunk, r1 = r0 + rchunk < R ? r0 + rchunk : R;
    float acc = 0.f;
    for (int r = r0 + q; r < r1; r += 16) acc += d[(size_t)r * N + cc];
    part[q][lane] = acc;
    __syncthreads();
    if (q == 0 && c < N) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t += part[k][lane];
        out[(size_t)blockIdx.y * N + c] = t;
    }
}

// dz = dh * LeakyReLU'(h) in place (the slope from the sign of the stored activation); top != null: dh[r][c] = dy[row_mol[r]] * W[c] first
// (SumRows and InnerProduct backward)
__global__ void mf_dz(const float *__restrict__ h, float *__restrict__ dh, const float *__restrict__ dy, const float *__restrict__ W,
                      const int *__restrict__ row_mol, size_t n, int C) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / (size_t)C;
        const float g = dy ? dy[row_mol[r]] * W[i - r * (size_t)C] : dh[i];
        dh[i] = h[i] > 0.f ? g : 0.01f * g;
    }
}

// g[m][c] = sum over the molecule's rows of h[v][c] (SumRows), ascending
__global__ void mf_rowsum(const float *__restrict__ h, const int *__restrict__ mol_ptr, float *__restrict__ g, int nMol, int C) {
    const size_t n = (size_t)nMol * C;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int m = (int)(i / (size_t)C), c = (int)(i - (size_t)m * C);
        float acc = 0.f;
        for (int v = mol_ptr[m]; v < mol_ptr[m + 1]; ++v) acc += h[(size_t)v * C + c];
        g[i] = acc;
    }
}

// yhat[m] = <W, g[m]> (InnerProduct), loss = 0.5 (yhat - t)^2, dy = yhat - t (SquaredLoss); one wave per molecule
__global__ __launch_bounds__(64) void mf_readout(const float *__restrict__ g, const float *__restrict__ W, const float *__restrict__ target,
                                                 float *__restrict__ yhat, float *__restrict__ loss, float *__restrict__ dy, int C) {
    const int m = blockIdx.x;
    float part = 0.f;
    for (int c = threadIdx.x; c < C; c += 64) part = fmaf(g[(size_t)m * C + c], W[c], part);
    part = wave_sum(part);
    GF_STORE_PREDICTION(m, part, target, yhat, loss, dy);
}

// dW[c] += sum_m dy[m] g[m][c], the molecules in 16 classes folded in order; dg (optional) [nMol][C] = dy[m] W[c]
__global__ __launch_bounds__(1024) void mf_readout_dW(const float *__restrict__ dy, const float *__restrict__ g, const float *__restrict__ W,
                                                      float *__restrict__ dW, float *__restrict__ dg, int C, int nMol) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const int cc = c < C ? c : C - 1;
    const float w = W[cc];
    float acc = 0.f;
    for (int m = q; m < nMol; m += 16) {
        acc = fmaf(dy[m], g[(size_t)m * C + cc], acc);
        if (dg && c < C) dg[(size_t)m * C + c] = dy[m] * w;
    }
    part[q][lane] = acc;
    __syncthreads();
    if (q == 0 && c < C) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t += part[k][lane];
        dW[c] += t;
    }
}

inline unsigned grid_of(size_t n) {
    const size_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 65535 ? 65535 : b);
}

inline DevList dev(const RowList &l) { return DevList{l.ptr, l.src, l.slot, l.coef, l.sptr}; }

}  // namespace

// Row chunks of the weight gradient: whole k-steps, as many chunks as bring the launch to about 512 workgroups (a [64][64] gradient is ONE
// tile: without the split a level's whole batch would run on one compute unit), at most kRowlistSplits partial images.  Above 64 images
// splitk_fold adds in two stages and keeps the first stage's sums behind the images: room for kRowlistSplits / 32 more.
static int wgrad_chunk(int R, int K, int N) {
    const int tiles = ((K + BM - 1) / BM) * ((N + BN - 1) / BN);
    int want = (512 + tiles - 1) / tiles;
    want = want < 1 ? 1 : want > kRowlistSplits ? kRowlistSplits : want;
    const int per = (R + want - 1) / want;
    return (per + BK - 1) / BK * BK;
}
size_t smp_rowlist_wgrad_ws_bytes(int R, int K, int N) {
    const int rchunk = wgrad_chunk(R, K, N), splits = (R + rchunk - 1) / rchunk;
    return sizeof(float) * (size_t)(splits + kRowlistSplits / 32) * (size_t)K * (size_t)N;
}

gf_status smp_rowlist_product(gf_ctx *ctx, const RowList &list, bool tb, int R, int slots, int Cin, int N, const float *X, const float *B,
                              const float *bias, int act, float *out) {
    const long long tiles = (long long)((R + BM - 1) / BM) * ((N + BN - 1) / BN);
    if (tiles > 0x7fffffffll) return fail(ctx, GF_ERR_UNSUPPORTED, "row-list product: %lld tiles", tiles);
    if (tb)
        GF_LAUNCH(ctx, "rowlist_gemm_t", rowlist_gemm<true>, dim3((unsigned)tiles), dim3(kThreads), 0, dev(list), X, Cin, slots, B, bias, out, R, N, act);
    else
        GF_LAUNCH(ctx, "rowlist_gemm", rowlist_gemm<false>, dim3((unsigned)tiles), dim3(kThreads), 0, dev(list), X, Cin, slots, B, bias, out, R, N, act);
    return GF_OK;
}

gf_status smp_rowlist_wgrad(gf_ctx *ctx, const RowList &list, int R, int slots, int Cin, int N, const float *X, const float *dOut, float *dB) {
    const int K = slots * Cin, rchunk = wgrad_chunk(R, K, N), splits = (R + rchunk - 1) / rchunk;
    const gf_status st = ensure_ws(ctx, smp_rowlist_wgrad_ws_bytes(R, K, N));
    if (st != GF_OK) return st;
    const long long tiles = (long long)((K + BM - 1) / BM) * ((N + BN - 1) / BN) * splits;
    if (tiles > 0x7fffffffll) return fail(ctx, GF_ERR_UNSUPPORTED, "row-list weight gradient: %lld tiles", tiles);
    float *part = static_cast<float *>(ctx->ws);
    GF_LAUNCH(ctx, "rowlist_wgrad", rowlist_wgrad, dim3((unsigned)tiles), dim3(kThreads), 0, dev(list), X, Cin, slots, dOut, part, R, N, rchunk);
    return splitk_fold(ctx, part, dB, (size_t)K * N, splits, /*accumulate=*/1);
}

gf_status smp_rowlist_bias_grad(gf_ctx *ctx, const float *dOut, int R, int N, float *db) {
    const int rchunk = (R + 63) / 64 < 16 ? 16 : (R + 63) / 64, chunks = (R + rchunk - 1) / rchunk;   // (at most 64: one stage of splitk_fold)
    const gf_status st = ensure_ws(ctx, sizeof(float) * (size_t)chunks * N);
    if (st != GF_OK) return st;
    float *part = static_cast<float *>(ctx->ws);
    GF_LAUNCH(ctx, "rowlist_colsum", colsum_chunks, dim3((unsigned)((N + 63) / 64), (unsigned)chunks), dim3(1024), 0, dOut, part, R, N, rchunk);
    return splitk_fold(ctx, part, db, (size_t)N, chunks, /*accumulate=*/1);
}

namespace {

// GCN_MW: W_0 [F'][H]; W_l [H][H], l = 1..L; W [H].  LCNN: F1 [k][F'][C1], b1; F2 [k][C1][C2], b2; Dm [nDense][V C2]; W [nDense].
template <typename P>
struct View {
    std::vector<P *> W;   // GCN_MW: W_l
    P *F1, *b1, *F2, *b2, *Dm, *Wout;
    View(const gfsmp::Config &c, P *p) {
        std::vector<P *> K, b;
        P *first;
        view_params<P>(c, p, &first, &K, &b, &Wout);
        F1 = b1 = F2 = b2 = Dm = nullptr;
        if (c.matrix_form == 1) {   // (the matrix block of level 1 is b1 then F2, of level 2 b2 then Dm)
            F1 = first;
            b1 = K[1], F2 = K[1] + c.level_blocks(1).mat[0].n;
            b2 = K[2], Dm = K[2] + c.level_blocks(2).mat[0].n;
        } else {
            W = K;
            W[0] = first;
        }
    }
};

gf_status readout(gf_smp *s, const float *W, const float *targets, float *predict, float *loss, float *graph_feature, int width) {
    gf_ctx *ctx = s->ctx;
    const int nMol = s->lay.nMol;
    GF_LAUNCH(ctx, "mf_readout", mf_readout, dim3(nMol), dim3(64), 0, s->g, W, targets, s->yhat, loss, s->dy, width);
    return finish_forward(s, targets != nullptr, predict, graph_feature, width);
}

gf_status gcn_mw_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, FD = s->cfg.fdim(), nMol = s->lay.nMol, nV = s->lay.level[0].nNodes;
    const View<const float> p(s->cfg, params);
    for (int l = 0; l <= L; ++l) {   // h_l = LeakyReLU((A-hat h_{l-1}) W_l)
        const gf_status st = smp_rowlist_product(ctx, s->rl_fwd, false, nV, 1, l ? H : FD, H, l ? s->lv[l - 1].f : s->x, p.W[l], nullptr, 1, s->lv[l].f);
        if (st != GF_OK) return st;
    }
    GF_LAUNCH(ctx, "mf_rowsum", mf_rowsum, dim3(grid_of((size_t)nMol * H)), dim3(256), 0, s->lv[L].f, s->mol_ptr, s->g, nMol, H);
    return readout(s, p.Wout, targets, predict, loss, graph_feature, H);
}

gf_status gcn_mw_backward(gf_smp *s, const float *params, float *grads) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, H = s->cfg.nChanels, FD = s->cfg.fdim(), nMol = s->lay.nMol, nV = s->lay.level[0].nNodes;
    const View<const float> p(s->cfg, params);
    const View<float> d(s->cfg, grads);
    GF_LAUNCH(ctx, "mf_readout_dW", mf_readout_dW, dim3((unsigned)((H + 63) / 64)), dim3(1024), 0, s->dy, s->g, p.Wout, d.Wout, (float *)nullptr, H, nMol);
    for (int l = L; l >= 0; --l) {
        const int Cin = l ? H : FD;
        GF_LAUNCH(ctx, "mf_dz", mf_dz, dim3(grid_of((size_t)nV * H)), dim3(256), 0, s->lv[l].f, s->lv[l].df, l == L ? s->dy : (const float *)nullptr,
                  p.Wout, s->top_node_mol, (size_t)nV * H, H);
        gf_status st = smp_rowlist_wgrad(ctx, s->rl_fwd, nV, 1, Cin, H, l ? s->lv[l - 1].f : s->x, s->lv[l].df, d.W[l]);
        // dh_{l-1} = A-hat^T (dz_l W_l^T): the transposed list over dz_l against W_l transposed
        if (st == GF_OK && l) st = smp_rowlist_product(ctx, s->rl_bwd, true, nV, 1, H, H, s->lv[l].df, p.W[l], nullptr, 0, s->lv[l - 1].df);
        if (st != GF_OK) return st;
    }
    return GF_OK;
}

gf_status lcnn_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &c = s->cfg;
    const int k = c.nNeighbors, C1 = c.nChanels, C2 = c.nChanels2, nD = c.nDense, V = c.max_nVertices, FD = c.fdim(), nMol = s->lay.nMol, R = nMol * V;
    const View<const float> p(c, params);
    // c1 = rows(x) F1 + b1, a1 = LeakyReLU(c1); c2 = rows(a1) F2 + b2 -- the class indexes a1, whose rows are rank positions, with the
    // sequence's vertex ids, so both layers read through the same list
    gf_status st = smp_rowlist_product(ctx, s->rl_fwd, false, R, k, FD, C1, s->x, p.F1, p.b1, 1, s->lv[1].f);
    if (st == GF_OK) st = smp_rowlist_product(ctx, s->rl_fwd, false, R, k, C1, C2, s->lv[1].f, p.F2, p.b2, 0, s->lv[2].f);
    // dense [nMol][nDense] = vec(c2) Dm^T (the second LeakyReLU feeds nothing)
    if (st == GF_OK) st = gemm(ctx, false, true, nMol, nD, V * C2, s->lv[2].f, V * C2, 0, p.Dm, V * C2, 0, s->g, nD, 0, 1, 0);
    if (st != GF_OK) return st;
    return readout(s, p.Wout, targets, predict, loss, graph_feature, nD);
}

gf_status lcnn_backward(gf_smp *s, const float *params, float *grads) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &c = s->cfg;
    const int k = c.nNeighbors, C1 = c.nChanels, C2 = c.nChanels2, nD = c.nDense, V = c.max_nVertices, FD = c.fdim(), nMol = s->lay.nMol, R = nMol * V;
    const View<const float> p(c, params);
    const View<float> d(c, grads);
    float *ddense = s->lv[2].Q;
    GF_LAUNCH(ctx, "mf_readout_dW", mf_readout_dW, dim3((unsigned)((nD + 63) / 64)), dim3(1024), 0, s->dy, s->g, p.Wout, d.Wout, ddense, nD, nMol);
    // dDm [nDense][V C2] += ddense^T vec(c2);  dc2 = ddense Dm
    gf_status st = gemm(ctx, true, false, nD, V * C2, nMol, ddense, nD, 0, s->lv[2].f, V * C2, 0, d.Dm, V * C2, 0, 1, 1);
    if (st == GF_OK) st = gemm(ctx, false, false, nMol, V * C2, nD, ddense, nD, 0, p.Dm, V * C2, 0, s->lv[2].df, V * C2, 0, 1, 0);
    if (st == GF_OK) st = smp_rowlist_bias_grad(ctx, s->lv[2].df, R, C2, d.b2);
    if (st == GF_OK) st = smp_rowlist_wgrad(ctx, s->rl_fwd, R, k, C1, C2, s->lv[1].f, s->lv[2].df, d.F2);
    // da1 [u] = sum over the (i, j) with seq[i][j] = u of dc2[i] F2[j]^T, then dc1 = da1 LeakyReLU'(a1)
    if (st == GF_OK) st = smp_rowlist_product(ctx, s->rl_bwd, true, R, k, C2, C1, s->lv[2].df, p.F2, nullptr, 0, s->lv[1].df);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "mf_dz", mf_dz, dim3(grid_of((size_t)R * C1)), dim3(256), 0, s->lv[1].f, s->lv[1].df, (const float *)nullptr, (const float *)nullptr,
              (const int *)nullptr, (size_t)R * C1, C1);
    st = smp_rowlist_bias_grad(ctx, s->lv[1].df, R, C1, d.b1);
    if (st == GF_OK) st = smp_rowlist_wgrad(ctx, s->rl_fwd, R, k, FD, C1, s->x, s->lv[1].df, d.F1);
    return st;
}

}  // namespace

gf_status smp_matrix_form_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    return s->cfg.matrix_form == 1 ? lcnn_forward(s, params, targets, predict, loss, graph_feature)
                                   : gcn_mw_forward(s, params, targets, predict, loss, graph_feature);
}

// The reverse sweep from the loss of the last forward; nothing a second sweep needs is overwritten (dz is rebuilt from dy downwards).
gf_status smp_matrix_form_backward(gf_smp *s, const float *params, float *grads, int accumulate) {
    gf_ctx *ctx = s->ctx;
    if (!accumulate) GF_HIP_TRY(ctx, hipMemsetAsync(grads, 0, sizeof(float) * param_count(s->cfg), ctx->stream));
    const gf_status st = s->cfg.matrix_form == 1 ? lcnn_backward(s, params, grads) : gcn_mw_backward(s, params, grads);
    if (st == GF_OK) mark_used(s);
    return st;
}

}  // namespace gf

// ---- the two products as stand-alone operators (include/gf_hip.h; tests/test_rowlist_ops_gpu.py) ----
namespace {

// the list of a stand-alone call, checked on the host (one blocking copy: these are test operators): ptr starts at 0 and never decreases,
// every source row lies in [0, nX), every slot in [0, slots) and a row's slots never decrease
gf_status check_rowlist(gf_ctx *ctx, const char *who, int R, int slots, int nX, const long long *ptr, const int *src, const int *slot) {
    std::vector<long long> p((size_t)R + 1);
    GF_HIP_TRY(ctx, hipMemcpyAsync(p.data(), ptr, sizeof(long long) * p.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (p[0] != 0) return gf::fail(ctx, GF_ERR_INVALID, "%s: ptr starts at %lld, not at 0", who, p[0]);
    for (int r = 0; r < R; ++r)
        if (p[r + 1] < p[r]) return gf::fail(ctx, GF_ERR_INVALID, "%s: ptr decreases at entry %d", who, r + 1);
    if (p[R] > 0x7fffffffll) return gf::fail(ctx, GF_ERR_INVALID, "%s: ptr ends at %lld: more than 2^31 entries", who, p[R]);
    const size_t n = (size_t)p[R];
    std::vector<int> hs(n), hl(n);
    if (n) {
        GF_HIP_TRY(ctx, hipMemcpyAsync(hs.data(), src, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
        GF_HIP_TRY(ctx, hipMemcpyAsync(hl.data(), slot, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
        GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (int r = 0; r < R; ++r)
        for (long long e = p[r]; e < p[r + 1]; ++e) {
            if (hs[(size_t)e] < 0 || hs[(size_t)e] >= nX) return gf::fail(ctx, GF_ERR_INVALID, "%s: src[%lld] = %d outside [0, %d)", who, e, hs[(size_t)e], nX);
            if (hl[(size_t)e] < 0 || hl[(size_t)e] >= slots)
                return gf::fail(ctx, GF_ERR_INVALID, "%s: slot[%lld] = %d outside [0, %d)", who, e, hl[(size_t)e], slots);
            if (e > p[r] && hl[(size_t)e] < hl[(size_t)e - 1]) return gf::fail(ctx, GF_ERR_INVALID, "%s: the slots of row %d decrease at entry %lld", who, r, e);
        }
    return GF_OK;
}

gf_status check_rowlist_shape(gf_ctx *ctx, const char *who, int R, int slots, int Cin, int N, int nX) {
    if (R < 1 || nX < 1 || slots < 1 || Cin < 1 || N < 1) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad shape", who);
    if ((long long)slots * Cin > gf::kRowlistMaxWidth || N > gf::kRowlistMaxWidth)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: slots * Cin = %lld, N = %d (at most %d each)", who, (long long)slots * Cin, N, gf::kRowlistMaxWidth);
    return GF_OK;
}

}  // namespace

extern "C" {

gf_status gf_smp_rowlist_product_ex_f32(gf_ctx *ctx, int transposed_b, int R, int slots, int Cin, int N, int nX, const long long *ptr, const int *src,
                                        const int *slot, const float *coef, const float *X, const float *B, const float *bias, int act, float *out) {
    static const char *who = "gf_smp_rowlist_product_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = check_rowlist_shape(ctx, who, R, slots, Cin, N, nX);
    if (st != GF_OK) return st;
    if (!ptr || !src || !slot || !X || !B || !out) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = check_rowlist(ctx, who, R, slots, nX, ptr, src, slot);
    if (st != GF_OK) return st;
    return gf::smp_rowlist_product(ctx, gf::RowList{ptr, src, slot, coef, nullptr}, transposed_b != 0, R, slots, Cin, N, X, B, bias, act ? 1 : 0, out);
}

gf_status gf_smp_rowlist_wgrad_ex_f32(gf_ctx *ctx, int R, int slots, int Cin, int N, int nX, const long long *ptr, const int *src, const int *slot,
                                      const float *coef, const float *X, const float *dOut, float *dB, float *db) {
    static const char *who = "gf_smp_rowlist_wgrad_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = check_rowlist_shape(ctx, who, R, slots, Cin, N, nX);
    if (st != GF_OK) return st;
    if (!ptr || !src || !slot || !X || !dOut || !dB) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = check_rowlist(ctx, who, R, slots, nX, ptr, src, slot);
    if (st != GF_OK) return st;
    st = gf::smp_rowlist_wgrad(ctx, gf::RowList{ptr, src, slot, coef, nullptr}, R, slots, Cin, N, X, dOut, dB);
    if (st == GF_OK && db) st = gf::smp_rowlist_bias_grad(ctx, dOut, R, N, db);
    return st;
}

}  // extern "C"
