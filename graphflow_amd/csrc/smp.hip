// smp.hip -- batched SMP_omega (second-order CCN) forward/backward on the device.
//
// Reproduces the op DAG that SMP_omega::complete_computation_graph builds per molecule
// (GraphFlow/SMP_omega.h:607-692) for a whole BATCH of molecules at once:
//   level 0   f_0[v] = LeakyReLU(H x_v)                                         (:617-626)
//   level l   T_w = X_vw f_{l-1}[w] X_vw^T  for w in phi_l(v)   -> index gather (MatTensorMul + TensorMatMul, :641-645)
//             P = stack_w T_w ; Q = RisiContraction_18(P, A_v)                  (:647-651)
//             f_l[v] = LeakyReLU(reshape(Q)[s^2,18C] K_l + b_l)                 (:654-669)
//   readout   g = sum_v LeakyReLU(sum_ij f_L[v]) ; y = <g, W> ; loss = (y - t)^2 / 2   (:676-692)
// and the reverse sweep (GraphFlow.h:729: reverse insertion order; every op `+=` into its inputs).
// The X matrices are 0/1 selections, so X F X^T is F[pi(i), pi(j)] or 0 (verified exact in the tests): the promotion
// is an index gather forward and a deterministic consumer-list gather backward (no atomics).
// Nodes of a level are bucketed by receptive-field size; each bucket is one uniform-N contraction launch and all
// buckets share one tall K-projection GEMM per level.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "smp_internal.h"
#include "r18_device.h"

namespace gf {
namespace {
using namespace dev;

constexpr float kAlpha = 0.01f;  // LeakyReLU3D.h:41, LeakyReLU.h default

#define GRID_STRIDE(idx, total) \
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < (total); idx += (size_t)gridDim.x * blockDim.x)
unsigned grid_for(size_t total, int per_block = 256) {
    size_t blocks = (total + per_block - 1) / per_block;
    return (unsigned)(blocks > 1048576 ? 1048576 : (blocks == 0 ? 1 : blocks));
}

__device__ __forceinline__ float lrelu(float z) { return z > 0.f ? z : kAlpha * z; }

// ---- promotion: P[n][a][b][c][:] = f_prev[src(n,a)][pi(b)][pi(c)][:] or 0 -------------------------------------------
// one workgroup per (node, neighbour) pair; threads run over (b, c, channel) with the channel fastest (coalesced)
__global__ void promote_forward(const float *__restrict__ fprev, float *__restrict__ P, const int *__restrict__ node_s,
                                const long long *__restrict__ node_row, const long long *__restrict__ node_p,
                                const long long *__restrict__ node_pair, const int *__restrict__ pair_node,
                                const long long *__restrict__ pair_src_row, const int *__restrict__ pair_src_s,
                                const short *__restrict__ pi, int C) {
    const long long e = blockIdx.x;
    const int n = pair_node[e];
    const int s = node_s[n], a = (int)(e - node_pair[n]), sw = pair_src_s[e];
    const short *map = pi + node_row[n] + (long long)a * s;
    const float *src = fprev + pair_src_row[e] * C;
    float *dst = P + (node_p[n] + (long long)a * s * s) * C;
    if ((C & 3) == 0) {  // 16 B per lane over the channel axis; (c, quad) flattened per row b
        const int Q = C >> 2, per_row = s * Q;
        for (int b = 0; b < s; ++b) {
            const int pb = map[b];
            float4 *drow = reinterpret_cast<float4 *>(dst + (size_t)b * s * C);
            for (int i = threadIdx.x; i < per_row; i += blockDim.x) {
                const int c = i / Q, q = i - c * Q;
                const int pc = map[c];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pb >= 0 && pc >= 0) v = reinterpret_cast<const float4 *>(src + ((size_t)pb * sw + pc) * C)[q];
                drow[i] = v;
            }
        }
        return;
    }
    const int total = s * s * C;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int f = i % C, bc = i / C;
        const int b = bc / s, c = bc - b * s;
        const int pb = map[b], pc = map[c];
        dst[i] = (pb >= 0 && pc >= 0) ? src[((size_t)pb * sw + pc) * C + f] : 0.f;
    }
}

// backward: df_prev[w][p][q][:] = sum over consumers (n,a) of dP[n][a][inv(p)][inv(q)][:]
constexpr int kPromoteChunk = 64, kPromoteMaxS = 32;

__global__ void promote_backward(const float *__restrict__ dP, float *__restrict__ dfprev,
                                 const int *__restrict__ prev_s, const long long *__restrict__ prev_row,
                                 const long long *__restrict__ cons_ptr, const long long *__restrict__ cons_slab,
                                 const int *__restrict__ cons_s, const long long *__restrict__ cons_inv_off,
                                 const short *__restrict__ inv, int C,
                                 // compact-diagonal variant of the fused level (smp_fused.hip), else null: the gradients of
                                 // f[w][p,p] and f[w][p,c_w] arrive as dFdc[node_pair[w] + p] = [ .. | .. ]
                                 const float *__restrict__ dFdc, const long long *__restrict__ prev_pair,
                                 const int *__restrict__ prev_center) {
    const int w = blockIdx.x;
    const int sw = prev_s[w];
    const float *dfd = dFdc ? dFdc + (size_t)prev_pair[w] * 2 * C : nullptr;
    const int cw = dFdc ? prev_center[w] : -1;
    auto diag_terms = [&](int p, int q, int q4) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (dfd) {
            if (p == q) {
                const float4 v = reinterpret_cast<const float4 *>(dfd + (size_t)p * 2 * C)[q4];
                t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
            }
            if (q == cw) {
                const float4 v = reinterpret_cast<const float4 *>(dfd + (size_t)p * 2 * C + C)[q4];
                t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
            }
        }
        return t;
    };
    float *dst = dfprev + prev_row[w] * C;
    const long long c0 = cons_ptr[w], c1 = cons_ptr[w + 1];
    if ((C & 3) == 0 && sw <= kPromoteMaxS) {
        // consumer tables of this source node in LDS (chunks of kPromoteChunk consumers), then four consumers' loads in
        // flight per item: clamped address + 0/1 weight instead of a branch around every load.  Same summation order.
        __shared__ long long sSlab[kPromoteChunk];
        __shared__ int sS[kPromoteChunk];
        __shared__ short sInv[kPromoteChunk][kPromoteMaxS];
        const int Q = C >> 2, total4 = sw * sw * Q;
        const int npass = (total4 + (int)blockDim.x - 1) / (int)blockDim.x;
        for (long long cb = c0; cb < c1 || cb == c0; cb += kPromoteChunk) {
            const int nc = (int)((c1 - cb < kPromoteChunk) ? c1 - cb : kPromoteChunk);
            __syncthreads();
            for (int i = threadIdx.x; i < nc; i += blockDim.x) {
                sSlab[i] = cons_slab[cb + i];
                sS[i] = cons_s[cb + i];
            }
            for (int i = threadIdx.x; i < nc * sw; i += blockDim.x) sInv[i / sw][i % sw] = inv[cons_inv_off[cb + i / sw] + i % sw];
            __syncthreads();
            for (int pass = 0; pass < npass; ++pass) {
                const int i = pass * (int)blockDim.x + threadIdx.x;
                if (i >= total4) break;
                const int q4 = i % Q, pq = i / Q;
                const int p = pq / sw, q = pq - p * sw;
                float4 acc = (cb == c0) ? diag_terms(p, q, q4) : reinterpret_cast<float4 *>(dst)[i];
                for (int e0 = 0; e0 < nc; e0 += 4) {
                    float4 v[4];
                    float m[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int e = (e0 + j < nc) ? e0 + j : e0;
                        const int ib = sInv[e][p], ic = sInv[e][q];
                        const bool ok = e0 + j < nc && ib >= 0 && ic >= 0;
                        const long long pos = sSlab[e] + (ok ? (long long)ib * sS[e] + ic : 0);
                        v[j] = reinterpret_cast<const float4 *>(dP + pos * C)[q4];
                        m[j] = ok ? 1.f : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (m[j] != 0.f) {  // (select, not a multiply: a structurally-zero position holds stale data)
                            acc.x += v[j].x;
                            acc.y += v[j].y;
                            acc.z += v[j].z;
                            acc.w += v[j].w;
                        }
                    }
                }
                reinterpret_cast<float4 *>(dst)[i] = acc;
            }
            if (c1 == c0) break;
        }
        return;
    }
    if ((C & 3) == 0) {  // larger receptive fields than the LDS tables hold
        const int Q = C >> 2, total4 = sw * sw * Q;
        for (int i = threadIdx.x; i < total4; i += blockDim.x) {
            const int q4 = i % Q, pq = i / Q;
            const int p = pq / sw, q = pq - p * sw;
            float4 acc = diag_terms(p, q, q4);
            for (long long e = c0; e < c1; ++e) {
                const short *iv = inv + cons_inv_off[e];
                const int ib = iv[p], ic = iv[q];
                if (ib >= 0 && ic >= 0) {
                    const float4 v = reinterpret_cast<const float4 *>(dP + (cons_slab[e] + (long long)ib * cons_s[e] + ic) * C)[q4];
                    acc.x += v.x;
                    acc.y += v.y;
                    acc.z += v.z;
                    acc.w += v.w;
                }
            }
            reinterpret_cast<float4 *>(dst)[i] = acc;
        }
        return;
    }
    const int total = sw * sw * C;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int f = i % C, pq = i / C;
        const int p = pq / sw, q = pq - p * sw;
        float acc = 0.f;
        for (long long e = c0; e < c1; ++e) {
            const short *iv = inv + cons_inv_off[e];
            const int ib = iv[p], ic = iv[q];
            if (ib >= 0 && ic >= 0) acc += dP[(cons_slab[e] + (long long)ib * cons_s[e] + ic) * C + f];
        }
        dst[i] = acc;
    }
}

// ---- bias + LeakyReLU ---------------------------------------------------------------------------------------------
// (alpha: 0.01 everywhere but level 0 of SMP_1D_ver2 / ver3, whose LeakyReLU2D has slope 0 -- gfsmp::Config::level_slope)
__global__ void bias_lrelu_forward(float *__restrict__ Y, const float *__restrict__ b, int C, size_t total, float alpha) {
    GRID_STRIDE(i, total) {
        const float z = Y[i] + (b ? b[i % C] : 0.f);
        Y[i] = z > 0.f ? z : alpha * z;
    }
}

// dZ = dF * lrelu'(z), decided from the sign of the stored activation (LeakyReLU is monotone: f > 0 <=> z > 0);
// also leaves per-block partial column sums of dZ for the bias gradient (VectorAddTensor.h:61-72)
__global__ void lrelu_backward_colsum(const float *__restrict__ F, float *__restrict__ dF, float *__restrict__ part, int C,
                                      long long rows, int rows_per_block, float alpha) {
    __shared__ float red[256];
    const long long r0 = (long long)blockIdx.x * rows_per_block;
    const long long r1 = (r0 + rows_per_block < rows) ? r0 + rows_per_block : rows;
    const int lanes = (C < 256) ? C : 256;          // channel lanes per row
    const int rl = 256 / lanes;                     // rows handled concurrently
    const int f0 = threadIdx.x % lanes, rr = threadIdx.x / lanes;
    for (int fb = 0; fb < C; fb += lanes) {
        const int f = fb + f0;
        float s = 0.f;
        if (f < C && rr < rl)
            for (long long r = r0 + rr; r < r1; r += rl) {
                const size_t i = (size_t)r * C + f;
                const float d = dF[i] * (F[i] > 0.f ? 1.f : alpha);
                dF[i] = d;
                s += d;
            }
        red[threadIdx.x] = s;
        __syncthreads();
        if (rr == 0 && f < C) {
            float t = 0.f;
            for (int k = 0; k < rl; ++k) t += red[k * lanes + f0];
            part[(size_t)blockIdx.x * C + f] = t;
        }
        __syncthreads();
    }
}

// out[f] += sum_b part[b][f]; one workgroup, row lanes in parallel then a fixed-order fold
__global__ void colsum_finish(const float *__restrict__ part, float *__restrict__ out, int C, int nblocks) {
    __shared__ float red[256];
    const int lanes = (C < 256) ? C : 256, rl = 256 / lanes;
    const int f0 = threadIdx.x % lanes, rr = threadIdx.x / lanes;
    for (int fb = 0; fb < C; fb += lanes) {
        const int f = fb + f0;
        float s = 0.f;
        if (f < C && rr < rl)
            for (int b = rr; b < nblocks; b += rl) s += part[(size_t)b * C + f];
        red[threadIdx.x] = s;
        __syncthreads();
        if (rr == 0 && f < C) {
            float t = 0.f;
            for (int k = 0; k < rl; ++k) t += red[k * lanes + f0];
            out[f] += t;
        }
        __syncthreads();
    }
}

// ---- readout ----------------------------------------------------------------------------------------------------------
// sh[n][:] = sum_{ij} f_L[n][i][j][:]  (ShrinkTensor.h:37-50), vf = LeakyReLU(sh)
__global__ void readout_nodes(const float *__restrict__ fL, const int *__restrict__ node_s,
                              const long long *__restrict__ node_row, float *__restrict__ sh, float *__restrict__ vf,
                              int C, size_t total) {
    GRID_STRIDE(i, total) {
        const int f = i % C;
        const size_t n = i / C;
        const int s = node_s[n];
        const float *src = fL + node_row[n] * C + f;
        float acc = 0.f;
        for (int r = 0; r < s * s; ++r) acc += src[(size_t)r * C];
        sh[i] = acc;
        vf[i] = lrelu(acc);
    }
}

// C % 4 == 0 and C <= 1024: workgroup per node, 256 threads = (256 / (C/4)) row groups x C/4 float4 lanes; every group
// sums rows g, g+ng, ... with batched loads, the groups are folded through LDS in a fixed order (deterministic).
__global__ __launch_bounds__(256) void readout_nodes_v(const float *__restrict__ fL, const int *__restrict__ node_s,
                                                       const long long *__restrict__ node_row, float *__restrict__ sh,
                                                       float *__restrict__ vf, int C) {
    __shared__ __attribute__((aligned(16))) float red[1024];
    const int n = blockIdx.x, nl = C / 4, ng = 256 / nl;
    const int g = threadIdx.x / nl, fl = threadIdx.x % nl;
    const int rows = node_s[n] * node_s[n];
    if (g < ng) {
        const int cnt = (rows - g + ng - 1) / ng;
        const f4 acc = batched_sum(fL + ((size_t)node_row[n] + g) * C + 4 * fl, (size_t)ng * C, 0, cnt > 0 ? cnt : 0,
                                   [](int) { return 1.f; });
        st4(red + g * C + 4 * fl, acc);
    }
    __syncthreads();
    if (g == 0) {
        f4 t = ld4(red + 4 * fl);
        for (int k = 1; k < ng; ++k) t += ld4(red + k * C + 4 * fl);
        f4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = lrelu(t[j]);
        st4(sh + (size_t)n * C + 4 * fl, t);
        st4(vf + (size_t)n * C + 4 * fl, v);
    }
}

// the same sums from the row-panel partials the top level's combine-forward left behind (C = 64): thread per (node, channel),
// the node's panels in order
template <int CB>   // channels: 64 or 32
__global__ __launch_bounds__(256) void readout_nodes_panels(const float *__restrict__ psum, const int *__restrict__ node_panel, int nodes,
                                                            int npanels, float *__restrict__ sh, float *__restrict__ vf) {
    const int n = blockIdx.x * (256 / CB) + threadIdx.x / CB, c = threadIdx.x % CB;
    if (n >= nodes) return;
    const int p0 = node_panel[n], p1 = (n + 1 < nodes) ? node_panel[n + 1] : npanels;
    float t = 0.f;
    for (int p = p0; p < p1; ++p) t += psum[(size_t)p * CB + c];
    sh[(size_t)n * CB + c] = t;
    vf[(size_t)n * CB + c] = lrelu(t);
}

// one workgroup per molecule: g = sum_v vf (SumVectors), y = <g, W> (InnerProduct.h:39-46), loss (SquaredLoss.h:45-53)
// g_out / y_out (or null): the caller's graph_feature / predict, written here beside the handle's own g / yhat (which the reverse sweep
// reads) -- no copy kernels behind the read-out
__global__ void readout_molecules(const float *__restrict__ vf, const int *__restrict__ mol_ptr,
                                  const int *__restrict__ mol_nodes, const float *__restrict__ W,
                                  const float *__restrict__ target, float *__restrict__ g, float *__restrict__ yhat,
                                  float *__restrict__ loss, float *__restrict__ dy, int C, float *__restrict__ g_out,
                                  float *__restrict__ y_out) {
    __shared__ float red[256];
    const int m = blockIdx.x;
    float part = 0.f;
    for (int f = threadIdx.x; f < C; f += blockDim.x) {
        float acc = 0.f;
        for (int k = mol_ptr[m]; k < mol_ptr[m + 1]; ++k) acc += vf[(size_t)mol_nodes[k] * C + f];
        g[(size_t)m * C + f] = acc;
        if (g_out) g_out[(size_t)m * C + f] = acc;
        part += acc * W[f];
    }
    red[threadIdx.x] = part;
    __syncthreads();
    for (int st = blockDim.x / 2; st > 0; st >>= 1) {
        if (threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float y = red[0], t = target ? target[m] : 0.f;
        yhat[m] = y;
        if (y_out) y_out[m] = y;
        if (loss) loss[m] = 0.5f * (y - t) * (y - t);
        dy[m] = y - t;  // SquaredLoss::backward: predict->gradient += predict - target
    }
}

// dW[f] += sum_m dy[m] g[m][f]   (InnerProduct.h:48-53, second operand)
// One workgroup (C outputs): a thread's run of molecules m = rr, rr + rl, .. is REQUESTED sixteen at a time and summed in the run's
// order -- the same sums as a plain loop, which waited for one molecule's two loads per step (64 dependent round trips at 1,024
// molecules and C = 64).
__global__ __launch_bounds__(1024) void readout_dW(const float *__restrict__ dy, const float *__restrict__ g, float *__restrict__ dW,
                                                   int C, int nMol) {
    __shared__ float red[1024];
    constexpr int kAhead = 16;
    const int nt = (int)blockDim.x;
    const int lanes = (C < nt) ? C : nt, rl = nt / lanes;
    const int f0 = threadIdx.x % lanes, rr = threadIdx.x / lanes;
    for (int fb = 0; fb < C; fb += lanes) {
        const int f = fb + f0;
        float acc = 0.f;
        if (f < C && rr < rl)
            for (int m0 = rr; m0 < nMol; m0 += kAhead * rl) {
                float d[kAhead], v[kAhead];
#pragma unroll
                for (int k = 0; k < kAhead; ++k) {
                    const int m = m0 + k * rl;
                    const bool in = m < nMol;
                    d[k] = in ? dy[m] : 0.f;
                    v[k] = in ? g[(size_t)m * C + f] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < kAhead; ++k)
                    if (m0 + k * rl < nMol) acc += d[k] * v[k];
            }
        red[threadIdx.x] = acc;
        __syncthreads();
        if (rr == 0 && f < C) {
            float t = 0.f;
            for (int k = 0; k < rl; ++k) t += red[k * lanes + f0];
            dW[f] += t;
        }
        __syncthreads();
    }
}

// df_L[n][i][j][:] = dy[mol(n)] * W[:] * lrelu'(sh[n][:])   (InnerProduct first operand -> SumVectors -> LeakyReLU
// -> ShrinkTensor::backward broadcast, ShrinkTensor.h:52-61)
__global__ void readout_backward_nodes(const float *__restrict__ dy, const float *__restrict__ W, const float *__restrict__ sh,
                                       const int *__restrict__ node_mol, const int *__restrict__ node_s,
                                       const long long *__restrict__ node_row, float *__restrict__ dfL, int C) {
    const int n = blockIdx.x;
    const int s = node_s[n];
    float *dst = dfL + node_row[n] * C;
    const float d = dy[node_mol[n]];
    const int total = s * s * C;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int f = i % C;
        dst[i] = d * W[f] * (sh[(size_t)n * C + f] > 0.f ? 1.f : kAlpha);
    }
}

// the same per node only: dsh[n][:] = dy[mol(n)] * W[:] * lrelu'(sh[n][:]) -- the fused top level reads this vector instead
// of a broadcast copy of it at every (i,j)
__global__ void readout_backward_nodevec(const float *__restrict__ dy, const float *__restrict__ W, const float *__restrict__ sh,
                                         const int *__restrict__ node_mol, float *__restrict__ dsh, int C, size_t total) {
    GRID_STRIDE(i, total) {
        const int f = i % C;
        const size_t n = i / C;
        dsh[i] = dy[node_mol[n]] * W[f] * (sh[i] > 0.f ? 1.f : kAlpha);
    }
}

__global__ void zero_f32(float *p, size_t n) { GRID_STRIDE(i, n) p[i] = 0.f; }

// RisiContraction_18_dropout over the nodes of a level: slice k of node n is multiplied by scale if bit k of keep[n] is set,
// else zeroed (RisiContraction_18_dropout.h:106-132 forward, :479-510 backward: dropped slices neither produce nor receive)
// (round 4: a dropped slice is a store of zeros, a kept one at scale 1 -- train mode -- is not touched at all, and the channels move as
//  float4 where C % 4 == 0: the kernel read and wrote all of Q element by element, 5.9 of the 34 ms of an SMP_sigma_pairgraphs step)
template <int VW>
__global__ void node_slice_scale(float *__restrict__ Q, const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                 const unsigned *__restrict__ keep, float scale, int C) {
    const int n = blockIdx.x;
    const unsigned m = keep[n];
    const int cv = C / VW;
    const size_t cnt = (size_t)node_s[n] * node_s[n] * 18 * cv;
    float *q = Q + (size_t)node_row[n] * 18 * C;
    for (size_t i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int k = (int)((i / cv) % 18);
        const bool kept = (m >> k) & 1u;
        if (kept && scale == 1.f) continue;
        if constexpr (VW == 4) {
            float4 *p4 = reinterpret_cast<float4 *>(q) + i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kept) {
                v = *p4;
                v.x *= scale, v.y *= scale, v.z *= scale, v.w *= scale;
            }
            *p4 = v;
        } else {
            q[i] = kept ? q[i] * scale : 0.f;
        }
    }
}
static gf_status launch_node_slice_scale(gf_ctx *ctx, float *Q, const int *node_s, const long long *node_row, const unsigned *keep, float scale, int C,
                                         int nNodes) {
    LaunchTimer lt__(ctx, "smp_slice_dropout");
    if (C % 4 == 0 && (((uintptr_t)Q) & 15) == 0)
        hipLaunchKernelGGL(node_slice_scale<4>, dim3(nNodes), dim3(256), 0, ctx->stream, Q, node_s, node_row, keep, scale, C);
    else
        hipLaunchKernelGGL(node_slice_scale<1>, dim3(nNodes), dim3(256), 0, ctx->stream, Q, node_s, node_row, keep, scale, C);
    lt__.done();
    GF_LAUNCH_CHECK(ctx, "smp_slice_dropout");
    return GF_OK;
}

// physics towers: level_feature[l] = sum over the molecule's vertices of LeakyReLU(sum_ij f_l[v]) (SMP_omega_physics.h:572-588),
// written into columns [off, off + C) of the molecule's feature row (ConcatVectors, :590)
__global__ void level_feature_sum(const float *__restrict__ vf, const int *__restrict__ mol_ptr, const int *__restrict__ node_of_vertex,
                                  float *__restrict__ feat, int C, int width, int off) {
    const int m = blockIdx.x;
    for (int f = threadIdx.x; f < C; f += blockDim.x) {
        float acc = 0.f;
        for (int k = mol_ptr[m]; k < mol_ptr[m + 1]; ++k) acc += vf[(size_t)node_of_vertex[k] * C + f];
        feat[(size_t)m * width + off + f] = acc;
    }
}

// the same gradient as ONE vector per node (a fused level's combine-backward adds it to every row of the node itself)
__global__ void level_feature_nodevec(const float *__restrict__ dfeat, const float *__restrict__ sh, const int *__restrict__ node_mol,
                                      float *__restrict__ out, int C, int width, int off, size_t total) {
    GRID_STRIDE(i, total) {
        const int c = (int)(i % C);
        const size_t n = i / C;
        out[i] = dfeat[(size_t)node_mol[n] * width + off + c] * (sh[i] > 0.f ? 1.f : kAlpha);
    }
}

// reverse: df_l[n][i][j][:] (+)= dfeat[mol(n)][off + :] * lrelu'(sh_l[n][:])   (SumVectors -> LeakyReLU -> ShrinkTensor::backward)
__global__ void level_feature_backward(const float *__restrict__ dfeat, const float *__restrict__ sh, const int *__restrict__ node_mol,
                                       const int *__restrict__ node_s, const long long *__restrict__ node_row, float *__restrict__ df,
                                       int C, int width, int off, int accumulate) {
    const int n = blockIdx.x;
    const int s = node_s[n];
    float *dst = df + node_row[n] * C;
    const float *g = dfeat + (size_t)node_mol[n] * width + off;
    const int total = s * s * C;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int f = i % C;
        const float v = g[f] * (sh[(size_t)n * C + f] > 0.f ? 1.f : kAlpha);
        dst[i] = accumulate ? dst[i] + v : v;
    }
}

// RisiContraction_18 over every node of level l.  Nodes are sorted by receptive-field size, so consecutive buckets are
// merged into at most four launches (size classes s <= PPW, 2 PPW, 4 PPW, 8 PPW of the slab kernels) through the ragged
// entry points; anything larger falls back to one uniform launch per bucket.
gf_status smp_contract(gf_smp *s, int l, bool backward) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const gf_smp::DevLevel &d = s->lv[l];
    const int C = s->cfg.level_channels(l - 1), nK = s->cfg.nContractions;  // the contraction runs on the level below's channels
    const int ppw = (C <= 16) ? 16 : (C <= 32) ? 8 : 4;
    const gf_ragged_nodes t = {d.pair_node, d.node_s, d.node_p, d.node_row, d.node_pair, (long long)h.rows, (long long)h.pairs};
    gf_status st = ensure_P(s);
    if (st != GF_OK) return st;
    // (_10 / _50 of the SMP_2D_ver6 / ver7 wirings: one uniform launch per size bucket)
    const bool ragged_ok = nK == 18 && r18_ragged_supported(ppw, C, s->P, d.Q);
    size_t k = 0;
    for (int cls = 1; cls <= 8 && ragged_ok && k < h.buckets.size(); cls *= 2) {
        const int smax_cls = cls * ppw;
        const size_t k0 = k;
        int smax = 0;
        while (k < h.buckets.size() && h.buckets[k].s <= smax_cls) smax = h.buckets[k++].s;
        if (k == k0) continue;
        const long long lo = h.node_pair[h.buckets[k0].first_node];
        const long long hi = (k < h.buckets.size()) ? h.node_pair[h.buckets[k].first_node] : (long long)h.pairs;
        st = backward ? r18_backward_ragged(ctx, d.Q, d.adj, s->P, t, lo, hi, smax, C, 0)
                      : r18_forward_ragged(ctx, s->P, d.adj, d.Q, t, lo, hi, smax, C);
        if (st != GF_OK) return st;
    }
    for (; k < h.buckets.size(); ++k) {  // sizes beyond the slab kernels (or unaligned C): uniform launches
        const gfsmp::Bucket &bk = h.buckets[k];
        float *Pb = s->P + bk.first_p * C, *Qb = d.Q + bk.first_row * (long long)(nK * C);
        st = backward ? gf_contract_backward_f32(ctx, nK, Qb, d.adj + bk.first_row, Pb, bk.s, C, bk.count, 0)
                      : gf_contract_forward_f32(ctx, nK, Pb, d.adj + bk.first_row, Qb, bk.s, C, bk.count);
        if (st != GF_OK) return st;
    }
    return GF_OK;
}

}  // namespace

LevelKind smp_level_kind(const gf_smp *s, int l) {
    if (s->cfg.neighbourhood) return LevelKind::Neighbourhood;
    if (s->cfg.unrestricted) return LevelKind::Unrestricted;
    if (s->cfg.first_order) return LevelKind::Theta;   // (one plan: gf_smp_set_fused has no effect)
    if (s->cfg.steerable_2d) return LevelKind::Steerable2D;
    if (s->fused && smp_fused_supported(s, l)) return LevelKind::Fused18;
    return smp_gamma_fused(s, l) ? LevelKind::Gamma : LevelKind::OpByOp;
}

// Data-parallel reverse sweep.  The flat gradient buffer is H | K_1 b_1 | ... | K_L b_L | W; the segment of level l is
// [K_l | b_l] (plus W for l = L: the readout gradient is the first thing the sweep computes) and H for l = 0.  The segment is
// final on the context's current stream when this is called: the communicator's stream waits for that point and runs the
// all-reduce there, while the sweep continues with the table gradients and the levels below.
gf_status smp_dp_level_done(gf_smp *s, int l) {
    if (!s->dp_grads) return GF_OK;
    gf_ctx *ctx = s->ctx;
    const gfsmp::Config &c = s->cfg;
    const size_t C = (size_t)c.nChanels, nH = C * c.fdim(), per = (size_t)c.nContractions * C * C + C;
    float *seg = s->dp_grads;
    size_t n = nH;
    if (l >= 1) {
        seg += nH + (size_t)(l - 1) * per;
        n = per + (l == c.nLevels ? (size_t)c.readout_rows() * C : 0);
    }
    hipStream_t comm = dist_stream(ctx);
    GF_HIP_TRY(ctx, hipEventRecord(s->ev_grad, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamWaitEvent(comm, s->ev_grad, 0));
    char what[64];
    if (l >= 1) std::snprintf(what, sizeof what, "gf_smp_backward: gradient segment [K_%d | b_%d%s]", l, l, l == c.nLevels ? " | W" : "");
    else std::snprintf(what, sizeof what, "gf_smp_backward: gradient segment [H]");
    gf_status st = dist_allreduce_on(ctx, seg, n, comm, what);
    if (st == GF_OK && l == 0 && s->n_extra)   // (SMP_2D_ver7 on the 18-slice level: the extra products' blocks sit behind W; every level has written its own by now)
        st = dist_allreduce_on(ctx, s->dp_grads + param_count(c), (size_t)c.nLevels * s->n_extra * C * C, comm, "gf_smp_backward: gradient segment [X_1 .. X_L]");
    return st;
}

// Slice dropout in TEST mode: the fused level cannot run the reference's unscaled test-mode sweep (smp_fused_backward_level).  Refused
// BEFORE a gradient is written or a collective handed to RCCL -- not in the middle of the level loop, where the readout's gradients
// were already there and the peers of a data-parallel run were left waiting for segments that never came (round-5 advice).  The
// composite model asks before its head's backward as well (gf_smp_model_backward).
gf_status smp_backward_admissible(const gf_smp *s) {
    if (s->drop_on && s->drop_scale != 1.f && s->prepared)
        for (int l = 1; l <= s->cfg.nLevels; ++l)
            if (smp_level_kind(s, l) == LevelKind::Fused18)
                return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_backward: fused level %d under slice dropout in test mode (scale %.4f): set GF_SMP_FUSED_DROPOUT=0 "
                                                        "for the reference's unscaled test-mode sweep", l, (double)s->drop_scale);
    return GF_OK;
}
}  // namespace gf

using gf::fail;

// What the device computes with (gf_smp::cfg, dup_channels, n_extra), derived from the caller's configuration (gf_smp::ucfg).
// allow_embed = false: the `_10` / `_50` families on their own op-by-op levels whatever the environment says -- gf_smp_prepare switches a
// handle to that plan for a batch the embedding in the 18-slice level cannot take (an asymmetric adjacency, Coulomb entries <= 0, a `_50`
// Coulomb batch) and back for the next batch it can (round-5 advice: the refusal used to surface mid-epoch, with an environment variable
// read at create time as the only way out).  The caller's parameter layout does not depend on the plan.
void gf::smp_derive_plan(gf_smp *s, bool allow_embed) {
    // Round 4: the channel count the DEVICE computes with.  The dedicated kernels of the fused level exist at 32 and 64 channels, the
    // generic fused level needs C % 4 == 0, and anything else ran the op-by-op level on the one-thread-per-element contraction kernels
    // (the reference's own tests use nChanels = 10: 35.8 ms per 1024-molecule step, against 8.0 ms at 12 channels and 4.1 ms at 32).
    // A model is therefore computed with its channels PADDED to 32 / 64 (above 64: to a multiple of 4): padded weights, biases and
    // features are zero, LeakyReLU(0) = 0 keeps them zero through every level, so the real channels see exactly the sums they saw
    // before (plus zero terms).  ucfg keeps the caller's layout: parameters, gradients, features and activations cross the C ABI in
    // it and are padded / cropped at the boundary (gf_smp_forward / gf_smp_backward).  GF_SMP_PAD_CHANNELS=0: compute at nChanels.
    const bool pad_channels = s->req_pad_channels;
    const int min_pad = s->req_min_pad;
    s->cfg = s->ucfg;
    s->dup_channels = 0;
    s->n_extra = 0;
    if (s->cfg.per_size()) return;   // (the first-order and the steerable levels take any channel count: computed at the caller's)
    {
        const bool no_pad = gf::env_is("GF_SMP_PAD_CHANNELS", '0');
        const int C = s->cfg.nChanels;
        int Cc = C;
        if ((pad_channels || gf::env_is("GF_SMP_PAD_CHANNELS", '2')) && !no_pad && s->cfg.nContractions == 18 && s->cfg.nLevels < gf::kPadMaxLevels) {   // (2: tests)
            // (round 5: a 16-channel build of the row-panel family -- the reference's own models have nChanels = 10; min_pad = 32 keeps a
            //  tower that will run under slice dropout on the 32-channel kernels, the only ones with per-product row factors)
            if (C <= 16 && min_pad <= 16) Cc = 16;
            else if (C <= 32) Cc = 32;
            else if (C <= 64) Cc = 64;
            else Cc = (C + 3) & ~3;
            // a physics tower (channels halve per level, SMP_omega_physics.h:141-151) is computed at ONE width: K_l [18 C_{l-1}][C_l]
            // sits in the corner of a square [18 Cc][Cc] block, the level features are cropped level by level
            if (s->cfg.physics) s->cfg.uniform = 1;
        }
        // SMP_2D_ver6 (RisiContraction_10) embedded in the 18-slice fused level (see gf_smp::dup_channels): 2 C channels padded to 16 / 32 / 64.
        // GF_SMP_VER6_FUSED=0: the `_10` contraction op by op.  gf_smp_prepare switches to that plan by itself for a batch with an asymmetric adjacency.
        // (only where every field fits the fused level -- max_receptive_field <= 64 (32 until round 6): on an op-by-op level the 18-slice model at 2 C padded
        //  channels moves more than the `_10` / `_50` contraction at C)
        auto embed = [&](const char *name) {   // (kFusedMaxField: 64 since round 6, fields of 33 .. 64 positions stay fused)
            return allow_embed && !gf::env_is(name, '0') && s->cfg.max_receptive_field <= gf::kFusedMaxField;
        };
        if (pad_channels && !no_pad && s->cfg.nContractions == 10 && 2 * C <= 64 && s->cfg.nLevels < gf::kPadMaxLevels && !s->cfg.physics &&
            embed("GF_SMP_VER6_FUSED")) {
            s->dup_channels = C;
            s->cfg.nContractions = 18;
            s->cfg.custom_matmul = 0;   // (the device's own copy of the weights is in the [18 Cc][Cc] layout whatever the caller's is)
            Cc = 2 * C <= 16 ? 16 : 2 * C <= 32 ? 32 : 64;
        }
        // SMP_2D_ver7 (RisiContraction_50) the same way, with three extra products per level (gf_smp::n_extra).  GF_SMP_VER7_FUSED=0: op by op.
        if (pad_channels && !no_pad && s->cfg.nContractions == 50 && 2 * C <= 64 && s->cfg.nLevels < gf::kPadMaxLevels && !s->cfg.physics &&
            embed("GF_SMP_VER7_FUSED")) {
            s->dup_channels = C;
            s->n_extra = 3;
            s->cfg.nContractions = 18;
            s->cfg.custom_matmul = 0;
            Cc = 2 * C <= 16 ? 16 : 2 * C <= 32 ? 32 : 64;
        }
        // the `_10` / `_50` wirings (SMP_2D_ver6 / ver7: op-by-op levels): a channel count that is not a multiple of 4 runs the contraction
        // kernels at one channel per lane; padded to the next multiple (10 -> 12) they take the float4 / one-stream-per-graph kernels
        if (pad_channels && !no_pad && s->cfg.nContractions != 18 && !s->dup_channels && s->cfg.nLevels < gf::kPadMaxLevels && !s->cfg.physics)
            Cc = (C + 3) & ~3;
        s->cfg.nChanels = Cc;
    }
}

// pad_channels = false: compute at the configuration's own channel counts (the towers of a model with RisiContraction_18_dropout --
// SMP_sigma_pairgraphs -- whose levels run op by op, where a padded width only costs)
gf_status gf::smp_create(gf_ctx *ctx, const gf_smp_config *cfg, const gfsmp::ConfigEntry &entry, bool pad_channels, gf_smp **out, int min_pad) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    gfsmp::Config c;
    char why[640];
    const gf_status verdict = gfsmp::resolve_config(out ? cfg : nullptr, entry, &c, why, sizeof why);   // (a null `out` is a null argument)
    if (verdict != GF_OK) return fail(ctx, verdict, "%s", why);
    gfsmp::table_alloc = gf::pinned_table_alloc;   // (before the first table is built; idempotent)
    gfsmp::table_free = gf::pinned_table_free;
    gf_smp *s = new gf_smp();
    s->ctx = ctx;
    s->ucfg = c;
    if (c.per_size() || c.neighbourhood || c.matrix_form || c.covariant) s->grad_allreduce = 0;   // (no data-parallel exchange: gf_smp_set_grad_allreduce(.., 1) is refused)
    s->req_pad_channels = pad_channels;
    s->req_min_pad = min_pad;
    if (c.neighbourhood || c.matrix_form || c.covariant) {   // (no padding, one plan, none of the fused level's switches)
        s->cfg = c;
    } else {
        gf::smp_derive_plan(s, /*allow_embed=*/true);
        s->bwd_gather = gf::env_is("GF_SMP_BWD_GATHER", '0') ? 0 : 1;   // 0: keep the two-kernel tables-backward + consumer gather
    }
    *out = s;
    return GF_OK;
}

// Moves a handle between its two plans (see smp_derive_plan).  Everything sized by the device-side configuration goes: the batch's
// buffers (release), the padded parameter / gradient / feature copies.  What is in the caller's layout stays: the handle-owned model,
// the optimiser's moments, the pool of device blocks.
gf_status gf::smp_switch_plan(gf_smp *s, bool embed) {
    gf_ctx *ctx = s->ctx;
    if (s->ev_last && s->used) GF_HIP_TRY(ctx, hipEventSynchronize(s->ev_last));   // (the handle's last launch: its padded buffers are about to go)
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    gf::release(s);
    if (s->pad_p) (void)hipFree(s->pad_p);
    if (s->pad_g) (void)hipFree(s->pad_g);
    if (s->pad_feat) (void)hipFree(s->pad_feat);
    s->pad_p = s->pad_g = s->pad_feat = nullptr;
    s->pad_feat_n = 0;
    s->extra_w = nullptr;
    s->extra_g = nullptr;
    gf::smp_derive_plan(s, embed);
    s->embed_auto_off = !embed;
    return GF_OK;
}

extern "C" {

gf_status gf_smp_create(gf_ctx *ctx, const gf_smp_config *cfg, gf_smp **out) {
    return gf::smp_create(ctx, cfg, gfsmp::kHandleEntry, /*pad_channels=*/true, out);
}

gf_status gf_smp_destroy(gf_smp *s) {
    if (!s) return GF_OK;
    gf::release(s);
    gf::release_pool(s);
    if (s->upload) (void)hipStreamDestroy(s->upload);
    for (hipEvent_t e : {s->ev_last, s->ev_grad, s->ev_comm})
        if (e) (void)hipEventDestroy(e);
    if (s->ev_mask) {
        (void)hipEventSynchronize(s->ev_mask);
        (void)hipEventDestroy(s->ev_mask);
    }
    if (s->mask_stage) (void)hipHostFree(s->mask_stage);
    for (float *p : {s->rs_inv, s->adam_m, s->adam_v, s->own_p, s->own_g, s->pad_p, s->pad_g, s->pad_feat, s->fit_cache})
        if (p) (void)hipFree(p);
    if (s->fit_sum) (void)hipFree(s->fit_sum);
    gf::optim_free(&s->optim);
    delete s;
    return GF_OK;
}

size_t gf_smp_param_count(const gf_smp *s) { return s ? gf::param_count(s->ucfg) : 0; }

// The `_classification` models (smp_readout_classes.hip): the levels of gf_smp_create, W [nClass][C] read out by MatVecMul + LogLoss
gf_status gf_smp_create_classifier(gf_ctx *ctx, const gf_smp_config *cfg, int nClass, gf_smp **out) {
    return gf::smp_create(ctx, cfg, {gfsmp::ConfigEntry::Classifier, nClass, 0.0}, /*pad_channels=*/true, out);
}

int gf_smp_classes(const gf_smp *s) { return s ? s->ucfg.nClass : 0; }

// scores = predict->value (MatVecMul), probability = LogLoss::probability of the last forward; device pointers, either may be NULL
gf_status gf_smp_class_scores(gf_smp *s, float *scores, float *probability) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!s->ucfg.nClass) return fail(ctx, GF_ERR_INVALID, "gf_smp_class_scores: not a classifier handle (gf_smp_create_classifier)");
    if (!s->forwarded) return fail(ctx, GF_ERR_INVALID, "gf_smp_class_scores before gf_smp_forward");
    const size_t bytes = sizeof(float) * (size_t)s->lay.nMol * s->ucfg.nClass;
    if (scores) GF_HIP_TRY(ctx, hipMemcpyAsync(scores, s->cls_scores, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    if (probability) GF_HIP_TRY(ctx, hipMemcpyAsync(probability, s->cls_prob, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return GF_OK;
}

}  // extern "C"

// ---- the two sweeps -----------------------------------------------------------------------------------------------------------
namespace gf {
namespace {

bool padded_channels(const gf_smp *s) { return s->cfg.nChanels != s->ucfg.nChanels || s->cfg.uniform != s->ucfg.uniform; }

// What gf_smp_forward refuses, padded model or not, before anything is launched.  *params == null: the handle's own model.
gf_status forward_check(gf_smp *s, const float **params, const float *targets, const float *predict, const float *loss, const float *graph_feature) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!s->prepared) return fail(ctx, GF_ERR_INVALID, "gf_smp_forward before gf_smp_prepare");
    if (!*params) {  // the handle's own model (gf_smp_parameters_upload)
        if (!s->own_p) return fail(ctx, GF_ERR_INVALID, "gf_smp_forward: null params and no handle-owned model");
        *params = s->own_p;
    }
    if (s->cfg.physics && (targets || predict || loss))
        return fail(ctx, GF_ERR_INVALID, "gf_smp_forward: a physics tower only produces graph_feature (the head owns targets, predict and loss)");
    if (s->cfg.readout == 2 && (targets || predict || graph_feature))
        return fail(ctx, GF_ERR_INVALID, "gf_smp_forward: a Gram handle (readout = 2) has no targets, predict or graph_feature: its target is the batch's "
                                         "adjacency, its prediction comes through gf_smp_gram");
    return GF_OK;
}

// promotion, contraction, K-projection, bias + LeakyReLU as separate kernels
gf_status forward_level_opbyop(gf_smp *s, int l, const float *Kl, const float *bl) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const gf_smp::DevLevel &d = s->lv[l];
    s->lv[l].t_zeros = s->lv[l].t_filled = false;  // (the op-by-op level uses all of Q: the zeros kept in the fused level's T region are gone)
    gf_status st = ensure_P(s);
    if (st != GF_OK) return st;
    const int Cp = s->cfg.level_channels(l - 1), Cc = s->cfg.level_channels(l);  // (equal unless a physics tower)
    GF_LAUNCH(ctx, "smp_promote_fwd", promote_forward, dim3((unsigned)h.pairs), dim3(256), 0, s->lv[l - 1].f, s->P,
              d.node_s, d.node_row, d.node_p, d.node_pair, d.pair_node, d.pair_src_row, d.pair_src_s, d.pi, Cp);
    st = smp_contract(s, l, /*backward=*/false);
    if (st == GF_OK && s->drop_on) st = launch_node_slice_scale(ctx, d.Q, d.node_s, d.node_row, d.keep_mask, s->drop_scale, Cp, h.nNodes);
    if (st != GF_OK) return st;
    // K-projection over all buckets at once: [rows, KC] x [KC, C]  (CustomMatMulTensor layout: x K_l^T, K_l = [C, KC])
    const int KC = s->cfg.nContractions * Cp;
    st = s->cfg.custom_matmul ? gemm(ctx, false, true, (int)h.rows, Cc, KC, d.Q, KC, 0, Kl, KC, 0, d.f, Cc, 0, 1, 0)
                              : gemm(ctx, false, false, (int)h.rows, Cc, KC, d.Q, KC, 0, Kl, Cc, 0, d.f, Cc, 0, 1, 0);
    if (st == GF_OK) st = extra_products_forward(s, l);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "smp_bias_lrelu", bias_lrelu_forward, dim3(grid_for((size_t)h.rows * Cc)), dim3(256), 0, d.f, bl, Cc, (size_t)h.rows * Cc, kAlpha);
    return GF_OK;
}

// The read-out of level l: sh[n] = sum over (i, j) of f_l[n], vf = LeakyReLU(sh).  panels: a fused level left the column sums of its row
// panels behind (DevLevel::psum).  The nodes above 32 positions have no panels -- an empty range in the panel read-out -- and take theirs
// from the rows of f_l; nodes are numbered by size.
gf_status readout_level(gf_smp *s, int l, float *sh, float *vf, bool panels) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const gf_smp::DevLevel &d = s->lv[l];
    const int Cc = s->cfg.level_channels(l), nodes = h.nNodes;
    if (s->cfg.first_order) return smp_theta_readout(s, l, sh, vf);   // (column sums over the node's s rows: f_l[v] is [s][C])
    const auto from_panels = !panels ? nullptr : Cc == 64 ? readout_nodes_panels<64> : Cc == 32 ? readout_nodes_panels<32>
                                              : Cc == 16 ? readout_nodes_panels<16> : nullptr;   // (smp_panel_channels)
    if (from_panels)   // 256 / Cc nodes per workgroup
        GF_LAUNCH(ctx, "smp_readout_nodes", from_panels, dim3((unsigned)((nodes + 256 / Cc - 1) / (256 / Cc))), dim3(256), 0, d.psum, d.node_panel, nodes,
                  d.fwd_npanels, sh, vf);
    else if (Cc % 4 == 0 && Cc <= 1024)   // (workgroup per node, float4 lanes)
        GF_LAUNCH(ctx, "smp_readout_nodes", readout_nodes_v, dim3(nodes), dim3(256), 0, d.f, d.node_s, d.node_row, sh, vf, Cc);
    else
        GF_LAUNCH(ctx, "smp_readout_nodes", readout_nodes, dim3(grid_for((size_t)nodes * Cc)), dim3(256), 0, d.f, d.node_s, d.node_row, sh, vf, Cc,
                  (size_t)nodes * Cc);
    if (!from_panels) return GF_OK;
    int n0 = nodes;
    for (const gfsmp::Bucket &bk : h.buckets)
        if (bk.s > 32) {
            n0 = bk.first_node;
            break;
        }
    if (n0 < nodes)
        GF_LAUNCH(ctx, "smp_readout_nodes", readout_nodes_v, dim3(nodes - n0), dim3(256), 0, d.f, d.node_s + n0, d.node_row + n0, sh + (size_t)n0 * Cc,
                  vf + (size_t)n0 * Cc, Cc);
    return GF_OK;
}

// params in the device's layout (gf_smp::cfg); the arguments have passed forward_check
gf_status forward_sweep(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    gf_status st = ensure_ws(ctx, s->ws_need);
    if (st != GF_OK) return st;
    if (s->cfg.matrix_form) return smp_matrix_form_forward(s, params, targets, predict, loss, graph_feature);   // (LCNN, GCN_MW: smp_level_rowlist.hip)
    if (s->cfg.covariant) return smp_covariant_forward(s, params, targets, predict, loss, graph_feature);   // (CGCN_1D, CGCN_2D: smp_level_covariant.hip)
    if (s->cfg.distance_channel) return smp_distance_forward(s, params, targets, predict, loss, graph_feature);   // (two channels of that kind)
    if (s->cfg.gated()) return smp_gru_forward(s, params, targets, predict, loss, graph_feature);   // (the neighbourhood kind's second set of sweeps)
    if (s->cfg.neighbourhood) return smp_neighbourhood_forward(s, params, targets, predict, loss, graph_feature);   // (its own level 0 and read-out)
    const gfsmp::BatchLayout &B = s->lay;
    const int L = s->cfg.nLevels, C = s->cfg.nChanels, FD = s->cfg.fdim();
    const int CL = s->cfg.top_channels();   // (the read-out's width: C but for the channel-doubling SMP_1D_ver2 / ver3)
    const float *H, *W;
    std::vector<const float *> K, b;
    view_params<const float>(s->cfg, params, &H, &K, &b, &W);
    s->extra_w = s->n_extra ? params + param_count(s->cfg) : nullptr;   // (SMP_2D_ver7 on the 18-slice level: [.. W | X_1 .. X_L])
    std::vector<LevelKind> kind(L + 1, LevelKind::OpByOp);   // (asked once per pass; [0]: level 0 is nobody's fused level)
    for (int l = 1; l <= L; ++l) kind[l] = smp_level_kind(s, l);
    // level 0: f_0 = LeakyReLU(X H^T)   (MatMul(H, x_v) per vertex, SMP_omega.h:618)
    const int nV = B.level[0].nNodes;
    st = gemm(ctx, false, true, nV, C, FD, s->x, FD, 0, H, FD, 0, s->lv[0].f, C, 0, 1, 0);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "smp_bias_lrelu", bias_lrelu_forward, dim3(grid_for((size_t)nV * C)), dim3(256), 0, s->lv[0].f, (const float *)nullptr, C,
              (size_t)nV * C, s->cfg.level_slope());
    for (int l = 0; l <= L; ++l) s->lv[l].psum_ready = s->lv[l].pmax_ready = s->lv[l].sgn_ready = false;
    s->bwd_consumed = false;
    st = dup_level(s, 0);   // (SMP_2D_ver6 on the 18-slice level: channels [C, 2C) <- the transposed matrices; level 0: copies)
    if (st != GF_OK) return st;
    if (s->fused && !s->cfg.per_size()) {
        if (s->wbound && C == 64) GF_HIP_TRY(ctx, hipMemsetAsync(s->wbound, 0, sizeof(unsigned) * smp_wgrad_words(64, false) * (size_t)(L + 1), ctx->stream));
        st = smp_fused_stack_all(s, K);
        if (st != GF_OK) return st;
    }
    for (int l = 1; l <= L; ++l) {
        switch (kind[l]) {
        case LevelKind::Fused18: st = smp_fused_forward_level(s, l, K[l], b[l]); break;
        case LevelKind::Gamma: st = smp_gamma_forward_level(s, l, K[l], b[l]); break;   // products on the rows of level l - 1, one gather into f_l
        case LevelKind::Theta:          // the same shape of level, first order (b[l]: the per-size block); SMP_1D*: no [2 C'][C] matrix
        case LevelKind::Steerable2D:    // (K[l]: scalar_l -- SMP_2D_ver5: K_l then scalar_l --, b[l]: the per-size block)
        case LevelKind::Unrestricted:   // (the same two)
            st = smp_field_forward_level(s, l, K[l], b[l]);
            break;
        case LevelKind::OpByOp: st = forward_level_opbyop(s, l, K[l], b[l]); break;
        case LevelKind::Neighbourhood: break;   // (never here: smp_neighbourhood_forward took the pass above)
        }
        if (st == GF_OK && l < L) st = dup_level(s, l);
        if (st != GF_OK) return st;
    }
    if (s->cfg.physics) {  // every level read out into its block of the feature row; the head (MLP, loss) is the caller's
        const int width = (int)feature_width(s->cfg);
        int off = 0;
        for (int l = 0; l <= L; ++l) {
            const gf_smp::DevLevel &d = s->lv[l];
            const int Cc = s->cfg.level_channels(l);
            st = readout_level(s, l, d.sh, d.vf, l >= 1 && d.psum && d.psum_ready);
            if (st != GF_OK) return st;
            GF_LAUNCH(ctx, "smp_level_feature", level_feature_sum, dim3(B.nMol), dim3(64), 0, d.vf, s->mol_ptr, d.node_of_vertex, s->g, Cc, width, off);
            off += Cc;
        }
    } else {
        st = readout_level(s, L, s->sh, s->vf, s->lv[L].psum_ready);
        if (st != GF_OK) return st;
        if (s->cfg.nClass) {   // (a classifier: logits, softmax, arg-max label into predict, log p[label] into loss)
            st = readout_classes_forward(s, W, targets, predict, loss);
            if (st != GF_OK) return st;
        } else {
            // (predict and graph_feature are written by the kernel itself; a caller's buffer that IS the handle's own is written once)
            float *g_out = graph_feature == s->g ? nullptr : graph_feature, *y_out = predict == s->yhat ? nullptr : predict;
            GF_LAUNCH(ctx, "smp_readout_mol", readout_molecules, dim3(B.nMol), dim3(256), 0, s->vf, s->mol_ptr, s->mol_nodes, W, targets, s->g, s->yhat,
                      loss, s->dy, CL, g_out, y_out);
            graph_feature = nullptr;
        }
    }
    const size_t gwidth = s->cfg.physics ? feature_width(s->cfg) : (size_t)CL;
    if (graph_feature) GF_HIP_TRY(ctx, hipMemcpyAsync(graph_feature, s->g, sizeof(float) * B.nMol * gwidth, hipMemcpyDeviceToDevice, ctx->stream));
    s->forwarded = true;
    s->has_targets = targets != nullptr;   // (never a tower: forward_check)
    mark_used(s);
    return GF_OK;
}

bool data_parallel(const gf_smp *s) {   // (towers: the composite model reduces its own flat buffer)
    return dist_active(s->ctx) && s->grad_allreduce && !s->cfg.physics;
}

// What a reverse sweep refuses, padded model or not, before a gradient is written or a collective handed to RCCL.  *params == *grads ==
// null: the handle's own model.
gf_status backward_check(gf_smp *s, const float **params, float **grads, int accumulate, const float *dfeat) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (!s->forwarded) return fail(ctx, GF_ERR_INVALID, "gf_smp_backward before gf_smp_forward");
    if (!dfeat && !s->has_targets)  // Predict / Feature forward: dy would be y - 0, a gradient against a target nobody gave
        return fail(ctx, GF_ERR_INVALID, "gf_smp_backward: the last gf_smp_forward had no targets");
    if ((dfeat != nullptr) != (s->cfg.physics != 0))
        return fail(ctx, GF_ERR_INVALID, s->cfg.physics ? "a physics tower is differentiated with gf_smp_backward_features"
                                                         : "gf_smp_backward_features needs a physics tower");
    if (!*params && !*grads && s->own_p) {
        *params = s->own_p;
        *grads = s->own_g;
    }
    if (!*params || !*grads) return fail(ctx, GF_ERR_INVALID, "gf_smp_backward: null argument");
    gf_status st = smp_backward_admissible(s);
    if (st != GF_OK) return st;
    if (accumulate && data_parallel(s))
        return fail(ctx, GF_ERR_INVALID, "gf_smp_backward: accumulate with a communicator would re-sum earlier global sums "
                                         "(gf_smp_set_grad_allreduce(smp, 0) and reduce once at the end instead)");
    if (s->bwd_consumed && s->cfg.readout == 2)   // (the top level's dz_L has replaced the dh_L that gram_readout left)
        return fail(ctx, GF_ERR_INVALID, "gf_smp_backward: a second reverse sweep of a Gram handle needs a new gf_smp_forward (dz_L replaced dh_L in place)");
    if (s->bwd_consumed)   // (an op-by-op level's reverse sweep overwrites its Q with dQ: the forward state is gone)
        return fail(ctx, GF_ERR_INVALID, "gf_smp_backward: a second reverse sweep needs a new gf_smp_forward (op-by-op levels keep dQ in place of Q)");
    return GF_OK;
}

int feature_offset(const gfsmp::Config &c, int l) {   // first column of level l's block in a tower's feature row
    int off = 0;
    for (int k = 0; k < l; ++k) off += c.level_channels(k);
    return off;
}
// physics: the read-out of level l adds  dfeat[mol][block l] * lrelu'(sh_l)  at every position of every node of the level
gf_status feature_backward(gf_smp *s, const float *dfeat, int l, int acc) {
    const gf_smp::DevLevel &dl = s->lv[l];
    GF_LAUNCH(s->ctx, "smp_level_feature_bwd", level_feature_backward, dim3(s->lay.level[l].nNodes), dim3(256), 0, dfeat, dl.sh, dl.node_mol, dl.node_s,
              dl.node_row, dl.df, s->cfg.level_channels(l), (int)feature_width(s->cfg), feature_offset(s->cfg, l), acc);
    return GF_OK;
}
// a tower's FUSED level takes its read-out gradient as one vector per node (combine-backward adds it to the node's rows): the pass
// that broadcast it into df_l -- a read-modify-write of every row -- only runs for the other kinds and level 0
gf_status feature_nodevec(gf_smp *s, const float *dfeat, int l) {
    const gf_smp::DevLevel &dl = s->lv[l];
    const size_t n = (size_t)s->lay.level[l].nNodes * s->cfg.level_channels(l);
    GF_LAUNCH(s->ctx, "smp_level_feature_bwd", level_feature_nodevec, dim3(grid_for(n)), dim3(256), 0, dfeat, dl.sh, dl.node_mol, dl.dshl,
              s->cfg.level_channels(l), (int)feature_width(s->cfg), feature_offset(s->cfg, l), n);
    return GF_OK;
}

// dZ = dF * lrelu'(z) in place; db_l += column sums
gf_status bias_gradient(gf_smp *s, int l, float *dbl) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const long long rows = s->lay.level[l].rows;
    const int Cc = s->cfg.level_channels(l), rpb = 1024, nb = (int)((rows + rpb - 1) / rpb);
    GF_LAUNCH(ctx, "smp_lrelu_bwd", lrelu_backward_colsum, dim3(nb), dim3(256), 0, d.f, d.df, s->colpart, Cc, rows, rpb, kAlpha);
    GF_LAUNCH(ctx, "smp_colsum", colsum_finish, dim3(1), dim3(256), 0, s->colpart, dbl, Cc, nb);
    return GF_OK;
}

// behind bias_gradient: dK_l += Q^T dZ (MatMul::backward second operand), dQ = dZ K_l^T overwrites Q (first operand), the contraction's
// backward leaves dP in the promoted stack
gf_status backward_level_opbyop(gf_smp *s, int l, const float *Kl, float *dKl) {
    gf_ctx *ctx = s->ctx;
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const gf_smp::DevLevel &d = s->lv[l];
    const int Cc = s->cfg.level_channels(l), Cq = s->cfg.level_channels(l - 1);  // (equal unless a physics tower)
    const int KC = s->cfg.nContractions * Cq;
    gf_status st = extra_products_wgrad(s, l);
    if (st != GF_OK) return st;
    if (s->cfg.custom_matmul) {  // CustomMatMulTensor::backward (CustomMatMulTensor.h:70-85): dK_l [C, KC] += dZ^T Q, dQ = dZ K_l
        st = gemm(ctx, true, false, Cc, KC, (int)h.rows, d.df, Cc, 0, d.Q, KC, 0, dKl, KC, 0, 1, 1);
        if (st == GF_OK) st = gemm(ctx, false, false, (int)h.rows, KC, Cc, d.df, Cc, 0, Kl, KC, 0, d.Q, KC, 0, 1, 0);
    } else {
        st = gemm(ctx, true, false, KC, Cc, (int)h.rows, d.Q, KC, 0, d.df, Cc, 0, dKl, Cc, 0, 1, 1);
        if (st == GF_OK) st = gemm(ctx, false, true, (int)h.rows, KC, Cc, d.df, Cc, 0, Kl, Cc, 0, d.Q, KC, 0, 1, 0);
    }
    if (st == GF_OK) st = extra_products_backward(s, l);
    if (st == GF_OK) st = smp_dp_level_done(s, l);
    if (st == GF_OK && s->drop_on)   // the dropped slices receive no gradient
        st = launch_node_slice_scale(ctx, d.Q, d.node_s, d.node_row, d.keep_mask, 1.f, Cq, h.nNodes);
    return st == GF_OK ? smp_contract(s, l, /*backward=*/true) : st;
}

// df_{l-1} from what level l left: the fused level's folded consumer gather, else the consumer-list gather of dP (a fused level's D_bb /
// D_ac gradients arrive through dFdc beside it); the gamma level has written df_{l-1} itself
gf_status send_df_down(gf_smp *s, int l, LevelKind kind) {
    if (kind == LevelKind::Gamma || is_field_level(kind)) return GF_OK;
    const bool fused = kind == LevelKind::Fused18;
    if (fused && smp_fused_gather_enabled(s, l)) return smp_fused_gather_backward(s, l);
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    GF_LAUNCH(s->ctx, "smp_promote_bwd", promote_backward, dim3(s->lay.level[l - 1].nNodes), dim3(256), 0, s->P, pv.df, pv.node_s, pv.node_row,
              d.cons_ptr, d.cons_slab, d.cons_s, d.cons_inv_off, d.inv, s->cfg.level_channels(l - 1), fused ? d.dFdc : (const float *)nullptr,
              pv.node_pair, pv.node_center);
    return GF_OK;
}

// level 0: dZ0 = dF0 * lrelu'; dH += dZ0^T X
gf_status backward_level0(gf_smp *s, float *dH) {
    gf_ctx *ctx = s->ctx;
    const int nV = s->lay.level[0].nNodes, C = s->cfg.nChanels, FD = s->cfg.fdim();
    gf_status st = fold_level(s, 0);
    if (st != GF_OK) return st;
    // (level 0 has no bias: the column sums are discarded, so small row blocks cost nothing downstream; colpart holds
    //  maxrows / 1024 + maxpairs / 256 + 2 rows and level 0 has at most maxpairs / 64 blocks... keep nb within it)
    int rpb = 64;
    while ((nV + rpb - 1) / rpb > (int)s->colpart_rows && rpb < 1024) rpb *= 2;
    const int nb = (nV + rpb - 1) / rpb;
    GF_LAUNCH(ctx, "smp_lrelu_bwd", lrelu_backward_colsum, dim3(nb), dim3(256), 0, s->lv[0].f, s->lv[0].df, s->colpart, C, (long long)nV, rpb, s->cfg.level_slope());
    return gemm(ctx, true, false, C, FD, nV, s->lv[0].df, C, 0, s->x, FD, 0, dH, FD, 0, 1, 1);
}

// The reverse sweep.  dfeat == nullptr: from the loss of the last forward (SMP_omega / SMP_beta / SMP_2D).  dfeat != nullptr
// (physics towers): from the gradient of the tower's feature rows, [nMol][feature_width], given by the caller's head.
// params, grads in the device's layout (gf_smp::cfg); the arguments have passed backward_check.
gf_status backward_sweep(gf_smp *s, const float *params, float *grads, int accumulate, const float *dfeat) {
    gf_ctx *ctx = s->ctx;
    // (a no-op after this batch's forward; it makes the reverse sweep independent of who grew the context's workspace last)
    gf_status st = ensure_ws(ctx, s->ws_need);
    if (st != GF_OK) return st;
    if (s->cfg.matrix_form) return smp_matrix_form_backward(s, params, grads, accumulate);
    if (s->cfg.covariant) return smp_covariant_backward(s, params, grads, accumulate);
    if (s->cfg.distance_channel) return smp_distance_backward(s, params, grads, accumulate);
    if (s->cfg.gated()) return smp_gru_backward(s, params, grads, accumulate);
    if (s->cfg.neighbourhood) return smp_neighbourhood_backward(s, params, grads, accumulate);   // (never a tower: gf_smp_backward_features refuses)
    const gfsmp::BatchLayout &B = s->lay;
    const int L = s->cfg.nLevels, C = s->cfg.top_channels();   // (the read-out's width)
    const float *H, *W;
    std::vector<const float *> K, b;
    view_params<const float>(s->cfg, params, &H, &K, &b, &W);
    float *dH, *dW;
    std::vector<float *> dK, db;
    view_params<float>(s->cfg, grads, &dH, &dK, &db, &dW);
    const size_t np = param_count(s->cfg);
    s->extra_w = s->n_extra ? params + np : nullptr;
    s->extra_g = s->n_extra ? grads + np : nullptr;   // (every level writes its own blocks: nothing to clear)
    std::vector<LevelKind> kind(L + 1, LevelKind::OpByOp);   // (asked once per pass; [0]: level 0 is nobody's fused level)
    for (int l = 1; l <= L; ++l) kind[l] = smp_level_kind(s, l);
    // data-parallel (the context has a communicator): the gradient segment of a level is all-reduced as soon as it is complete
    const bool dp = data_parallel(s);
    s->dp_grads = nullptr;
    if (dp) {
        if (!s->ev_grad) GF_HIP_TRY(ctx, hipEventCreateWithFlags(&s->ev_grad, hipEventDisableTiming));
        if (!s->ev_comm) GF_HIP_TRY(ctx, hipEventCreateWithFlags(&s->ev_comm, hipEventDisableTiming));
        // Watchdog: the join of the PREVIOUS sweep's all-reduces is waited for here, by polling under GF_DIST_TIMEOUT_S -- a rank whose
        // peers never joined an exchange fails with its rank, the world and the segment in gf_last_error instead of queueing work
        // behind a collective that will never finish.  (The host may still run a whole forward pass ahead of the device.)
        if (s->dp_join_pending) {
            s->dp_join_pending = false;
            st = dist_wait_event(ctx, s->ev_comm, "the join of the previous gf_smp_backward's gradient all-reduces");
            if (st != GF_OK) return st;
        }
        s->dp_grads = grads;
    }
    struct DpScope {  // whatever the exit path, the next call starts clean
        gf_smp *s;
        ~DpScope() { s->dp_grads = nullptr; }
    } dp_scope = {s};
    if (!accumulate) GF_LAUNCH(ctx, "smp_zero", zero_f32, dim3(grid_for(np)), dim3(256), 0, grads, np);
    // the read-out's gradient into the top level: a fused level reads it as one vector per node, the others at every (i, j)
    const gfsmp::LevelLayout &top = B.level[L];
    // (a first-order level takes the read-out's gradient the same way: one vector per node, added inside its per-node kernel)
    const bool top_fused = !dfeat && (kind[L] == LevelKind::Fused18 || is_field_level(kind[L]));
    const bool classes = !dfeat && s->cfg.nClass;   // (a classifier: dg [nMol][C] goes down instead of dy[mol] * W)
    if (!dfeat && !classes) GF_LAUNCH(ctx, "smp_readout_dW", readout_dW, dim3(1), dim3(1024), 0, s->dy, s->g, dW, C, B.nMol);
    if (dfeat) {
        if (kind[L] != LevelKind::Fused18 && kind[L] != LevelKind::Theta) st = feature_backward(s, dfeat, L, 0);
        if (st != GF_OK) return st;
    } else if (classes) {
        st = readout_classes_dW(s, dW);
        if (st == GF_OK) st = readout_classes_backward(s, /*per_node=*/top_fused);
        if (st != GF_OK) return st;
    } else if (top_fused) {
        GF_LAUNCH(ctx, "smp_readout_bwd", readout_backward_nodevec, dim3(grid_for((size_t)top.nNodes * C)), dim3(256), 0, s->dy, W, s->sh,
                  s->top_node_mol, s->dsh, C, (size_t)top.nNodes * C);
    } else {
        GF_LAUNCH(ctx, "smp_readout_bwd", readout_backward_nodes, dim3(top.nNodes), dim3(256), 0, s->dy, W, s->sh, s->top_node_mol, s->lv[L].node_s,
                  s->lv[L].node_row, s->lv[L].df, C);
    }
    for (int l = L; l >= 1; --l) {
        if (l < L) st = fold_level(s, l);   // (SMP_2D_ver6 on the 18-slice level: the gradient of the transposed copies joins the matrices')
        if (st != GF_OK) return st;
        if (kind[l] != LevelKind::Fused18 && !is_field_level(kind[l]))
            s->bwd_consumed = true;   // (a first-order, steerable or unrestricted level keeps f, A, B: repeatable)
        switch (kind[l]) {
        case LevelKind::Fused18:
            if (dfeat) st = feature_nodevec(s, dfeat, l);
            if (st == GF_OK)
                st = smp_fused_backward_level(s, l, dK[l], db[l], dfeat ? s->lv[l].dshl : (l == L && top_fused) ? s->dsh : nullptr,
                                              /*rows_too=*/dfeat && l < L);
            break;
        case LevelKind::Gamma:   // dG gathered from dz, dK_l and df_{l-1} on the rows of level l - 1
            st = bias_gradient(s, l, db[l]);
            if (st == GF_OK) st = smp_gamma_backward_level(s, l, K[l], dK[l], smp_dp_level_done);
            break;
        case LevelKind::OpByOp:
            st = bias_gradient(s, l, db[l]);
            if (st == GF_OK) st = backward_level_opbyop(s, l, K[l], dK[l]);
            break;
        case LevelKind::Theta:   // dz, the per-size gradients, dG gathered from dz, dK_l and df_{l-1} on the rows of level l - 1
            if (dfeat) st = feature_nodevec(s, dfeat, l);
            if (st == GF_OK)
                st = smp_field_backward_level(s, l, K[l], b[l], dK[l], db[l], dfeat ? s->lv[l].dshl : l == L ? s->dsh : nullptr, /*rows_too=*/l < L,
                                              smp_dp_level_done);
            break;
        case LevelKind::Steerable2D:    // dz, dS in place, the per-size gradients and dscalar_l, df_{l-1} gathered from dS (never a tower)
        case LevelKind::Unrestricted:   // dz in place, dS beside it, the per-size gradients (and dscalar_l), df_{l-1} gathered from dS (never a tower)
            st = smp_field_backward_level(s, l, K[l], b[l], dK[l], db[l], l == L ? s->dsh : nullptr, /*rows_too=*/l < L, smp_dp_level_done);
            break;
        case LevelKind::Neighbourhood: break;   // (never here: smp_neighbourhood_backward took the pass above)
        }
        if (st == GF_OK) st = send_df_down(s, l, kind[l]);
        // a tower: level l - 1 is read out too, and its own contribution joins what its consumers sent down (a fused level adds its own)
        if (st == GF_OK && dfeat && kind[l - 1] != LevelKind::Fused18 && kind[l - 1] != LevelKind::Theta) st = feature_backward(s, dfeat, l - 1, 1);
        if (st != GF_OK) return st;
    }
    st = backward_level0(s, dH);
    if (st == GF_OK && dp) st = smp_dp_level_done(s, 0);
    if (st != GF_OK) return st;
    if (dp) {  // dH reduced, then join: everything after this call on the context's stream sees the global sums
        GF_HIP_TRY(ctx, hipEventRecord(s->ev_comm, dist_stream(ctx)));
        GF_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s->ev_comm, 0));
        s->dp_join_pending = true;
    }
    mark_used(s);
    return GF_OK;
}

// a checked reverse sweep at the C ABI: a padded model's parameters (and feature gradient) go in padded, its gradients come back cropped
gf_status backward_run(gf_smp *s, const float *params, float *grads, int accumulate, const float *dfeat) {
    gf_ctx *ctx = s->ctx;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!padded_channels(s)) return backward_sweep(s, params, grads, accumulate, dfeat);
    gf_status st = pad_params_now(s, params);   // (the caller may have stepped the parameters since the forward pass: same values then)
    if (st == GF_OK && dfeat) st = pad_feature_buffer(s);
    if (st == GF_OK && dfeat) st = copy_feature_blocks(s, const_cast<float *>(dfeat), s->pad_feat, /*to_user=*/false);
    if (st == GF_OK) st = backward_sweep(s, s->pad_p, s->pad_g, 0, dfeat ? s->pad_feat : nullptr);   // (with a communicator: the padded segments are all-reduced)
    if (st == GF_OK) st = crop_grads_now(s, grads, accumulate);
    return st;
}

}  // namespace
}  // namespace gf

extern "C" {

gf_status gf_smp_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss,
                         float *graph_feature) {
    gf_status st = gf::forward_check(s, &params, targets, predict, loss, graph_feature);
    if (st != GF_OK) return st;
    gf_ctx *ctx = s->ctx;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!gf::padded_channels(s)) return gf::forward_sweep(s, params, targets, predict, loss, graph_feature);
    st = gf::pad_params_now(s, params);
    if (st == GF_OK && graph_feature) st = gf::pad_feature_buffer(s);
    if (st == GF_OK) st = gf::forward_sweep(s, s->pad_p, targets, predict, loss, graph_feature ? s->pad_feat : nullptr);
    if (st == GF_OK && graph_feature) st = gf::copy_feature_blocks(s, graph_feature, s->pad_feat, /*to_user=*/true);   // (the padded columns are cropped)
    return st;
}

// RisiContraction_18_dropout for the next forward / backward of a physics tower (SMP_sigma_pairgraphs): masks[(l-1) * nVertices + gv]
// = kept-slice bits of the contraction of global vertex gv (molecules back to back) at level l, drawn by the caller in the
// reference's order; scale = 1 (train) or nKept / 18 with all bits set (test).  masks == NULL: plain RisiContraction_18.
gf_status gf_smp_dropout_masks(gf_smp *s, const unsigned *masks, float scale) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    gf_ctx *ctx = s->ctx;
    if (s->cfg.per_size() || s->cfg.neighbourhood)
        return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_dropout_masks: a first-order, steerable_2d or neighbourhood handle has no contraction slices to drop");
    if (s->cfg.matrix_form) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_dropout_masks: a matrix-form handle (LCNN, GCN_MW) has no contraction slices to drop");
    if (s->cfg.covariant) return fail(ctx, GF_ERR_UNSUPPORTED, "gf_smp_dropout_masks: a covariant handle (CGCN_1D, CGCN_2D) has no contraction slices to drop");
    if (!masks) {
        s->drop_on = false;
        return GF_OK;
    }
    if (!s->prepared || !s->cfg.physics) return fail(ctx, GF_ERR_INVALID, "gf_smp_dropout_masks: needs a prepared physics tower");
    const gfsmp::BatchLayout &B = s->lay;
    const int totalV = B.mol_first_vertex[B.nMol];
    // The masks go up through a page-locked staging table of the handle, all levels at once, behind an event: a pageable source makes
    // every copy a blocking one and the old per-level hipStreamSynchronize drained the context's stream three times per tower and
    // step (the host then drew the next masks -- a million rand() calls per 1024-sample step -- with the device idle).
    const size_t need = (size_t)s->cfg.nLevels * totalV;
    if (s->mask_stage_n < need) {
        if (s->mask_stage) (void)hipHostFree(s->mask_stage);
        s->mask_stage = nullptr;
        s->mask_stage_n = 0;
        GF_HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void **>(&s->mask_stage), need * sizeof(unsigned), hipHostMallocDefault));
        s->mask_stage_n = need;
    }
    if (!s->ev_mask) GF_HIP_TRY(ctx, hipEventCreateWithFlags(&s->ev_mask, hipEventDisableTiming));
    else GF_HIP_TRY(ctx, hipEventSynchronize(s->ev_mask));   // (the previous step's copies have left the table: long done)
    for (int l = 1; l <= s->cfg.nLevels; ++l) {
        unsigned *by_node = s->mask_stage + (size_t)(l - 1) * totalV;
        for (int gv = 0; gv < totalV; ++gv) by_node[(size_t)B.node_of_vertex[l][gv]] = masks[(size_t)(l - 1) * totalV + gv];
        GF_HIP_TRY(ctx, hipMemcpyAsync(s->lv[l].keep_mask, by_node, sizeof(unsigned) * totalV, hipMemcpyHostToDevice, ctx->stream));
    }
    GF_HIP_TRY(ctx, hipEventRecord(s->ev_mask, ctx->stream));
    // the factor tables of the fused levels (smp_fused.hip: build_dropout_factors fills them at every forward): towers computed at 32 channels
    if (s->cfg.square() && (s->cfg.nChanels == 32 || s->cfg.nChanels == 16))
        for (int l = 1; l <= s->cfg.nLevels; ++l) {
            gf_smp::DevLevel &d = s->lv[l];
            if (d.nodefac && d.rowfac8) continue;
            gf_status st = gf::upload(s, &d.nodefac, nullptr, (size_t)B.level[l].nNodes * 18);
            if (st == GF_OK) st = gf::upload(s, &d.rowfac8, nullptr, (size_t)B.level[l].rows * 8);
            if (st != GF_OK) return st;
        }
    s->drop_on = true;
    s->drop_scale = scale;
    return GF_OK;
}

gf_status gf_smp_set_grad_allreduce(gf_smp *s, int on) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (on && (s->cfg.per_size() || s->cfg.neighbourhood))
        return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_set_grad_allreduce: a first-order, steerable_2d or neighbourhood handle has no data-parallel "
                                                "exchange (reduce the flat gradient)");
    if (on && s->cfg.matrix_form)
        return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_set_grad_allreduce: a matrix-form handle (LCNN, GCN_MW) has no data-parallel exchange (reduce the "
                                                "flat gradient)");
    if (on && s->cfg.covariant)
        return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_set_grad_allreduce: a covariant handle (CGCN_1D, CGCN_2D) has no data-parallel exchange (reduce the "
                                                "flat gradient)");
    s->grad_allreduce = on ? 1 : 0;
    return GF_OK;
}

gf_status gf_smp_backward(gf_smp *s, const float *params, float *grads, int accumulate) {
    gf_status st = gf::backward_check(s, &params, &grads, accumulate, nullptr);
    return st == GF_OK ? gf::backward_run(s, params, grads, accumulate, nullptr) : st;
}

gf_status gf_smp_backward_features(gf_smp *s, const float *params, float *grads, const float *d_feature, int accumulate) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (s->cfg.steerable_2d || s->cfg.unrestricted || s->cfg.neighbourhood)
        return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_backward_features: a steerable_2d, unrestricted or neighbourhood handle is no tower");
    if (s->cfg.matrix_form) return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_backward_features: a matrix-form handle (LCNN, GCN_MW) is no tower");
    if (s->cfg.covariant) return fail(s->ctx, GF_ERR_UNSUPPORTED, "gf_smp_backward_features: a covariant handle (CGCN_1D, CGCN_2D) is no tower");
    if (!d_feature) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_backward_features: null feature gradient");
    gf_status st = gf::backward_check(s, &params, &grads, accumulate, d_feature);
    return st == GF_OK ? gf::backward_run(s, params, grads, accumulate, d_feature) : st;
}

size_t gf_smp_feature_width(const gf_smp *s) {
    if (!s) return 0;
    return s->cfg.physics ? gf::feature_width(s->ucfg) : (size_t)s->ucfg.top_channels();
}

/* 1 (default): fused level kernels where the shape allows; 0: the op-by-op pipeline (promotion, RisiContraction_18,
 * MatMul, VectorAddTensor, LeakyReLU3D as separate kernels).  Both produce the same results within fp32 rounding. */
gf_status gf_smp_device_bytes(const gf_smp *s, size_t *in_use, size_t *reserved) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    size_t u = 0, r = 0;
    for (const gf_smp::Block &b : s->pool) {
        r += b.bytes;
        if (b.used) u += b.bytes;
    }
    if (in_use) *in_use = u;
    if (reserved) *reserved = r;
    return GF_OK;
}

gf_status gf_smp_set_fused(gf_smp *s, int on) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    s->fused = on ? 1 : 0;
    s->forwarded = false;
    return GF_OK;
}

/* introspection for parity tests: how often this handle launched the single-vertex-source kernels of level 1 (the launch names are the
 * general kernels', so the timing table cannot tell) */
long long gf_smp_single_vertex_launches(const gf_smp *s) { return s ? s->single_launches : 0; }
/* ... and how many level passes skipped the projected matrix of their empty rows (FusedRoute::skip_empty) */
long long gf_smp_empty_row_calls(const gf_smp *s) { return s ? s->empty_row_calls : 0; }
gf_status gf_smp_level_projected_f32(gf_smp *s, int level, float *out) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (!s->prepared || !s->forwarded || level < 1 || level > s->cfg.nLevels || !out || (int)s->lv.size() <= level)
        return fail(s->ctx, GF_ERR_INVALID, "gf_smp_level_projected_f32: bad argument, or no forward pass yet");
    if (s->cfg.nChanels != s->ucfg.nChanels) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_level_projected_f32: a handle computed at padded channels");
    GF_HIP_TRY(s->ctx, hipSetDevice(s->ctx->device));
    return gf::smp_fused_copy_projected(s, level, out);
}

/* introspection for parity tests: receptive field phi_level(v) of molecule mol; returns its size */
int gf_smp_receptive_field(const gf_smp *s, int mol, int level, int v, int *out, int capacity) {
    if (!s || !s->prepared || mol < 0 || mol >= s->lay.nMol || level < 0 || level > s->cfg.nLevels) return -1;
    const gfsmp::Molecule &M = s->lay.mols[mol];
    if (s->cfg.matrix_form == 1) {   // LCNN: the k entries of rank position v's sequence (level 0: the vertex at that position)
        const int V = s->cfg.max_nVertices, k = s->cfg.nNeighbors;
        if (v < 0 || v >= V) return -1;
        if (level == 0) {
            if (capacity > 0) out[0] = s->lay.rl.order[(size_t)mol * V + v];
            return 1;
        }
        for (int j = 0; j < k && j < capacity; ++j) out[j] = s->lay.rl.seq[((size_t)mol * V + v) * k + j];
        return k;
    }
    if (v < 0 || v >= M.V) return -1;
    if (s->cfg.matrix_form) {   // GCN_MW: the non-zero columns of row v of A-hat, ascending (the same at every level)
        const int v0 = s->lay.mol_first_vertex[mol];
        const long long e0 = s->lay.rl.ptr[(size_t)v0 + v], n = s->lay.rl.ptr[(size_t)v0 + v + 1] - e0;
        for (long long i = 0; i < n && i < capacity; ++i) out[i] = s->lay.rl.src[(size_t)(e0 + i)] - v0;
        return (int)n;
    }
    if (s->cfg.covariant) {   // the mask of level `level`: { u : sp[u][v] <= level }, ascending
        int n = 0;
        for (int u = 0; u < M.V; ++u)
            if (M.hops[(size_t)u * M.V + v] <= level) {
                if (n < capacity) out[n] = u;
                ++n;
            }
        return n;
    }
    if (s->cfg.neighbourhood) {   // N_level(v), ascending (level 0: the vertex itself)
        if (level == 0) {
            if (capacity > 0) out[0] = v;
            return 1;
        }
        const gfsmp::BatchLayout::NeighbourList &nl = s->lay.nb_lists[(size_t)s->lay.nb_list_of_level[level]];
        const int v0 = s->lay.mol_first_vertex[mol];
        const long long e0 = nl.ptr[(size_t)v0 + v], n = nl.ptr[(size_t)v0 + v + 1] - e0;
        for (long long i = 0; i < n && i < capacity; ++i) out[i] = nl.idx[(size_t)(e0 + i)] - v0;
        return (int)n;
    }
    const std::vector<int> &f = M.phi[level][v];
    for (int i = 0; i < (int)f.size() && i < capacity; ++i) out[i] = f[i];
    return (int)f.size();
}

/* introspection for parity tests: the level-`level` activation f_l[v] of molecule `mol` ([s][s][C], what level[l]->f[v]->value
 * holds in the reference after forward(), SMP_omega.h:667-669) or its reduced adjacency ([s][s], level[l]->adj[v], :556-581),
 * copied to a HOST buffer.  Returns the element count, or -1 (bad argument / capacity too small / not forwarded).  Blocking. */
static long long smp_read_node(gf_smp *s, int mol, int level, int v, float *out, size_t capacity, bool adjacency) {
    if (!s || !s->prepared || !out || mol < 0 || mol >= s->lay.nMol || level < 0 || level > s->cfg.nLevels) return -1;
    if (adjacency ? level < 1 : !s->forwarded) return -1;
    if (s->cfg.matrix_form) {   // GCN_MW: h_level[v] [H]; LCNN: a1[i] [C1] (level 1), c2[i] [C2] (level 2), i a rank position; no reduced adjacency
        const bool lcnn = s->cfg.matrix_form == 1;
        const size_t W = lcnn && level == 2 ? (size_t)s->cfg.nChanels2 : (size_t)s->cfg.nChanels;
        const int nrows = lcnn ? s->cfg.max_nVertices : s->lay.mols[mol].V;
        if (adjacency || (lcnn && level == 0) || v < 0 || v >= nrows || W > capacity) return -1;
        const float *src = s->lv[level].f + ((size_t)s->lay.mol_first_vertex[mol] + v) * W;
        if (hipMemcpyAsync(out, src, W * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream) != hipSuccess) return -1;
        if (hipStreamSynchronize(s->ctx->stream) != hipSuccess) return -1;
        return (long long)W;
    }
    if (s->cfg.covariant) {   // h_level[v] [M]; no reduced adjacency
        const size_t W = (size_t)s->cfg.max_nVertices, nV = (size_t)s->lay.level[0].nNodes;
        if (adjacency || v < 0 || v >= s->lay.mols[mol].V || W > capacity) return -1;
        const float *src = s->cov_h + ((size_t)level * nV + (size_t)s->lay.mol_first_vertex[mol] + v) * W;
        if (hipMemcpyAsync(out, src, W * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream) != hipSuccess) return -1;
        if (hipStreamSynchronize(s->ctx->stream) != hipSuccess) return -1;
        return (long long)W;
    }
    if (s->cfg.neighbourhood) {   // h_level[v] [H] (a distance handle: [h^v | h^d], 2 H); the models have no reduced adjacency
        const size_t H = (size_t)s->cfg.nChanels, width = s->cfg.distance_channel ? 2 * H : H;
        if (adjacency || v < 0 || v >= s->lay.mols[mol].V || width > capacity) return -1;
        const size_t at = ((size_t)s->lay.mol_first_vertex[mol] + v) * H;
        if (hipMemcpyAsync(out, s->lv[level].f + at, H * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream) != hipSuccess) return -1;
        if (s->cfg.distance_channel &&
            hipMemcpyAsync(out + H, s->lvd[level].f + at, H * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream) != hipSuccess)
            return -1;
        if (hipStreamSynchronize(s->ctx->stream) != hipSuccess) return -1;
        return (long long)width;
    }
    const gfsmp::LevelLayout &h = s->lay.level[level];
    int n = -1;
    if (level == 0) {
        const int g = s->lay.mol_first_vertex[mol] + v;
        if (v >= 0 && g < s->lay.mol_first_vertex[mol + 1]) n = g;
    } else {
        for (int i = 0; i < h.nNodes && n < 0; ++i)
            if (h.node_mol[i] == mol && h.node_vertex[i] == v) n = i;
    }
    if (n < 0) return -1;
    const size_t sz = (size_t)h.node_s[n], C = (size_t)s->cfg.level_channels(level);  // (physics towers halve per level)
    const size_t Cu = (size_t)s->ucfg.level_channels(level);                              // (the caller's channels: the padded ones are cropped)
    const size_t npos = s->cfg.first_order ? sz : sz * sz;   // (a first-order activation is [s][C])
    if (adjacency && s->cfg.first_order) return -1;          // (... and the model has no reduced adjacency)
    const size_t count = adjacency ? sz * sz : npos * Cu;
    if (count > capacity) return -1;
    const float *src = adjacency ? s->lv[level].adj + h.node_row[n] : s->lv[level].f + (size_t)h.node_row[n] * C;
    if (!adjacency && Cu != C) {
        if (hipMemcpy2DAsync(out, Cu * sizeof(float), src, C * sizeof(float), Cu * sizeof(float), npos, hipMemcpyDeviceToHost, s->ctx->stream) != hipSuccess)
            return -1;
    } else if (hipMemcpyAsync(out, src, count * sizeof(float), hipMemcpyDeviceToHost, s->ctx->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(s->ctx->stream) != hipSuccess) return -1;
    return (long long)count;
}
long long gf_smp_read_activation(gf_smp *s, int mol, int level, int v, float *out, size_t capacity) {
    return smp_read_node(s, mol, level, v, out, capacity, false);
}
long long gf_smp_read_reduced_adjacency(gf_smp *s, int mol, int level, int v, float *out, size_t capacity) {
    return smp_read_node(s, mol, level, v, out, capacity, true);
}

/* counts used by the bench to report algorithmic work: rows = sum s^2, ppos = sum s^3 at a level */
gf_status gf_smp_level_sizes(const gf_smp *s, int level, long long *nodes, long long *rows, long long *ppos) {
    if (!s) return fail(nullptr, GF_ERR_INVALID, "null smp handle");
    if (!s->prepared || level < 0 || level > s->cfg.nLevels) return fail(s->ctx, GF_ERR_INVALID, "gf_smp_level_sizes: bad level");
    const gfsmp::LevelLayout &h = s->lay.level[level];
    if (nodes) *nodes = h.nNodes;
    if (rows) *rows = h.rows;
    if (ppos) *ppos = h.ppos;
    return GF_OK;
}
long long gf_smp_level_pairs(const gf_smp *s, int level) {
    if (!s || !s->prepared || level < 0 || level > s->cfg.nLevels) return -1;
    return s->lay.level[level].pairs;
}
long long gf_smp_level_covered_rows(const gf_smp *s, int level) {
    if (!s || !s->prepared || level < 0 || level > s->cfg.nLevels) return -1;
    const gfsmp::LevelLayout &h = s->lay.level[level];
    if (level == 0 || !s->lv[level].rowflag || h.rows == 0) return h.rows;
    gf_smp *ms = const_cast<gf_smp *>(s);   // (cached per prepared batch; see the header for the threading contract)
    if (ms->h_covered.size() != (size_t)s->cfg.nLevels + 1) ms->h_covered.assign((size_t)s->cfg.nLevels + 1, -1);
    if (ms->h_covered[level] >= 0) return ms->h_covered[level];
    std::vector<unsigned char> fl((size_t)h.rows);
    hipStream_t up = s->upload ? s->upload : s->ctx->stream;
    if (hipMemcpyAsync(&fl[0], s->lv[level].rowflag, fl.size(), hipMemcpyDeviceToHost, up) != hipSuccess || hipStreamSynchronize(up) != hipSuccess)
        return -1;
    long long n = 0;
    for (size_t i = 0; i < fl.size(); ++i) n += (fl[i] >> 1) & 1;
    ms->h_covered[level] = n;
    return n;
}
long long gf_smp_level_present_rows(const gf_smp *s, int level) {
    if (!s || !s->prepared || level < 0 || level > s->cfg.nLevels) return -1;
    const gfsmp::LevelLayout &h = s->lay.level[level];
    if (level >= 1 && s->lay.device_tables && s->tab_stats) {
        gf_smp *ms = const_cast<gf_smp *>(s);   // (lazily: the statistics words the table kernels left on the device)
        if (ms->h_tab_stats.empty()) {
            ms->h_tab_stats.assign((size_t)4 * (s->cfg.nLevels + 1), 0u);
            hipStream_t up = s->upload ? s->upload : s->ctx->stream;
            if (hipMemcpyAsync(&ms->h_tab_stats[0], s->tab_stats, sizeof(unsigned) * ms->h_tab_stats.size(), hipMemcpyDeviceToHost, up) != hipSuccess ||
                hipStreamSynchronize(up) != hipSuccess) {
                ms->h_tab_stats.clear();
                return -1;
            }
        }
        unsigned long long n = 0;
        std::memcpy(&n, &s->h_tab_stats[(size_t)4 * level + 2], sizeof(n));
        return (long long)n;
    }
    if (level == 0 || h.pi.size() != (size_t)h.rows) return h.rows;
    long long n = 0;
    for (size_t i = 0; i < h.pi.size(); ++i) n += h.pi[i] >= 0;
    return n;
}

}  // extern "C"
