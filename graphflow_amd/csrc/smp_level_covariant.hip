// smp_level_covariant.hip -- the whole-network covariant vertex level: CGCN_1D and CGCN_2D (GraphFlow/CGCN_1D.h, CGCN_2D.h),
// gf_smp_config.covariant = 1, 2.  A vertex carries ONE vector h_l[v] of length M = max_nVertices, indexed by the molecule's vertex ids; a
// level's learned matrix is F_l [M][M]; the update is masked by the receptive field.  For one molecule of V <= M vertices:
//
//   h_0[v]    = e_v <x[v], H>                                                                        (VertexRepresentation)
//   n_l[v]    = sum_{u in N(v)} h_{l-1}[u]                                                           (form 1: RisiLayer1D)
//   n_l[v][i] = sum_{u in N(v)} h_{l-1}[u][i] E_{v,u},  E_{v,u} = sum_{w in N(v), w != u} s_w,  s_u = sum_k h_{l-1}[u][k]   (form 2: RisiLayer2D)
//   h_l[v][i] = LeakyReLU(sp[i][v] <= l ? (F_l n_l[v])[i] : 0)                                       (MatVecMul, Masking, LeakyReLU 0.01)
//   g = sum_v h_L[v],  predict = sum_i g[i],  loss = 0.5 (predict - target)^2                        (SumVectors, SumComponents, SquaredLoss)
//
// N(v) = { u : adj[u][v] > 0 } (column v of the adjacency, ascending).  Every position i >= V and every position outside the mask is zero in
// every h_l, so a level only touches F_l[:V, :V] and a molecule's whole network is a few KB: one level of a 1,024-molecule batch is about 30
// MFLOP, and a level-by-level formulation would be nothing but launch latency.  Two kernels instead, each ONE launch for all levels:
//   cov_network_fwd   one workgroup per molecule.  h_{l-1} and h_l ping-pong in LDS as [V][V | 1]; F_l[:V, :V] is staged per level with the
//                     same odd row stride; lanes run over the position i, so the F_l[i][j] of a half-wave are 32 different banks (an odd
//                     stride is a unit modulo 32) and n_l[v][j] is one address (a broadcast).  The exclusive sums E_{v,u} are evaluated
//                     directly -- at most deg^2 additions per vertex -- never as S - s_u, which cancels in fp32.  Writes what the reverse
//                     needs (every h_l[v] and n_l[v], zero beyond V), the graph feature, predict, loss and dy, each summed in a fixed order.
//   cov_network_bwd   one workgroup per CHUNK of ceil(nMol / chunks) consecutive molecules, chunks = min(nMol, kCovariantSplits): the
//                     boundaries depend on nMol only.  Per molecule the levels in reverse:
//                       dz = dh_l LeakyReLU'(h_l) mask;  dF_l[i][j] += dz_v[i] n_v[j];  dn_v = F_l^T dz_v;
//                       form 1: dh_{l-1}[u] = sum_{v : u in N(v)} dn_v
//                       form 2: dh_{l-1}[u][j] = sum_v (dn_v[j] E_{v,u} + c_{v,u}),  c_{v,u} = sum_{w in N(v), w != u} <dn_v, h_{l-1}[w]>
//                     (c is sum_i dn_v[i] (T_v[i] - h_u[i]), T_v = sum_{u in N(v)} h_u, with the subtraction taken out: the pair dots
//                     are summed directly).  dh_{l-1} is a GATHER over the transposed lists in ascending v.  The chunk's gradient image [H | F_1 ..
//                     F_L] lives in the context's workspace; element e of it is only ever touched by thread e mod 256 of the chunk's
//                     workgroup, so the read-modify-write needs neither atomics nor fences.  dH = sum_v dh_0[v][v] x[v] joins it.
//   cov_fold          grads[e] (+)= the chunks' images in ascending order.
// RisiLayer2D::backward and SumComponents::backward of the classes also put gradient on positions outside the mask and on positions >= V;
// the mask one level down and VertexRepresentation::backward (which reads gradient[vertex] only) discard them, so they are never formed.
// No matrix pipe: V x V x V products at V <= 64 are about 50 MFLOP per level over the whole batch -- the step is bound by launches and LDS
// latency (arithmetic, not a measurement: DESIGN.md).  No float atomics: two runs give the same bits.  Both kernels are also operators of
// the C ABI on caller-supplied operands (gf_smp_covariant_forward_ex_f32, gf_smp_covariant_backward_ex_f32 at the end of the file).
#include <vector>

#include "smp_config.h"
#include "smp_vertex_level.h"

namespace gf {
using namespace vertex_level;
namespace {

constexpr float kSlope = 0.01f;

// The network of one molecule per workgroup.  LDS (gf::smp_covariant_lds_bytes): five of the seven [V][Vp] images, Vp = V | 1, the vector of
// row sums, and the hop counts hp[v][i] = sp[i][v] as bytes.  s0 != NULL: the level-0 scalars are given; else they are <x[v], H>.
template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void cov_network_fwd(const int *__restrict__ mol_ptr, const long long *__restrict__ nb_ptr,
                                                          const int *__restrict__ nb_idx, const unsigned char *__restrict__ hop,
                                                          const float *__restrict__ s0, const float *__restrict__ x, const float *__restrict__ Hw,
                                                          int FD, const float *__restrict__ F, const float *__restrict__ target,
                                                          float *__restrict__ h, float *__restrict__ n, float *__restrict__ g,
                                                          float *__restrict__ yhat, float *__restrict__ loss, float *__restrict__ dy, int L, int M,
                                                          int nV) {
    extern __shared__ __align__(16) float lds[];
    const int m = blockIdx.x, tid = threadIdx.x, v0 = mol_ptr[m], V = mol_ptr[m + 1] - v0;
    if (V <= 0) {   // (uniform for the workgroup: an empty molecule of a stand-alone call)
        for (int k = tid; k < M; k += kBlock) g[(size_t)m * M + k] = 0.f;
        if (tid == 0) {
            const float t = target ? target[m] : 0.f;
            yhat[m] = 0.f;
            if (loss) loss[m] = 0.5f * t * t;
            if (dy) dy[m] = -t;
        }
        return;
    }
    const int Vp = V | 1, VV = V * Vp;
    float *P = lds, *Q = P + VV, *N = Q + VV, *Fs = N + VV, *EX = Fs + VV;   // h_{l-1}, h_l, n_l, F_l[:V, :V], E_{v,u}
    float *sv = lds + 7 * VV;                                                 // [V] row sums (behind the reverse kernel's seven images)
    unsigned char *hp = reinterpret_cast<unsigned char *>(sv + 2 * V + 8);   // [V][V]
    for (int i = tid; i < V * V; i += kBlock) {
        const int v = i / V, k = i - v * V;
        hp[i] = hop[(size_t)(v0 + v) * M + k];
        P[v * Vp + k] = 0.f;
    }
    __syncthreads();
    for (int v = tid; v < V; v += kBlock) {   // level 0: a dot product per vertex
        float d;
        if (s0) {
            d = s0[v0 + v];
        } else {
            const float *xv = x + (size_t)(v0 + v) * FD;
            d = 0.f;
            for (int f = 0; f < FD; ++f) d = fmaf(xv[f], Hw[f], d);
        }
        P[v * Vp + v] = d;
    }
    __syncthreads();
    for (int i = tid; i < V * M; i += kBlock) {
        const int v = i / M, k = i - v * M;
        h[(size_t)(v0 + v) * M + k] = k < V ? P[v * Vp + k] : 0.f;
    }
    for (int l = 1; l <= L; ++l) {
        const float *Fl = F + (size_t)(l - 1) * M * M;
        for (int i = tid; i < V * V; i += kBlock) {
            const int r = i / V, c = i - r * V;
            Fs[r * Vp + c] = Fl[(size_t)r * M + c];
        }
        if (PAIRS)
            for (int u = tid; u < V; u += kBlock) {
                float acc = 0.f;
                for (int k = 0; k < V; ++k) acc += P[u * Vp + k];
                sv[u] = acc;
            }
        __syncthreads();
        if (PAIRS) {   // E_{v,u}: the other members' row sums, added directly
            for (int i = tid; i < V * V; i += kBlock) {
                const int v = i / V, u = i - v * V;
                const long long e1 = nb_ptr[v0 + v + 1];
                float acc = 0.f;
                bool member = false;
                for (long long e = nb_ptr[v0 + v]; e < e1; ++e) {
                    const int w = nb_idx[e] - v0;
                    if (w == u) member = true;
                    else acc += sv[w];
                }
                EX[v * Vp + u] = member ? acc : 0.f;
            }
            __syncthreads();
        }
        for (int i = tid; i < V * V; i += kBlock) {   // the aggregate
            const int v = i / V, k = i - v * V;
            const long long e1 = nb_ptr[v0 + v + 1];
            float acc = 0.f;
            for (long long e = nb_ptr[v0 + v]; e < e1; ++e) {
                const int u = nb_idx[e] - v0;
                acc = PAIRS ? fmaf(P[u * Vp + k], EX[v * Vp + u], acc) : acc + P[u * Vp + k];
            }
            N[v * Vp + k] = acc;
        }
        __syncthreads();
        float *nl = n + ((size_t)(l - 1) * nV + v0) * M, *hl = h + ((size_t)l * nV + v0) * M;
        for (int i = tid; i < V * M; i += kBlock) {
            const int v = i / M, k = i - v * M;
            nl[i] = k < V ? N[v * Vp + k] : 0.f;
        }
        for (int i = tid; i < V * V; i += kBlock) {   // z = F_l n, the mask, LeakyReLU: lanes over the position k
            const int v = i / V, k = i - v * V;
            const float *fr = Fs + k * Vp, *nv = N + v * Vp;
            float acc = 0.f;
            for (int j = 0; j < V; ++j) acc = fmaf(fr[j], nv[j], acc);
            const float z = (int)hp[i] <= l ? acc : 0.f;
            Q[v * Vp + k] = z > 0.f ? z : kSlope * z;
        }
        __syncthreads();
        for (int i = tid; i < V * M; i += kBlock) {
            const int v = i / M, k = i - v * M;
            hl[i] = k < V ? Q[v * Vp + k] : 0.f;
        }
        float *t = P;
        P = Q;
        Q = t;
    }
    // the read-out: g[i] = sum_v h_L[v][i] in ascending v, predict = sum_i g[i] in ascending i
    for (int k = tid; k < V; k += kBlock) {
        float acc = 0.f;
        for (int v = 0; v < V; ++v) acc += P[v * Vp + k];
        sv[V + k] = acc;
    }
    __syncthreads();
    for (int k = tid; k < M; k += kBlock) g[(size_t)m * M + k] = k < V ? sv[V + k] : 0.f;
    if (tid == 0) {
        float y = 0.f;
        for (int k = 0; k < V; ++k) y += sv[V + k];
        const float t = target ? target[m] : 0.f;
        yhat[m] = y;
        if (loss) loss[m] = 0.5f * (y - t) * (y - t);
        if (dy) dy[m] = y - t;   // SquaredLoss::backward
    }
}

// The reverse of the molecules m0 .. m1 - 1 of one chunk, one after another.  LDS: the seven [V][Vp] images (D = dh_l / dz, D2 = dh_{l-1},
// N = n_l then dn, Fs = F_l[:V, :V] then the pair dots, P = h_{l-1}, EX, CC), sv [V], hp.  img = the chunk's gradient image [FD | L M M]:
// element e belongs to thread e mod kBlock from the zero fill to the last addition.
template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void cov_network_bwd(const int *__restrict__ mol_ptr, const long long *__restrict__ nb_ptr,
                                                          const int *__restrict__ nb_idx, const long long *__restrict__ nb_tptr,
                                                          const int *__restrict__ nb_tidx, const unsigned char *__restrict__ hop,
                                                          const float *__restrict__ x, int FD, const float *__restrict__ F,
                                                          const float *__restrict__ h, const float *__restrict__ n, const float *__restrict__ dy,
                                                          float *__restrict__ part, float *__restrict__ ds0, int L, int M, int nV, int nMol, int per,
                                                          int maxV) {
    extern __shared__ __align__(16) float lds[];
    const int tid = threadIdx.x, m0 = blockIdx.x * per, m1 = m0 + per < nMol ? m0 + per : nMol;
    const size_t image = (size_t)FD + (size_t)L * M * M;
    float *img = part + (size_t)blockIdx.x * image;
    for (size_t e = tid; e < image; e += kBlock) img[e] = 0.f;
    for (int m = m0; m < m1; ++m) {
        const int v0 = mol_ptr[m], V = mol_ptr[m + 1] - v0;
        if (V <= 0 || V > maxV) continue;   // (uniform; the launchers have checked V against the LDS they asked for)
        const int Vp = V | 1, VV = V * Vp;
        float *D = lds, *D2 = D + VV, *N = D2 + VV, *Fs = N + VV, *P = Fs + VV, *EX = P + VV, *CC = EX + VV, *sv = CC + VV;
        unsigned char *hp = reinterpret_cast<unsigned char *>(sv + 2 * V + 8);
        __syncthreads();   // (the molecule before is done with the images)
        const float d = dy[m];
        for (int i = tid; i < V * V; i += kBlock) {   // SumComponents and SumVectors: dh_L[v][i] = dy
            const int v = i / V, k = i - v * V;
            hp[i] = hop[(size_t)(v0 + v) * M + k];
            D[v * Vp + k] = d;
        }
        __syncthreads();
        for (int l = L; l >= 1; --l) {
            const float *hl = h + ((size_t)l * nV + v0) * M, *hq = h + ((size_t)(l - 1) * nV + v0) * M;
            const float *nl = n + ((size_t)(l - 1) * nV + v0) * M, *Fl = F + (size_t)(l - 1) * M * M;
            for (int i = tid; i < V * V; i += kBlock) {   // dz in place; n_l, F_l[:V, :V] (and h_{l-1}) staged
                const int v = i / V, k = i - v * V;
                const float a = hl[(size_t)v * M + k], dh = D[v * Vp + k];
                D[v * Vp + k] = (int)hp[i] <= l ? (a > 0.f ? dh : kSlope * dh) : 0.f;
                N[v * Vp + k] = nl[(size_t)v * M + k];
                Fs[v * Vp + k] = Fl[(size_t)v * M + k];
                if (PAIRS) P[v * Vp + k] = hq[(size_t)v * M + k];
            }
            __syncthreads();
            {   // dF_l[i][j] += sum_v dz_v[i] n_v[j]: this thread's elements of the image
                const size_t base = (size_t)FD + (size_t)(l - 1) * M * M;
                const int first = (int)(((size_t)tid + kBlock - base % kBlock) % kBlock);
                for (int r = first; r < M * M; r += kBlock) {
                    const int i = r / M, j = r - i * M;
                    if (i >= V || j >= V) continue;
                    float acc = 0.f;
                    for (int v = 0; v < V; ++v) acc = fmaf(D[v * Vp + i], N[v * Vp + j], acc);
                    img[base + r] += acc;
                }
            }
            if (PAIRS)
                for (int u = tid; u < V; u += kBlock) {
                    float acc = 0.f;
                    for (int k = 0; k < V; ++k) acc += P[u * Vp + k];
                    sv[u] = acc;
                }
            __syncthreads();
            for (int i = tid; i < V * V; i += kBlock) {   // dn_v = F_l^T dz_v over n_l: lanes over j
                const int v = i / V, j = i - v * V;
                float acc = 0.f;
                for (int k = 0; k < V; ++k) acc = fmaf(Fs[k * Vp + j], D[v * Vp + k], acc);
                N[v * Vp + j] = acc;
            }
            __syncthreads();
            if (PAIRS) {
                for (int i = tid; i < V * V; i += kBlock) {   // the pair dots <dn_v, h_u> over F_l's image, and E_{v,u}
                    const int v = i / V, u = i - v * V;
                    const long long e1 = nb_ptr[v0 + v + 1];
                    float ex = 0.f;
                    bool member = false;
                    for (long long e = nb_ptr[v0 + v]; e < e1; ++e) {
                        const int w = nb_idx[e] - v0;
                        if (w == u) member = true;
                        else ex += sv[w];
                    }
                    float q = 0.f;
                    if (member)
                        for (int k = 0; k < V; ++k) q = fmaf(N[v * Vp + k], P[u * Vp + k], q);
                    Fs[v * Vp + u] = q;
                    EX[v * Vp + u] = member ? ex : 0.f;
                }
                __syncthreads();
                for (int i = tid; i < V * V; i += kBlock) {   // c_{v,u}: the other members' dots, added directly
                    const int v = i / V, u = i - v * V;
                    const long long e1 = nb_ptr[v0 + v + 1];
                    float acc = 0.f;
                    bool member = false;
                    for (long long e = nb_ptr[v0 + v]; e < e1; ++e) {
                        const int w = nb_idx[e] - v0;
                        if (w == u) member = true;
                        else acc += Fs[v * Vp + w];
                    }
                    CC[v * Vp + u] = member ? acc : 0.f;
                }
                __syncthreads();
            }
            for (int i = tid; i < V * V; i += kBlock) {   // dh_{l-1}[u]: gathered over the consumers of u in ascending order
                const int u = i / V, j = i - u * V;
                const long long e1 = nb_tptr[v0 + u + 1];
                float acc = 0.f;
                for (long long e = nb_tptr[v0 + u]; e < e1; ++e) {
                    const int v = nb_tidx[e] - v0;
                    acc += PAIRS ? fmaf(N[v * Vp + j], EX[v * Vp + u], CC[v * Vp + u]) : N[v * Vp + j];
                }
                D2[u * Vp + j] = acc;
            }
            __syncthreads();
            float *t = D;
            D = D2;
            D2 = t;
        }
        for (int v = tid; v < V; v += kBlock) {   // VertexRepresentation::backward reads gradient[vertex] only
            const float dv = D[v * Vp + v];
            ds0[v0 + v] = dv;
            sv[V + v] = dv;
        }
        __syncthreads();
        if (x)
            for (int f = tid; f < FD; f += kBlock) {   // dH += sum_v dh_0[v][v] x[v]
                float acc = 0.f;
                for (int v = 0; v < V; ++v) acc = fmaf(sv[V + v], x[(size_t)(v0 + v) * FD + f], acc);
                img[f] += acc;
            }
    }
}

// grads[e] (+)= the images' element e in ascending order of the chunks
__global__ __launch_bounds__(kBlock) void cov_fold(const float *__restrict__ part, float *__restrict__ out, size_t image, size_t skip, size_t count,
                                                   int chunks, int accumulate) {
    const size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= count) return;
    float acc = accumulate ? out[e] : 0.f;
    for (int c = 0; c < chunks; ++c) acc += part[(size_t)c * image + skip + e];
    out[e] = acc;
}

int chunk_count(int nMol) { return nMol < kCovariantSplits ? nMol : kCovariantSplits; }

struct CovOperands {
    int form, L, M, nV, nMol, maxV;
    const int *mol_ptr;
    const long long *ptr, *tptr;
    const int *idx, *tidx;
    const unsigned char *hop;
};

gf_status fwd_launch(gf_ctx *ctx, const CovOperands &o, const float *s0, const float *x, const float *Hw, int FD, const float *F,
                     const float *target, float *h, float *n, float *g, float *yhat, float *loss, float *dy) {
    const size_t bytes = smp_covariant_lds_bytes(o.maxV);
    const bool pairs = o.form == 2;
    gf_status st = pairs ? opt_in_lds(ctx, cov_network_fwd<true>, bytes) : opt_in_lds(ctx, cov_network_fwd<false>, bytes);
    if (st != GF_OK) return st;
    if (pairs)
        GF_LAUNCH(ctx, "cov_network_fwd", cov_network_fwd<true>, dim3((unsigned)o.nMol), dim3(kBlock), bytes, o.mol_ptr, o.ptr, o.idx, o.hop, s0, x, Hw,
                  FD, F, target, h, n, g, yhat, loss, dy, o.L, o.M, o.nV);
    else
        GF_LAUNCH(ctx, "cov_network_fwd", cov_network_fwd<false>, dim3((unsigned)o.nMol), dim3(kBlock), bytes, o.mol_ptr, o.ptr, o.idx, o.hop, s0, x, Hw,
                  FD, F, target, h, n, g, yhat, loss, dy, o.L, o.M, o.nV);
    return GF_OK;
}

// the reverse launch into the workspace's images, then the fold: dH (FD floats, NULL x: none) and dF [L][M][M], each `+=` where accumulate
gf_status bwd_launch(gf_ctx *ctx, const CovOperands &o, const float *x, int FD, const float *F, const float *h, const float *n, const float *dy,
                     float *dH, float *dF, float *ds0, int accumulate) {
    const size_t bytes = smp_covariant_lds_bytes(o.maxV), nF = (size_t)o.L * o.M * o.M, image = (size_t)FD + nF;
    const int chunks = chunk_count(o.nMol), per = (o.nMol + chunks - 1) / chunks, used = (o.nMol + per - 1) / per;
    const bool pairs = o.form == 2;
    gf_status st = ensure_ws(ctx, smp_covariant_ws_bytes(o.nMol, image));
    if (st == GF_OK) st = pairs ? opt_in_lds(ctx, cov_network_bwd<true>, bytes) : opt_in_lds(ctx, cov_network_bwd<false>, bytes);
    if (st != GF_OK) return st;
    float *part = static_cast<float *>(ctx->ws);
    if (pairs)
        GF_LAUNCH(ctx, "cov_network_bwd", cov_network_bwd<true>, dim3((unsigned)used), dim3(kBlock), bytes, o.mol_ptr, o.ptr, o.idx, o.tptr, o.tidx, o.hop,
                  x, FD, F, h, n, dy, part, ds0, o.L, o.M, o.nV, o.nMol, per, o.maxV);
    else
        GF_LAUNCH(ctx, "cov_network_bwd", cov_network_bwd<false>, dim3((unsigned)used), dim3(kBlock), bytes, o.mol_ptr, o.ptr, o.idx, o.tptr, o.tidx,
                  o.hop, x, FD, F, h, n, dy, part, ds0, o.L, o.M, o.nV, o.nMol, per, o.maxV);
    // dH given: a handle's gradient vector, dF directly behind dH -- the image's own layout, one fold; else dF alone
    float *dst = dH ? dH : dF;
    const size_t skip = dH ? 0 : (size_t)FD, count = dH ? image : nF;
    if (count)
        GF_LAUNCH(ctx, "cov_fold", cov_fold, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, part, dst, image, skip, count, used,
                  accumulate);
    return GF_OK;
}

CovOperands of_handle(const gf_smp *s) {
    return CovOperands{s->cfg.covariant, s->cfg.nLevels, s->cfg.max_nVertices, s->lay.level[0].nNodes, s->lay.nMol, s->lay.max_vertices,
                       s->mol_ptr, s->cov_ptr, s->cov_tptr, s->cov_idx, s->cov_tidx, s->cov_hop};
}

}  // namespace

size_t smp_covariant_ws_bytes(int nMol, size_t image_floats) { return sizeof(float) * (size_t)chunk_count(nMol < 1 ? 1 : nMol) * image_floats + 256; }

gf_status smp_covariant_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature) {
    gf_ctx *ctx = s->ctx;
    const int FD = s->cfg.fdim(), M = s->cfg.max_nVertices;
    const gf_status st = fwd_launch(ctx, of_handle(s), nullptr, s->x, params, FD, params + FD, targets, s->cov_h, s->cov_n, s->g, s->yhat, loss, s->dy);
    return st == GF_OK ? finish_forward(s, targets != nullptr, predict, graph_feature, M) : st;
}

// The reverse sweep from the loss of the last forward; nothing a second sweep needs is overwritten.
gf_status smp_covariant_backward(gf_smp *s, const float *params, float *grads, int accumulate) {
    const int FD = s->cfg.fdim();
    const gf_status st = bwd_launch(s->ctx, of_handle(s), s->x, FD, params + FD, s->cov_h, s->cov_n, s->dy, grads, grads + FD, s->cov_ds0, accumulate);
    if (st == GF_OK) mark_used(s);
    return st;
}

}  // namespace gf

// ---- the two network kernels as stand-alone operators (include/gf_hip.h; tests/test_cgcn_ops_gpu.py) ----
namespace {

// The operands of a stand-alone call, checked on the host (blocking copies: these are test operators).  mol_ptr from 0, never decreasing,
// ending at nV, every molecule within M vertices; a list from 0, never decreasing, every entry inside its vertex's own molecule and a
// vertex's entries strictly ascending (a set: the kernels index a molecule's LDS images with them).  *maxV: the largest molecule.
gf_status check_cov_list(gf_ctx *ctx, const char *who, const char *what, const std::vector<int> &mp, int nV, const long long *ptr, const int *idx) {
    std::vector<long long> p((size_t)nV + 1);
    GF_HIP_TRY(ctx, hipMemcpyAsync(p.data(), ptr, sizeof(long long) * p.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (p[0] != 0) return gf::fail(ctx, GF_ERR_INVALID, "%s: %s starts at %lld, not at 0", who, what, p[0]);
    for (int v = 0; v < nV; ++v)
        if (p[(size_t)v + 1] < p[(size_t)v]) return gf::fail(ctx, GF_ERR_INVALID, "%s: %s decreases at entry %d", who, what, v + 1);
    if (p[(size_t)nV] > 0x7fffffffll) return gf::fail(ctx, GF_ERR_INVALID, "%s: %s ends at %lld: more than 2^31 entries", who, what, p[(size_t)nV]);
    std::vector<int> hi((size_t)p[(size_t)nV]);
    if (!hi.empty()) {
        GF_HIP_TRY(ctx, hipMemcpyAsync(hi.data(), idx, sizeof(int) * hi.size(), hipMemcpyDeviceToHost, ctx->stream));
        GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (size_t m = 0; m + 1 < mp.size(); ++m)
        for (int v = mp[m]; v < mp[m + 1]; ++v)
            for (long long e = p[(size_t)v]; e < p[(size_t)v + 1]; ++e) {
                const int u = hi[(size_t)e];
                if (u < mp[m] || u >= mp[m + 1])
                    return gf::fail(ctx, GF_ERR_INVALID, "%s: %s entry %lld of vertex %d is vertex %d, outside its molecule %zu (%d .. %d)", who, what, e, v, u,
                                    m, mp[m], mp[m + 1] - 1);
                if (e > p[(size_t)v] && u <= hi[(size_t)e - 1])
                    return gf::fail(ctx, GF_ERR_INVALID, "%s: the %s entries of vertex %d do not ascend at entry %lld", who, what, v, e);
            }
    return GF_OK;
}

gf_status check_cov_operands(gf_ctx *ctx, const char *who, int form, int L, int M, int nV, int nMol, const int *mol_ptr, const long long *ptr,
                             const int *idx, const long long *tptr, const int *tidx, int *maxV) {
    if (form < 1 || form > 2) return gf::fail(ctx, GF_ERR_INVALID, "%s: form = %d (1: the sum aggregate, 2: RisiLayer2D)", who, form);
    if (L < 0 || L > 64) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d levels (0 .. 64)", who, L);
    if (M < 1 || M > gf::kCovariantMaxVertices) return gf::fail(ctx, GF_ERR_INVALID, "%s: M = %d (1 .. %d)", who, M, gf::kCovariantMaxVertices);
    if (nV < 1 || nMol < 1) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d vertices, %d molecules", who, nV, nMol);
    if ((unsigned long long)nV * (unsigned long long)M * (unsigned long long)(L + 1) > 0x7fffffffull)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: (L + 1) nV M = %llu activations (below 2^31)", who,
                        (unsigned long long)nV * (unsigned long long)M * (unsigned long long)(L + 1));
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<int> mp((size_t)nMol + 1);
    GF_HIP_TRY(ctx, hipMemcpyAsync(mp.data(), mol_ptr, sizeof(int) * mp.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (mp[0] != 0) return gf::fail(ctx, GF_ERR_INVALID, "%s: mol_ptr starts at %d, not at 0", who, mp[0]);
    *maxV = 1;
    for (int m = 0; m < nMol; ++m) {
        const int V = mp[(size_t)m + 1] - mp[(size_t)m];
        if (V < 0) return gf::fail(ctx, GF_ERR_INVALID, "%s: mol_ptr decreases at entry %d", who, m + 1);
        if (V > M) return gf::fail(ctx, GF_ERR_INVALID, "%s: molecule %d has %d vertices, M = %d", who, m, V, M);
        *maxV = V > *maxV ? V : *maxV;
    }
    if (mp[(size_t)nMol] != nV) return gf::fail(ctx, GF_ERR_INVALID, "%s: mol_ptr ends at %d, the call has %d vertices", who, mp[(size_t)nMol], nV);
    gf_status st = check_cov_list(ctx, who, "nb_ptr / nb_idx", mp, nV, ptr, idx);
    if (st == GF_OK && tptr) st = check_cov_list(ctx, who, "nb_tptr / nb_tidx", mp, nV, tptr, tidx);
    return st;
}

}  // namespace

extern "C" {

gf_status gf_smp_covariant_forward_ex_f32(gf_ctx *ctx, int form, int L, int M, int nV, int nMol, const int *mol_ptr, const long long *nb_ptr,
                                          const int *nb_idx, const unsigned char *hop, const float *s0, const float *F, const float *target,
                                          float *h, float *n, float *g, float *yhat, float *loss, float *dy) {
    static const char *who = "gf_smp_covariant_forward_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (!mol_ptr || !nb_ptr || !nb_idx || !hop || !s0 || (L > 0 && (!F || !n)) || !h || !g || !yhat)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    int maxV = 1;
    const gf_status st = check_cov_operands(ctx, who, form, L, M, nV, nMol, mol_ptr, nb_ptr, nb_idx, nullptr, nullptr, &maxV);
    if (st != GF_OK) return st;
    const gf::CovOperands o = {form, L, M, nV, nMol, maxV, mol_ptr, nb_ptr, nullptr, nb_idx, nullptr, hop};
    return gf::fwd_launch(ctx, o, s0, nullptr, nullptr, 0, F, target, h, n, g, yhat, loss, dy);
}

gf_status gf_smp_covariant_backward_ex_f32(gf_ctx *ctx, int form, int L, int M, int nV, int nMol, const int *mol_ptr, const long long *nb_ptr,
                                           const int *nb_idx, const long long *nb_tptr, const int *nb_tidx, const unsigned char *hop,
                                           const float *F, const float *h, const float *n, const float *dy, float *dF, float *ds0) {
    static const char *who = "gf_smp_covariant_backward_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (!mol_ptr || !nb_ptr || !nb_idx || !nb_tptr || !nb_tidx || !hop || (L > 0 && (!F || !n || !dF)) || !h || !dy || !ds0)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    int maxV = 1;
    const gf_status st = check_cov_operands(ctx, who, form, L, M, nV, nMol, mol_ptr, nb_ptr, nb_idx, nb_tptr, nb_tidx, &maxV);
    if (st != GF_OK) return st;
    const gf::CovOperands o = {form, L, M, nV, nMol, maxV, mol_ptr, nb_ptr, nb_tptr, nb_idx, nb_tidx, hop};
    return gf::bwd_launch(ctx, o, nullptr, 0, F, h, n, dy, nullptr, dF, ds0, /*accumulate=*/1);
}

}  // extern "C"
