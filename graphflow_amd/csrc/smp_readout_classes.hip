// smp_readout_classes.hip -- the multi-class read-out of the SMP_2D_ver6 / ver7 classification models (gf_smp_create_classifier).
//
// Above graph_feature the reference's classifiers (GraphFlow/SMP_2D_ver6_classification.h:189-200, :560-563, :699-713; ver7 alike) replace
// the regression head  y = InnerProduct(g, W[C]) -> SquaredLoss  by
//   z = MatVecMul(W[nClass][C], g)                                    (MatVecMul.h: z_c = <W[c], g>; dW[c][f] += dz_c g_f; dg_f += sum_c dz_c W[c][f])
//   p = softmax(z), value = log p[label] (<= 0), LOG_ZERO = -256 where p[label] underflows     (LogLoss.h:37-62)
//   dz_c = p_c - [c == label]                                                                   (LogLoss.h:64-76)
//   Predict = the first arg-max of z (strict `>`, :706-712)
// Everything below graph_feature is shared with the regression models.  The regression read-out sends  dy[mol] * W[f]  down into the top
// level; here that vector is  dg[mol][f] = sum_c dz[mol][c] W[c][f], stored per molecule, and the two kernels that broadcast it (per node
// for a fused top level, per row for an op-by-op one) are twins of readout_backward_nodevec / readout_backward_nodes (smp.hip).
// Every reduction has a fixed order (no float atomics): two runs give the same bits.
#include "smp_internal.h"

namespace gf {
namespace {

constexpr float kAlpha = 0.01f;          // LeakyReLU.h default (the read-out's activation)
constexpr float kLogZero = -256.f;       // LogLoss.h:20
// exp(d) in the reference's fp64 is 0 -- and LogLoss::forward returns LOG_ZERO -- once d < ln(2^-1075)
constexpr float kExpUnderflowF64 = -745.13321f;

// One workgroup (4 waves) per molecule.  LDS: g [C] | z [nClass] | dz [nClass].
//   g = sum_v vf (SumVectors), z_c = <W[c], g> one wave per class in turn, softmax / arg-max / loss from the z in LDS, dz, dg.
// The loss is (z_label - max) - log(sum exp(z - max)): a log of the fp32 probability would be -inf from a gap of ~104 on, where the
// reference's fp64 still holds a finite value up to ~745.
// target == nullptr (Predict / Feature): scores, probabilities and predict only; dz = dg = 0.
// A label outside [0, nClass) (NaN included): loss = NaN, dz = dg = 0 -- the molecule contributes no gradient, nothing is indexed by it.
__global__ __launch_bounds__(256) void readout_molecules_classes(const float *__restrict__ vf, const int *__restrict__ mol_ptr,
                                                                 const int *__restrict__ mol_nodes, const float *__restrict__ W,
                                                                 const float *__restrict__ target, float *__restrict__ g,
                                                                 float *__restrict__ scores, float *__restrict__ prob, float *__restrict__ dz,
                                                                 float *__restrict__ dg, float *__restrict__ predict, float *__restrict__ loss,
                                                                 int C, int nClass) {
    extern __shared__ float lds[];
    float *sg = lds, *sz = lds + C, *sdz = sz + nClass;
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = (int)blockDim.x >> 6;
    for (int f = tid; f < C; f += blockDim.x) {
        float acc = 0.f;
        for (int k = mol_ptr[m]; k < mol_ptr[m + 1]; ++k) acc += vf[(size_t)mol_nodes[k] * C + f];
        g[(size_t)m * C + f] = acc;
        sg[f] = acc;
    }
    __syncthreads();
    for (int c = wave; c < nClass; c += nwaves) {
        const float *w = W + (size_t)c * C;
        float part = 0.f;
        for (int f = lane; f < C; f += 64) part += w[f] * sg[f];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);   // (butterfly: the same tree on every lane, every run)
        if (lane == 0) sz[c] = part;
    }
    __syncthreads();
    // every thread walks the nClass logits in the same order (LDS broadcasts): no second reduction, no divergence between threads
    float zmax = sz[0];
    int best = 0;
    for (int c = 1; c < nClass; ++c) {
        const float z = sz[c];
        if (z > zmax) zmax = z, best = c;   // strict: the lowest index wins a tie (Predict, :706-712)
    }
    float sum = 0.f;
    for (int c = 0; c < nClass; ++c) sum += expf(sz[c] - zmax);
    const float t = target ? target[m] : -1.f;
    const bool valid = target && t >= 0.f && t < (float)nClass;   // (false for NaN)
    const int label = valid ? (int)t : -1;                        // (int)target, LogLoss.h:38
    for (int c = tid; c < nClass; c += blockDim.x) {
        const float z = sz[c], p = expf(z - zmax) / sum;
        if (scores) scores[(size_t)m * nClass + c] = z;
        if (prob) prob[(size_t)m * nClass + c] = p;
        const float d = valid ? p - (c == label ? 1.f : 0.f) : 0.f;
        dz[(size_t)m * nClass + c] = d;
        sdz[c] = d;
    }
    if (tid == 0) {
        if (predict) predict[m] = (float)best;
        if (loss && target) {
            float v = __builtin_nanf("");
            if (valid) {
                const float gap = sz[label] - zmax;
                v = gap < kExpUnderflowF64 ? kLogZero : gap - logf(sum);
            }
            loss[m] = v;
        }
    }
    __syncthreads();
    for (int f = tid; f < C; f += blockDim.x) {
        float acc = 0.f;
        for (int c = 0; c < nClass; ++c) acc += sdz[c] * W[(size_t)c * C + f];
        dg[(size_t)m * C + f] = acc;
    }
}

// dW[c][f] += sum_m dz[m][c] g[m][f]   (MatVecMul::backward, the matrix operand).  Grid (f tiles of 16, c); 16 groups of 16 lanes take the
// molecules m = r, r + 16, ... in order, then the sixteen partial sums are folded in a fixed tree.
__global__ __launch_bounds__(256) void readout_dW_classes(const float *__restrict__ dz, const float *__restrict__ g, float *__restrict__ dW, int C,
                                                          int nClass, int nMol) {
    __shared__ float red[256];
    const int c = blockIdx.y, fl = threadIdx.x & 15, r = threadIdx.x >> 4, f = blockIdx.x * 16 + fl;
    float acc = 0.f;
    if (f < C)
        for (int m = r; m < nMol; m += 16) acc += dz[(size_t)m * nClass + c] * g[(size_t)m * C + f];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 8; st > 0; st >>= 1) {   // rows r and r + st: the same pairs on every run
        if (r < st) red[threadIdx.x] += red[threadIdx.x + st * 16];
        __syncthreads();
    }
    if (r == 0 && f < C) dW[(size_t)c * C + f] += red[fl];
}

// df_L[n][i][j][:] = dg[mol(n)][:] * lrelu'(sh[n][:])   (MatVecMul's vector operand -> SumVectors -> LeakyReLU -> ShrinkTensor::backward)
__global__ void readout_backward_nodes_classes(const float *__restrict__ dg, const float *__restrict__ sh, const int *__restrict__ node_mol,
                                               const int *__restrict__ node_s, const long long *__restrict__ node_row, float *__restrict__ dfL,
                                               int C) {
    const int n = blockIdx.x;
    const int s = node_s[n];
    float *dst = dfL + node_row[n] * C;
    const float *d = dg + (size_t)node_mol[n] * C;
    const int total = s * s * C;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int f = i % C;
        dst[i] = d[f] * (sh[(size_t)n * C + f] > 0.f ? 1.f : kAlpha);
    }
}

// the same per node only (the fused top level adds the vector to every row of the node itself)
__global__ void readout_backward_nodevec_classes(const float *__restrict__ dg, const float *__restrict__ sh, const int *__restrict__ node_mol,
                                                 float *__restrict__ dsh, int C, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % C);
        const size_t n = i / C;
        dsh[i] = dg[(size_t)node_mol[n] * C + f] * (sh[i] > 0.f ? 1.f : kAlpha);
    }
}

}  // namespace

// W [nClass][C] in the device's layout (C = gf_smp::cfg.top_channels(): nChanels -- padded channels carry zero weights -- or, for the
// channel-doubling first-order forms SMP_1D_ver2 / ver3, the top level's width)
gf_status readout_classes_forward(gf_smp *s, const float *W, const float *targets, float *predict, float *loss) {
    gf_ctx *ctx = s->ctx;
    const int C = s->cfg.top_channels(), nClass = s->cfg.nClass, nMol = s->lay.nMol;
    const size_t lds = sizeof(float) * ((size_t)C + 2 * (size_t)nClass);
    if (lds > 48 * 1024) return fail(ctx, GF_ERR_UNSUPPORTED, "classifier read-out: %d channels and %d classes exceed its LDS image", C, nClass);
    GF_LAUNCH(ctx, "smp_readout_mol_classes", readout_molecules_classes, dim3(nMol), dim3(256), lds, s->vf, s->mol_ptr, s->mol_nodes, W, targets, s->g,
              s->cls_scores, s->cls_prob, s->cls_dz, s->cls_dg, predict, loss, C, nClass);
    return GF_OK;
}

gf_status readout_classes_dW(gf_smp *s, float *dW) {
    const int C = s->cfg.top_channels(), nClass = s->cfg.nClass;
    GF_LAUNCH(s->ctx, "smp_readout_dW_classes", readout_dW_classes, dim3((unsigned)((C + 15) / 16), (unsigned)nClass), dim3(256), 0, s->cls_dz, s->g, dW, C,
              nClass, s->lay.nMol);
    return GF_OK;
}

// per_node: into gf_smp::dsh [nodes][C] for a fused top level; else into df_L at every (i, j) of every node
gf_status readout_classes_backward(gf_smp *s, bool per_node) {
    gf_ctx *ctx = s->ctx;
    const int L = s->cfg.nLevels, C = s->cfg.top_channels();
    const int nodes = s->lay.level[L].nNodes;
    const size_t total = (size_t)nodes * C;
    if (per_node) {
        const size_t blocks = (total + 255) / 256;
        GF_LAUNCH(ctx, "smp_readout_bwd_classes", readout_backward_nodevec_classes, dim3((unsigned)(blocks > 1048576 ? 1048576 : blocks ? blocks : 1)),
                  dim3(256), 0, s->cls_dg, s->sh, s->top_node_mol, s->dsh, C, total);
    } else {
        GF_LAUNCH(ctx, "smp_readout_bwd_classes", readout_backward_nodes_classes, dim3(nodes), dim3(256), 0, s->cls_dg, s->sh, s->top_node_mol,
                  s->lv[L].node_s, s->lv[L].node_row, s->lv[L].df, C);
    }
    return GF_OK;
}

}  // namespace gf
