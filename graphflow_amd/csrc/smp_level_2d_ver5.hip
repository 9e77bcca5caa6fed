// smp_level_2d_ver5.hip -- what SMP_2D_ver5 (GraphFlow/SMP_2D_ver5.h:135-137, 581-609; gfsmp::Config::steerable_2d = 5) adds to the steerable
// level of smp_level_2d.hip: SMP_2D_ver4's level at a constant channel count C, the 2 C concatenated channels projected back to C by a
// learned K_l [C][2 C] = [K1 | K2] (CustomMatMulTensor).  Fields, children, pi / inv, buckets, multiplicities and the reduced adjacency
// are ver4's.  Per channel vector, with S and col as in smp_level_2d.hip:
//   u[j]    = K2 (lambda2_s . col[j]) + b_s                                  on the sum s columns of the level
//   z[i][j] = K1 (lambda1_s . S[i][j]) + u[j],   f_l = LeakyReLU3D(z)        on its sum s^2 rows: the one matrix product of the family
// Forward: store_S (the gather of smp_level_2d.hip's pass 1: S, col and the row / column tables, nothing of f_l), col_proj (u), row_proj
// (32-row tiles on v_mfma_f32_32x32x2_f32, K1 staged once per workgroup in LDS and zero-padded to 32 in both dimensions, lambda1_s applied
// per ROW while the operand is loaded -- a tile spans nodes of different sizes --, u[j], LeakyReLU and the store of f_l in the epilogue).
// S is read once, f_l written once; the 2 C-wide concatenation never exists in memory.
// Backward: dz in place from the sign of f_l with cz[j] = sum_i dz[i][j] (dz); dE = dz K1 (row_proj with the transposed image); dO[j] =
// cz[j] K2 (col_proj); dK1 = sum_rows dz^T (lambda1_s . S), dK2 = sum_columns cz^T (lambda2_s . col) as MFMA reductions over fixed chunks
// (kV5Chunk rows each, interleaved), one partial image per chunk, folded in chunk order (wgrad, wgrad_fold); dS = lambda1_s . dE + lambda2_s . dO[j] over
// dz in df_l with the column partials of smp_level_2d.hip's layout (combine); then its bucket partials, finish and the df_{l-1} gather.
// K_l is ONE node of the reference's graph (added in the preamble) and every vertex's CustomMatMulTensor adds into K_l->gradient itself:
// dK_l is the plain derivative, unlike dlambda (th_weight = j, through the shared W_eye[s] / W_one[s]).
// fp32 operands and accumulation throughout; no atomics, every sum in a fixed order; every buffer written before it is read.
// The projections and the weight gradients are also operators of the C ABI on caller-supplied operands (gf_smp_2d_ver5_rows_ex_f32,
// _cols_ex_f32, _wgrad_ex_f32 at the end of this file): what tests/test_smp_2d_ver5_ops_gpu.py holds to the fp64 product row by row.
#include "smp_field_level.h"

namespace gf {
using namespace field_level;
namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

constexpr int kV5Chunk = 512;    // rows (columns) per partial image of dK1 (dK2): a level of n rows writes ceil(n / kV5Chunk) images
constexpr int kV5Steps = 8;      // MFMA steps of two rows whose operands a wave of wgrad loads together
constexpr int kV5FoldGroups = 16;   // runs of consecutive partial images the fold sums side by side before it adds the runs in order

// Pass 1 of smp_level_2d.hip's forward, storing only: items (node, column j, vector q); S[i][j] gathered, + scalar adj, stored and summed
// into col[j].  Also the tables the projections read: row_cs[row] = (column index, s) by the lane of the row's first vector, col_s[column].
template <int V>
__global__ __launch_bounds__(256) void v5_store_S(const float *__restrict__ fp, const float *__restrict__ scalar, const float *__restrict__ adj,
                                                  float *__restrict__ S, float *__restrict__ col, int2 *__restrict__ row_cs, int *__restrict__ col_s,
                                                  const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                                  const long long *__restrict__ node_pair, const long long *__restrict__ child_ptr,
                                                  const long long *__restrict__ src_row, const int *__restrict__ src_s,
                                                  const long long *__restrict__ pi_off, const short *__restrict__ pi, int C, int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const Run run = pack_run(off, node_s, nodes, npw, C / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, C / V);
        const int n = run.nb + x.j, s = node_s[n], j = x.pos, cq = x.cq;
        const long long r0 = node_row[n], e0 = child_ptr[n], e1 = child_ptr[n + 1], cj = node_pair[n] + j;
        const Vf<V> sc = vld<V>(scalar + cq);
        Vf<V> cs = vzero<V>();
        for (int i = 0; i < s; ++i) {
            Vf<V> a = gather_pair<V>(fp, C, cq, e0, e1, src_row, src_s, pi_off, pi, i, j);
            const long long row = r0 + (long long)i * s + j;
            const float av = adj[row];
#pragma unroll
            for (int c = 0; c < V; ++c) a.v[c] += sc.v[c] * av;
            vst<V>(S + row * C + cq, a);
            vadd(cs, a);
            if (cq == 0) row_cs[row] = make_int2((int)cj, s);
        }
        vst<V>(col + cj * C + cq, cs);
        if (cq == 0) col_s[cj] = s;
    }
}

// The products on the sum s columns.  M [C][C] in LDS with out[o] = sum_k x[k] M[k][o]:
//   forward  (fwd = 1): x = lambda2_s . col[j],  M[d][c'] = K2[c'][d],  out = u[j] = x M + b_s
//   backward (fwd = 0): x = cz[j] (rows of `in` are ldin floats apart),  M[c'][d] = K2[c'][d],  out = dO[j]
// K2 = the right half of K [C][2 C].  Items (column, o), grid-stride; the lanes of a column read the same x: broadcast loads.
__global__ __launch_bounds__(256) void v5_col_proj(const float *__restrict__ K, const float *__restrict__ in, int ldin, const float *__restrict__ sizes,
                                                   const int *__restrict__ col_s, float *__restrict__ out, long long cols, int C, int fwd) {
    extern __shared__ float Ms[];
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
        const int k = i / C, o = i - k * C;
        Ms[i] = fwd ? K[(size_t)o * 2 * C + C + k] : K[(size_t)k * 2 * C + C + o];
    }
    __syncthreads();
    const long long total = cols * C;
    for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
        const long long cj = it / C;
        const int o = (int)(it - cj * C);
        const float *x = in + cj * ldin;
        float a = 0.f;
        if (fwd) {
            const float *se = size_entry_v5(sizes, col_s[cj], C);
            for (int k = 0; k < C; ++k) a += (se[C + k] * x[k]) * Ms[k * C + o];
            a += se[2 * C + o];
        } else {
            for (int k = 0; k < C; ++k) a += x[k] * Ms[k * C + o];
        }
        out[cj * C + o] = a;
    }
}

// The product on the sum s^2 rows: out[row][o] = sum_k x[row][k] M[o][k], 32-row tiles, one per wave, grid-stride over the tiles.
//   forward  (FWD): x = lambda1_s(row) . S[row],  M[c'][d] = K1[c'][d],  out = f_l = LeakyReLU(x M^T + u[column of the row])
//   backward      : x = dz[row],                  M[d][c'] = K1[c'][d],  out = dE
// M sits in LDS as [CP][CP + 4], CP = 32 NT >= C, zero outside C x C (the + 4: the lanes of a 16 B read spread over the banks).
// v_mfma_f32_32x32x2_f32 with the image as the A operand (rows o) and the tile as B (columns = the tile's rows): lane (li = lane & 31,
// lh = lane >> 5) loads x[row li][8 t + 4 lh .. + 3] in one 16 B load and feeds it to steps q = 0 .. 3 against M[o][8 t + 4 lh + q] -- the
// order of the reduction index inside a step is free as long as both operands agree.  The accumulator's register r holds o = 8 (r >> 2)
// + 4 lh + (r & 3) of row li: four consecutive channels per lane, 16 B stores.  VEC: 4 | C (else scalar loads and stores, guarded).
template <int NT, bool VEC, bool FWD>
__global__ __launch_bounds__(256) void v5_row_proj(const float *__restrict__ K, const float *__restrict__ X, const float *__restrict__ sizes,
                                                   const float *__restrict__ u, const int2 *__restrict__ row_cs, float *__restrict__ out,
                                                   long long rows, int C, float alpha) {
    constexpr int CP = 32 * NT, LD = CP + 4;
    extern __shared__ float Ms[];
    for (int i = threadIdx.x; i < CP * CP; i += blockDim.x) {
        const int o = i / CP, k = i - o * CP;
        float v = 0.f;
        if (o < C && k < C) v = FWD ? K[(size_t)o * 2 * C + k] : K[(size_t)k * 2 * C + o];
        Ms[o * LD + k] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5, wave = threadIdx.x >> 6;
    const long long ntiles = (rows + 31) / 32;
    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long long)gridDim.x * 4) {
        const long long row = tile * 32 + li;
        const bool valid = row < rows;
        int2 cs = make_int2(0, 1);
        if (valid && FWD) cs = row_cs[row];
        // (operands outside the level / C: read at a clamped address -- written data, finite -- and multiplied by 0, so that the loads
        //  of a tile sit in one block and are issued together instead of one guarded branch each)
        const float *xr = X + (valid ? row : rows - 1) * C, *lam = size_entry_v5(sizes, cs.y, C);
        const float mv = valid ? 1.f : 0.f;
        f16v acc[NT];
#pragma unroll
        for (int m = 0; m < NT; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
#pragma unroll
        for (int t = 0; t < CP / 8; ++t) {
            const int d0 = 8 * t + 4 * lh;
            f4v x;
            if (VEC) {   // (4 | C: a chunk is inside C or outside)
                const int dc = d0 < C ? d0 : 0;
                x = *reinterpret_cast<const f4v *>(xr + dc) * (d0 < C ? mv : 0.f);
                if (FWD) x *= *reinterpret_cast<const f4v *>(lam + dc);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int dc = d0 + q < C ? d0 + q : 0;
                    x[q] = xr[dc] * (d0 + q < C ? mv : 0.f);
                    if (FWD) x[q] *= lam[dc];
                }
            }
#pragma unroll
            for (int m = 0; m < NT; ++m) {
                const f4v a = *reinterpret_cast<const f4v *>(Ms + (32 * m + li) * LD + d0);
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], x[q], acc[m], 0, 0, 0);
            }
        }
        if (!valid) continue;
        const float *ur = FWD ? u + (long long)cs.x * C : nullptr;
        float *orow = out + row * C;
#pragma unroll
        for (int m = 0; m < NT; ++m)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int o0 = 32 * m + 8 * g + 4 * lh;
                f4v z = {acc[m][4 * g], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]};
                if (VEC) {
                    if (o0 >= C) continue;
                    if (FWD) {
                        z += *reinterpret_cast<const f4v *>(ur + o0);
#pragma unroll
                        for (int q = 0; q < 4; ++q) z[q] = z[q] > 0.f ? z[q] : alpha * z[q];
                    }
                    *reinterpret_cast<f4v *>(orow + o0) = z;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (o0 + q >= C) continue;
                        float v = z[q];
                        if (FWD) {
                            v += ur[o0 + q];
                            v = v > 0.f ? v : alpha * v;
                        }
                        orow[o0 + q] = v;
                    }
                }
            }
    }
}

// dz = (df_l (has_df) + dvec[n] (the read-out's gradient, one vector per node, optional)) * lrelu'(f_l) over df_l, and cz[j] = sum_i
// dz[i][j] into the first C floats of the column's partial (part rows are 4 C floats: smp_level_2d.hip's [db | dlambda1 | dlambda2 |
// dscalar]).  Items (node, column j, vector q).  df is read back by the lane that wrote it: not __restrict__.
template <int V>
__global__ __launch_bounds__(256) void v5_dz(const float *__restrict__ f, float *df, const float *__restrict__ dvec, float *__restrict__ part,
                                             const int *__restrict__ node_s, const long long *__restrict__ node_row,
                                             const long long *__restrict__ node_pair, int C, float alpha, int nodes, int npw, int has_df) {
    __shared__ int off[kMaxPack + 1];
    const Run run = pack_run(off, node_s, nodes, npw, C / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, C / V);
        const int n = run.nb + x.j, s = node_s[n], j = x.pos, cq = x.cq;
        const long long r0 = node_row[n];
        Vf<V> dv = vzero<V>(), cz = vzero<V>();
        if (dvec) dv = vld<V>(dvec + (long long)n * C + cq);
        for (int i = 0; i < s; ++i) {
            const long long o = (r0 + (long long)i * s + j) * C + cq;
            const Vf<V> d = dz_of<V>(f, df, o, dv, has_df, alpha);
            vadd(cz, d);
            vst<V>(df + o, d);
        }
        vst<V>(part + (node_pair[n] + j) * 4 * C + cq, cz);
    }
}

// Partial image `chunk` of dK = sum_r A[r]^T (lambda_s(r) . B[r]) over the chunk's rows of A (lda floats apart) and B (C apart):
// part[chunk][c'][d].  With n = gridDim.x chunks (ceil(rows / kV5Chunk): a function of the level alone), chunk c owns the groups of
// 2 kV5Steps rows c, c + n, c + 2 n, .. -- interleaved, so that the workgroups running side by side stream one contiguous region instead
// of n addresses a whole chunk apart.  lambda_s(r) = the size entry of sz[r * sz_stride + sz_off] at lam_off (0: lambda1, C: lambda2).  Wave m of
// the workgroup's NT holds the image's rows c' in [32 m, + 32) as NT accumulators: A as the MFMA's A operand (lane li: channel 32 m + li
// of the step's row lh), B as its B operand (lane li: channel 32 n + li of the same row).  The rows of a chunk are summed in ascending order.
template <int NT>
__global__ __launch_bounds__(64 * NT) void v5_wgrad(const float *__restrict__ A, int lda, const float *__restrict__ B, const float *__restrict__ sizes,
                                                    int lam_off, const int *__restrict__ sz, int sz_stride, int sz_off, float *__restrict__ part,
                                                    long long rows, int C) {
    const int lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5, m = threadIdx.x >> 6;
    f16v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    // kV5Steps MFMA steps (one group of 2 kV5Steps rows) per trip, their loads issued together: a row or channel outside the level / C is
    // read at a clamped address (written data: finite) and multiplied by 0 -- a guard around the load makes the compiler branch around
    // every one of them and wait for each in turn (measured at 64 channels on the cfg3 batch: 4.1 ms for the level's six launches)
    const int ca = 32 * m + li, cac = ca < C ? ca : 0;
    const float ma = ca < C ? 1.f : 0.f;
    float mb[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) mb[n] = 32 * n + li < C ? 1.f : 0.f;
    // (the sizes of a group's rows are fetched one trip ahead: the lambda loads depend on them, and would add a round trip to every trip)
    const long long stride = (long long)gridDim.x * 2 * kV5Steps;
    int sc[kV5Steps];
#pragma unroll
    for (int k = 0; k < kV5Steps; ++k) {
        const long long r = (long long)blockIdx.x * 2 * kV5Steps + 2 * k + lh;
        sc[k] = sz[(r < rows ? r : rows - 1) * sz_stride + sz_off];
    }
    for (long long rb = (long long)blockIdx.x * 2 * kV5Steps; rb < rows; rb += stride) {
        float a[kV5Steps], b[kV5Steps][NT];
        int sn[kV5Steps];
#pragma unroll
        for (int k = 0; k < kV5Steps; ++k) {
            const long long r = rb + stride + 2 * k + lh;
            sn[k] = sz[(r < rows ? r : rows - 1) * sz_stride + sz_off];
        }
#pragma unroll
        for (int k = 0; k < kV5Steps; ++k) {
            const long long r = rb + 2 * k + lh;
            const bool valid = r < rows;
            const long long rc = valid ? r : rows - 1;
            const float *lam = size_entry_v5(sizes, sc[k], C) + lam_off;
            const float mv = valid ? 1.f : 0.f;
            a[k] = A[rc * lda + cac] * (ma * mv);
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const int cb = 32 * n + li, cbc = cb < C ? cb : 0;
                b[k][n] = lam[cbc] * B[rc * C + cbc] * (mb[n] * mv);
            }
        }
#pragma unroll
        for (int k = 0; k < kV5Steps; ++k)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k], b[k][n], acc[n], 0, 0, 0);
#pragma unroll
        for (int k = 0; k < kV5Steps; ++k) sc[k] = sn[k];
    }
    float *o = part + (size_t)blockIdx.x * C * C;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const int d = 32 * n + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 32 * m + 8 * (r >> 2) + 4 * lh + (r & 3);
            if (c < C && d < C) o[(size_t)c * C + d] = acc[n][r];
        }
    }
}

// dK [C][2 C] += the n1 partial images of dK1 (left half) and the n2 of dK2 (right half, behind them).  Workgroup = 64 elements x
// kV5FoldGroups runs: run g sums the images [g per, (g + 1) per) of a half in chunk order (per = ceil(n / kV5FoldGroups): a function of n
// alone), then one thread per element adds the runs in order.
__global__ __launch_bounds__(64 * kV5FoldGroups) void v5_wgrad_fold(const float *__restrict__ part, float *__restrict__ dK, int n1, int n2, int C) {
    __shared__ float red[2][kV5FoldGroups][64];
    const int e = threadIdx.x & 63, g = threadIdx.x >> 6, i = blockIdx.x * 64 + e;
    const int per1 = (n1 + kV5FoldGroups - 1) / kV5FoldGroups, per2 = (n2 + kV5FoldGroups - 1) / kV5FoldGroups;
    float t1 = 0.f, t2 = 0.f;
    if (i < C * C) {
        const int e1 = (g + 1) * per1 < n1 ? (g + 1) * per1 : n1, e2 = (g + 1) * per2 < n2 ? (g + 1) * per2 : n2;
        for (int k = g * per1; k < e1; ++k) t1 += part[(size_t)k * C * C + i];
        for (int k = g * per2; k < e2; ++k) t2 += part[(size_t)(n1 + k) * C * C + i];
    }
    red[0][g][e] = t1;
    red[1][g][e] = t2;
    __syncthreads();
    if (g != 0 || i >= C * C) return;
    t1 = t2 = 0.f;
    for (int k = 0; k < kV5FoldGroups; ++k) {
        t1 += red[0][k][e];
        t2 += red[1][k][e];
    }
    const int c = i / C, d = i - c * C;
    dK[(size_t)c * 2 * C + d] += t1;
    dK[(size_t)c * 2 * C + C + d] += t2;
}

// dS[i][j] = lambda1_s dE[i][j] + lambda2_s dO[j] over dz in df_l, and the rest of the column's partial behind cz: [ . | k_n sum_i dE[i][j]
// S[i][j] | k_n dO[j] col[j] | sum_i adj[i][j] dS[i][j] ].  Items (node, column j, vector q).
template <int V>
__global__ __launch_bounds__(256) void v5_combine(const float *__restrict__ dE, const float *__restrict__ dO, const float *__restrict__ S,
                                                  const float *__restrict__ col, const float *__restrict__ sizes, const float *__restrict__ adj,
                                                  float *__restrict__ df, float *__restrict__ part, const int *__restrict__ node_s,
                                                  const long long *__restrict__ node_row, const long long *__restrict__ node_pair,
                                                  const int *__restrict__ weight, int C, int nodes, int npw) {
    __shared__ int off[kMaxPack + 1];
    const Run run = pack_run(off, node_s, nodes, npw, C / V);
    for (int it = threadIdx.x; it < run.total; it += blockDim.x) {
        const Item x = pack_item<V>(off, run.np, it, C / V);
        const int n = run.nb + x.j, s = node_s[n], j = x.pos, cq = x.cq;
        const long long r0 = node_row[n], cj = node_pair[n] + j;
        const float *se = size_entry_v5(sizes, s, C);
        const Vf<V> l1 = vld<V>(se + cq), l2 = vld<V>(se + C + cq), dov = vld<V>(dO + cj * C + cq), cv = vld<V>(col + cj * C + cq);
        const float kn = (float)weight[n];
        Vf<V> pa = vzero<V>(), ps = vzero<V>(), pb;
        for (int i = 0; i < s; ++i) {
            const long long row = r0 + (long long)i * s + j;
            const Vf<V> e = vld<V>(dE + row * C + cq), sv = vld<V>(S + row * C + cq);
            const float av = adj[row];
            Vf<V> d;
#pragma unroll
            for (int c = 0; c < V; ++c) {
                pa.v[c] += e.v[c] * sv.v[c];
                d.v[c] = l1.v[c] * e.v[c] + l2.v[c] * dov.v[c];
                ps.v[c] += av * d.v[c];
            }
            vst<V>(df + row * C + cq, d);
        }
#pragma unroll
        for (int c = 0; c < V; ++c) {
            pa.v[c] *= kn;
            pb.v[c] = kn * (dov.v[c] * cv.v[c]);
        }
        float *pr = part + cj * 4 * C;
        vst<V>(pr + C + cq, pa);
        vst<V>(pr + 2 * C + cq, pb);
        vst<V>(pr + 3 * C + cq, ps);
    }
}

gf_status col_proj(gf_ctx *ctx, const char *name, const float *K, const float *in, int ldin, const float *sizes, const int *col_s, float *out,
                   long long cols, int C, int fwd) {
    const size_t lds = (size_t)C * C * sizeof(float);
    gf_status st = opt_in_lds(ctx, v5_col_proj, lds);
    if (st != GF_OK) return st;
    const long long blocks = (cols * C + 255) / 256;
    GF_LAUNCH(ctx, name, v5_col_proj, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(256), lds, K, in, ldin, sizes, col_s, out, cols, C, fwd);
    return GF_OK;
}

template <int NT, bool VEC, bool FWD>
gf_status row_proj_launch(gf_ctx *ctx, const float *K, const float *X, const float *sizes, const float *u, const int2 *row_cs, float *out,
                          long long rows, int C, float alpha, int max_workgroups) {
    constexpr size_t lds = (size_t)(32 * NT) * (32 * NT + 4) * sizeof(float);
    gf_status st = opt_in_lds(ctx, v5_row_proj<NT, VEC, FWD>, lds);
    if (st != GF_OK) return st;
    // four tiles (waves) per workgroup; no more workgroups than the device holds at once (they stride over the tiles): a second round of a
    // few workgroups would stage the image again for a fraction of the machine
    static int resident[64] = {};
    const int di = ctx->device & 63;
    if (!resident[di]) {
        int per_cu = 0;
        GF_HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, v5_row_proj<NT, VEC, FWD>, 256, lds));
        resident[di] = device_cu_count(ctx) * (per_cu < 1 ? 1 : per_cu);
    }
    // (max_workgroups > 0: a smaller grid still, for the stand-alone operator -- a small input then strides; the level passes 0)
    long long blocks = ((rows + 31) / 32 + 3) / 4;
    if (blocks > resident[di]) blocks = resident[di];
    if (max_workgroups > 0 && blocks > max_workgroups) blocks = max_workgroups;
    GF_LAUNCH(ctx, FWD ? "smp2d5_row_proj" : "smp2d5_row_proj_bwd", (v5_row_proj<NT, VEC, FWD>), dim3((unsigned)blocks), dim3(256), lds, K, X, sizes, u,
              row_cs, out, rows, C, alpha);
    return GF_OK;
}
template <bool FWD>
gf_status row_proj(gf_ctx *ctx, const float *K, const float *X, const float *sizes, const float *u, const int2 *row_cs, float *out, long long rows,
                   int C, float alpha, int max_workgroups) {
    const int nt = (C + 31) / 32;
#define GF_V5_ROW(NT) (C % 4 == 0 ? row_proj_launch<NT, true, FWD>(ctx, K, X, sizes, u, row_cs, out, rows, C, alpha, max_workgroups) \
                                  : row_proj_launch<NT, false, FWD>(ctx, K, X, sizes, u, row_cs, out, rows, C, alpha, max_workgroups))
    switch (nt) {
        case 1: return GF_V5_ROW(1);
        case 2: return GF_V5_ROW(2);
        case 3: return GF_V5_ROW(3);
        case 4: return GF_V5_ROW(4);
    }
#undef GF_V5_ROW
    return fail(ctx, GF_ERR_INVALID, "SMP_2D_ver5 level: %d channels (at most 128)", C);
}

gf_status wgrad(gf_ctx *ctx, const float *A, int lda, const float *B, const float *sizes, int lam_off, const int *sz, int sz_stride, int sz_off,
                float *part, long long rows, int C) {
    const unsigned chunks = (unsigned)((rows + kV5Chunk - 1) / kV5Chunk);
    if (!chunks) return GF_OK;
#define GF_V5_WG(NT) GF_LAUNCH(ctx, "smp2d5_wgrad", v5_wgrad<NT>, dim3(chunks), dim3(64 * NT), 0, A, lda, B, sizes, lam_off, sz, sz_stride, sz_off, part, rows, C)
    switch ((C + 31) / 32) {
        case 1: GF_V5_WG(1); break;
        case 2: GF_V5_WG(2); break;
        case 3: GF_V5_WG(3); break;
        default: GF_V5_WG(4); break;
    }
#undef GF_V5_WG
    return GF_OK;
}

// dK [C][2 C] += (dK1 | dK2): the two chunked reductions, their partial images back to back in `part` (smp_2d_ver5_wgrad_chunks(rows,
// cols) images of C x C floats), and the fold
gf_status wgrad_both(gf_ctx *ctx, const float *dz, const float *S, const int2 *row_cs, long long rows, const float *cz, int ldcz, const float *col,
                     const int *col_s, long long cols, const float *sizes, float *part, float *dK, int C) {
    const int n1 = (int)((rows + kV5Chunk - 1) / kV5Chunk), n2 = (int)((cols + kV5Chunk - 1) / kV5Chunk);
    gf_status st = wgrad(ctx, dz, C, S, sizes, 0, reinterpret_cast<const int *>(row_cs), 2, 1, part, rows, C);
    if (st == GF_OK) st = wgrad(ctx, cz, ldcz, col, sizes, C, col_s, 1, 0, part + (size_t)n1 * C * C, cols, C);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "smp2d5_wgrad_fold", v5_wgrad_fold, dim3((unsigned)((C * C + 63) / 64)), dim3(64 * kV5FoldGroups), 0, part, dK, n1, n2, C);
    return GF_OK;
}

// A table of a stand-alone call, checked on the host (one blocking copy: these are test operators): col_s (stride 1) or row_cs (stride 2:
// (column, s)).  Every s in 1 .. nsizes -- the kernels index the size entries with it -- and every column of row_cs inside the cols columns.
gf_status check_table(gf_ctx *ctx, const char *who, const char *what, const int *tab, int n, int stride, int nsizes, int cols) {
    std::vector<int> t((size_t)n * stride);
    GF_HIP_TRY(ctx, hipMemcpyAsync(t.data(), tab, sizeof(int) * t.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; ++i) {
        const int s = t[(size_t)i * stride + stride - 1];
        if (s < 1 || s > nsizes) return fail(ctx, GF_ERR_INVALID, "%s: %s[%d] has size %d outside 1 .. %d", who, what, i, s, nsizes);
        if (stride == 2 && (t[(size_t)i * 2] < 0 || t[(size_t)i * 2] >= cols))
            return fail(ctx, GF_ERR_INVALID, "%s: %s[%d] names column %d outside the %d columns", who, what, i, t[(size_t)i * 2], cols);
    }
    return GF_OK;
}

}  // namespace

size_t smp_2d_ver5_wgrad_chunks(long long rows, long long cols) {
    return (size_t)((rows + kV5Chunk - 1) / kV5Chunk + (cols + kV5Chunk - 1) / kV5Chunk);
}

// f_l from f_{l-1}: the storing gather, u on the columns, the row projection
gf_status smp_2d_ver5_forward_level(gf_smp *s, int l, const float *Kl, const float *sizes) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l], &pv = s->lv[l - 1];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const int C = s->cfg.nChanels, nodes = h.nNodes, V = lane_vector(C);
    const float *scalar = Kl + (size_t)2 * C * C;
    if (nodes == 0) return GF_OK;
    const long long cols = h.node_pair.back() + h.node_s.back();   // sum s
    const RunGrid g = run_grid(h, true, C / V);
    gf_status st = with_lane_vector(V, [&](auto v) -> gf_status {
        GF_LAUNCH(ctx, "smp2d5_store_S", v5_store_S<v>, g.grid, dim3(256), 0, pv.f, scalar, d.adj, d.th_A, d.th_B, d.v5_row_cs, d.v5_col_s, d.node_s,
                  d.node_row, d.node_pair, d.th_child_ptr, d.th_src_row, d.th_src_s, d.th_pi_off, d.th_pi, C, nodes, g.npw);
        return GF_OK;
    });
    if (st == GF_OK) st = col_proj(ctx, "smp2d5_col_proj", Kl, d.th_B, C, sizes, d.v5_col_s, d.v5_u, cols, C, 1);
    if (st != GF_OK) return st;
    return row_proj<true>(ctx, Kl, d.th_A, sizes, d.v5_u, d.v5_row_cs, d.f, h.rows, C, s->cfg.level_slope(), 0);
}

// dz in place, dE and dO, dK_l, dS over dz with the column partials; then the steerable level's own reductions and the df_{l-1} gather
gf_status smp_2d_ver5_backward_level(gf_smp *s, int l, const float *Kl, const float *sizes, float *dKl, float *dsizes, const float *node_df,
                                     bool rows_too, gf_status (*)(gf_smp *, int)) {
    gf_ctx *ctx = s->ctx;
    const gf_smp::DevLevel &d = s->lv[l];
    const gfsmp::LevelLayout &h = s->lay.level[l];
    const int C = s->cfg.nChanels, nodes = h.nNodes, V = lane_vector(C);
    if (!node_df && !rows_too) return fail(ctx, GF_ERR_INVALID, "steerable level %d: no gradient to back-propagate", l);
    if (nodes > 0) {
        const long long rows = h.rows, cols = h.node_pair.back() + h.node_s.back();   // sum s^2, sum s
        const RunGrid g = run_grid(h, true, C / V);
        gf_status st = with_lane_vector(V, [&](auto v) -> gf_status {
            GF_LAUNCH(ctx, "smp2d5_dz", v5_dz<v>, g.grid, dim3(256), 0, d.f, d.df, node_df, d.th_node, d.node_s, d.node_row, d.node_pair, C,
                      s->cfg.level_slope(), nodes, g.npw, rows_too ? 1 : 0);
            return GF_OK;
        });
        if (st == GF_OK) st = row_proj<false>(ctx, Kl, d.df, sizes, nullptr, d.v5_row_cs, d.Q, rows, C, 0.f, 0);
        if (st == GF_OK) st = col_proj(ctx, "smp2d5_col_proj_bwd", Kl, d.th_node, 4 * C, sizes, d.v5_col_s, d.v5_dO, cols, C, 0);
        // dK1 over the rows (dz is still in df_l), dK2 over the columns
        if (st == GF_OK) st = wgrad_both(ctx, d.df, d.th_A, d.v5_row_cs, rows, d.th_node, 4 * C, d.th_B, d.v5_col_s, cols, sizes, d.v5_dKpart, dKl, C);
        if (st != GF_OK) return st;
        st = with_lane_vector(V, [&](auto v) -> gf_status {
            GF_LAUNCH(ctx, "smp2d5_combine", v5_combine<v>, g.grid, dim3(256), 0, d.Q, d.v5_dO, d.th_A, d.th_B, sizes, d.adj, d.df, d.th_node, d.node_s,
                      d.node_row, d.node_pair, d.th_weight, C, nodes, g.npw);
            return GF_OK;
        });
        if (st == GF_OK) st = smp_2d_size_grads(s, l, dKl + (size_t)2 * C * C, dsizes);
        if (st != GF_OK) return st;
    }
    return smp_field_gather_down(s, l, d.df, C, true, "smp2d_gather_bwd");
}

}  // namespace gf

// ---- the level's projections and weight gradients as stand-alone operators (include/gf_hip.h; tests/test_smp_2d_ver5_ops_gpu.py) ----
extern "C" {

gf_status gf_smp_2d_ver5_rows_ex_f32(gf_ctx *ctx, int backward, int C, int rows, int cols, int nsizes, const float *K, const float *X,
                                     const float *sizes, const float *u, const int *row_cs, float alpha, int max_workgroups, float *out) {
    static const char *who = "gf_smp_2d_ver5_rows_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (C < 1 || C > 128) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d channels (1 .. 128)", who, C);
    if (rows < 1 || max_workgroups < 0 || !K || !X || !out) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    if (!backward && (cols < 1 || nsizes < 1 || !sizes || !u || !row_cs)) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument of the forward", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (backward) return gf::row_proj<false>(ctx, K, X, nullptr, nullptr, nullptr, out, rows, C, 0.f, max_workgroups);
    const gf_status st = gf::check_table(ctx, who, "row_cs", row_cs, rows, 2, nsizes, cols);
    if (st != GF_OK) return st;
    return gf::row_proj<true>(ctx, K, X, sizes, u, reinterpret_cast<const int2 *>(row_cs), out, rows, C, alpha, max_workgroups);
}

gf_status gf_smp_2d_ver5_cols_ex_f32(gf_ctx *ctx, int backward, int C, int cols, int nsizes, const float *K, const float *in, int ldin,
                                     const float *sizes, const int *col_s, float *out) {
    static const char *who = "gf_smp_2d_ver5_cols_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (C < 1 || C > 128) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d channels (1 .. 128)", who, C);
    if (cols < 1 || ldin < C || !K || !in || !out) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    if (!backward && (nsizes < 1 || !sizes || !col_s)) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument of the forward", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (backward) return gf::col_proj(ctx, "smp2d5_col_proj_bwd", K, in, ldin, nullptr, nullptr, out, cols, C, 0);
    const gf_status st = gf::check_table(ctx, who, "col_s", col_s, cols, 1, nsizes, 0);
    if (st != GF_OK) return st;
    return gf::col_proj(ctx, "smp2d5_col_proj", K, in, ldin, sizes, col_s, out, cols, C, 1);
}

gf_status gf_smp_2d_ver5_wgrad_ex_f32(gf_ctx *ctx, int C, int rows, int cols, int nsizes, const float *dz, const float *S, const int *row_cs,
                                      const float *cz, int ldcz, const float *col, const int *col_s, const float *sizes, float *dK) {
    static const char *who = "gf_smp_2d_ver5_wgrad_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    if (C < 1 || C > 128) return gf::fail(ctx, GF_ERR_INVALID, "%s: %d channels (1 .. 128)", who, C);
    if (rows < 1 || cols < 1 || nsizes < 1 || ldcz < C || !dz || !S || !row_cs || !cz || !col || !col_s || !sizes || !dK)
        return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    gf_status st = gf::check_table(ctx, who, "row_cs", row_cs, rows, 2, nsizes, cols);
    if (st == GF_OK) st = gf::check_table(ctx, who, "col_s", col_s, cols, 1, nsizes, 0);
    // workspace: the partial images of both halves
    if (st == GF_OK) st = gf::ensure_ws(ctx, sizeof(float) * gf::smp_2d_ver5_wgrad_chunks(rows, cols) * C * C + 256);
    if (st != GF_OK) return st;
    return gf::wgrad_both(ctx, dz, S, reinterpret_cast<const int2 *>(row_cs), rows, cz, ldcz, col, col_s, cols, sizes, static_cast<float *>(ctx->ws), dK, C);
}

}  // extern "C"
