// smp_level_third.hip -- the aggregate of GCN_3D and GRU_GCN_3D (cfg.neighbourhood = 6, 7; GraphFlow/GCN_3D.h, GRU_GCN_3D.h, RisiLayer3D.h,
// KMax.h): n_l[v] = the H largest of the H^3 entries of
//   T[x, y, z] = sum over ordered triples (i, j, k) of distinct members of N_l(v) of a_i[x] a_j[y] a_k[z],   a_u = h_{l-1}[u],
// ascending (n[H - 1] the largest), and its reverse.  Everything else of the two models is smp_level_neighbourhood.hip / smp_level_gru.hip.
// T is symmetric in (x, y, z): its entries fall into H (H + 1) (H + 2) / 6 classes x <= y <= z of 6, 3 or 1 equal entries, and which
// members of a class are kept changes neither a pooled value nor a gradient.  With A = sum_u a_u, B_pq = sum_u a_u[p] a_u[q]:
//   T[x, y, z] = A_x A_y A_z - B_yz A_x - B_xz A_y - B_xy A_z + 2 sum_u a_u[x] a_u[y] a_u[z]
//   da_u[x] += g D_u(y, z), da_u[y] += g D_u(x, z), da_u[z] += g D_u(x, y) per kept entry with gradient g,
//   D_u(p, q) = (A_p - a_u[p]) (A_q - a_u[q]) - (B_pq - a_u[p] a_u[q])
//   third_pool_fwd   one workgroup per vertex: the members, A and B in LDS; a class is one lane's m fused multiply-adds (x by x, the
//                    workgroup's lanes over the pairs y <= z at or above x).  The selection is an exact radix select over the 50-bit key
//                    (order-preserving bits of the fp32 value, canonical flat index z H^2 + y H + x): a histogram of 11 bits per pass,
//                    weighted by the class's multiplicity, integer LDS adds only, the classes recomputed in every pass by one function
//                    of fixed rounding; as soon as the classes at or above the cut's bin are known to fit kThirdCand slots they are
//                    collected, ranked by counting (the keys are distinct) and laid out with their multiplicity.  Two passes and the
//                    collection in the usual case; all five when values tie exactly.  Under three members: n = 0, sel = -1, exactly.
//   third_pool_bwd   one wave per source vertex w: its consumers v in ascending order (the transposed list), per consumer lane r takes
//                    rank r: A and B at the rank's triple recomputed from v's members, three (channel, value) pairs through LDS, lane c
//                    sums channel c's in index order.  The sums and D are fp64 (D cancels where the members' signs are mixed).
// Exact fp32 ties between two different classes: the key orders them by canonical flat index, the larger first -- the class's own rule
// (sort by (value, index)) applied to the classes' largest entries.  The pooled values do not depend on it.
// No float atomics; every sum in a fixed order; two runs give the same bits.  The two kernels are also operators of the C ABI on
// caller-supplied operands (gf_smp_third_order_pool_fwd_ex_f32, _bwd_ex_f32 at the end of the file).
#include <cmath>

#include "smp_vertex_level.h"

namespace gf {
using namespace vertex_level;
namespace {

constexpr int kDigit = 11;    // key bits per pass: kThirdBins = 1 << kDigit
constexpr int kKeyBits = 50;  // 32 of the value, 18 of the flat index
typedef unsigned long long u64;
static_assert(kThirdBins == 1 << kDigit && kThirdBins == 8 * kBlock, "one thread folds eight bins");

// (mul_rounded, smp_vertex_level.h: a class's value must be the same bits wherever it is recomputed)
// fp32 bits <-> an unsigned that orders as the values do
__device__ __forceinline__ unsigned ord_key(float t) {
    const unsigned b = __float_as_uint(t);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// f(key, multiplicity) for every canonical class x <= y <= z, each once, by the lane that owns it: x by x, the workgroup's lanes over the
// (H - x) (H - x + 1) / 2 pairs y <= z at or above x (q = z' (z' + 1) / 2 + y', y' = y - x <= z' = z - x), so that a wave reads a_u[x] and
// mostly a_u[z] as broadcasts and a_u[y] from consecutive banks, and nine lanes in ten have a class
template <typename F>
__device__ __forceinline__ void each_class(int H, int m, const float *mem, const float *A, const float *B, F &&f) {
    for (int x = 0; x < H; ++x) {
        const int hx = H - x, npair = hx * (hx + 1) / 2;
        for (int q = threadIdx.x; q < npair; q += kBlock) {
            int zz = (int)((sqrtf(8.f * (float)q + 1.f) - 1.f) * 0.5f);
            while (zz * (zz + 1) / 2 > q) --zz;
            while ((zz + 1) * (zz + 2) / 2 <= q) ++zz;
            const int y = x + q - zz * (zz + 1) / 2, z = x + zz;
            float s3 = 0.f;
            for (int u = 0; u < m; ++u) {
                const float *a = mem + u * H;
                s3 = fmaf(mul_rounded(a[x], a[y]), a[z], s3);
            }
            float t = mul_rounded(mul_rounded(A[x], A[y]), A[z]);
            t = fmaf(-B[y * H + z], A[x], t);
            t = fmaf(-B[x * H + z], A[y], t);
            t = fmaf(-B[x * H + y], A[z], t);
            t = fmaf(2.f, s3, t);
            const u64 key = ((u64)ord_key(t) << 18) | (unsigned)((z * H + y) * H + x);
            f(key, (x == y && y == z) ? 1u : (x == y || y == z) ? 3u : 6u);
        }
    }
}

__global__ __launch_bounds__(kBlock) void third_pool_fwd(const float *__restrict__ hprev, const long long *__restrict__ ptr,
                                                         const int *__restrict__ idx, float *__restrict__ n, int *__restrict__ sel, int H,
                                                         int cap) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    u64 *cand = reinterpret_cast<u64 *>(lds_raw);   // [kThirdCand] as collected
    u64 *sorted = cand + kThirdCand;                // [kThirdCand] descending
    unsigned *hist = reinterpret_cast<unsigned *>(sorted + kThirdCand);   // [kThirdBins]
    unsigned *part = hist + kThirdBins;             // [kBlock] eight bins each
    unsigned *ctrl = part + kBlock;                 // [8]
    float *A = reinterpret_cast<float *>(ctrl + 8); // [H]
    float *B = A + H;                               // [H][H]
    float *mem = B + H * H;                         // [m][H]
    const size_t v = blockIdx.x;
    const int tid = threadIdx.x;
    const long long e0 = ptr[v];
    const long long len = ptr[v + 1] - e0;
    if (len < 3 || len > cap) {   // (uniform.  Under three members T = 0 exactly; a list beyond the LDS the launch took does not occur)
        for (int c = tid; c < H; c += kBlock) n[v * H + c] = 0.f, sel[v * H + c] = -1;
        return;
    }
    const int m = (int)len;
    for (int i = tid; i < m * H; i += kBlock) {
        const int u = i / H, c = i - u * H;
        mem[i] = hprev[(size_t)idx[e0 + u] * H + c];
    }
    __syncthreads();
    for (int c = tid; c < H; c += kBlock) {
        float a = 0.f;
        for (int u = 0; u < m; ++u) a += mem[u * H + c];
        A[c] = a;
    }
    for (int i = tid; i < H * H; i += kBlock) {
        const int p = i / H, q = i - p * H;
        float b = 0.f;
        for (int u = 0; u < m; ++u) b = fmaf(mem[u * H + p], mem[u * H + q], b);
        B[i] = b;
    }
    __syncthreads();
    // the H-th largest entry, counted with multiplicity: bits [hi, 50) of its key are `prefix`'s, it is the need-th largest under them
    u64 prefix = 0;
    int hi = kKeyBits;
    unsigned need = (unsigned)H;
    for (;;) {   // (every quantity that steers the loop is the workgroup's: the same trips in every wave)
        const int w = hi >= kDigit ? kDigit : hi, s = hi - w;
        for (int i = tid; i < kThirdBins; i += kBlock) hist[i] = 0u;
        __syncthreads();
        each_class(H, m, mem, A, B, [&](u64 key, unsigned mult) {
            if ((key >> hi) == (prefix >> hi)) atomicAdd(&hist[(unsigned)(key >> s) & ((1u << w) - 1u)], mult);
        });
        __syncthreads();
        unsigned fold = 0u;
        for (int k = 0; k < 8; ++k) fold += hist[8 * tid + k];
        part[tid] = fold;
        __syncthreads();
        if (tid == 0) {   // the bin of the need-th largest, from the top
            unsigned above = 0u;
            int c = kBlock - 1;
            while (c > 0 && above + part[c] < need) above += part[c], --c;
            int b = 8 * c + 7;
            while (b > 8 * c && above + hist[b] < need) above += hist[b], --b;
            ctrl[0] = (unsigned)b;
            ctrl[1] = need - above;
            ctrl[2] = hist[b];
        }
        __syncthreads();
        const unsigned inbin = ctrl[2];
        prefix |= (u64)ctrl[0] << s;
        need = ctrl[1];
        hi = s;
        __syncthreads();   // (ctrl and hist are rewritten by the next pass)
        // fewer than H classes lie above the bin and at most inbin in it; at hi = 0 the bin is one key
        if (hi == 0 || inbin + (unsigned)H <= (unsigned)kThirdCand) break;
    }
    if (tid == 0) ctrl[3] = 0u;
    __syncthreads();
    each_class(H, m, mem, A, B, [&](u64 key, unsigned) {
        if (key >= prefix) {
            const unsigned slot = atomicAdd(&ctrl[3], 1u);
            if (slot < (unsigned)kThirdCand) cand[slot] = key;
        }
    });
    __syncthreads();
    const int cnt = ctrl[3] < (unsigned)kThirdCand ? (int)ctrl[3] : kThirdCand;
    for (int i = tid; i < cnt; i += kBlock) {   // the keys are distinct: a rank by counting is a permutation
        const u64 key = cand[i];
        int r = 0;
        for (int j = 0; j < cnt; ++j) r += cand[j] > key ? 1 : 0;
        sorted[r] = key;
    }
    __syncthreads();
    if (tid == 0) {
        int filled = 0;
        for (int i = 0; i < cnt && filled < H; ++i) {
            const u64 key = sorted[i];
            const int flat = (int)(key & 0x3ffffu), x = flat % H, y = (flat / H) % H, z = flat / (H * H);
            const int mult = (x == y && y == z) ? 1 : (x == y || y == z) ? 3 : 6;
            const float val = key_value((unsigned)(key >> 18));
            for (int j = 0; j < mult && filled < H; ++j, ++filled) {
                n[v * H + (H - 1 - filled)] = val;
                sel[v * H + (H - 1 - filled)] = x | (y << 8) | (z << 16);
            }
        }
        for (; filled < H; ++filled) n[v * H + (H - 1 - filled)] = 0.f, sel[v * H + (H - 1 - filled)] = -1;   // (never: the candidates weigh H or more)
    }
}

__global__ __launch_bounds__(64) void third_pool_bwd(const long long *__restrict__ ptr, const int *__restrict__ idx,
                                                     const long long *__restrict__ tptr, const int *__restrict__ tidx,
                                                     const float *__restrict__ hprev, const int *__restrict__ sel, const float *__restrict__ dn,
                                                     float *__restrict__ dhprev, int H) {
    __shared__ int ch[3 * 64];
    __shared__ double val[3 * 64];
    const size_t w = blockIdx.x;
    const int r = threadIdx.x;
    const bool ok = r < H;
    const int rr = ok ? r : H - 1;
    const float *aw = hprev + w * H;
    double acc = 0.0;
    const long long t1 = tptr[w + 1];
    for (long long e = tptr[w]; e < t1; ++e) {
        const size_t v = (size_t)tidx[e];
        if (sel[v * H] < 0) continue;   // (the wave's: under three members every rank is -1)
        const int s0 = sel[v * H + rr], s = s0 < 0 ? 0 : s0, x = s & 255, y = (s >> 8) & 255, z = (s >> 16) & 255;   // (a stray -1: no entry)
        // D_w is the difference of two sums of like size where the members' signs are mixed: the six sums and D in fp64, which holds the
        // products of two floats exactly; a consumer costs 6 m multiply-adds per lane
        double Ax = 0.0, Ay = 0.0, Az = 0.0, Bxy = 0.0, Bxz = 0.0, Byz = 0.0;
        const long long q1 = ptr[v + 1];
        for (long long q = ptr[v]; q < q1; ++q) {
            const float *a = hprev + (size_t)idx[q] * H;
            const double ax = a[x], ay = a[y], az = a[z];
            Ax += ax, Ay += ay, Az += az;
            Bxy = fma(ax, ay, Bxy), Bxz = fma(ax, az, Bxz), Byz = fma(ay, az, Byz);
        }
        const double wx = aw[x], wy = aw[y], wz = aw[z], g = s0 < 0 ? 0.0 : (double)dn[v * H + rr];
        const double dx = Ax - wx, dy = Ay - wy, dz = Az - wz;
        if (ok) {
            ch[3 * r] = x, val[3 * r] = g * (dy * dz - (Byz - wy * wz));
            ch[3 * r + 1] = y, val[3 * r + 1] = g * (dx * dz - (Bxz - wx * wz));
            ch[3 * r + 2] = z, val[3 * r + 2] = g * (dx * dy - (Bxy - wx * wy));
        }
        __syncthreads();
        if (ok)
            for (int i = 0; i < 3 * H; ++i)
                if (ch[i] == r) acc += val[i];
        __syncthreads();
    }
    if (ok) dhprev[w * H + r] = (float)acc;
}

}  // namespace

gf_status smp_third_pool_fwd_launch(gf_ctx *ctx, int H, int nV, int max_members, const float *hprev, const long long *ptr, const int *idx, float *n,
                                    int *sel) {
    const int cap = max_members < 3 ? 3 : max_members;
    const size_t bytes = smp_third_lds_bytes(H, cap);
    if (H < 1 || H > kThirdMaxChanels || bytes > 160 * 1024)
        return fail(ctx, GF_ERR_INVALID, "third_pool_fwd: %d channels, lists of up to %d members need %zu bytes of LDS (160 KiB)", H, cap, bytes);
    const gf_status st = opt_in_lds(ctx, third_pool_fwd, bytes);
    if (st != GF_OK) return st;
    GF_LAUNCH(ctx, "third_pool_fwd", third_pool_fwd, dim3((unsigned)nV), dim3(kBlock), bytes, hprev, ptr, idx, n, sel, H, cap);
    return GF_OK;
}

gf_status smp_third_pool_bwd_launch(gf_ctx *ctx, int H, int nV, const long long *ptr, const int *idx, const long long *tptr, const int *tidx,
                                    const float *hprev, const int *sel, const float *dn, float *dhprev) {
    if (H < 1 || H > kThirdMaxChanels) return fail(ctx, GF_ERR_INVALID, "third_pool_bwd: %d channels (1 .. %d)", H, kThirdMaxChanels);
    GF_LAUNCH(ctx, "third_pool_bwd", third_pool_bwd, dim3((unsigned)nV), dim3(64), 0, ptr, idx, tptr, tidx, hprev, sel, dn, dhprev, H);
    return GF_OK;
}

}  // namespace gf

// ---- the two kernels as stand-alone operators (include/gf_hip.h; tests/test_smp_third_order_ops_gpu.py) ----
extern "C" {

gf_status gf_smp_third_order_pool_fwd_ex_f32(gf_ctx *ctx, int H, int nV, const long long *ptr, const int *idx, const float *hprev, float *n, int *sel) {
    static const char *who = "gf_smp_third_order_pool_fwd_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kThirdMaxChanels, nV, 0);
    if (st != GF_OK) return st;
    if (!ptr || !idx || !hprev || !n || !sel) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    long long longest = 0;
    st = gf::check_list(ctx, who, "ptr", ptr, idx, nV, nV, &longest);
    if (st != GF_OK) return st;
    if (longest > gf::smp_third_max_members(H))
        return gf::fail(ctx, GF_ERR_INVALID, "%s: a list of %lld members at %d channels (at most %d: the members are staged in LDS)", who, longest, H,
                        gf::smp_third_max_members(H));
    return gf::smp_third_pool_fwd_launch(ctx, H, nV, (int)longest, hprev, ptr, idx, n, sel);
}

gf_status gf_smp_third_order_pool_bwd_ex_f32(gf_ctx *ctx, int H, int nV, const long long *ptr, const int *idx, const long long *tptr, const int *tidx,
                                             const float *hprev, const int *sel, const float *dn, float *dhprev) {
    static const char *who = "gf_smp_third_order_pool_bwd_ex_f32";
    if (!ctx) return gf::fail(nullptr, GF_ERR_INVALID, "null context");
    gf_status st = gf::check_shape(ctx, who, H, gf::kThirdMaxChanels, nV, 0);
    if (st != GF_OK) return st;
    if (!ptr || !idx || !tptr || !tidx || !hprev || !sel || !dn || !dhprev) return gf::fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = gf::check_list(ctx, who, "ptr", ptr, idx, nV, nV);
    if (st == GF_OK) st = gf::check_list(ctx, who, "tptr", tptr, tidx, nV, nV);
    if (st != GF_OK) return st;
    std::vector<int> t((size_t)nV * H);   // the record's triples index hprev's channels
    GF_HIP_TRY(ctx, hipMemcpyAsync(t.data(), sel, sizeof(int) * t.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < t.size(); ++i) {
        const int x = t[i] & 255, y = (t[i] >> 8) & 255, z = (t[i] >> 16) & 255;
        if (t[i] != -1 && (t[i] < 0 || (t[i] >> 24) || x > y || y > z || z >= H))
            return gf::fail(ctx, GF_ERR_INVALID, "%s: sel[%zu] = %d is no triple x <= y <= z < %d", who, i, t[i], H);
    }
    return gf::smp_third_pool_bwd_launch(ctx, H, nV, ptr, idx, tptr, tidx, hprev, sel, dn, dhprev);
}

}  // extern "C"
