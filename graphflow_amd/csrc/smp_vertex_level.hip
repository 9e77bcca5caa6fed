// smp_vertex_level.hip -- what more than one vertex level launches or asks (smp_vertex_level.h names the levels): the read-outs' dW and
// the host checks of a stand-alone operator's lists.
#include <vector>

#include "smp_vertex_level.h"

namespace gf {
namespace {

// dW[c] += sum_m dy[m] g[m][c] (InnerProduct::backward, second operand): 64 columns per workgroup, row r of its 16 sums the molecules
// r, r + 16, .., the 16 partials are folded in order
__global__ __launch_bounds__(1024) void vertex_readout_dW(const float *__restrict__ dy, const float *__restrict__ g, float *__restrict__ dW, int width,
                                                          int n) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const int cc = c < width ? c : width - 1;
    float acc = 0.f;
    for (int m = r; m < n; m += 16) acc = fmaf(dy[m], g[(size_t)m * width + cc], acc);
    part[r][lane] = acc;
    __syncthreads();
    if (r == 0 && c < width) {
        float t = 0.f;
        for (int k = 0; k < 16; ++k) t += part[k][lane];
        dW[c] += t;
    }
}

// ptr [n + 1] starts at 0 and never decreases.  `idx` null: ptr alone (32-bit: mol_ptr), its last entry at most `bound`.
template <typename P>
gf_status check_list_of(gf_ctx *ctx, const char *who, const char *what, const P *ptr, const int *idx, int n, int bound, long long *longest) {
    std::vector<P> p((size_t)n + 1);
    GF_HIP_TRY(ctx, hipMemcpyAsync(p.data(), ptr, sizeof(P) * p.size(), hipMemcpyDeviceToHost, ctx->stream));
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (p[0] != 0) return fail(ctx, GF_ERR_INVALID, "%s: %s starts at %lld, not at 0", who, what, (long long)p[0]);
    long long most = 0;
    for (int i = 0; i < n; ++i) {
        if (p[i + 1] < p[i]) return fail(ctx, GF_ERR_INVALID, "%s: %s decreases at entry %d", who, what, i + 1);
        if (p[i + 1] - p[i] > most) most = p[i + 1] - p[i];
    }
    if (longest) *longest = most;
    if (!idx) {
        if ((long long)p[n] > bound) return fail(ctx, GF_ERR_INVALID, "%s: %s ends at %lld, beyond the %d rows", who, what, (long long)p[n], bound);
        return GF_OK;
    }
    if ((long long)p[n] > (1ll << 31)) return fail(ctx, GF_ERR_INVALID, "%s: %s ends at %lld: more than 2^31 members", who, what, (long long)p[n]);
    return vertex_level::check_members(ctx, who, what, idx, (size_t)p[n], bound);
}

}  // namespace

gf_status smp_vertex_readout_dW(gf_ctx *ctx, const char *timer, int width, int n, const float *dy, const float *g, float *dW) {
    GF_LAUNCH(ctx, timer, vertex_readout_dW, dim3((unsigned)((width + 63) / 64)), dim3(1024), 0, dy, g, dW, width, n);
    return GF_OK;
}

namespace vertex_level {

gf_status check_members(gf_ctx *ctx, const char *who, const char *what, const int *idx, size_t n, int bound) {
    std::vector<int> t(n);
    if (n) {
        GF_HIP_TRY(ctx, hipMemcpyAsync(t.data(), idx, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
        GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (size_t i = 0; i < n; ++i)
        if (t[i] < 0 || t[i] >= bound) return fail(ctx, GF_ERR_INVALID, "%s: %s[%zu] = %d outside [0, %d)", who, what, i, t[i], bound);
    return GF_OK;
}
gf_status check_list(gf_ctx *ctx, const char *who, const char *what, const long long *ptr, const int *idx, int n, int bound, long long *longest) {
    return check_list_of(ctx, who, what, ptr, idx, n, bound, longest);
}
gf_status check_ptr(gf_ctx *ctx, const char *who, const char *what, const int *ptr, int n, int bound) {
    return check_list_of<int>(ctx, who, what, ptr, nullptr, n, bound, nullptr);
}

}  // namespace vertex_level
}  // namespace gf
