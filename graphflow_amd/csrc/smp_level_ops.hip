// smp_level_ops.hip -- the block products of the fused SMP level as stand-alone operators of the C ABI
// (gf_smp_level_products_f32 / gf_smp_level_wgrad_f32 at C = 64, gf_smp_level_products_ex_f32 / gf_smp_level_wgrad_ex_f32 for every
// variant the level has -- 128 channels as four 64-channel sub-block passes included --, include/gf_hip.h): the same kernels gf_smp_forward / gf_smp_backward launch
// on a level's rows (smp_level_c64.hip on the fp32 matrix pipe, smp_level_c64_split.hip / smp_level_wgrad_split.hip on the f16 pipe with two-half operands),
// on caller-supplied matrices.  They replace, for the rows of one level, the K-projection MatMul of the reference
// (GraphFlow/SMP_omega.h:654-657 forward, MatMul.h:69-82 backward) in its regrouped form (smp_fused.hip header) -- and they are
// what the parity suite uses to hold the split-operand arithmetic to the fp64 product per output ROW and per weight-gradient ROW,
// on operands whose dynamic range the whole-network tests cannot steer (tests/test_level_ops_gpu.py), and with rows placed on the
// panel, slice and gather-window edges (tests/test_level_ops_ex_gpu.py).
#include <cstring>
#include <vector>

#include "smp_internal.h"

using gf::fail;

namespace gf {
namespace {

// out[0] = max(1, largest per-product factor of a product that is bounded through `tot` (0, 1, 5, 6, 7)), out[1] = largest factor of
// product 2 (bounded through `tr`), out[2] = max(1, largest factor of products 3, 4 -- they have no row factor in the level's bounds,
// scale_words widens the channel maxima by it): float bits, atomicMax on words the caller zeroed.  rf [rows][8]
__global__ __launch_bounds__(256) void rowfac8_absmax(const float *__restrict__ rf, int rows, unsigned *__restrict__ out) {
    float a = 1.f, b = 0.f, c = 1.f;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
        const float *f = rf + 8 * (size_t)r;
        a = fmaxf(a, fmaxf(fmaxf(fabsf(f[0]), fabsf(f[1])), fmaxf(fabsf(f[5]), fmaxf(fabsf(f[6]), fabsf(f[7])))));
        b = fmaxf(b, fabsf(f[2]));
        c = fmaxf(c, fmaxf(fabsf(f[3]), fabsf(f[4])));
    }
    atomicMax(&out[0], __float_as_uint(a));
    atomicMax(&out[1], __float_as_uint(b));
    atomicMax(&out[2], __float_as_uint(c));
}
__global__ void scale_words(unsigned *__restrict__ w, int n, const unsigned *__restrict__ by) {   // w[i] (float bits) *= by[0]
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = __float_as_uint(__uint_as_float(w[i]) * __uint_as_float(by[0]));
}

// rows the gathered operand dU[trow] of the weight-gradient kernels may lie from its own row (kTrowWindow of smp_level_wgrad_split.hip)
constexpr long long kGatherWindow = (long long)kFusedMaxField * kFusedMaxField;

// The tables of a stand-alone call, checked on the host (one blocking copy each: these are test operators): every trow inside the
// matrix and, `window` > 0, within that many rows of its own row (`beyond` given: reported there instead of refused); the low 29 bits
// of a packed entry equal to the plain one.
gf_status check_tables(gf_ctx *ctx, const char *who, int rows, const int *trow, const int *trowf, long long window, bool *beyond = nullptr) {
    std::vector<int> t((size_t)rows), f;
    GF_HIP_TRY(ctx, hipMemcpyAsync(t.data(), trow, sizeof(int) * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    if (trowf) {
        f.resize((size_t)rows);
        GF_HIP_TRY(ctx, hipMemcpyAsync(f.data(), trowf, sizeof(int) * (size_t)rows, hipMemcpyDeviceToHost, ctx->stream));
    }
    GF_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < rows; ++r) {
        if (t[r] < 0 || t[r] >= rows) return fail(ctx, GF_ERR_INVALID, "%s: trow[%d] = %d outside the %d rows", who, r, t[r], rows);
        const long long d = (long long)t[r] - r;
        if (window > 0 && (d > window || -d > window) && beyond) *beyond = true;
        else if (window > 0 && (d > window || -d > window))
            return fail(ctx, GF_ERR_INVALID, "%s: trow[%d] = %d lies more than %lld rows from its row (the gather window of the level)", who, r, t[r], window);
        if (trowf && (f[r] & 0x1fffffff) != t[r])
            return fail(ctx, GF_ERR_INVALID, "%s: trowf[%d] holds row %d, trow[%d] = %d", who, r, f[r] & 0x1fffffff, r, t[r]);
    }
    return GF_OK;
}

// the variants the level's weight-gradient kernels have (before any launch): 0, or the status with the reason recorded
// (at C = 64: with a packed table only -- `packed` -- the plain table is gf_smp_level_wgrad_f32's).  The products' variants:
// smp_row_products_admissible.
gf_status check_wgrad_variant(gf_ctx *ctx, const char *who, int C, int nf, int nx, bool packed) {
    if (!(C == 16 || C == 32 || (C == 64 && packed) || C == 128)) return fail(ctx, GF_ERR_UNSUPPORTED, "%s: %d channels", who, C);
    if (C == 64 && !smp_split_products(ctx))   // (the fp32 kernel does not mask: it would read the absent blocks)
        return fail(ctx, GF_ERR_UNSUPPORTED, "%s: the packed table at 64 channels on the fp32 matrix pipe", who);
    if ((nf != 2 && nf != 8) || (nx != 0 && nx != 3)) return fail(ctx, GF_ERR_UNSUPPORTED, "%s: %d row factors / %d extra products", who, nf, nx);
    if (nx == 3 && nf == 8) return fail(ctx, GF_ERR_UNSUPPORTED, "%s: the extra products take the plain (tot, tr) row factors", who);
    if ((C == 64 || C == 128) && (nx != 0 || nf != 2)) return fail(ctx, GF_ERR_UNSUPPORTED, "%s: %d row factors / %d extra products at %d channels", who, nf, nx, C);
    if (C != 64 && !smp_split_products(ctx)) return fail(ctx, GF_ERR_UNSUPPORTED, "%s: %d channels on the fp32 matrix pipe", who, C);
    return GF_OK;
}

}  // namespace
}  // namespace gf

extern "C" {

gf_status gf_smp_level_products_f32(gf_ctx *ctx, int backward, int rows, const float *A, const float *rowscale, const float *Wst,
                                    const int *trow, float *Out) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (rows < 0 || (rows > 0 && (!A || !rowscale || !Wst || !trow || !Out)))
        return fail(ctx, GF_ERR_INVALID, "gf_smp_level_products_f32: null argument");
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const gf::RowProductsCall call = {backward == 0, A, rowscale, Wst, Out, rows, trow};
    return gf::smp_row_products(ctx, call);
}

gf_status gf_smp_level_wgrad_f32(gf_ctx *ctx, int rows, const float *T, const float *dO, const float *rowscale, const int *trow,
                                 float *dWst) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (rows < 1 || !T || !dO || !rowscale || !trow || !dWst) return fail(ctx, GF_ERR_INVALID, "gf_smp_level_wgrad_f32: bad argument");
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // The split kernel reaches dU[trow] through the gather window of a level and would load zeros beyond it.  This operator takes any
    // permutation of the rows: a table that leaves the window is served through one descriptor over all of dO (WgradCall::any_trow; the
    // launch refuses it on a dO of 1 GiB or more), a row outside the matrix is refused here.
    bool beyond = false;
    gf_status st = gf::check_tables(ctx, "gf_smp_level_wgrad_f32", rows, trow, nullptr, gf::kGatherWindow, &beyond);
    if (st != GF_OK) return st;
    if (beyond && gf::smp_split_products(ctx) && (size_t)rows * 128 * sizeof(float) >= gf::kWgradWholeBytes)
        return fail(ctx, GF_ERR_INVALID, "gf_smp_level_wgrad_f32: a table beyond the gather window of %lld rows on a dO of 1 GiB or more", gf::kGatherWindow);
    // workspace: the partial images, then the scratch words of the operands' column bounds (exact maxima: there is no level behind them)
    const size_t part_floats = gf::smp_wgrad_part_floats(ctx, rows, 64);
    st = gf::ensure_ws(ctx, sizeof(float) * (part_floats + gf::smp_wgrad_words(64)) + 256);
    if (st != GF_OK) return st;
    float *ws = static_cast<float *>(ctx->ws);
    const gf::WgradCall wc = {T, dO, rowscale, rows, 64, 2, trow, nullptr, gf::WgradScales(), reinterpret_cast<unsigned *>(ws + part_floats), ws, part_floats, beyond};
    gf::FoldGroup fg;
    st = gf::smp_wgrad_partials(ctx, wc, &fg);
    if (st != GF_OK) return st;
    return gf::splitk_fold(ctx, fg.part, dWst, fg.n, fg.splits, 0);
}

gf_status gf_smp_level_products_ex_f32(gf_ctx *ctx, int backward, int C, int nf, int nx, int rows, const float *A, const float *rowfac,
                                       const float *Wst, const float *X, const int *trow, const int *trowf, int skip_zero_grads, float *Out) {
    static const char *who = "gf_smp_level_products_ex_f32";
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (rows < 0 || (rows > 0 && (!A || !rowfac || !Wst || !trow || !Out))) return fail(ctx, GF_ERR_INVALID, "%s: null argument", who);
    if (nx == 3 && !X) return fail(ctx, GF_ERR_INVALID, "%s: three extra products without their weight blocks", who);
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    gf::RowProductsCall call = {backward == 0, A, rowfac, Wst, Out, rows, trow};
    call.trowf = trowf, call.C = C, call.nf = nf, call.nx = nx, call.skip_zero_grads = skip_zero_grads != 0;
    // On the split kernels the call carries what a level prepares for them: its prebuilt weight images (both directions) and, for a
    // packed table at C = 64, the table's row classes (the level builds them once per batch).  Their room in the workspace comes first,
    // so that the choice sees the whole call, refusals come before anything is launched, and an empty matrix is refused like any other.
    const size_t CC = (size_t)C * C, img_bytes = gf::align_up(gf::smp_split_image_bytes(C), 256), w_bytes = gf::align_up(sizeof(float) * 18 * CC, 256);
    const bool split = gf::smp_split_products(ctx), classes = split && trowf && C == 64 && rows < (1 << 29);
    gf_status st = GF_OK;
    int *cls = nullptr;
    if (split) {
        st = gf::ensure_ws(ctx, img_bytes + w_bytes + (classes ? sizeof(int) * gf::smp_row_class_ints(rows) : 0) + 256);
        if (st != GF_OK) return st;
        call.wimg = ctx->ws;
        if (classes) call.rowcls = cls = reinterpret_cast<int *>(static_cast<char *>(ctx->ws) + img_bytes + w_bytes);
    }
    st = gf::smp_row_products_admissible(ctx, call);
    if (st != GF_OK) return st;
    if (rows == 0) return GF_OK;
    st = gf::check_tables(ctx, who, rows, trow, trowf, 0);
    if (st != GF_OK) return st;
    if (split) {
        if (cls) {
            st = gf::smp_build_row_classes(ctx, ctx->stream, trowf, rows, cls);
            if (st != GF_OK) return st;
        }
        // the builder reads the level's EIGHTEEN stacked blocks: the eight row products' first, the other ten as zeros
        void *img = ctx->ws;
        float *w18 = reinterpret_cast<float *>(static_cast<char *>(ctx->ws) + img_bytes);
        GF_HIP_TRY(ctx, hipMemcpyAsync(w18, Wst, sizeof(float) * 8 * CC, hipMemcpyDeviceToDevice, ctx->stream));
        GF_HIP_TRY(ctx, hipMemsetAsync(w18 + 8 * CC, 0, sizeof(float) * 10 * CC, ctx->stream));
        const float *wp = w18, *xp = nx == 3 ? X : nullptr;
        st = gf::smp_split_build_images(ctx, &wp, &img, 1, C, &xp);
        if (st != GF_OK) return st;
    }
    return gf::smp_row_products(ctx, call);
}

gf_status gf_smp_level_row_classes(gf_ctx *ctx, int rows, const int *trowf, int *lists) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (rows < 1 || rows >= (1 << 29) || !trowf || !lists) return fail(ctx, GF_ERR_INVALID, "gf_smp_level_row_classes: bad argument");
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return gf::smp_build_row_classes(ctx, ctx->stream, trowf, rows, lists);
}
gf_status gf_smp_level_row_classes_ex(gf_ctx *ctx, int rows, const int *trowf, int *lists, int live_only) {
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (rows < 1 || rows >= (1 << 29) || !trowf || !lists) return fail(ctx, GF_ERR_INVALID, "gf_smp_level_row_classes_ex: bad argument");
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return gf::smp_build_row_classes(ctx, ctx->stream, trowf, rows, lists, live_only != 0);
}

gf_status gf_smp_level_wgrad_ex_f32(gf_ctx *ctx, int C, int nf, int nx, int rows, const float *T, const float *dO, const float *rowfac,
                                    const int *trow, const int *trowf, float *dWst, float *dX) {
    static const char *who = "gf_smp_level_wgrad_ex_f32";
    if (!ctx) return fail(nullptr, GF_ERR_INVALID, "null context");
    if (rows < 1 || !T || !dO || !rowfac || !trow || !dWst) return fail(ctx, GF_ERR_INVALID, "%s: bad argument", who);
    if (nx == 3 && !dX) return fail(ctx, GF_ERR_INVALID, "%s: three extra products without a place for their gradients", who);
    gf_status st = gf::check_wgrad_variant(ctx, who, C, nf, nx, trowf != nullptr);
    if (st != GF_OK) return st;
    GF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    st = gf::check_tables(ctx, who, rows, trow, trowf, gf::kGatherWindow);
    if (st != GF_OK) return st;
    // workspace: the eight products' partial images and the extra products' (each with its fold's second stage), the scratch words of
    // the column bounds, three words of row-factor maxima
    const size_t part_floats = gf::smp_wgrad_part_floats(ctx, rows, C, nx), words = gf::smp_wgrad_words(C);
    st = gf::ensure_ws(ctx, sizeof(float) * (part_floats + words + 4) + 256);
    if (st != GF_OK) return st;
    float *part = static_cast<float *>(ctx->ws);
    unsigned *bw = reinterpret_cast<unsigned *>(part + part_floats), *rmax = bw + words;
    gf::WgradCall wc = {T, dO, rowfac, rows, C, nf, trow, trowf, gf::WgradScales(), bw, part, part_floats};
    if (nf == 8) {
        // per-product row factors: the kernel takes the level's bounds, not exact ones.  Any upper bound will do: chan = the largest
        // magnitude of every channel over the four blocks of T | over the two of dO (widened by the factors of products 3 and 4),
        // smax = 1, row_max = the largest factors that ride on tot / on tr
        GF_HIP_TRY(ctx, hipMemsetAsync(bw, 0, sizeof(unsigned) * (words + 4), ctx->stream));
        for (int k = 0; k < 4; ++k) {
            st = gf::smp_wgrad_channel_maxima(ctx, T + k * C, rows, 4 * C, dO + (k & 1) * C, k < 2 ? rows : 0, 2 * C, C, bw);
            if (st != GF_OK) return st;
        }
        GF_LAUNCH(ctx, "smpf_colmax", gf::rowfac8_absmax, dim3(64), dim3(256), 0, rowfac, rows, rmax);
        GF_LAUNCH(ctx, "smpf_colmax", gf::scale_words, dim3(1), dim3(64), 0, bw + C, C, rmax + 2);
        wc.bounds.chan = bw, wc.bounds.smax = 1.f, wc.bounds.row_max = rmax;
    }
    gf::FoldGroup fg, xg = {nullptr, 0, 0};
    st = gf::smp_wgrad_partials(ctx, wc, &fg, nx == 3 ? &xg : nullptr);
    if (st != GF_OK) return st;
    st = gf::splitk_fold(ctx, fg.part, dWst, fg.n, fg.splits, 0);
    if (st != GF_OK || nx != 3) return st;
    if (!xg.splits) return fail(ctx, GF_ERR_UNSUPPORTED, "%s: no kernel with the three extra products at %d channels / %d row factors", who, C, nf);
    return gf::splitk_fold(ctx, xg.part, dX, xg.n, xg.splits, 0);
}

}  // extern "C"
