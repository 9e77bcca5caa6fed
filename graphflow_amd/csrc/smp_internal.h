// smp_internal.h -- state of one gf_smp handle (gf_smp_batch: what one prepared batch owns; gf_smp: what survives it) and what its translation
// units share: smp.hip (create / plan, the sweeps, op-by-op levels), smp_prepare.hip (buffer pool, device-built tables, every path of
// gf_smp_prepare* on one begin_batch / finish_batch skeleton), smp_pad.hip (channel padding, the ver6 / ver7
// embedding), smp_optim.hip (host-pointer mode, optimisers, checkpoints), smp_fused.hip + smp_level_*.hip (fused levels; the fused level's block products
// and their weight gradients are called through RowProductsCall / WgradCall below, their two files share smp_split.h), smp_model.hip.
// Which configurations become a handle is smp_config.h's business, the parameter layout smp_prep.h's (gfsmp::Config::level_blocks).
#ifndef GF_SMP_INTERNAL_H_INCLUDED
#define GF_SMP_INTERNAL_H_INCLUDED

#include <vector>

#include "gf_internal.h"
#include "smp_config.h"
#include "smp_optimisers.h"
#include "smp_prep.h"

namespace gf {
gf_status gemm(gf_ctx *ctx, bool ta, bool tb, int M, int N, int K, const float *A, int lda, long long sA, const float *B,
               int ldb, long long sB, float *C, int ldc, long long sC, int batch, int accumulate);
gf_status gemm_rs(gf_ctx *ctx, bool ta, bool tb, int M, int N, int K, const float *A, int lda, long long sA, const float *B,
                  int ldb, long long sB, float *C, int ldc, long long sC, int batch, int accumulate, const float *rs,
                  int rs_ld, int scol);
// one GEMM of a grouped launch (mixers.hip): op(A)[M,K] op(B)[K,N] -> C[M,N]; nseg > 0 splits K into pieces
struct GemmSpec {
    const float *A, *B;
    float *C;
    int M, N, K, lda, ldb, ldc;
    int nseg;
    long long a_off[4], b_off[4];
    int klen[4];
    const float *rs;  // optional per-row scaling of op(A) (GemmArgs::rs in mixers.hip); nullptr = none
    int rs_ld;
    int scol[4];      // column of rs per K piece (piece 0 when nseg == 0), < 0 = unscaled piece
};
// partial images of one product of a split launch: `splits` images of n floats back to back from `part` on
struct FoldGroup {
    const float *part;
    int splits;
    size_t n;
};
gf_status gemm_grouped_free(gf_ctx *ctx, bool tb, const GemmSpec *specs, int n, const char *name);
gf_status gemm_grouped_free_tn(gf_ctx *ctx, const GemmSpec *specs, int n, float *part, size_t part_floats, FoldGroup *out,
                               const char *name);
bool gemm_grouped_supported(const GemmSpec *specs, int n, bool ta, bool tb);
gf_status gemm_grouped_rows(gf_ctx *ctx, bool ta, bool tb, const GemmSpec *specs, int n, int rows, int accumulate = 0);
gf_status gemm_grouped_splitk(gf_ctx *ctx, const GemmSpec *specs, int n, int rows, float *dest, int accumulate);
// ---- the eight row block products of a fused level (smp_level_c64_split.hip; the fp32 pipe's kernel: smp_level_c64.hip), C = 16 / 32 / 64 / 128 ----
// dz (backward, C = 64, the row-class kernel -- smp_row_products_can_form_dz; else its members null): the L block of dO is formed by the
// kernel from the read-out's per-node vector and the level's sign words instead of read (see smp_rowpanel_split, DZ)
struct RowpanelDz {
    const float *node_df = nullptr;   // [nodes][64]
    const unsigned *sgn = nullptr;    // [rows][2]
    const int *ent_node = nullptr;    // [class-list entries] node of the entry's row
};
// One call: forward O from T = [S_ab|S_bc|T6|T10], or backward dT from dO, on `rows` rows.
struct RowProductsCall {
    bool forward;
    const float *A, *rowscale, *Wst;   // the operand rows, nf factors per row, the level's stacked weights
    float *Out;
    int rows;
    const int *trow;             // != nullptr: compact O / dO layout ([O_loc | U], 2C wide) with the transposed-row gather inside the product (see kernel)
    const int *trowf = nullptr;  // (optional) the level's packed table with the presence bits of the S_ab / T6 blocks (DevLevel::trowf)
    const int *rowcls = nullptr; // the table's row classes (C = 64 with trowf: panels of one class, see smp_rowpanel_split)
    const void *wimg = nullptr;  // the level's prebuilt weight images (smp_split_build_images); C != 64: split products with prebuilt images only
    int C = 64;
    int nf = 2, nx = 0;          // row factors per row of `rowscale`: 2 = (tot, tr); 8 = one per product (slice dropout, C = 32 / 16); nx = 3: SMP_2D_ver7's extra products
    bool skip_zero_grads = false;   // backward: the gradients of the structurally-zero S_ab / T6 blocks have no reader and are not stored
    bool skip_empty = false;     // forward, C = 64, packed table: rows without any data are not stored (FusedRoute::skip_empty)
    RowpanelDz dz;               // dz.node_df null: none
};
// THE entry point: picks the kernel (row_products_kernel of smp_level_c64_split.hip -- the one place that decides which kernel runs and
// whether a call is admissible) and launches it.  Every output element is produced by one wave in a fixed order: results do not depend
// on the grid size.
gf_status smp_row_products(gf_ctx *ctx, const RowProductsCall &call);
// the refusal of a call the choice does not admit (status, reason recorded), before anything is launched; GF_OK otherwise
gf_status smp_row_products_admissible(gf_ctx *ctx, const RowProductsCall &call);
// will this backward call run the row-class kernel (the one that can form dz itself)?  Asked with call.dz still empty.
bool smp_row_products_can_form_dz(const gf_ctx *ctx, const RowProductsCall &call);
// the compact-layout products on the f16 matrix pipe with two-half fp32 operands (smp_level_c64_split.hip; GF_SMP_SPLIT=0: fp32 MFMA)
bool smp_split_products(const gf_ctx *ctx);
// (smp_level_c64.hip: the fp32 kernel's launch, for smp_row_products; trow null: the three-block O layout)
gf_status smp_row_products_fp32_c64(gf_ctx *ctx, bool forward, const float *A, const float *rowscale, const float *Wst, float *Out, int rows, const int *trow);
// the row classes of a level's packed table (smp_prepare.hip: row_class_count): buffer size in ints, and the builder
// live_only: a row with none of the three presence bits (an EMPTY row: no data in any block of T) goes into neither list
size_t smp_row_class_ints(int rows, bool live_only = false);
gf_status smp_build_row_classes(gf_ctx *ctx, hipStream_t stream, const int *trowf, int rows, int *buf, bool live_only = false);
// ... and the node of every entry of the two lists (rows + 64 ints), for the kernel that forms dz from a per-node vector
gf_status smp_build_row_class_nodes(gf_ctx *ctx, hipStream_t stream, const int *buf, int rows, const long long *node_row, int nodes, int *ent_node);
// the split kernels' weight images of a level (both directions), built once per forward pass (smp_level_c64_split.hip)
size_t smp_split_image_bytes(int C = 64);   // (C = 128: four sets, one per 64 x 64 sub-block of the 128 x 128 weight blocks)
gf_status smp_split_build_images(gf_ctx *ctx, const float *const *Wst, void *const *img, int n, int C = 64, const float *const *X = nullptr);
gf_status smp_small_split_c64(gf_ctx *ctx, bool transposed, int n, const int *prog, const float *const *In, float *const *Out, const int *rows,
                              const int *pos0, const void *wimg, const char *name, int C = 64);
gf_status splitk_fold(gf_ctx *ctx, const float *part, float *dest, size_t total, int splits, int accumulate);

// ---- the weight gradients of a fused level's eight row block products (smp_level_wgrad_split.hip), C = 16 / 32 / 64 / 128 ----
// Where the split-operand kernels take their per-column exponents from: the level's per-channel maxima `chan` ([2 C] float bits: max
// |f_{l-1}| then max |dz_l|, smp_wgrad_channel_maxima) with the largest receptive field and row factors of the level -- or nothing: exact
// column bounds are then taken from the operands themselves (one extra pass over T and dO).
struct WgradScales {
    const unsigned *chan = nullptr;
    float smax = 0.f, max_tot = 0.f, max_tr = 0.f;
    const unsigned *row_max = nullptr;   // {max |tot|, max |tr|} as float bits in device memory; they replace max_tot / max_tr at 64
    // channels (device-built tables) and are the only form the 32- / 16-channel kernel takes
    bool level(int C) const { return chan && (C == 64 || row_max); }
};
// One call: the operands T [rows][4 C], dO [rows][2 C] (compact layout; trow null at 64 channels: [rows][3 C] on the fp32 pipe) and
// rowscale [rows][nf] (nf = 2: (tot, tr); 8: one factor per product, 32 / 16 channels with level bounds only), the level's plain and
// packed transposed-row tables, the bounds, and the workspace: smp_wgrad_words(C) scratch words for exact bounds (null at 64 channels =
// none: without level maxima the fp32 kernel runs, as it does when the split products are switched off) and room for the images.
struct WgradCall {
    const float *T, *dO, *rowscale;
    int rows, C, nf;
    const int *trow, *trowf;
    WgradScales bounds;
    unsigned *words;
    float *part;
    size_t part_floats;
    bool any_trow = false;   // trow may leave the gather window of the split kernels (a caller's table at 64 channels): smp_wgrad_split then
                             // reaches dU[trow] through one descriptor over all of dO, which must be smaller than kWgradWholeBytes
    bool skip_empty = false; // 64 channels, packed table: dO of a row without any data was not written and is not read (FusedRoute::skip_empty)
};
constexpr size_t kWgradWholeBytes = 0x40000000;   // (1 GiB: the out-of-range offset of an absent block must stay beyond that descriptor)
// scratch words per level; exact = false: of a level that only ever keeps its channel maxima there (the 64-channel levels of a model)
size_t smp_wgrad_words(int C, bool exact = true);
// floats of partial images a call of `rows` rows may need, the folds' second stage and nx extra products' images included
size_t smp_wgrad_part_floats(gf_ctx *ctx, int rows, int C, int nx = 0);
// will this call read the absent S_ab / T6 blocks of T?  Then they must hold their zeros before it runs (smp_fused_ensure_zero_fill).
bool smp_wgrad_reads_absent_blocks(const gf_ctx *ctx, const WgradCall &call);
// Picks the kernel -- fp32 pipe or smp_wgrad_split at 64 channels, smp_wgrad_all<32 | 16>, four sub-block launches of smp_wgrad_split at
// 128 -- and leaves out->splits partial images of 8 C^2 floats in call.part for the caller to fold in order.  xout (optional): the three
// extra products of SMP_2D_ver7 in the same launch, images of 3 C^2 floats; xout->splits == 0 where the kernel or the room does not allow.
gf_status smp_wgrad_partials(gf_ctx *ctx, const WgradCall &call, FoldGroup *out, FoldGroup *xout = nullptr);
gf_status smp_wgrad_channel_maxima(gf_ctx *ctx, const float *fprev, long long prev_rows, int ld0, const float *dsrc, long long drows, int ld1, int C,
                                   unsigned *words);
gf_status smp_wgrad_fp32_c64(gf_ctx *ctx, const float *T, const float *dO, const float *rowscale, int rows, int kchunk, int splits, float *part,
                             const int *trow);   // (smp_level_c64.hip: the fp32 kernel's launch, for smp_wgrad_partials)

// ---- the row-list GEMM level (smp_level_rowlist.hip): A[r][slot * Cin + c] = sum over the entries e of row r with that slot of
// coef[e] * X[src[e]][c], as a CSR list whose rows are in ascending slot order; device pointers ----
struct RowList {
    const long long *ptr = nullptr;   // [R + 1]
    const int *src = nullptr, *slot = nullptr;
    const float *coef = nullptr;      // null: every coefficient is 1
    const long long *sptr = nullptr;  // optional [R slots + 1]: the first entry of every (row, slot); the kernels then search nothing
};
// out [R][N] = act(A B + bias) (act 1: LeakyReLU 0.01; bias may be null); tb: B is the forward's [slots][N][Cin], read transposed per slot
gf_status smp_rowlist_product(gf_ctx *ctx, const RowList &list, bool tb, int R, int slots, int Cin, int N, const float *X, const float *B,
                              const float *bias, int act, float *out);
// dB [slots Cin][N] += A^T dOut, at most kRowlistSplits partial images in the context's workspace, folded in ascending order
gf_status smp_rowlist_wgrad(gf_ctx *ctx, const RowList &list, int R, int slots, int Cin, int N, const float *X, const float *dOut, float *dB);
size_t smp_rowlist_wgrad_ws_bytes(int R, int K, int N);
gf_status smp_rowlist_bias_grad(gf_ctx *ctx, const float *dOut, int R, int N, float *db);   // db [N] += the column sums of dOut
}


namespace gf {
// The handle of a configuration as `entry` asks for it (gfsmp::resolve_config decides, before anything is allocated).
// pad_channels = false: compute at the configuration's own channel counts; min_pad: the smallest padded width the handle may compute at
// (32 for the towers of a slice-dropout model)
gf_status smp_create(gf_ctx *ctx, const gf_smp_config *cfg, const gfsmp::ConfigEntry &entry, bool pad_channels, gf_smp **out, int min_pad = 0);
void smp_derive_plan(gf_smp *s, bool allow_embed);
gf_status smp_switch_plan(gf_smp *s, bool embed);
constexpr int kPadMaxLevels = 15;   // levels a padded model's layout map holds (gf_smp_create: deeper models compute at nChanels)
}
// The state of ONE prepared batch.  The rule: from the pool (upload_bytes) or derived from the batch => here; release() resets all of it, with
// one assignment of a value-initialised gf_smp_batch, so no pointer outlives the block behind it and no prepare path nulls a field by hand.
// What survives a batch is gf_smp's: configuration and plan, the pool, the upload stream, `lay` (its host vectors are reused for their
// capacity), everything from hipMalloc (rs_inv, pad_*, own_p / own_g, adam_*, mask_stage), the per-pass flags (the passes' own business).
struct gf_smp_batch {
    bool prepared = false, forwarded = false;
    // context workspace this batch needs.  gf_smp_prepare only RECORDS it (prepare may run on a loader thread while another
    // handle's step uses the context's workspace on the compute thread); gf_smp_forward / gf_smp_backward grow the workspace, on
    // the thread that owns the context's stream
    size_t ws_need = 0;
    // device buffers (from the pool)
    struct DevLevel {
        int *node_s = nullptr;
        long long *node_row = nullptr, *node_p = nullptr, *node_pair = nullptr;
        float *adj = nullptr, *rsum = nullptr, *rowscale = nullptr, *node_scale = nullptr;
        int *quad_node = nullptr, *quad_b0 = nullptr, *quad_order = nullptr;
        int *pair_node = nullptr, *pair_src_s = nullptr, *cons_s = nullptr;
        long long *pair_src_row = nullptr, *cons_ptr = nullptr, *cons_slab = nullptr, *cons_inv_off = nullptr;
        short *pi = nullptr, *inv = nullptr;
        int4 *cons_hdr = nullptr, *cons_qrec = nullptr;  // tables of smp_bwd_gather_v2 (smp_fused.hip: build_gather_records)
        long long *cons_qbase = nullptr;                 // [nodes of level l-1] first record of the source's consumer entries
        // fused forward level at C = 64 (smp_level_c64_fwd.hip): row panels of whole (node, x) groups, per-row gather indices
        int4 *fwd_pan = nullptr;
        int *cons_of_pair = nullptr;       // [pairs] index of a pair in its source's consumer list (build_node_tables)
        bool node_tables_merged = false;   // this batch's rows-sized tables of the level came from build_node_tables (smp_prepare.hip)
        int *fwd_pan_node = nullptr, *node_panel = nullptr;
        int2 *fwd_goff = nullptr;
        int fwd_npanels = 0;
        // Rows (a, b) of T whose source a does not contain vertex b (pi < 0: half of them at QM9 sizes) are structurally zero in
        // the S_ab and T6 blocks.  Their zeros are written ONCE per prepared batch (tables_zero_fill, the first fused forward) and
        // tables-forward then skips them; rowflag[row] = 1 where the row is written every step.  t_zeros goes false whenever
        // something else may have overwritten the T region of Q (an op-by-op forward of the level).
        bool t_zeros = false;
        bool t_filled = false;   // ... and the zeros are physically there (tables_zero_fill ran: some reader of T does not mask them)
        unsigned char *rowflag = nullptr;
        int *trow = nullptr;  // [rows] row of (e, x) for row (x, e) of the same node (compact O layout of the fused C = 64 level)
        int4 *tf_recs = nullptr;  // [2 nNodes] records of tables-forward in launch order (build_tf_records)
        float *psum = nullptr;     // top level, C = 64: [fwd_npanels][64] column sums of the row panels of f_L (readout)
        float *dshl = nullptr;     // towers: [nodes][C] gradient of the level's read-out per node (the fused level's combine-backward adds it)
        bool psum_ready = false;   // ... written by this forward pass
        // C = 64: [rows][2] sign words of z_l, written by the panel combine-forward (bit c of word h: z[row][32 h + c] > 0).  The reverse
        // sweep takes LeakyReLU'(f_l) from them instead of reading f_l (smp_sign_mask).  Rows of nodes above 32 positions: not written.
        unsigned *sgn = nullptr;
        bool sgn_ready = false;    // ... written by this forward pass
        // per-channel maxima for the weight gradients' column exponents (smp_level_wgrad_split.hip: WgradScales::chan):
        float *pmax = nullptr;     // [fwd_npanels][64] largest |f_l| of every row panel, left by combine-forward (levels below the top)
        float *dzmax = nullptr;    // [max(quads, row panels)][64] largest |dz| of every workgroup / panel of combine-backward
        long long dz_rows = 0;     // ... rows of it the last combine-backward wrote
        int dz_ld = 64;            // ... and their width in floats
        long long dz_rows2 = 0, dz_off2 = 0;   // a second set behind them (floats from dzmax), of another width: the workgroup kernel's rows for the
        int dz_ld2 = 64;                       // nodes above 32 positions of a 32- / 16-channel level (panel rows are C floats wide, its rows 32 / 64)
        bool pmax_ready = false;
        void *wimg = nullptr;  // the split product kernels' weight images of this pass (smp_split_build_images), C = 64
        bool wimg_ready = false;
        bool fwd_c64 = false;  // the last forward ran this level's products on the dedicated row-panel kernels (compact O = [O_loc | U])
        int *trowf = nullptr;  // [rows] trow | bit 31: rowflag of the row | bit 30: rowflag of the transposed row (smp_rowpanel_split)
        int *rowcls = nullptr;  // C = 64: the rows with and without S_ab / T6 data as two padded lists (smp_prepare.hip: row_class_count)
        int *rowcls_node = nullptr;  // ... the node of every list entry (top level of a plain model: the backward products form dz themselves)
        // C = 64: one word per combine panel, bit i = row pan[p].x + i has data in some block of T (any of bits 31 / 30 / 29 of trowf);
        // with it the level's lists in rowcls leave the empty rows out (smp_prepare.hip: row_class_count, live_only)
        unsigned *pan_live = nullptr;
        float max_tot = 0.f, max_tr = 0.f;  // largest |tot|, |tr| of the level's row factors (split-operand weight gradients' column bounds)
        const unsigned *row_max = nullptr;  // the same two as float bits in device memory when the tables are built there
        long long *pair_src_pair = nullptr, *cons_row = nullptr, *cons_pair = nullptr;  // compact diagonal path (smp_prep.h)
        int *node_center = nullptr, *cons_a = nullptr, *mol_order = nullptr, *gather_items = nullptr;
        float *Fdc = nullptr, *Gc = nullptr, *dGc = nullptr, *dFdc = nullptr;  // [pairs of level l-1][2C] each
        float *f = nullptr, *df = nullptr, *Q = nullptr;  // activations [rows][C], their gradient, contraction out [rows][18C]
        // physics towers (every level is read out): per-node sums of f, their LeakyReLU, vertex -> node and node -> molecule maps
        float *sh = nullptr, *vf = nullptr;
        int *node_of_vertex = nullptr, *node_mol = nullptr;
        int *node_present = nullptr;  // [nodes] rows with data of the node (device-built tables)
        int *field = nullptr;  // [pairs] receptive fields back to back (device-built level tables: smp_prepare.hip build_level_rows)
        unsigned *keep_mask = nullptr;  // [nodes] slice masks of RisiContraction_18_dropout for this forward (gf_smp_dropout_masks)
        float *nodefac = nullptr, *rowfac8 = nullptr;  // fused levels under slice dropout: [nodes][18] slice factors, [rows][8] per-product row factors
        // fused level (smp_fused.hip): small per-(node,x) / per-node tables and stacked weights
        float *Vt = nullptr, *dVt = nullptr;        // [pairs][4C]  rowsum_a | colsum_b | D8 | D11
        float *St = nullptr, *dSt = nullptr;        // [nodes][4C]  total | s14 | s15 | s18
        float *scal = nullptr;                      // [pairs][4C]  partial scalars owned by (node, b)
        float *Vout = nullptr, *dVout = nullptr;    // [pairs][C]
        float *Sout = nullptr, *dSout = nullptr;    // [nodes][C]
        float *dSpart = nullptr, *dbpart = nullptr; // [pairs][C]
        float *Wst = nullptr, *dWst = nullptr;      // [18][C][C] block-permuted K_l and its gradient
        // first-order level (smp_level_theta.hip, smp_field_level.h; tables of smp_prep.h: th_*): G / dG live in Q, the weight views in Wst / dWst
        long long *th_child_ptr = nullptr, *th_src_row = nullptr, *th_pi_off = nullptr, *th_cons_ptr = nullptr, *th_cons_row = nullptr,
                  *th_inv_off = nullptr;
        int *th_src_s = nullptr, *th_cons_s = nullptr, *th_cons_node = nullptr, *th_bucket = nullptr, *th_weight = nullptr;
        short *th_pi = nullptr, *th_inv = nullptr;
        float *th_A = nullptr;     // [rows][Cc] A[i] = sum over the children of G_top (kept for dlambda1)
        float *th_B = nullptr;     // [nodes][Cc] B = sum over positions and children of G_bot (kept for dlambda2)
        float *th_node = nullptr;  // [nodes][3 Cc] reverse sweep: sum_i dz[i] | sum_i dz[i] A[i] | (sum_i dz[i]) B
        // steerable second-order level (smp_level_2d.hip): th_A = S [rows][Cp], th_B = col [sum s][Cp], th_node = [sum s][Cc + 3 Cp] column
        // partials of the reverse sweep, adj / node_pair as in gfsmp::LevelLayout, part2d = [blocks][Cp] partial sums of dscalar
        float *part2d = nullptr;
        // SMP_2D_ver5 (smp_level_2d_ver5.hip) beside them: row -> (column, s) and column -> s (written by its forward gather), u and dO
        // [sum s][C], dE in Q [rows][C], the chunk partials of dK_l [smp_2d_ver5_wgrad_chunks][C][C]
        int2 *v5_row_cs = nullptr;
        int *v5_col_s = nullptr;
        float *v5_u = nullptr, *v5_dO = nullptr, *v5_dKpart = nullptr;
        // unrestricted level (smp_level_unrestricted.hip): th_A = S [rows][Cp], Q = dS [rows][Cp], part2d = the chunk partials of the
        // per-size entries at un_part_off (gfsmp::LevelLayout), th_node = [sum s][2 Cp] column partials (db | dscalar) in form 3
        long long *un_part_off = nullptr;
        // neighbourhood level (smp_level_neighbourhood.hip; every buffer [vertices][H] unless noted): f = h_l, df = dh_l and then dz_l in
        // place, th_A = n_l, Q = dn_l; form 3: th_B = A = sum of the members' h_{l-1}, th_node = dn_l Tt, nb_T [vertices] = sum_k h_l[v][k],
        // nb_Tt [vertices] = sum of the members' nb_T of level l - 1, nb_sA [vertices] = <dn_l, A>.  The lists are shared between the levels
        // of one radius (gfsmp::BatchLayout::nb_lists).
        const long long *nb_ptr = nullptr, *nb_tptr = nullptr;
        const int *nb_idx = nullptr, *nb_tidx = nullptr;
        float *nb_T = nullptr, *nb_Tt = nullptr, *nb_sA = nullptr;
        // gated level (smp_level_gru.hip; levels >= 1, [vertices][H] each) beside them: the gates z_l, r_l, the candidate c_l, q = r h_{l-1};
        // dz', dr', dc' (the operands of the six weight gradients) and the direct part of dh_{l-1}.  nb_T of a level >= 1 is the sum of an
        // arbitrary vector.  The read-out's sigmoid, tanh and their two gradients live in the handle (gf_smp::gru_*).
        float *gru_z = nullptr, *gru_r = nullptr, *gru_c = nullptr, *gru_q = nullptr;
        float *gru_dz = nullptr, *gru_dr = nullptr, *gru_dc = nullptr, *gru_direct = nullptr;
        // third-order pool (smp_level_third.hip; neighbourhood = 6, 7; levels >= 1): nb_sel [vertices][H] = the canonical triple per rank
        // (x | y << 8 | z << 16, -1 under three members), nb_pool [vertices][H] = the pooled n_l where the update kernel reads it through
        // the identity list (form 6; form 7's cell reads th_A), nb_max_members = the longest list of the level
        int *nb_sel = nullptr;
        float *nb_pool = nullptr;
        int nb_max_members = 0;
    };
    // matrix-form handles (cfg.matrix_form; smp_level_rowlist.hip): the level's row lists, forward and transposed.  GCN_MW: lv[l].f = h_l,
    // lv[l].df = dh_l and then dz_l in place, [vertices][H].  LCNN: lv[1].f = a1 and lv[1].df = da1 / dc1 [nMol V][C1], lv[2].f = c2 and
    // lv[2].df = dc2 [nMol V][C2], lv[2].Q = the gradient of the dense layer [nMol][nDense]; g = the dense layer itself.
    gf::RowList rl_fwd, rl_bwd;
    // covariant handles (cfg.covariant; smp_level_covariant.hip): the column lists N(v) and their transposes over global vertex ids, the hop
    // counts cov_hop [vertices][M] (gfsmp::BatchLayout::cov_hop), and what the forward leaves for the reverse: cov_h [L + 1][vertices][M] =
    // every h_l[v], cov_n [L][vertices][M] = every n_l[v] (l = 1 .. L), cov_ds0 [vertices] = the gradient of <x[v], H>.  g is [nMol][M].
    const long long *cov_ptr = nullptr, *cov_tptr = nullptr;
    const int *cov_idx = nullptr, *cov_tidx = nullptr;
    unsigned char *cov_hop = nullptr;
    float *cov_h = nullptr, *cov_n = nullptr, *cov_ds0 = nullptr;
    // the list N(v) = {v} over the batch's vertices (form 6: the sum instantiation of nbh_level_fwd over it hands the pooled n on unchanged)
    long long *nb_id_ptr = nullptr;
    int *nb_id_idx = nullptr;
    std::vector<DevLevel> lv;
    // distance handles (cfg.distance_channel; smp_level_distance.hip): the distance channel's levels -- the neighbourhood level's buffers of
    // DevLevel, the lists shared with lv -- its input rows xd [vertices][max_nVertices] (dist_rows_sort), and what the sort reads: the
    // molecules' distance matrices and their offsets.  g is [nMol][2 H].
    std::vector<DevLevel> lvd;
    float *xd = nullptr;
    double *mol_dist = nullptr;
    long long *mol_dist_off = nullptr;
    // Gram handles (cfg.readout = 2; smp_level_readouts.hip): the molecules' adjacency VALUES as floats and the last forward's Gram matrices,
    // V_m^2 floats each, back to back (gram_count together), gram_off [nMol + 1] the molecules' first entries
    float *gram_adj = nullptr, *gram = nullptr;
    long long *gram_off = nullptr;
    size_t gram_count = 0;
    // device-built level tables: the batch's adjacency matrices and the per-level statistics the kernels leave behind
    int *mol_nv = nullptr, *mol_adj = nullptr;
    long long *mol_adj_off = nullptr;
    double *mol_coul = nullptr;
    unsigned *tab_stats = nullptr;          // [levels + 1][4]: max |tot|, max |tr| (float bits), rows with data (two words)
    std::vector<unsigned> h_tab_stats;
    std::vector<long long> h_covered;       // [levels + 1] cache of gf_smp_level_covered_rows (-1 = not read yet), cleared by prepare
    // [levels + 1][smp_wgrad_words(C, C != 64)] scratch words of the levels' weight gradients (smp_level_wgrad_split.hip: wgrad_words): the
    // per-channel maxima of f_{l-1} and of dz_l (at C = 64 nothing else, zeroed at the start of every forward) and the exact column bounds
    unsigned *wbound = nullptr;
    float *x = nullptr;      // [nVertices][FD]
    float *P = nullptr;      // shared promotion / dP buffer, max over levels of ppos*C; allocated on first use (ensure_P):
    size_t P_count = 0;      // the fused levels with the folded backward gather never materialise it
    float *sh = nullptr, *vf = nullptr;  // [nNodes][C] readout pre/post activation
    float *dsh = nullptr;                // [nNodes][C] gradient of sh (the fused top level reads it per node)
    float *g = nullptr;      // [nMol][C] graph features
    float *yhat = nullptr, *dy = nullptr;  // [nMol]
    // gated read-out (smp_level_gru.hip; [vertices][H] each): sigmoid(W_g h_L), tanh(U_g h_L), and the gradients of their arguments
    float *gru_s = nullptr, *gru_t = nullptr, *gru_ds = nullptr, *gru_dt = nullptr;
    float *gru_acc = nullptr;   // [param_count] the sweep of a gf_smp_backward with accumulate = 1, before it is added (taken on first use)
    // classifier handles (cfg.nClass >= 2, smp_readout_classes.hip): logits, softmax, dz = p - onehot [nMol][nClass]; dg = W^T dz [nMol][C]
    float *cls_scores = nullptr, *cls_prob = nullptr, *cls_dz = nullptr, *cls_dg = nullptr;
    float *colpart = nullptr;  // partial column sums for bias gradients, [colpart_rows][C]
    size_t colpart_rows = 0;
    int *top_node_mol = nullptr, *mol_ptr = nullptr, *mol_nodes = nullptr;
    float *own_t = nullptr, *own_y = nullptr, *own_loss = nullptr, *own_feat = nullptr;  // per-batch, freed by release()
    float *fit_t = nullptr, *fit_y = nullptr, *fit_loss = nullptr, *fit_feat = nullptr;  // the same per SAMPLE (smp_fit.hip: a pair, else a molecule)
    float *fit_gram = nullptr;   // [gram_count] staging of gf_smp_gram_host
};
struct gf_smp : gf_smp_batch {
    gf_ctx *ctx = nullptr;
    gfsmp::Config cfg;    // what the device computes with: nChanels padded to 32 / 64 / a multiple of 4 (gf_smp_create, round 4)
    bool bwd_consumed = false;   // an op-by-op level's reverse sweep has overwritten its Q since the last forward
    long long single_launches = 0;   // launches of smp_tables_fwd_single / smp_bwd_gather_single so far (gf_smp_single_vertex_launches)
    long long empty_row_calls = 0;   // level passes, forward or backward, that ran with FusedRoute::skip_empty (gf_smp_empty_row_calls)
    gfsmp::Config ucfg;   // the caller's configuration: the layout of parameters, gradients, features and activations at the C ABI
    float *pad_p = nullptr, *pad_g = nullptr, *pad_feat = nullptr;   // padded copies (cfg.nChanels != ucfg.nChanels)
    // Round 5, SMP_2D_ver6 (RisiContraction_10) on the fused RisiContraction_18 level: != 0 = the caller's channel count C.  With a symmetric
    // reduced adjacency every one of the ten "1+1+1" slices is a slice of RisiContraction_18 applied to f_{l-1} or to its per-node
    // TRANSPOSE (smp_pad.hip: v6_slot), so the device computes an 18-slice model on [f | f^T | 0] channels: channels [C, 2C) of every level's
    // activations hold the transposed matrices (dup_transposed_channels after each level, fold_transposed_channels in the reverse sweep)
    int dup_channels = 0;
    // ... and SMP_2D_ver7 (RisiContraction_50) likewise: 46 of its 50 slices are slices of RisiContraction_18 on f or f^T; the other four
    // (cases 25, 41, 42, 45: S_bc tr and the three pair marginals weighted by the adjacency's diagonal, which is 1 in a reduced adjacency)
    // are n_extra = 3 more C x C products on the level's tables -- (S_ab, 1), (S_bc, 1), (S_bc, tr) -- whose weights X_l sit BEHIND the
    // padded parameter vector ([.. W | X_1 | .. | X_L], three [Cc][Cc] blocks per level) and run as plain fp32 GEMMs on T
    int n_extra = 0;
    // what gf_smp_create was asked for (smp_derive_plan re-derives cfg / dup_channels / n_extra from ucfg and these), and whether the handle
    // currently runs its `_10` / `_50` levels op by op because the prepared batch cannot be embedded (gf_smp_prepare switches per batch)
    bool req_pad_channels = true, embed_auto_off = false;
    int req_min_pad = 0;
    const float *extra_w = nullptr;   // X of the running pass (set by gf_smp_forward / gf_smp_backward)
    float *extra_g = nullptr;         // ... and its gradient
    float *rs_inv = nullptr;          // [rows of the largest level][2] (1 / tot, tr / tot): the extra products of an op-by-op level
    size_t rs_inv_rows = 0;
    size_t pad_feat_n = 0;
    gfsmp::BatchLayout lay;
    bool has_targets = false;  // the last gf_smp_forward was given targets: only then does dy hold a loss gradient
    // data-parallel reverse sweep (the context has a communicator, gf_dist.hip): the gradient segment of a level is
    // all-reduced on the communicator's stream as soon as it is complete, beside the rest of the sweep
    bool drop_on = false;      // RisiContraction_18_dropout instead of RisiContraction_18 (SMP_sigma_pairgraphs)
    float drop_scale = 1.f;    // test mode: nKept / 18 on every slice
    unsigned *mask_stage = nullptr;   // page-locked staging of the slice masks, [levels][vertices] in node order (gf_smp_dropout_masks)
    size_t mask_stage_n = 0;
    hipEvent_t ev_mask = nullptr;     // the last upload out of mask_stage
    int grad_allreduce = 1;
    float *dp_grads = nullptr;           // gradient buffer of the running gf_smp_backward, null when not data-parallel
    hipEvent_t ev_grad = nullptr, ev_comm = nullptr;
    bool dp_join_pending = false;        // ev_comm was recorded behind the last sweep's all-reduces and nobody has waited for it on the host yet
    int fused = 1;  // use the fused level path where supported (gf_smp_set_fused)
    int bwd_gather = 0;  // fused levels: evaluate dP inside the consumer gather instead of materialising it (GF_SMP_BWD_GATHER)
    // device buffers of the current batch come from a pool that survives gf_smp_prepare: a training loop prepares a new
    // batch every step, and hipMalloc of the level buffers (GBs) cost 4x the host graph preparation itself
    struct Block {
        void *p;
        size_t bytes;
        bool used;
        int idle;  // consecutive prepares that did not use the block
    };
    std::vector<Block> pool;
    // Two handles on one context can alternate (prepare of one while the device runs the step of the other): uploads go
    // through the handle's own stream, and recycling the handle's buffers waits for ITS last launch only, not for the stream.
    hipStream_t upload = nullptr;
    hipEvent_t ev_last = nullptr;
    bool used = false;
    // Adam state (gf_smp_adam_step); survives gf_smp_prepare, freed by gf_smp_destroy
    float *adam_m = nullptr, *adam_v = nullptr;
    // handle-owned model (host-pointer mode of the driver): parameters and their gradient, [param_count] each
    float *own_p = nullptr, *own_g = nullptr;
    unsigned long long adam_n = 0;  // parameter elements processed so far (the reference's running beta powers)
    // the kind of the last optimiser step, and what SGD / AdaMax / AdaDelta keep beside adam_m / adam_v (smp_optimisers.h)
    gf::OptimState optim;
    // smp_fit.hip: the parameter cache of gf_smp_parameters_snapshot / _rollback [param_count] and the 8 bytes of the loop's loss sum;
    // taken on first use, freed by gf_smp_destroy
    float *fit_cache = nullptr;
    double *fit_sum = nullptr;
};

namespace gf {
// channel counts the row-panel kernel family of the fused level is built for (models are padded to the next one: gf_smp_create)
inline bool smp_panel_channels(int C) { return C == 64 || C == 32 || C == 16; }
// A plain 18-slice 128-channel handle runs its block products as 64-channel sub-block passes of that family (smp_fused.hip:
// smp_c128_kernels) unless GF_SMP_C128=0.  Read when a batch is prepared -- the transposed-row tables and the four image sets are taken
// only then: a handle prepared under =0 is what it was before the path existed -- and per call: a pass runs the sub-block kernels when
// neither saw the 0.
inline bool smp_c128_switch() { return !env_is("GF_SMP_C128", '0'); }
// GF_SMP_LEVEL1=0 (read per call: the parity tests switch it): a fused level whose sources are all single vertices (level 1) runs the
// general kernels -- smp_tables_fwd_w, a workgroup per node, and smp_bwd_gather_all, a wave per source -- instead of
// smp_tables_fwd_single (smp_fused_tables.hip) and smp_bwd_gather_single (smp_fused_gather.hip)
inline bool smp_level1_switch() { return !env_is("GF_SMP_LEVEL1", '0'); }
// The reverse sweep of fused level l takes LeakyReLU'(f_l) from the sign words this pass's panel combine-forward left (DevLevel::sgn)
// instead of reading f_l.  64 channels; not where f_l's upper channels were overwritten after combine-forward (dup_level: SMP_2D_ver6 on
// the 18-slice level).  GF_SMP_SIGN_MASK=0 (read per call: the parity test switches it): f_l is read, dz is stored and read, as before.
inline bool smp_sign_mask(const gf_smp *s, int l) {
    return s->cfg.nChanels == 64 && !s->dup_channels && s->lv[l].sgn && s->lv[l].sgn_ready && !env_is("GF_SMP_SIGN_MASK", '0');
}
// Largest receptive field a fused level takes (round 6): up to 32 positions every kernel of the level; 33 .. 64 at C = 64 -- the few such
// nodes of a level (a 48-atom molecule's level-3 fields reach 35) run tables-forward and the two combine steps on workgroup kernels,
// everything else is row-based and does not care (smp_fused.hip: big_part)
constexpr int kFusedMaxField = 64;
// What runs level l >= 1 of a pass: the fused 18-slice level (smp_fused.hip) where gf_smp_set_fused allows and smp_fused_supported takes the
// shape, else the SMP_gamma level where smp_gamma_fused does, else the op-by-op pipeline (smp.hip); nobody else asks the two predicates.
// Constant for the length of a pass, NOT between passes (gf_smp_set_fused, gf_smp_dropout_masks): a sweep asks at its start, keeps nothing.
enum class LevelKind { OpByOp, Fused18, Gamma, Theta, Steerable2D, Unrestricted, Neighbourhood };   // Theta: every level of a first-order handle (cfg.first_order), Steerable2D: of a cfg.steerable_2d one, Unrestricted: of a cfg.unrestricted one (asked first), Neighbourhood: of a cfg.neighbourhood one (level 0 and the read-out too: its sweeps are smp_neighbourhood_forward / _backward, smp_gru_forward / _backward where cfg.gated()), nothing else
LevelKind smp_level_kind(const gf_smp *s, int l);
// the kinds on the th_* tables (smp_field_level.h): (namespace gf::field_level holds their kit) they take the read-out's gradient as one vector per node, write df_{l-1} themselves and
// keep what a second reverse sweep needs
inline bool is_field_level(LevelKind k) { return k == LevelKind::Theta || k == LevelKind::Steerable2D || k == LevelKind::Unrestricted; }
bool smp_fused_supported(const gf_smp *s, int l);
gf_status smp_backward_admissible(const gf_smp *s);   // smp.hip: refusals of a reverse sweep that must come before any work is issued
gf_status smp_fused_forward_level(gf_smp *s, int l, const float *Kl, const float *bl);
gf_status smp_fused_ensure_zero_fill(gf_smp *s, int l);
// node_df != nullptr (top level): df_l is the same C-vector at every position of a node, given as [nodes][C]
gf_status smp_fused_backward_level(gf_smp *s, int l, float *dKl, float *dbl, const float *node_df, bool rows_too = false);
gf_status smp_fused_gather_backward(gf_smp *s, int l);
// SMP_gamma levels (RisiContraction_4, smp_level_gamma.hip): G = f_{l-1} [K0 | K1 | K2 | K3] on the rows of level l - 1 into Q, then one gather
// with bias + LeakyReLU into f_l; backward the consumer gather of dG from dz, dK_l and df_{l-1} as products on the rows of level l - 1.
// Scratch: Wst [8 Cp Cc] (the weight views), dWst [4 Cp Cc]; Q at least [rows of level l - 1][4 Cc].  Cp = C_{l-1}, Cc = C_l: equal
// (C) for SMP_gamma, halving in a tower of SMP_gamma_physics / _pairgraphs (packed gathers gamma_tower_fwd / _bwd).
bool smp_gamma_fused(const gf_smp *s, int l);
gf_status smp_gamma_forward_level(gf_smp *s, int l, const float *Kl, const float *bl);
gf_status smp_gamma_backward_level(gf_smp *s, int l, const float *Kl, float *dKl, gf_status (*wgrad_done)(gf_smp *, int));
// The field levels: one pair of signatures.  K / sizes = the level's two parameter blocks, dK / dsizes their gradients (`+=`); backward:
// d.df holds df_l where rows_too (levels below the top), node_df = the read-out's gradient as one vector per node ([nodes][Cc]) or null;
// *wgrad_done(s, l) is called by the levels with a matrix product once the level's gradients are final and before df_{l-1} is formed; a
// level ignores what it does not need.  smp_field_*_level (smp_field_level.hip) pick the file from cfg in smp_level_kind's order.
gf_status smp_field_forward_level(gf_smp *s, int l, const float *K, const float *sizes);
gf_status smp_field_backward_level(gf_smp *s, int l, const float *K, const float *sizes, float *dK, float *dsizes, const float *node_df,
                                   bool rows_too, gf_status (*wgrad_done)(gf_smp *, int));
// SMP_theta (cfg.first_order = 1, smp_level_theta.hip).  sizes = (lambda1, lambda2, b[Cc]) x max_nVertices, K = K_l [2 Cp][Cc].
// forward: G = f_{l-1} [K_top | K_bot] on the rows of level l - 1, one gather into f_l (A and B kept).  backward: dz in place, the per-size
// gradients as segment reductions over the size buckets, dG gathered per source node, dK_l, *wgrad_done, df_{l-1}.
gf_status smp_theta_forward_level(gf_smp *s, int l, const float *K, const float *sizes);
gf_status smp_theta_backward_level(gf_smp *s, int l, const float *K, const float *sizes, float *dK, float *dsizes, const float *node_df,
                                   bool rows_too, gf_status (*wgrad_done)(gf_smp *, int));
// SMP_1D, SMP_1D_ver2, SMP_1D_ver3 (cfg.first_order = 2, 3, 4; smp_level_1d.hip): the same tables and sizes; K / dK are read by ver3 only
// (K_eye, K_one).  No GEMM in SMP_1D / ver2; one forward and two backward in ver3.
gf_status smp_1d_forward_level(gf_smp *s, int l, const float *K, const float *sizes);
gf_status smp_1d_backward_level(gf_smp *s, int l, const float *K, const float *sizes, float *dK, float *dsizes, const float *node_df,
                                bool rows_too, gf_status (*wgrad_done)(gf_smp *, int));
// SMP_2D and SMP_2D_ver4 (cfg.steerable_2d = 1, 2; smp_level_2d.hip): sizes = (lambda1[Cp], lambda2[Cp], b[Cc]) x max_nVertices, K =
// scalar_l[Cp].  No GEMM.  backward: dS is left in the first Cp columns of d.df.
gf_status smp_2d_forward_level(gf_smp *s, int l, const float *K, const float *sizes);
gf_status smp_2d_backward_level(gf_smp *s, int l, const float *K, const float *sizes, float *dK, float *dsizes, const float *node_df,
                                bool rows_too, gf_status (*wgrad_done)(gf_smp *, int));
// ... its reduction, shared with SMP_2D_ver5: the column partials in d.th_node over the size buckets into dsizes and dscalar
gf_status smp_2d_size_grads(gf_smp *s, int l, float *dscalar, float *dsizes);
// SMP_2D_ver5 (cfg.steerable_2d = 5; smp_level_2d_ver5.hip): K = K_l [C][2 C] then scalar_l[C], sizes as above with Cp = Cc = C.
// Two small products on the columns and one MFMA row projection per direction, dK_l as chunked MFMA reductions.
gf_status smp_2d_ver5_forward_level(gf_smp *s, int l, const float *K, const float *sizes);
gf_status smp_2d_ver5_backward_level(gf_smp *s, int l, const float *K, const float *sizes, float *dK, float *dsizes, const float *node_df,
                                     bool rows_too, gf_status (*wgrad_done)(gf_smp *, int));
size_t smp_2d_ver5_wgrad_chunks(long long rows, long long cols);   // partial images of dK_l a level of that many rows and columns writes
// Unrestricted_SMP_1D, _1D_ver2 and _2D (cfg.unrestricted = 1, 2, 3; smp_level_unrestricted.hip): sizes = (filter_s, b_s[Cc]) x
// max_nVertices, K = scalar_l[Cp] (form 3, else unused).  No GEMM.  backward: dS is left in d.Q.
gf_status smp_unrestricted_forward_level(gf_smp *s, int l, const float *K, const float *sizes);
gf_status smp_unrestricted_backward_level(gf_smp *s, int l, const float *K, const float *sizes, float *dK, float *dsizes, const float *node_df,
                                          bool rows_too, gf_status (*wgrad_done)(gf_smp *, int));
// NeuralFingerprint, GCN_1D, GCN_2D (cfg.neighbourhood = 1, 2, 3; smp_level_neighbourhood.hip): the whole sweeps of such a handle -- level 0
// and the read-out are softmax / plain sums, not the other kinds' -- and its gf_smp_prepare.  params / grads: W1_0; (W1_l, W2_l); W.
gf_status smp_neighbourhood_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature);
gf_status smp_neighbourhood_backward(gf_smp *s, const float *params, float *grads, int accumulate);
// (the launches of its three level kernels on operand sets, for the gated and the distance level: smp_vertex_level.h)
// GCN_1D_Distance, GCN_2D_Distance, GCN_3D_Distance (cfg.distance_channel; smp_level_distance.hip): the sweeps of a distance handle, its
// gf_smp_prepare_distance (smp_prepare.hip) and the sort that builds the distance channel's input rows on the handle's upload stream.
// params / grads: per level W1^v, W1^d (, W2^v, W2^d); W [2 H].
gf_status smp_distance_rows_launch(gf_ctx *ctx, hipStream_t stream, int nV, int M, const double *dist, const long long *mat_off, const int *mol_ptr,
                                   const int *vmol, float *xd);
gf_status smp_distance_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature);
gf_status smp_distance_backward(gf_smp *s, const float *params, float *grads, int accumulate);
// the classes' save_model order against the registration order: perm[i] = the flat index of the i-th value of a checkpoint
void smp_distance_checkpoint_order(const gfsmp::Config &c, std::vector<size_t> *perm);
// GCN_*D_Kernel and GCA_1D (cfg.readout = 1, 2; smp_level_readouts.hip): what smp_neighbourhood_forward / _backward run in place of
// nbh_readout and nbh_readout_dW.  forward: s->g, s->yhat, s->dy (pairs) or s->gram (Gram), the loss, and dh_L in lv[L].df -- the top level's
// nbh_node_bwd then runs with dy = NULL; dW: the pair model's dW [2 H] += the fold over the pairs (a Gram handle has no W).
gf_status smp_readout_forward(gf_smp *s, const float *W, const float *targets, float *predict, float *loss, float *graph_feature);
gf_status smp_readout_dW(gf_smp *s, const float *W, float *dW);
// GRU_GCN_1D, GRU_GCN_2D (cfg.neighbourhood = 4, 5; smp_level_gru.hip): the sweeps of a gated handle on the same lists and buffers.
// params / grads: W; W_z, U_z, W_r, U_r, W_h, U_h, W_g, U_g (shared by the levels: their gradients accumulate across them); U.
gf_status smp_gru_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature);
gf_status smp_gru_backward(gf_smp *s, const float *params, float *grads, int accumulate);
// GCN_3D, GRU_GCN_3D (cfg.neighbourhood = 6, 7; smp_level_third.hip): the aggregate n_l[v] = KMax(RisiLayer3D) of the two sweeps above, on
// raw operands.  forward: n, sel [nV][H] from hprev over the list (max_members = its longest entry); backward: dhprev [nV][H] from dn over
// the transposed list, consumer by consumer in ascending order.
gf_status smp_third_pool_fwd_launch(gf_ctx *ctx, int H, int nV, int max_members, const float *hprev, const long long *ptr, const int *idx, float *n,
                                    int *sel);
gf_status smp_third_pool_bwd_launch(gf_ctx *ctx, int H, int nV, const long long *ptr, const int *idx, const long long *tptr, const int *tidx,
                                    const float *hprev, const int *sel, const float *dn, float *dhprev);
// LCNN, GCN_MW (cfg.matrix_form = 1, 2; smp_level_rowlist.hip): the whole sweeps of such a handle, and its gf_smp_prepare (smp_prepare.hip).
// params / grads: GCN_MW W_0; W_l; W.  LCNN F1, b1, F2, b2, Dm, W.
gf_status smp_matrix_form_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature);
gf_status smp_matrix_form_backward(gf_smp *s, const float *params, float *grads, int accumulate);
// CGCN_1D, CGCN_2D (cfg.covariant = 1, 2; smp_level_covariant.hip): the whole sweeps of such a handle -- one launch each for all levels, and
// one fold of the gradient's partial images -- the bytes of those images, and its gf_smp_prepare (smp_prepare.hip).  params / grads: H; F_l.
gf_status smp_covariant_forward(gf_smp *s, const float *params, const float *targets, float *predict, float *loss, float *graph_feature);
gf_status smp_covariant_backward(gf_smp *s, const float *params, float *grads, int accumulate);
size_t smp_covariant_ws_bytes(int nMol, size_t image_floats);
// the first-order read-out of level l (smp_field_level.hip): sh[n] = column sums over the node's s rows (ShrinkMatrix), vf = LeakyReLU(sh);
// and its reverse, df_l[n][i][:] (+)= dvec[n][:] at every row i of the node, dvec = one gradient vector per node
gf_status smp_theta_readout(gf_smp *s, int l, float *sh, float *vf);
gf_status smp_theta_readout_backward(gf_smp *s, int l, const float *dvec, int accumulate);
bool smp_fused_gather_enabled(const gf_smp *s, int l);
gf_status smp_fused_stack_all(gf_smp *s, const std::vector<const float *> &K);
gf_status smp_build_gather_records(gf_smp *s, int l, hipStream_t stream);
gf_status smp_build_tf_records(gf_smp *s, int l, hipStream_t stream);
gf_status smp_fwd_fused_build_tables(gf_smp *s, int l, hipStream_t stream, bool gather_offsets = true);
// the panels' live-row words (DevLevel::pan_live) from the packed table, behind build_fwd_panels and whatever wrote trowf on `stream`
gf_status smp_build_pan_live(gf_smp *s, int l, hipStream_t stream);
// skip_empty (C = 64): O / dO of the rows whose pan_live bit is clear are not requested / not stored
gf_status smp_combine_fwd_panels_c64(gf_smp *s, int l, const float *O, const float *bias, float *psum = nullptr, float *pmax = nullptr,
                                     const float *nodefac = nullptr, bool skip_empty = false);
// combine-backward on the forward's row panels (C = 64 / 32, compact dO): dzmax = [fwd_npanels][C] per-panel column maxima of |dz| or null
gf_status smp_combine_bwd_panels_c64(gf_smp *s, int l, const float *dfrows, const float *node_df, float *dO, float *dzmax, bool skip_empty = false);
// the level's O / dO region [rows][2 C] (compact layout) copied to a caller's device buffer (gf_smp_level_projected_f32)
gf_status smp_fused_copy_projected(gf_smp *s, int l, float *out);
// level l's K_l / b_l gradients are complete on the context's CURRENT stream (l == 0: H): start their all-reduce
gf_status smp_dp_level_done(gf_smp *s, int l);

using gfsmp::param_count;   // the parameter layout: smp_prep.h
using gfsmp::view_params;
inline size_t feature_width(const gfsmp::Config &c) {  // physics tower: sum over the levels of their channel counts
    size_t w = 0;
    for (int l = 0; l <= c.nLevels; ++l) w += (size_t)c.level_channels(l);
    return w;
}

// ---- smp_prepare.hip: the handle's pool of device blocks and the page-locked allocator of the per-batch host tables ----
// A buffer of `count` elements of `elem` bytes (at least one) from the pool -- the best-fitting idle block, else a new hipMalloc --
// filled from `src` on the handle's upload stream when given
gf_status upload_bytes(gf_smp *s, void **dst, const void *src, size_t elem, size_t count);
template <typename T>
inline gf_status upload(gf_smp *s, T **dst, const void *src, size_t count) {
    void *p = nullptr;
    const gf_status st = upload_bytes(s, &p, src, sizeof(T), count);
    *dst = static_cast<T *>(p);
    return st;
}
gf_status ensure_P(gf_smp *s);
void mark_used(gf_smp *s);      // the handle's buffers were last touched by the launches before this mark
void release(gf_smp *s);        // end of a batch: its buffers go back to the pool
void release_pool(gf_smp *s);
void *pinned_table_alloc(size_t bytes);
void pinned_table_free(void *p);
gf_status own_model(gf_smp *s);   // smp_optim.hip: the handle-owned parameter / gradient buffers (host-pointer mode), created on first use
// ---- smp_pad.hip: the caller's layout against the device's (channel padding, SMP_2D_ver6 / ver7 on the 18-slice level) ----
gf_status pad_params_now(gf_smp *s, const float *params);           // caller's parameters -> s->pad_p
gf_status crop_grads_now(gf_smp *s, float *grads, int accumulate);  // s->pad_g -> caller's gradients
gf_status pad_feature_buffer(gf_smp *s);                            // s->pad_feat: [nMol][feature width of cfg]
gf_status copy_feature_blocks(gf_smp *s, float *user, float *padded, bool to_user);
gf_status dup_level(gf_smp *s, int l);    // no-ops unless gf_smp::dup_channels
gf_status fold_level(gf_smp *s, int l);
gf_status extra_products_forward(gf_smp *s, int l);   // no-ops unless gf_smp::n_extra
gf_status extra_products_wgrad(gf_smp *s, int l);
gf_status extra_products_backward(gf_smp *s, int l);
// ---- smp_readout_classes.hip: the read-out of a classifier handle (cfg.nClass >= 2); W [nClass][cfg.nChanels] ----
gf_status readout_classes_forward(gf_smp *s, const float *W, const float *targets, float *predict, float *loss);
gf_status readout_classes_dW(gf_smp *s, float *dW);
gf_status readout_classes_backward(gf_smp *s, bool per_node);   // per_node: gf_smp::dsh for a fused top level, else df_L row by row
}
#endif
