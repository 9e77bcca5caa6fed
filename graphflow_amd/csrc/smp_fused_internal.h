// smp_fused_internal.h -- what the four files of the fused SMP level share: smp_fused.hip (the route, the drivers and the small kernels),
// smp_fused_tables.hip, smp_fused_combine.hip and smp_fused_gather.hip (the kernels named in their file names, with their launchers).
#ifndef GF_SMP_FUSED_INTERNAL_H_INCLUDED
#define GF_SMP_FUSED_INTERNAL_H_INCLUDED

#include <algorithm>
#include <type_traits>
#include <vector>

#include "r18_device.h"
#include "smp_internal.h"

namespace gf {

// column blocks of the table matrix T [rows][4C]
enum { T_SAB = 0, T_SBC = 1, T_T6 = 2, T_T10 = 3, T_COLS = 4 };
// column blocks of the projected matrix O [rows][3C].  O_LOC = tot O_tot + tr O_tr + O_dir: the per-node factors tot and
// tr (the level's rowscale table) are applied to the T operand inside the GEMM, so the three row-local products
// accumulate into one block.
enum { O_LOC = 0, O_Z = 1, O_ZP = 2, O_COLS = 3 };

// channel counts that are whole 32-channel windows but not whole 64-channel ones (C = 32, 96): the workgroup-per-(node, x) kernels run
// with eight lanes per row instead of sixteen half-idle ones
inline bool smp_half_window(int C) { return C % 32 == 0 && C % 64 != 0; }
// ... and whole 16-channel windows only (C = 16, 48, ...): four lanes per position in tables-forward (round 5: the 16-channel kernel family)
inline bool smp_quarter_window(int C) { return C == 16; }
// tables-forward keeps smp_vectors' sums itself (C % 64 == 0, and the 32- / 16-channel windows; other channel counts: the separate pass)
inline bool smp_tables_fold_vectors(const gf_smp *s) {
    return (s->cfg.nChanels & 63) == 0 || smp_half_window(s->cfg.nChanels) || smp_quarter_window(s->cfg.nChanels);
}

// threads of a workgroup-per-node kernel whose items are (position, channel quad): the level's largest node decides (a level of
// 3-vertex fields left 200 of 256 threads idle, and a quarter of the workgroups a CU could hold)
inline int node_block(const gfsmp::LevelLayout &h, int C) {
    const int smax = h.buckets.empty() ? 1 : h.buckets.back().s;
    int t = (smax * (C / 4) + 63) / 64 * 64;
    return t < 64 ? 64 : t > 256 ? 256 : t;
}

// What one call of the level runs on: every path decision of smp_fused_forward_level / smp_fused_backward_level, taken once at the
// call's entry (fused_route) from the handle, the level's buffers and the environment switches as they are at that moment.  Nothing of it
// is kept between calls: the reverse sweep fills its own and refuses where `panels` differs from what the forward pass recorded
// (DevLevel::fwd_c64).
struct FusedRoute {
    bool panels = false;            // block products on the row-panel kernel family (64 / 32 / 16 channels, 128 as sub-block passes); else tiled GEMMs
    int ocols = O_COLS;             // ... which fixes the layout of O / dO: 2 = compact [O_loc | U], 3 = [O_loc | Z | Z']
    bool split = false;             // the compact-layout products run on the f16 pipe with two-half operands (smp_split_products)
    bool skip_zero_rows = false;    // tables-forward leaves the structurally-zero rows of T unwritten (DevLevel::t_zeros) ...
    bool readers_mask = false;      // ... and every reader of T masks them: no zero fill needed before the products
    int lpc = 16;                   // lanes per position of tables-forward: 16 / 8 / 4 (64- / 32- / 16-channel windows)
    bool fold_vectors = false;      // tables-forward keeps the sums over b itself (else smp_vectors runs behind it)
    bool small_split = false;       // the small products (V, S, Gc and their transposes) on the split pipe; else one grouped GEMM launch
    bool extras_in_kernel = false;  // SMP_2D_ver7's extra products inside the row-panel kernels; else as GEMMs on T
    bool panel_combine = false;     // combine-forward / -backward on the row panels; else the workgroup kernels for every node
    bool gather = false;            // df_{l-1} by the consumer gather; else tables-backward writes dP
    bool fuse_small = false;        // reverse sweep: the pair reduction and the diagonal gather in one launch
    bool sign_mask = false;         // reverse sweep: LeakyReLU' from the forward's sign words (smp_sign_mask)
    bool drop = false;              // slice dropout ...
    int nf = 2;                     // ... and the row factors per row it implies: 8 (one per product), else 2 = (tot, tr)
    // C = 64: O / dO of the level's EMPTY rows (no data in any block of T: none of bits 31 / 30 / 29 of trowf) is neither stored nor
    // read -- true only where every writer and reader of the region in this call is a kernel that masks them (fused_route)
    bool skip_empty = false;
};
FusedRoute fused_route(const gf_smp *s, int l);

// The nodes of a level above 32 positions (nodes are numbered by size: they come last), see kFusedMaxField: first node / row / pair /
// workgroup-kernel quad of that range and its extents.  nodes == 0: none.
struct BigPart {
    int n0 = 0, nodes = 0, quad0 = 0, quads = 0, smax = 0;
    long long row0 = 0, pair0 = 0, pairs = 0;
};

// a run of the level's (node, four x) quads for the workgroup combine kernels, and the largest receptive field in it
struct QuadRange {
    int quad0, quads, smax;
};
inline QuadRange all_quads(const gfsmp::LevelLayout &h) { return {0, (int)h.quad_node.size(), h.buckets.back().s}; }
inline QuadRange big_quads(const BigPart &b) { return {b.quad0, b.quads, b.smax}; }

// ---- smp_fused_tables.hip ----
struct SizeClass {
    long long lo, hi;  // pair range
    int smax, ni;
};
// the level's size buckets merged into the NI classes of tables-forward / -backward at ppw positions per wave load
std::vector<SizeClass> classes_of(const gfsmp::LevelLayout &h, int ppw);
gf_status launch_tables_fwd(gf_smp *s, int l, const SizeClass &c, const FusedRoute &r);
gf_status launch_tables_fwd_big(gf_smp *s, int l, const BigPart &big);
// the sums over b where tables-forward did not keep them: every node, or the big part behind smp_tables_fwd_big
gf_status launch_vectors(gf_smp *s, int l, const FusedRoute &r, const BigPart &big);
gf_status launch_tables_bwd(gf_smp *s, int l, const SizeClass &c, const float *dT);

// ---- smp_fused_combine.hip: the workgroup kernels over a quad range, under the launch name given ----
// wide: the 64-position build (a level with nodes above 32 positions)
gf_status launch_combine_fwd(gf_smp *s, int l, const QuadRange &q, const char *name, bool wide, const float *O, const float *bias, int ocols,
                             const float *nodefac);
// eight lanes per row at the half-window channel counts, else sixteen
gf_status launch_combine_bwd(gf_smp *s, int l, const QuadRange &q, const char *name, const float *dfrows, const float *node_df, float *dO, int ocols,
                             float *dzmax);

}  // namespace gf

#endif
