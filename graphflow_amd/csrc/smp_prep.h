// smp_prep.h -- host-side graph preparation of the batched SMP_omega driver.
//
// Restates, per molecule, what SMP_omega::complete_computation_graph does before it builds the op DAG
// (GraphFlow/SMP_omega.h:584-605): Floyd-Warshall hop distances (:358-380), Weisfeiler-Lehman histogram features
// (:382-404), lexicographic vertex ranking (:406-434), receptive fields phi_l(v) with the omega cap (:476-537),
// selection maps (the 0/1 matrices X of :461-474, :539-554, kept as index lists) and reduced adjacencies (:556-581).
// Then it lays a BATCH of molecules out for the device: per level, nodes (= one (molecule, vertex) pair) are sorted
// into buckets of equal receptive-field size so each bucket is one uniform-N contraction launch.
#ifndef GF_SMP_PREP_H_INCLUDED
#define GF_SMP_PREP_H_INCLUDED

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <vector>

namespace gfsmp {

// Host memory of the tables that are uploaded every batch comes from these hooks: plain malloc / free by default (this file
// is pure host C++), page-locked memory once the HIP side installs its pair -- an upload from pageable memory is staged through
// blit KERNELS that queue behind the running step's compute kernels, from pinned memory it is a DMA-engine copy that overlaps.
extern void *(*table_alloc)(size_t bytes);
extern void (*table_free)(void *p);
template <class T>
struct TableAlloc {
    typedef T value_type;
    TableAlloc() {}
    template <class U>
    TableAlloc(const TableAlloc<U> &) {}
    T *allocate(size_t n) { return static_cast<T *>(table_alloc(n * sizeof(T))); }
    void deallocate(T *p, size_t) { table_free(p); }
    template <class U>
    bool operator==(const TableAlloc<U> &) const { return true; }
    template <class U>
    bool operator!=(const TableAlloc<U> &) const { return false; }
};
template <class T>
using tvec = std::vector<T, TableAlloc<T> >;

constexpr int kUnrestrictedSplit = 16;   // node chunks per size bucket in the reduction of a dense filter's gradient

constexpr int kCcnMinChanels = 16;      // CCN_1D_MINIMUM_NUMBER_OF_CHANELS (GraphFlow/CCN_1D.h:30)

struct Config {
    int nLevels, nChanels, nFeatures, nDepth, max_receptive_field, has_WL_ordering;
    int nContractions = 18;  // contraction family of the levels: 18 (SMP_omega/beta, SMP_2D_ver8), 10 (ver6), 50 (ver7)
    int custom_matmul = 0;   // 1: K_l is [C][nContractions C] and applied by CustomMatMulTensor (SMP_2D_ver6-8)
    // 1: the `_physics` / `_pairgraphs` family (GraphFlow/SMP_omega_physics.h): raw vertex features (no WL histogram, no
    // WL ordering, and the cap orders by hop distance only, :436-450), channels halve from level to level (:141-151), every
    // level is read out (:572-590).  One such model body is a "tower": its output is the concatenated level features.
    int physics = 0;
    // 1 (a physics tower's DEVICE configuration, gf_smp_create): every level is computed at nChanels -- the halving channel counts
    // zero-padded to one width -- so the tower's levels run the fused level kernels
    int uniform = 0;
    // >= 2: the `_classification` models (gf_smp_create_classifier): the read-out weights are W [nClass][nChanels] (MatVecMul + LogLoss
    // instead of InnerProduct + SquaredLoss); 0: regression, W [nChanels] -- one row
    int nClass = 0;
    // 1: the first-order models (GraphFlow/SMP_theta.h, gf_smp_config.first_order): f_l[v] is [s][C], nContractions = 2 (K_l = [2 C'][C]),
    // and every level has a (lambda1, lambda2, b[C_l]) block per field size 1 .. max_nVertices in front of K_l
    // 2, 3, 4: SMP_1D, SMP_1D_ver2, SMP_1D_ver3 (GraphFlow/SMP_1D*.h; smp_level_1d.hip) -- the same fields without a cap, children and
    // per-size blocks, but no [2 C'][C] matrix: z = lambda1 S + lambda2 sumS + b (2: additive, C_l = C), [lambda1 S | lambda2 sumS] + b
    // (3: concatenating, C_l = 2 C_{l-1}), [lambda1 S K_eye | lambda2 sumS K_one] + b (4: two [C_{l-1}][C_{l-1}] matrices BEHIND the
    // per-size blocks).  LeakyReLU2D slope 0 instead of 0.01 in 3 and 4, level 0 included.
    int first_order = 0, max_nVertices = 0;
    // 1, 2: the second-order steerable models SMP_2D and SMP_2D_ver4 (GraphFlow/SMP_2D.h, SMP_2D_ver4.h; gf_smp_config.steerable_2d;
    // smp_level_2d.hip): f_l[v] is [s][s][C_l], the fields, children and pi are the first-order models' (no cap), applied to both indices.
    // Per level: for size = 1 .. max_nVertices (lambda1_s[C_{l-1}], lambda2_s[C_{l-1}], b_s[C_l]), then scalar_l[C_{l-1}] (the "matrix
    // block").  1: z = lambda1 S + lambda2 col + b, C_l = C; 2: z = [lambda1 S | lambda2 col] + b, C_l = 2 C_{l-1}.  Slope 0.01 everywhere.
    // 5: SMP_2D_ver5 (SMP_2D_ver5.h; smp_level_2d_ver5.hip): ver4's level with z = K_l [lambda1 S | lambda2 col] + b, K_l [C][2 C] in front of
    // scalar_l in the matrix block, C_l = C.  The value is the class's version number: there is no 3 or 4.
    int steerable_2d = 0;
    // 1, 2, 3: Unrestricted_SMP_1D, Unrestricted_SMP_1D_ver2, Unrestricted_SMP_2D (GraphFlow/Unrestricted_SMP_*.h;
    // gf_smp_config.unrestricted; smp_level_unrestricted.hip): SMP_1D, SMP_1D_ver2 and SMP_2D with a dense learned filter per field size
    // in place of lambda1_s I + lambda2_s 1 1^T.  Everything but the level and its per-size block is the restricted sibling's, so the
    // handle's Config ALSO carries the sibling's form -- first_order = 2 (form 1), 3 (form 2), steerable_2d = 1 (form 3) -- for the rows,
    // tables, channel counts, slopes, read-out and scalar_l; gf_smp_config itself asks for first_order = steerable_2d = 0.
    // Per level: for size = 1 .. max_nVertices (W_s [s][s] | W1_s, W2_s [s][s] | W_s [s][s][C], then b_s[C_l]); form 3: then scalar_l.
    int unrestricted = 0;
    // > 0: a tower of CCN_1D (GraphFlow/CCN_1D.h:200, :217; gf_smp_model_config.ccn_1d): C_0 = nChanels, C_l = max(int(ceil(C_{l-1} * decay)), 16),
    // the product in double as the class writes it.  0: the halving of the other towers.
    double decay = 0.0;
    // 1, 2, 3: NeuralFingerprint, GCN_1D, GCN_2D (GraphFlow/NeuralFingerprint.h, GCN_1D.h, GCN_2D.h; gf_smp_config.neighbourhood;
    // smp_level_neighbourhood.hip): one vector h_l[v] [nChanels] per vertex and level, aggregated over a neighbourhood N_l(v) (adjacency | hop
    // distance <= min(l, max_Radius) | <= l) by a sum or, in form 3, RisiLayer2D; softmax at every level.  Parameters: W1_0 [H][F']; for l =
    // 1..L: W1_l [H][F'], W2_l [H][H]; W [H].  None of the other forms' fields is set: the handle has no fields, rows or per-size blocks.
    // 4, 5: GRU_GCN_1D, GRU_GCN_2D (GraphFlow/GRU_GCN_1D.h, GRU_GCN_2D.h; smp_level_gru.hip): forms 2 and 3 with a GRU cell as the level's
    // update and a gated read-out; N_l(v) = hop distance <= min(l, max_Radius) in BOTH (GRU_GCN_2D does read max_Radius).  Parameters, shared
    // by all levels: W [H][F']; W_z, U_z, W_r, U_r, W_h, U_h, W_g, U_g [H][H] (shared_blocks()); U [H].  The levels own nothing.
    // 6, 7: GCN_3D, GRU_GCN_3D (GraphFlow/GCN_3D.h, GRU_GCN_3D.h; smp_level_third.hip): forms 2 and 4 with n_l[v] = KMax(RisiLayer3D of the
    // members, K = nChanels) as the aggregate; N_l(v) = hop distance <= min(l, max_Radius) in both; the parameter blocks of forms 2 / 4.
    int neighbourhood = 0, max_Radius = 0;
    // 1: LCNN, 2: GCN_MW (GraphFlow/LCNN.h, GCN_MW.h; gf_smp_config.matrix_form; smp_level_rowlist.hip): products whose A operand is a short list
    // of rows of the level below per output row.  2: nChanels = H; W_0 [F'][H] (first_block), W_l [H][H] (one Matrix per level), W [H].
    // 1: nLevels = 2 (the two convolutions), nChanels = C1, max_nVertices = V, nNeighbors = k; F1 [k][F'][C1] (first_block); level 1: b1
    // [C1], F2 [k][C1][C2]; level 2: b2 [C2], Dm [nDense][V C2]; W [nDense] -- each drawn as a Vector.  None of the other forms' fields is set.
    int matrix_form = 0, nNeighbors = 0, nChanels2 = 0, nDense = 0;
    // 1 with neighbourhood = 2, 3, 6: GCN_1D_Distance, GCN_2D_Distance, GCN_3D_Distance (GraphFlow/GCN_*D_Distance.h; gf_smp_config.distance_channel;
    // smp_level_distance.hip): two copies of the form's level side by side, the vertex channel on x [F'] and the distance channel on the sorted
    // distance rows [max_nVertices], read out over [sum h^v_L | sum h^d_L].  Parameters: W1^v_0 [H][F'], W1^d_0 [H][M] (first_block()); for l =
    // 1..L: W1^v_l, W1^d_l, W2^v_l [H][H], W2^d_l [H][H]; W [2 H].  N_l(v) reads max_Radius in all three.
    int distance_channel = 0;
    // 1 with neighbourhood = 2, 3, 6: GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (GraphFlow/GCN_*D_Kernel.h; gf_smp_config.readout;
    // smp_level_readouts.hip): the form's levels on a batch of graph pairs X_0, Y_0, X_1, Y_1, .. (interleave_pairs), read out over
    // [sum h^X_L | sum h^Y_L].  Parameters: the form's W1_0; W1_l, W2_l; then W [2 H].  N_l(v) reads max_Radius in all three.
    // 2 with neighbourhood = 2: GCA_1D (GraphFlow/GCA_1D.h, LinearGram.h): GCN_1D's levels, read out as the Gram matrix of the top-level
    // vectors against the molecule's adjacency values.  Parameters: GCN_1D's without W (readout_block() is empty).
    int readout = 0;
    // 1, 2: CGCN_1D, CGCN_2D (GraphFlow/CGCN_1D.h, CGCN_2D.h; gf_smp_config.covariant; smp_level_covariant.hip): one vector h_l[v]
    // [max_nVertices] per vertex, indexed by the molecule's vertex ids; the aggregate over N(v) = column v of the adjacency is a sum (1) or
    // RisiLayer2D (2), the update F_l n masked by the receptive field { i : sp[i][v] <= l }, LeakyReLU 0.01; the graph feature is the sum of
    // the h_L[v], the prediction the sum of its components.  Parameters: H [F'] (first_block, a Vector); F_l [M][M] (a Matrix) per level; no W.
    int covariant = 0;
    bool gated() const { return neighbourhood == 4 || neighbourhood == 5 || neighbourhood == 7; }
    bool third_order() const { return neighbourhood == 6 || neighbourhood == 7; }
    int nb_radius(int l) const { return neighbourhood == 1 ? 1 : (neighbourhood == 3 && !distance_channel && readout != 1) || l < max_Radius ? l : max_Radius; }   // of N_l (form 1: the adjacency itself; 3 alone ignores max_Radius)
    size_t filter_floats(int l) const { return level_blocks(l).size_quad(); }   // of an unrestricted level's filter, per s^2
    bool per_size() const { return first_order || steerable_2d; }   // a handle on the th_* tables, per-size blocks in front of the matrix block
    bool concat() const { return first_order >= 3 || steerable_2d == 2; }   // C_l = 2 C_{l-1}
    float level_slope() const { return first_order >= 3 ? 0.f : 0.01f; }   // LeakyReLU2D / 3D of every level (the read-out's LeakyReLU stays at 0.01)
    // ---- The parameter blocks in registration order: first_block(); level_blocks(l) for l = 1 .. nLevels; readout_block().  This is the one
    // account of the layout: param_count, view_params, the tower segments of a composite model and the uniform_init functions all read it.
    // A Block is n floats that GraphFlow::uniform_init draws together, with the divisor 10 * div: its own size for a Vector, the row count
    // for a Matrix of the neighbourhood classes (uniform_init(Matrix*)).
    struct Block {
        size_t n, div;
    };
    // One level's segment: for size = 1 .. max_size an entry of nsize blocks (block i of a size: quad * size^2 + lin floats), then the nmat
    // blocks of the matrix block, then the bias.  A family has the per-size entries or the bias, never both.
    struct LevelBlocks {
        struct SizeTerm {
            size_t quad, lin;
        };
        size_t max_size = 0, bias = 0;
        int nsize = 0, nmat = 0;
        SizeTerm size[3];
        Block mat[4];
        size_t size_quad() const {
            size_t q = 0;
            for (int i = 0; i < nsize; ++i) q += size[i].quad;
            return q;
        }
        size_t sizes() const {   // the per-size entries together, in closed form: a sweep asks per pass, an unrestricted level has up to 4096 sizes
            size_t lin = 0;
            for (int i = 0; i < nsize; ++i) lin += size[i].lin;
            return size_quad() * (max_size * (max_size + 1) * (2 * max_size + 1) / 6) + lin * max_size;
        }
        size_t matrix() const {
            size_t n = 0;
            for (int i = 0; i < nmat; ++i) n += mat[i].n;
            return n;
        }
        size_t total() const { return sizes() + matrix() + bias; }
        template <class F>
        void each_draw(F f) const {   // f(Block) for every block uniform_init draws with a divisor of its own, in order
            for (size_t s = 1; s <= max_size; ++s)
                for (int i = 0; i < nsize; ++i) {
                    const size_t n = size[i].quad * s * s + size[i].lin;
                    f(Block{n, n});
                }
            for (int i = 0; i < nmat; ++i) f(mat[i]);
            if (bias) f(Block{bias, bias});
        }
    };
    // The segment all levels share, between first_block() and the levels' own: `count` blocks of one size, each drawn as a Vector (the
    // gated classes draw through sgd->params[i]).  Empty in every family but the gated neighbourhood forms.
    struct SharedBlocks {
        int count = 0;
        Block each = {0, 0};
        size_t total() const { return (size_t)count * each.n; }
        template <class F>
        void each_draw(F f) const {
            for (int i = 0; i < count; ++i) f(each);
        }
    };
    SharedBlocks shared_blocks() const {
        SharedBlocks sb;
        if (gated()) {   // W_z, U_z, W_r, U_r, W_h, U_h, W_g, U_g
            const size_t n = (size_t)nChanels * nChanels;
            sb.count = 8;
            sb.each = {n, n};
        }
        return sb;
    }
    LevelBlocks level_blocks(int l) const {
        const size_t Cp = (size_t)level_channels(l - 1), Cl = (size_t)level_channels(l);
        LevelBlocks b;
        if (gated()) return b;   // (every block is shared: shared_blocks())
        auto sizes = [&b](std::initializer_list<LevelBlocks::SizeTerm> t) { for (const LevelBlocks::SizeTerm &x : t) b.size[b.nsize++] = x; };
        auto matrix = [&b](size_t n, size_t div = 0) { b.mat[b.nmat++] = {n, div ? div : n}; };   // (div = 0: a Vector, divided by its own size)
        if (covariant) {   // F_l [M][M], a Matrix
            matrix((size_t)max_nVertices * (size_t)max_nVertices, (size_t)max_nVertices);
            return b;
        }
        if (matrix_form == 2) {   // W_l [H][H], a Matrix
            matrix(Cl * Cl, Cl);
            return b;
        }
        if (matrix_form == 1) {   // b1 then F2 (l = 1), b2 then Dm (l = 2)
            const size_t k = (size_t)nNeighbors, C1 = (size_t)nChanels, C2 = (size_t)nChanels2;
            matrix(l == 1 ? C1 : C2);
            matrix(l == 1 ? k * C1 * C2 : (size_t)nDense * (size_t)max_nVertices * C2);
            return b;
        }
        if (distance_channel) {   // W1^v_l [H][F'], W1^d_l [H][M], W2^v_l, W2^d_l [H][H]: the registration order interleaves the channels
            matrix(Cl * fdim(), Cl);
            matrix(Cl * (size_t)max_nVertices, Cl);
            matrix(Cl * Cl, Cl);
            matrix(Cl * Cl, Cl);
            return b;
        }
        if (neighbourhood) {   // W1_l [H][F'], W2_l [H][H]: no per-size entries, no bias (l = 0: W1_0 is first_block())
            matrix(Cl * fdim(), Cl);
            matrix(Cl * Cl, Cl);
            return b;
        }
        if (per_size()) b.max_size = (size_t)max_nVertices;
        if (unrestricted == 1) sizes({{1, 0}, {0, Cl}});                 // W_s [s][s], b_s
        else if (unrestricted == 2) sizes({{1, 0}, {1, 0}, {0, Cl}});    // W1_s, W2_s [s][s], b_s
        else if (unrestricted == 3) sizes({{Cp, 0}, {0, Cl}});           // W_s [s][s][C], b_s
        else if (steerable_2d) sizes({{0, Cp}, {0, Cp}, {0, Cl}});       // lambda1_s, lambda2_s [C_{l-1}], b_s (SMP_2D.h:228-235)
        else if (first_order) sizes({{0, 1}, {0, 1}, {0, Cl}});          // lambda1_s, lambda2_s, b_s (SMP_theta.h:254-264)
        else b.bias = Cl;
        if (steerable_2d == 5) {   // K_l [C][2 C] as one Vector, then scalar_l (SMP_2D_ver5.h:241-242)
            matrix(2 * Cp * Cp);
            matrix(Cp);
        } else if (steerable_2d) {   // scalar_l (SMP_2D / ver4, Unrestricted_SMP_2D)
            matrix(Cp);
        } else if (first_order == 4) {   // K_eye, K_one: one block each (SMP_1D_ver3.h:238-239)
            matrix(Cp * Cp);
            matrix(Cp * Cp);
        } else if (first_order < 2) {   // K_l [nContractions C_{l-1}][C_l]; SMP_1D / ver2 and their unrestricted forms have no matrix block
            matrix((size_t)nContractions * Cp * Cl);
        }
        return b;
    }
    Block first_block() const {   // H [C][F (D + 1)]; W1_0 [H][F'] of a neighbourhood form (a Matrix: 10 x rows), W of a gated one (a Vector)
        const size_t n = (size_t)nChanels * fdim();
        if (distance_channel) return {n + (size_t)nChanels * (size_t)max_nVertices, (size_t)nChanels};   // W1^v_0 then W1^d_0: two Matrices of H rows, one divisor
        if (matrix_form == 2) return {n, (size_t)fdim()};   // W_0 [F'][H], a Matrix of F' rows
        if (matrix_form == 1) return {n * (size_t)nNeighbors, n * (size_t)nNeighbors};   // F1 [k][F'][C1], a Vector
        return {n, neighbourhood && !gated() ? (size_t)nChanels : n};
    }
    // W [readout_rows()][top_channels()] (SMP_2D_ver6_classification.h:211-217), drawn as one Vector; none in a physics tower, which ends in
    // its level features: the head's weights are the caller's; none in GCA_1D (readout = 2: top_channels() is 0), W [2 H] of a pair model
    Block readout_block() const {
        const size_t n = physics || covariant ? 0 : (size_t)readout_rows() * top_channels();   // (CGCN_*: SumComponents, no W)
        return {n, n};
    }
    // f(n) for every block the class registers with sgd->add, in registration order: the draw blocks above, except that the distance
    // classes register W1^v_0 and W1^d_0 one by one (GCN_1D_Distance.h:168-169; uniform_init draws them with one divisor) and that an
    // empty read-out is not a block.  `levels` = false: H alone (a tower of a composite model interleaves its levels with its partner's).
    template <class F>
    void each_registered_first(F f) const {
        const size_t n = (size_t)nChanels * fdim();
        if (distance_channel) {
            f(n);
            f(first_block().n - n);
        } else {
            f(first_block().n);
        }
    }
    template <class F>
    void each_registered(F f) const {
        const auto size = [&f](const Block &b) { f(b.n); };
        each_registered_first(f);
        shared_blocks().each_draw(size);
        for (int l = 1; l <= nLevels; ++l) level_blocks(l).each_draw(size);
        if (readout_block().n) f(readout_block().n);
    }
    int top_channels() const { return covariant ? max_nVertices : readout == 2 ? 0 : distance_channel || readout == 1 ? 2 * nChanels : matrix_form == 1 ? nDense : first_order >= 2 || steerable_2d ? level_channels(nLevels) : nChanels;  }   // width of the graph feature and of W's rows
    int readout_rows() const { return nClass > 1 ? nClass : 1; }   // rows of W: [1][C] is the regression's [C]
    bool square() const { return !physics || uniform; }   // K_l is [nContractions C][C] at every level
    int level_channels(int l) const {
        if (decay > 0.0) {
            int c = nChanels;
            for (int k = 0; k < l; ++k) {
                const int d = int(std::ceil(c * decay));
                c = d > kCcnMinChanels ? d : kCcnMinChanels;
            }
            return c;
        }
        if (concat()) return nChanels << l;
        if (square()) return nChanels;
        int c = nChanels >> l;
        return c < 1 ? 1 : c;
    }
    int fdim() const { return nFeatures * (nDepth + 1); }
};

// ---- the flat parameter vector: H, (the shared segment,) then per level (per-size entries, matrix block, bias), then W -- the registration
// order of SMP_omega.h:289-295 (= save_model order); Config::level_blocks has what each family puts where ----
inline size_t param_count(const Config &c) {
    size_t n = c.first_block().n + c.shared_blocks().total() + c.readout_block().n;
    for (int l = 1; l <= c.nLevels; ++l) n += c.level_blocks(l).total();
    return n;
}
// K[l] = the level's matrix block (empty in SMP_1D / ver2: never read; W1_l then W2_l in a neighbourhood form), b[l] = its bias or, where
// the family has them instead, the first of its per-size entries; shared (optional) = the first block of Config::shared_blocks()
template <typename P>
void view_params(const Config &c, P *base, P **H, std::vector<P *> *K, std::vector<P *> *b, P **W, P **shared = nullptr) {
    P *p = base;
    *H = p;
    p += c.first_block().n;
    if (shared) *shared = p;
    p += c.shared_blocks().total();
    K->assign(c.nLevels + 1, nullptr);
    b->assign(c.nLevels + 1, nullptr);
    for (int l = 1; l <= c.nLevels; ++l) {
        const Config::LevelBlocks lb = c.level_blocks(l);
        P *sizes = p;
        p += lb.sizes();
        (*K)[l] = p;
        p += lb.matrix();
        (*b)[l] = lb.bias ? p : sizes;
        p += lb.bias;
    }
    *W = p;
}
// GraphFlow::uniform_init (GraphFlow.h:1297-1306) of one block, drawn from the C library's rand() exactly as the reference draws it
inline void uniform_draw(const Config::Block &blk, float **p) {
    for (size_t i = 0; i < blk.n; ++i) {
        double x = (double)(rand() % 10) / (10.0 * (double)blk.div);
        if (rand() % 2 == 1) x = -x;
        *(*p)++ = (float)x;
    }
}

// everything the reference derives from one molecule
struct Molecule {
    int V = 0;
    std::vector<int> hops;                            // [V][V] shortest paths
    std::vector<double> wl;                           // [V][F(D+1)] WL histogram features
    std::vector<int> rank;                            // [V]
    std::vector<std::vector<std::vector<int> > > phi;  // [L+1][V] receptive fields
};

void prepare_molecule(const Config &cfg, int V, const int *adj, const double *feature, Molecule *out);

struct Bucket {
    int s;             // receptive-field size of every node in the bucket
    int count;         // nodes
    int first_node;    // index of the first node (nodes of a level are numbered in bucket order)
    int64_t first_row; // offset in (i,j) rows (sum of s^2 before the bucket)
    int64_t first_p;   // offset in (a,b,c) positions (sum of s^3 before the bucket)
};

// one level of the batch, host copy of what gets uploaded
struct LevelLayout {
    int nNodes = 0;
    int64_t rows = 0;   // sum s^2
    int64_t ppos = 0;   // sum s^3
    int64_t pairs = 0;  // sum s   (one (node, neighbour) pair per promoted tensor)
    std::vector<Bucket> buckets;
    tvec<int> node_s, node_mol, node_vertex;
    tvec<int64_t> node_row, node_p, node_pair;
    // The rows-sized tables (adj, pi, inv) and what is summed from adj (rsum, rowscale) are built on the DEVICE when
    // BatchLayout::device_tables is set (smp_prepare.hip: build_level_rows / build_level_inv, from `field`, the pair tables and the
    // molecules' adjacency matrices); the host then leaves them empty.
    tvec<int> node_panel;  // [nNodes] first row panel of the node (combine-forward on row panels, smp_level_c64_fwd.hip)
    int npanels = 0;       //   a node of size s has ceil(s / gpp) panels of gpp = max(1, min(8, 32 / s)) row groups
    tvec<int> field;  // [pairs] the receptive fields back to back: field[node_pair[n] + i] = i-th vertex (index inside its molecule)
    int64_t inv_count = 0;  // elements of inv
    tvec<float> adj;  // [rows] reduced adjacency, node-major [s][s]
    tvec<float> rsum; // [pairs] r[d] = sum_e A+[d][e] (A+ = A where A > 0), pair = node_pair[n] + d
    tvec<float> rowscale;  // [nNodes][2] (tot, tr) of the node's gated adjacency: per-row factors of the level's block GEMMs
    // wave-per-pair kernels: one workgroup (4 waves) per group of 4 consecutive indices of one node
    tvec<int> quad_node, quad_b0;  // [quads]
    tvec<int> quad_order;          // [quads] quads by (size class 4/8/16/32, molecule): launch order of tables-forward
    // forward gather (levels >= 1): per pair e = node_pair[n] + a
    tvec<int> pair_node;        // [pairs]
    tvec<int64_t> pair_src_row;  // [pairs] first row of the source node's tensor in level l-1
    tvec<int> pair_src_s;       // [pairs]
    tvec<int16_t> pi;           // [rows]  pi[node_row[n] + a*s + p] = index of phi_l(v)[p] in phi_{l-1}(w_a), or -1
    // compact diagonal path (smp_fused.hip): the two tables D_bb[x,y] = P[x,y,y] and D_ac[x,y] = P[x,y,x] are plain gathers
    // of the diagonal / the centre column of f_{l-1}[w_x], so their block products run on the sum-s rows of the level below
    tvec<int64_t> pair_src_pair; // [pairs] node_pair (level l-1) of the source node of pair e
    tvec<int> node_center;       // [nNodes] position of the node's own vertex inside its receptive field (every level)
    tvec<int64_t> cons_row;      // [pairs] node_row (level l) of the consumer's node
    tvec<int> cons_a;            // [pairs] the consumer's neighbour index a
    tvec<int64_t> cons_pair;     // [pairs] the consumer's pair id e = node_pair[n] + a (level l)
    tvec<int> mol_order;         // [nNodes] the level's nodes by (size class 1/4/8/16/32, molecule): launch order of the
                                        // backward gather, so the sources that re-read one consumer's rows run together
    // ONE launch of smp_bwd_gather_all per level: wave-sized work items (source node, 64-lane chunk of its (row p, channel quad)
    // space, half of the positions q for sources above 16), the sources above 16 first, then every other source molecule by
    // molecule.  item = {node, chunk | qhalf << 16}
    tvec<int> gather_items;      // [2 * n_items]
    // backward gather, indexed by the SOURCE node (level l-1): consumers = pairs that read it
    tvec<int64_t> cons_ptr;      // [nNodes(l-1) + 1]
    tvec<int64_t> cons_slab;     // [pairs] position offset (units of C floats) of the consumer's [s][s] slab in P
    tvec<int> cons_s;           // [pairs] consumer's s
    tvec<int64_t> cons_inv_off;  // [pairs] offset into inv
    tvec<int16_t> inv;          // per consumer: [s_w] position in the consumer's field of source position p, or -1
    // records of the backward gather (smp_fused.hip: smp_bwd_gather_v2): gather_pad(s_w) four-dword records per consumer entry,
    // the entries of a source back to back from cons_qbase[w] on
    tvec<int64_t> cons_qbase;    // [nNodes(l-1)]
    int64_t qrec_total = 0;
    // ---- first-order levels (build_batch_theta; smp_level_theta.hip).  rows = sum s, node_row = first row of the node's [s][C] matrix.
    // Children of node n = (molecule, v): the vertices w at hop distance <= 1, ascending (SMP_theta.h:577-583) -- pairs th_child_ptr[n] ..
    tvec<int64_t> th_child_ptr;   // [nNodes + 1]
    tvec<int64_t> th_src_row;     // [child pairs] first row of the child's node in level l - 1
    tvec<int> th_src_s;           // [child pairs] its field size
    tvec<int64_t> th_pi_off;      // [child pairs] offset into th_pi of the pair's s_n entries
    tvec<int16_t> th_pi;          // index of phi_l(v)[i] in phi_{l-1}(w), or -1
    // reverse sweep, by SOURCE node w of level l - 1: its consumers (the nodes it is a child of), ascending vertex
    tvec<int64_t> th_cons_ptr;    // [nNodes(l-1) + 1]
    tvec<int64_t> th_cons_row;    // [child pairs] first row of the consumer's node (level l)
    tvec<int> th_cons_s;          // [child pairs] the consumer's field size
    tvec<int> th_cons_node;       // [child pairs] the consumer's node
    tvec<int64_t> th_inv_off;     // [child pairs] offset into th_inv of the entry's s_w values
    tvec<int16_t> th_inv;         // index of phi_{l-1}(w)[j] in phi_l(v), or -1
    tvec<int> th_bucket;          // [3 * buckets] (s, first node, count): the segments of the per-size weight gradients
    // How often the reference counts a node's contribution to dlambda1_s / dlambda2_s.  SMP_theta adds the SHARED ops W_eye[s] / W_one[s]
    // (ScalarMatMul) to the graph once per vertex of size s (SMP_theta.h:590-591), and GraphFlow::backward runs an op once per appearance:
    // the j-th vertex of size s of a molecule (ascending v) has its gradient handed to lambda_s j times.  th_weight[n] = that j.
    // SMP_1D (Config::first_order == 2) puts three shared ops between a vertex and lambda_s -- W[s] (Reshape2D), W_flat[s] (Add), W_eye[s] /
    // W_one[s] -- each run once per appearance on a gradient that keeps accumulating (SMP_1D.h:498-503): a running sum of a running sum of a
    // running sum, th_weight[n] = j (j + 1) (j + 2) / 6.
    // SMP_2D (Config::steerable_2d == 1) has two: W[s] (SumTensor3D) and W_eye[s] / W_one[s] (VectorBroadcastMat), SMP_2D.h:558-573 --
    // th_weight[n] = j (j + 1) / 2; SMP_2D_ver4 hands W_eye[s] / W_one[s] to the vertex's TensorMul directly (SMP_2D_ver4.h:603-608): j.
    // The Unrestricted_* classes (Config::unrestricted) register W_s / b_s once per graph, not per vertex: th_weight = 1, the plain derivative.
    tvec<int> th_weight;          // [nNodes]
    // Config::unrestricted: un_part_off[b] = first float of bucket b's kUnrestrictedSplit chunk partials of its per-size entry (filter,
    // b_s, and in form 3 scalar_l's share), [buckets + 1]: the entries grow with s^2, so the offsets are a table
    tvec<int64_t> un_part_off;
    // steerable second-order levels (Config::steerable_2d): rows = sum s^2, node_row = first row of the node's [s][s][C] tensor, node_pair
    // = first of its s columns (sum of s before it), adj = the class's reduced adjacency of phi_l(v) ([rows]; SMP_2D_ver4: unit diagonal,
    // rows divided by their sums, SMP_2D_ver4.h:478-503); the th_* tables as above, pi / inv applied to both indices
};

// Register classes of the backward gather: a source of size s_w runs the code path with gather_pad(s_w) accumulators (and
// gather_pad(s_w) records per consumer: no size test inside its loops).
#ifdef __HIPCC__
#define GF_PREP_HD __host__ __device__
#else
#define GF_PREP_HD
#endif
GF_PREP_HD inline int gather_pad(int s) {
    return s <= 1 ? 1 : s <= 2 ? 2 : s <= 4 ? 4 : s <= 5 ? 5 : s <= 6 ? 6 : s <= 8 ? 8 : s <= 10 ? 10 : s <= 12 ? 12 : s <= 16 ? 16 : s <= 32 ? 32 : 64;   // (64: round 6, sources of 33 .. 64 positions)
}

struct BatchLayout {
    bool device_tables = false;  // in: see LevelLayout::field
    // (device_tables) the batch's inputs in page-locked tables, for the device-side builder: vertex counts, V x V adjacency
    // (and Coulomb) matrices back to back, their offsets
    tvec<int> mol_nv, mol_adj;
    tvec<int64_t> mol_adj_off;
    tvec<double> mol_coul;
    int max_vertices = 1;
    int nMol = 0;
    std::vector<int> mol_first_vertex;  // [nMol+1] prefix sum of vertex counts (level-0 node = global vertex id)
    tvec<float> x;                      // [nVertices][F(D+1)] WL features, level-0 input
    std::vector<LevelLayout> level;     // [L+1]; level[0] has only node bookkeeping
    std::vector<int> top_node_of_vertex;  // [nVertices] node index at level L of global vertex id
    std::vector<std::vector<int> > node_of_vertex;  // [L+1][nVertices] the same for every level (per-level readout)
    std::vector<Molecule> mols;         // kept for introspection (receptive fields)
    // Config::neighbourhood (build_batch_neighbourhood): one CSR list per distinct neighbourhood the model uses, over GLOBAL vertex ids
    // (molecules back to back), members ascending; its transpose (t*: the vertices whose list holds u, ascending) for the reverse sweep --
    // form 1's adjacency may be asymmetric.  nb_list_of_level[l] = the list of N_l, l >= 1.  mols keep only V and the hop distances.
    struct NeighbourList {
        tvec<int64_t> ptr, tptr;   // [vertices + 1]
        tvec<int> idx, tidx;
    };
    std::vector<NeighbourList> nb_lists;
    std::vector<int> nb_list_of_level;   // [L + 1], [0] unused
    tvec<int> nb_vertex_mol;             // [vertices]
    // Config::matrix_form (build_batch_matrix_form): the row lists of the level's A operand, forward and transposed, as CSR over the batch's
    // rows (GCN_MW: global vertex ids; LCNN: molecule m's rows are m V .. m V + V - 1) -- per entry the source row, the slot and the
    // coefficient, a row's entries in ascending slot order and, inside a slot, ascending source row.  LCNN also keeps every molecule's
    // order [V] and sequence [V][k] for introspection; mols keep V (the molecule's own vertex count).
    struct RowLists {
        tvec<int64_t> ptr, tptr;   // [rows + 1]
        tvec<int64_t> sptr, tsptr;  // LCNN: [rows k + 1] the first entry of every (row, slot), so that the kernels search nothing (one slot: ptr itself)
        tvec<int> src, slot, tsrc, tslot;
        tvec<float> coef, tcoef;
        std::vector<int> order, seq;
    };
    RowLists rl;
    tvec<unsigned char> cov_hop;   // Config::covariant (build_batch_covariant)
};

// coulomb: NULL, or the molecules' V x V Coulomb matrices back to back (DenseGraph::coulomb) -- the reduced adjacency of
// the use_coulomb constructors (SMP_omega.h:568-579) is then coulomb[v1][v2], diagonal included.
void build_batch(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature,
                 const double *coulomb, BatchLayout *out);

// The batch of a first-order model (Config::first_order) or a steerable second-order one (Config::steerable_2d): molecules, level-0 input, nodes in bucket order, rows = field positions, and the
// th_* tables of every level >= 1; none of the tables of the 18-slice level.  Built on the host threads.
void build_batch_theta(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out);

// The batch of a neighbourhood model (Config::neighbourhood): hop distances, the shell-sum features x, the neighbour lists and their
// transposes; none of the field, selection or reduced-adjacency tables.  level[l]: nNodes = rows = vertices.
void build_batch_neighbourhood(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out);

// The batch of a pair model (Config::readout = 1) in gf_smp_prepare's convention: the 2 nPairs graphs X_0, Y_0, X_1, Y_1, .. -- graph 2 p is
// X_p (the first batch), 2 p + 1 is Y_p (the second); a global vertex's pair is its graph >> 1, its side its graph & 1.  Vertex counts,
// adjacency and feature matrices back to back in that order; nFeatures columns per feature row.  Plain copies: the result goes through
// build_batch_neighbourhood unchanged.
struct PairBatch {
    std::vector<int> nVertices, adj;
    std::vector<double> feature;
};
void interleave_pairs(int nFeatures, int nPairs, const int *nVertices1, const int *adj1, const double *feature1, const int *nVertices2,
                      const int *adj2, const double *feature2, PairBatch *out);

// One molecule of a matrix-form model (Config::matrix_form), as the class derives it.  LCNN (LCNN.h:175-320): the molecule padded to V =
// max_nVertices vertices, hops and wl of the padded graph, order [V] and seq [V][k]; a pad entry holds molV.  GCN_MW (DenseGraph.h:69-111,
// GCN_MW.h:166-206): hops, wl and norm_adj [molV][molV] = d_i (A + I)[i][j] d_j in double.
struct MatrixFormMolecule {
    std::vector<int> hops, order, seq;
    std::vector<double> wl, norm_adj;
};
void matrix_form_molecule(const Config &cfg, int molV, const int *adj, const double *feature, MatrixFormMolecule *out);
// does a sequence with pad entries read past the class's matrix (molV == max_nVertices)?
bool lcnn_reads_past(const Config &cfg, int molV, const std::vector<int> &seq);
// The batch of a matrix-form model: x, the row lists (BatchLayout::rl), level[l]: nNodes = rows = the batch's rows.  Returns the first
// molecule lcnn_reads_past, or -1 (the batch is then complete).
int build_batch_matrix_form(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out);

// The batch of a covariant model (Config::covariant): hop distances, the shell-sum features x, nb_lists[0] = the column lists N(v) = { u :
// adj[u][v] > 0 } with their transposes (global vertex ids, ascending), and cov_hop [vertices][max_nVertices]: cov_hop[v][i] = sp[i][v]
// clipped to 255 (unreachable), positions beyond the molecule 255.  level[l]: nNodes = rows = vertices.  Every molecule has at most
// max_nVertices vertices (the caller checks).
void build_batch_covariant(const Config &cfg, int nMol, const int *nVertices, const int *adj, const double *feature, BatchLayout *out);

}  // namespace gfsmp
#endif
