// smp_config.h -- the one place that decides which gf_smp_config a handle is built from, and what gfsmp::Config it becomes.
// Pure host C++ (smp_config.cpp, built beside smp_prep.cpp): gf_smp_create, gf_smp_create_classifier, the towers of gf_smp_model_create,
// the host-only gf_smp_*config_param_count / *_uniform_init_host and gf_smp_prepare_molecule_host all ask here, so they cannot disagree.
// A new model family edits two places: resolve_config below and gfsmp::Config::level_blocks (smp_prep.h).
#ifndef GF_SMP_CONFIG_H_INCLUDED
#define GF_SMP_CONFIG_H_INCLUDED

#include "../../include/gf_hip.h"
#include "smp_prep.h"

namespace gf {
// the neighbourhood level's kernels (smp_level_neighbourhood.hip) and the configurations they take: at most kNeighbourhoodMaxChanels
// channels, the forward level's LDS images within 160 KiB
constexpr int kNeighbourhoodMaxChanels = 128;
// the lanes that share one vertex in the level's kernels: the power of two at or above H, at least 8, at most a wave
inline int smp_neighbourhood_group_width(int H) { return H > 32 ? 64 : H > 16 ? 32 : H > 8 ? 16 : 8; }
// LDS of the forward level: W1_l^T [F'][H | 1] and W2_l^T [H][H | 1] (odd row strides), one vector of H floats per vertex slot of 256 lanes
inline size_t smp_neighbourhood_lds_bytes(int H, int FD) {
    return sizeof(float) * ((size_t)(FD + H) * (size_t)(H | 1) + (size_t)(256 / smp_neighbourhood_group_width(H)) * H);
}
// the gated level (smp_level_gru.hip; neighbourhood = 4, 5): six [H][H | 1] images and three vectors of H floats per vertex slot in LDS
// -- 99.8 KB at 64 channels, 396 KB at 128: one launch per level holds at most 64 channels in the 160 KiB
constexpr int kGruMaxChanels = 64;
inline size_t smp_gru_lds_bytes(int H) {
    return sizeof(float) * (6 * (size_t)H * (size_t)(H | 1) + 3 * (size_t)(256 / smp_neighbourhood_group_width(H)) * H);
}
// the third-order pool (smp_level_third.hip; neighbourhood = 6, 7): at most kThirdMaxChanels channels (a canonical triple packs into 18
// bits).  LDS of one vertex's workgroup: two arrays of kThirdCand 64-bit keys, kThirdBins + 256 + 8 counters, A [H], B [H][H] and the
// members' vectors [members][H] -- 42,272 bytes and 256 per member at 64 channels, so a neighbourhood holds at most 474 vertices there.
constexpr int kThirdMaxChanels = 64;
constexpr int kThirdBins = 2048, kThirdCand = 1024;
inline size_t smp_third_lds_bytes(int H, int members) {
    return 8 * 2 * (size_t)kThirdCand + 4 * ((size_t)kThirdBins + 256 + 8) + sizeof(float) * ((size_t)H + (size_t)H * H + (size_t)members * H);
}
inline int smp_third_max_members(int H) { return (int)((160 * 1024 - smp_third_lds_bytes(H, 0)) / (sizeof(float) * (size_t)H)); }
// the Gram read-out (smp_level_readouts.hip: gram_readout; readout = 2): one workgroup per molecule keeps h_L [V][H | 1] (the odd row stride
// serves both of its products without bank conflicts), E [V][V | 1] and four wave partials of the loss in LDS:
//   4 (V (H | 1) + V (V | 1) + 4) bytes -- 10,920 at V = 29, H = 64; within 160 KiB up to V = 147 at 128 channels, 172 at 64, 199 at 5
inline size_t smp_gram_lds_bytes(int V, int H) { return sizeof(float) * ((size_t)V * (size_t)(H | 1) + (size_t)V * (size_t)(V | 1) + 4); }
// the row-list level (smp_level_rowlist.hip; matrix_form = 1, 2): no weights resident in LDS, so no channel limit of that kind.  Its kernels
// index a column of an operand row and a tile of a launch with ints: a width (slots * Cin, or N) of at most 2^16 keeps slot * Cin + c, the
// 64-wide tiles of a row (2^10) and a partial image of width x width floats (2^32 elements, counted in a size_t) in range; every launch
// checks its own tile count (rows / 128 x 2^10, or 2^9 x 2^10 x splits) against 2^31 - 1.
constexpr int kRowlistMaxWidth = 65536;
constexpr int kRowlistSplits = 256;   // most partial images of a weight gradient, folded in ascending order
// the covariant level (smp_level_covariant.hip; covariant = 1, 2): one workgroup keeps a molecule's whole network in LDS -- seven [V][V | 1]
// images in the reverse kernel (dh_l / dz, dh_{l-1}, n_l / dn, F_l[:V, :V] / the pair dots, h_{l-1}, the exclusive sums, the pair
// constants; the forward kernel uses five of them), two vectors of V floats, eight floats of reductions and the V V hop counts as bytes:
//   4 (7 V (V | 1) + 2 V + 8) + V V bytes (rounded up to 16) -- 24,660 at V = 29, 121,120 at 64; within 160 KiB up to V = 75
inline size_t smp_covariant_lds_bytes(int V) {
    return sizeof(float) * (7 * (size_t)V * (size_t)(V | 1) + 2 * (size_t)V + 8) + (((size_t)V * (size_t)V + 15) & ~(size_t)15);
}
constexpr int kCovariantMaxVertices = 75;   // the largest V with smp_covariant_lds_bytes(V) <= 160 KiB
constexpr int kCovariantSplits = 256;       // most partial images of the gradient: chunks of ceil(nMol / 256) molecules, folded in ascending order
}  // namespace gf

namespace gfsmp {
// who asks: the three ways a handle comes to be
struct ConfigEntry {
    enum Kind { Handle, Classifier, Tower } kind;   // gf_smp_create, gf_smp_create_classifier, a tower of gf_smp_model_create
    int nClass;                                     // Classifier: rows of W
    double decay;                                   // Tower: > 0 = CCN_1D's width rule (Config::decay)
};
constexpr ConfigEntry kHandleEntry = {ConfigEntry::Handle, 0, 0.0};
// The caller's configuration as the Config in the caller's layout (gf_smp::ucfg), or the refusal: GF_ERR_INVALID / GF_ERR_UNSUPPORTED and,
// in why, the message gf_last_error gives.  Touches no device and allocates nothing.
gf_status resolve_config(const gf_smp_config *cfg, const ConfigEntry &entry, Config *out, char *why, size_t nwhy);
}  // namespace gfsmp

namespace gf {
struct ModelSeg { size_t model_off, tower_off, n; };   // a tower's contiguous run inside the model's parameter vector
// What gf_smp_model_create derives from a configuration before it touches the device: level widths, head widths, the segments of the
// towers inside the model vector.  false (and a message): a configuration it refuses.
struct ModelPlan {
    int nK = 18, maxV[2] = {0, 0}, fwidth = 0, nTowers = 0;
    double decay = 0.0;                       // > 0: CCN_1D's width rule (gfsmp::Config::decay)
    std::vector<int> lvlC, widths;
    std::vector<ModelSeg> segs[2];
    gf_smp_config tower_cfg[2];                // what gf_smp_create is asked for, tower by tower
    gfsmp::Config tower[2];                    // ... and what it makes of it
    size_t head_off = 0, head_params = 0, n_params = 0;
};
bool model_plan(const gf_smp_model_config *cfg, ModelPlan *p, char *why, size_t nwhy);
// f(n) for every block of the head in registration order: one [widths[i]][widths[i - 1]] matrix per layer, then the vector of the last width
template <class F>
void each_head_block(const std::vector<int> &widths, F f) {
    const int nLayers = (int)widths.size() - 1;
    for (int i = 1; i <= nLayers; ++i) f((size_t)widths[i] * (size_t)widths[i - 1]);
    f((size_t)widths[nLayers]);
}
// f(n) for every block a composite class registers with sgd->add: H of every tower; per level, tower by tower, the level's blocks; the head
// (SMP_omega_pairgraphs.h:361-375, CCN_1D.h:381-403)
template <class F>
void each_registered(const ModelPlan &p, F f) {
    const auto size = [&f](const gfsmp::Config::Block &b) { f(b.n); };
    for (int t = 0; t < p.nTowers; ++t) p.tower[t].each_registered_first(f);
    for (int l = 1; l <= p.tower[0].nLevels; ++l)
        for (int t = 0; t < p.nTowers; ++t) p.tower[t].level_blocks(l).each_draw(size);
    each_head_block(p.widths, f);
}
}  // namespace gf
#endif
