// smp_config.cpp -- resolve_config: see smp_config.h.  The checks run in the order the create functions have always made them; the
// first refusal wins.  Every product and shift of the caller's fields is guarded or widened first: the struct may hold anything.
#include <cstdio>

#include "smp_config.h"

namespace gfsmp {
namespace {

constexpr int kMaxFieldVertices = 4096;   // gf_smp_prepare takes no larger molecule
constexpr long long kMaxInt = 0x7fffffffll;

bool no_cap(const gf_smp_config *cfg) { return cfg->max_nVertices == cfg->max_receptive_field; }
bool plain_levels(const gf_smp_config *cfg) { return !cfg->nContractions && !cfg->custom_matmul && !cfg->physics; }   // no contraction family / custom product / tower
// the concatenating forms: C_l = C << l must stay a sane int
bool doubling_fits(const gf_smp_config *cfg) { return cfg->nLevels <= 16 && ((long long)cfg->nChanels << cfg->nLevels) <= (1 << 20); }

// first_order = 2, 3, 4 (SMP_1D, SMP_1D_ver2, SMP_1D_ver3): no cap, plain levels, channel counts and multiplicities that fit an int
bool rule_1d(const gf_smp_config *cfg) {
    if (cfg->first_order < 2 || cfg->first_order > 4 || !plain_levels(cfg) || !no_cap(cfg)) return false;
    if (cfg->first_order == 2) return cfg->max_nVertices <= 2000;   // (th_weight = j (j + 1) (j + 2) / 6, j <= max_nVertices)
    return doubling_fits(cfg);
}
// steerable_2d = 1, 2, 5 (SMP_2D, SMP_2D_ver4, SMP_2D_ver5; there is no 3 or 4): first_order = 0, no cap, plain levels, a multiplicity
// j (j + 1) / 2 (j <= max_nVertices) and channel counts that fit an int; 5: K1 [C][C] fits in LDS
bool rule_2d(const gf_smp_config *cfg) {
    if ((cfg->steerable_2d != 1 && cfg->steerable_2d != 2 && cfg->steerable_2d != 5) || cfg->first_order) return false;
    if (cfg->steerable_2d == 5 && cfg->nChanels > 128) return false;
    if (!plain_levels(cfg) || !no_cap(cfg) || cfg->max_nVertices > kMaxFieldVertices) return false;
    return cfg->steerable_2d != 2 || doubling_fits(cfg);
}
// unrestricted = 1, 2, 3 (Unrestricted_SMP_1D, _1D_ver2, _2D): first_order = steerable_2d = 0, no cap, plain levels, channel counts and a
// parameter count that fit an int
bool rule_unrestricted(const gf_smp_config *cfg) {
    if (cfg->unrestricted < 1 || cfg->unrestricted > 3 || cfg->first_order || cfg->steerable_2d) return false;
    if (!plain_levels(cfg) || !no_cap(cfg) || cfg->max_nVertices > kMaxFieldVertices || !doubling_fits(cfg)) return false;
    const long long FD = (long long)cfg->nFeatures * ((long long)cfg->nDepth + 1);
    if (FD > kMaxInt) return false;   // (H alone is too large; keeps the sum below inside a long long)
    const long long m = cfg->max_nVertices, sq = m * (m + 1) * (2 * m + 1) / 6;   // sum of s^2
    long long n = (long long)cfg->nChanels * FD, Cl = cfg->nChanels;
    for (int l = 1; l <= cfg->nLevels; ++l) {
        const long long Cp = Cl;
        if (cfg->unrestricted == 2) Cl *= 2;
        n += (cfg->unrestricted == 3 ? Cp : cfg->unrestricted) * sq + m * Cl + (cfg->unrestricted == 3 ? Cp : 0);
    }
    return n + Cl <= kMaxInt;
}
// neighbourhood = 1, 2, 3 (NeuralFingerprint, GCN_1D, GCN_2D): no other form, no cap, nLevels >= 0, what the level's kernels take
bool rule_neighbourhood(const gf_smp_config *cfg) {
    if (cfg->neighbourhood < 1 || cfg->neighbourhood > 3) return false;
    if (cfg->first_order || cfg->steerable_2d || cfg->unrestricted || !plain_levels(cfg)) return false;
    if (cfg->nLevels < 0 || cfg->nLevels > 64 || cfg->nChanels < 1 || cfg->nFeatures < 1 || cfg->nDepth < 0 || cfg->max_nVertices < 1) return false;
    if (!no_cap(cfg) || cfg->max_nVertices > kMaxFieldVertices) return false;
    if (cfg->neighbourhood == 1 && cfg->nDepth != 0) return false;
    if (cfg->neighbourhood == 2 && cfg->max_Radius < 0) return false;
    if (cfg->nChanels > gf::kNeighbourhoodMaxChanels) return false;
    const long long FD = (long long)cfg->nFeatures * ((long long)cfg->nDepth + 1);
    return FD <= 65536 && gf::smp_neighbourhood_lds_bytes(cfg->nChanels, (int)FD) <= 160 * 1024;
}
// neighbourhood = 4, 5 (GRU_GCN_1D, GRU_GCN_2D): form 2's rules -- both read max_Radius -- apart from the channel count, which the caller
// checks for a message of its own
bool rule_gated(const gf_smp_config *cfg) {
    gf_smp_config as2 = *cfg;
    as2.neighbourhood = 2;
    return (cfg->neighbourhood == 4 || cfg->neighbourhood == 5) && rule_neighbourhood(&as2);
}

// matrix_form = 1, 2 (LCNN, GCN_MW): no other form, no cap, the fields each class reads
bool rule_matrix_form(const gf_smp_config *cfg) {
    if (cfg->matrix_form < 1 || cfg->matrix_form > 2) return false;
    if (cfg->first_order || cfg->steerable_2d || cfg->unrestricted || cfg->neighbourhood || !plain_levels(cfg)) return false;
    if (cfg->nChanels < 1 || cfg->nFeatures < 1 || cfg->nDepth < 0 || cfg->max_nVertices < 1) return false;
    if (!no_cap(cfg) || cfg->max_nVertices > kMaxFieldVertices) return false;
    if (cfg->matrix_form == 2) return cfg->nLevels >= 0 && cfg->nLevels <= 64;
    return cfg->nLevels == 2 && cfg->nNeighbors >= 1 && cfg->nChanels2 >= 1 && cfg->nDense >= 1;
}
// ... and the widest operand row its kernels would index (rule_matrix_form holds)
long long matrix_form_widest(const gf_smp_config *cfg) {
    const long long FD = (long long)cfg->nFeatures * ((long long)cfg->nDepth + 1);
    long long w = FD > cfg->nChanels ? FD : cfg->nChanels;
    if (w > gf::kRowlistMaxWidth) return w;   // (keeps the products below inside a long long)
    if (cfg->matrix_form == 1)
        for (long long x : {(long long)cfg->nChanels2, (long long)cfg->nDense, (long long)cfg->nNeighbors * FD,
                            (long long)cfg->nNeighbors * cfg->nChanels, (long long)cfg->max_nVertices * cfg->nChanels2})
            w = x > w ? x : w;
    return w;
}

}  // namespace

#define GF_REFUSE(status, ...) return (std::snprintf(why, nwhy, __VA_ARGS__), (status))

gf_status resolve_config(const gf_smp_config *cfg, const ConfigEntry &entry, Config *out, char *why, size_t nwhy) {
    const int nClass = entry.kind == ConfigEntry::Classifier ? entry.nClass : 0;
    // ---- what the entry itself refuses ----
    if (entry.kind == ConfigEntry::Handle && cfg && cfg->physics) {   // (such towers are built by gf_smp_model_create only)
        if (cfg->first_order == 1)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: first_order = 1 has no single-handle physics tower: set physics = 0, or build SMP_theta_physics / "
                                      "SMP_theta_pairgraphs with gf_smp_model_create (first_order = 1)");
        if (cfg->nContractions == 4)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: nContractions = 4 (SMP_gamma) has no single-handle physics tower: set physics = 0, or build "
                                      "SMP_gamma_physics / SMP_gamma_pairgraphs with gf_smp_model_create (nContractions = 4)");
    }
    if (!cfg) GF_REFUSE(GF_ERR_INVALID, "%s: null argument", entry.kind == ConfigEntry::Classifier ? "gf_smp_create_classifier" : "gf_smp_create");
    if (entry.kind == ConfigEntry::Classifier) {   // (the first three before the configuration is looked at: there is no class to hold the handle to)
        if (cfg->first_order == 1)   // (SMP_theta has no `_classification` class; first_order = 2, 3, 4 do: SMP_1D*_classification)
            GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_create_classifier: a first-order model (first_order = 1) has no classifier read-out");
        if (cfg->unrestricted) GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_create_classifier: the Unrestricted_SMP_* models have no `_classification` class");
        if (cfg->covariant) GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_create_classifier: CGCN_1D / CGCN_2D have no `_classification` class");
        if (cfg->matrix_form) GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_create_classifier: LCNN / GCN_MW have no `_classification` class");
        if (cfg->neighbourhood == 6 || cfg->neighbourhood == 7)
            GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_create_classifier: GCN_3D / GRU_GCN_3D have no `_classification` class");
        if (cfg->neighbourhood)
            GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_create_classifier: NeuralFingerprint / GCN_1D / GCN_2D%s have no `_classification` class",
                      cfg->neighbourhood >= 4 ? " / GRU_GCN_1D / GRU_GCN_2D" : "");
        if (cfg->physics) GF_REFUSE(GF_ERR_INVALID, "gf_smp_create_classifier: a physics tower has no read-out of its own (physics = 0)");
        if (nClass < 2) GF_REFUSE(GF_ERR_INVALID, "gf_smp_create_classifier: nClass = %d (at least 2)", nClass);
    }
    // ---- the configuration, family by family ----
    if (cfg->covariant) {   // CGCN_1D, CGCN_2D (smp_level_covariant.hip): nLevels = 0 is a model
        if (entry.kind == ConfigEntry::Tower)
            GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_model_create: CGCN_1D / CGCN_2D (covariant = %d) are no towers", cfg->covariant);
        if (cfg->covariant < 1 || cfg->covariant > 2)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: covariant = %d: the covariant models are covariant = 1 (CGCN_1D) and 2 (CGCN_2D)", cfg->covariant);
        if (cfg->first_order || cfg->steerable_2d || cfg->unrestricted || cfg->neighbourhood || cfg->matrix_form || cfg->distance_channel ||
            cfg->readout || !plain_levels(cfg))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: covariant = %d needs every other form selector 0: first_order = steerable_2d = unrestricted = "
                                      "neighbourhood = matrix_form = distance_channel = readout = physics = nContractions = custom_matmul = 0",
                      cfg->covariant);
        if (cfg->nChanels != 1)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: covariant = %d with nChanels = %d: a vertex carries one vector over the vertex ids, nChanels = 1",
                      cfg->covariant, cfg->nChanels);
        if (cfg->nLevels < 0 || cfg->nLevels > 64)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: covariant = %d with nLevels = %d: nLevels in 0 .. 64", cfg->covariant, cfg->nLevels);
        if (cfg->nFeatures < 1 || cfg->nDepth < 0)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: covariant = %d with nFeatures = %d, nDepth = %d: nFeatures >= 1 and nDepth >= 0", cfg->covariant,
                      cfg->nFeatures, cfg->nDepth);
        if ((long long)cfg->nFeatures * ((long long)cfg->nDepth + 1) > 65536)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: covariant = %d with nFeatures (nDepth + 1) = %lld: at most 65536", cfg->covariant,
                      (long long)cfg->nFeatures * ((long long)cfg->nDepth + 1));
        if (cfg->max_nVertices < 1 || cfg->max_nVertices > gf::kCovariantMaxVertices ||
            gf::smp_covariant_lds_bytes(cfg->max_nVertices) > 160 * 1024)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: covariant = %d with max_nVertices = %d: the kernels keep a molecule's whole network in LDS, "
                                      "4 (7 M (M | 1) + 2 M + 8) + M M bytes against 160 KiB per workgroup: max_nVertices in 1 .. %d", cfg->covariant,
                      cfg->max_nVertices, gf::kCovariantMaxVertices);
        Config c = {cfg->nLevels, 1, cfg->nFeatures, cfg->nDepth, cfg->max_nVertices, 0};
        c.nContractions = 0;
        c.max_nVertices = cfg->max_nVertices;
        c.covariant = cfg->covariant;
        *out = c;
        return GF_OK;
    }
    if (cfg->readout) {   // GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (1: forms 2, 3, 6 on pairs), GCA_1D (2: form 2 under the Gram read-out); smp_level_readouts.hip
        const int form = cfg->neighbourhood, ro = cfg->readout;
        if (entry.kind == ConfigEntry::Tower) GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_model_create: the pair and Gram read-outs (readout = %d) are no towers", ro);
        const bool named = ro == 1 ? form == 2 || form == 3 || form == 6 : ro == 2 && form == 2;
        if (!named || cfg->distance_channel || cfg->matrix_form)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: readout = %d with neighbourhood = %d, distance_channel = %d, matrix_form = %d: the read-outs are "
                                      "readout = 1 (pairs) with neighbourhood = 2 (GCN_1D_Kernel), 3 (GCN_2D_Kernel) or 6 (GCN_3D_Kernel) and readout = 2 "
                                      "(Gram) with neighbourhood = 2 (GCA_1D), distance_channel = matrix_form = 0", ro, form, cfg->distance_channel,
                      cfg->matrix_form);
        if (form == 6 && cfg->nChanels > gf::kThirdMaxChanels)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: GCN_3D_Kernel with nChanels = %d: the third-order pool takes at most %d channels", cfg->nChanels,
                      gf::kThirdMaxChanels);
        gf_smp_config as2 = *cfg;   // (form 2's rules: all four classes read max_Radius)
        as2.neighbourhood = 2;
        as2.readout = 0;
        if (!rule_neighbourhood(&as2))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: readout = %d (neighbourhood = %d) needs first_order = steerable_2d = unrestricted = physics = "
                                      "nContractions = custom_matmul = 0, max_receptive_field (%d) == max_nVertices (%d) <= 4096, nLevels >= 0, "
                                      "max_Radius (%d) >= 0, nChanels (%d) <= %d and W1_l, W2_l within 160 KiB", ro, form, cfg->max_receptive_field,
                      cfg->max_nVertices, cfg->max_Radius, cfg->nChanels, gf::kNeighbourhoodMaxChanels);
        if (form == 6 && cfg->max_nVertices > gf::smp_third_max_members(cfg->nChanels))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: GCN_3D_Kernel with max_nVertices = %d: the third-order pool stages a neighbourhood's members in "
                                      "LDS: at most %d vertices at %d channels", cfg->max_nVertices, gf::smp_third_max_members(cfg->nChanels), cfg->nChanels);
        if (ro == 2 && gf::smp_gram_lds_bytes(cfg->max_nVertices, cfg->nChanels) > 160 * 1024)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: GCA_1D with max_nVertices = %d, nChanels = %d: the Gram read-out keeps a molecule's h_L and E in LDS, "
                                      "4 (V (H | 1) + V (V | 1) + 4) = %zu bytes against 160 KiB per workgroup", cfg->max_nVertices, cfg->nChanels,
                      gf::smp_gram_lds_bytes(cfg->max_nVertices, cfg->nChanels));
        Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, 0};
        c.nContractions = 0;
        c.max_nVertices = cfg->max_nVertices;
        c.neighbourhood = form;
        c.max_Radius = cfg->max_Radius;
        c.readout = ro;
        *out = c;
        return GF_OK;
    }
    if (cfg->distance_channel) {   // GCN_1D_Distance, GCN_2D_Distance, GCN_3D_Distance (smp_level_distance.hip): forms 2, 3, 6 on two channels
        const int form = cfg->neighbourhood;
        if (cfg->distance_channel != 1 || cfg->matrix_form || (form != 2 && form != 3 && form != 6))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: distance_channel = %d with neighbourhood = %d, matrix_form = %d: the distance models are "
                                      "distance_channel = 1 with neighbourhood = 2 (GCN_1D_Distance), 3 (GCN_2D_Distance) or 6 (GCN_3D_Distance)",
                      cfg->distance_channel, form, cfg->matrix_form);
        if (form == 6 && cfg->nChanels > gf::kThirdMaxChanels)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: GCN_3D_Distance with nChanels = %d: the third-order pool takes at most %d channels", cfg->nChanels,
                      gf::kThirdMaxChanels);
        gf_smp_config as2 = *cfg;   // (form 2's rules: all three read max_Radius)
        as2.neighbourhood = 2;
        as2.distance_channel = 0;
        if (!rule_neighbourhood(&as2) || gf::smp_neighbourhood_lds_bytes(cfg->nChanels, cfg->max_nVertices) > 160 * 1024)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: distance_channel = 1 (neighbourhood = %d) needs first_order = steerable_2d = unrestricted = physics "
                                      "= nContractions = custom_matmul = 0, max_receptive_field (%d) == max_nVertices (%d) <= 4096, nLevels >= 0, "
                                      "max_Radius (%d) >= 0, nChanels (%d) <= %d and the level's matrices within 160 KiB at both operand widths, F' and "
                                      "max_nVertices", form, cfg->max_receptive_field, cfg->max_nVertices, cfg->max_Radius, cfg->nChanels,
                      gf::kNeighbourhoodMaxChanels);
        if (form == 6 && cfg->max_nVertices > gf::smp_third_max_members(cfg->nChanels))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: GCN_3D_Distance with max_nVertices = %d: the third-order pool stages a neighbourhood's members in "
                                      "LDS: at most %d vertices at %d channels", cfg->max_nVertices, gf::smp_third_max_members(cfg->nChanels), cfg->nChanels);
        Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, 0};
        c.nContractions = 0;
        c.max_nVertices = cfg->max_nVertices;
        c.neighbourhood = form;
        c.max_Radius = cfg->max_Radius;
        c.distance_channel = 1;
        if (param_count(c) > (size_t)kMaxInt)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: distance_channel = 1 with %zu parameters: the count must fit an int", param_count(c));
        *out = c;
        return GF_OK;
    }
    if (cfg->matrix_form) {   // LCNN, GCN_MW (smp_level_rowlist.hip)
        if (entry.kind == ConfigEntry::Tower)
            GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_model_create: LCNN / GCN_MW (matrix_form = %d) are no towers", cfg->matrix_form);
        if (!rule_matrix_form(cfg))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: matrix_form = %d (1: LCNN, 2: GCN_MW) needs first_order = steerable_2d = unrestricted = "
                                      "neighbourhood = physics = nContractions = custom_matmul = 0, max_receptive_field (%d) == max_nVertices (%d) "
                                      "<= 4096, nChanels, nFeatures >= 1, nDepth >= 0, nLevels (%d) in 0 .. 64 for GCN_MW and == 2 for LCNN, and "
                                      "for LCNN nNeighbors (%d), nChanels2 (%d), nDense (%d) >= 1", cfg->matrix_form, cfg->max_receptive_field,
                      cfg->max_nVertices, cfg->nLevels, cfg->nNeighbors, cfg->nChanels2, cfg->nDense);
        const long long wide = matrix_form_widest(cfg);
        if (wide > gf::kRowlistMaxWidth)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: matrix_form = %d with an operand %lld floats wide: the row-list level indexes an operand row "
                                      "and its tile counts with ints: at most %d (F', nChanels, nChanels2, nDense, nNeighbors F', nNeighbors "
                                      "nChanels, max_nVertices nChanels2)", cfg->matrix_form, wide, gf::kRowlistMaxWidth);
        Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, 0};
        c.nContractions = 0;
        c.max_nVertices = cfg->max_nVertices;
        c.matrix_form = cfg->matrix_form;
        if (cfg->matrix_form == 1) c.nNeighbors = cfg->nNeighbors, c.nChanels2 = cfg->nChanels2, c.nDense = cfg->nDense;
        if (param_count(c) > (size_t)kMaxInt)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: matrix_form = %d with %zu parameters: the count must fit an int", cfg->matrix_form, param_count(c));
        *out = c;
        return GF_OK;
    }
    if (cfg->neighbourhood == 6 || cfg->neighbourhood == 7) {   // GCN_3D, GRU_GCN_3D (smp_level_third.hip): nLevels = 0 is a model
        if (cfg->nChanels > gf::kThirdMaxChanels)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: neighbourhood = %d (6: GCN_3D, 7: GRU_GCN_3D) with nChanels = %d: the third-order pool packs "
                                      "a triple of channels into 18 bits and keeps B [H][H] in LDS: at most %d channels",
                      cfg->neighbourhood, cfg->nChanels, gf::kThirdMaxChanels);
        gf_smp_config as2 = *cfg;
        as2.neighbourhood = 2;
        if (!rule_neighbourhood(&as2))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: neighbourhood = %d (6: GCN_3D, 7: GRU_GCN_3D) needs first_order = steerable_2d = unrestricted "
                                      "= physics = nContractions = custom_matmul = 0, max_receptive_field (%d) == max_nVertices (%d) <= 4096, "
                                      "nLevels >= 0, max_Radius (%d) >= 0 and the level's matrices within 160 KiB", cfg->neighbourhood,
                      cfg->max_receptive_field, cfg->max_nVertices, cfg->max_Radius);
        if (cfg->max_nVertices > gf::smp_third_max_members(cfg->nChanels))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: neighbourhood = %d (6: GCN_3D, 7: GRU_GCN_3D) with max_nVertices = %d: the third-order pool "
                                      "stages a neighbourhood's members in LDS (%zu bytes and %d per member at %d channels, 160 KiB per workgroup): "
                                      "at most %d vertices", cfg->neighbourhood, cfg->max_nVertices, gf::smp_third_lds_bytes(cfg->nChanels, 0),
                      4 * cfg->nChanels, cfg->nChanels, gf::smp_third_max_members(cfg->nChanels));
        Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, 0};
        c.nContractions = 0;
        c.max_nVertices = cfg->max_nVertices;
        c.neighbourhood = cfg->neighbourhood;
        c.max_Radius = cfg->max_Radius;
        *out = c;
        return GF_OK;
    }
    if (cfg->neighbourhood == 4 || cfg->neighbourhood == 5) {   // GRU_GCN_1D, GRU_GCN_2D (smp_level_gru.hip): nLevels = 0 is a model
        if (cfg->nChanels > gf::kGruMaxChanels)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: neighbourhood = %d with nChanels = %d: the six [H][H] matrices of a GRU cell are resident in "
                                      "LDS for the length of a level (%zu bytes at %d channels, 160 KiB per workgroup): at most %d channels",
                      cfg->neighbourhood, cfg->nChanels, gf::smp_gru_lds_bytes(cfg->nChanels), cfg->nChanels, gf::kGruMaxChanels);
        if (!rule_gated(cfg))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: neighbourhood = %d (4: GRU_GCN_1D, 5: GRU_GCN_2D) needs first_order = steerable_2d = unrestricted "
                                      "= physics = nContractions = custom_matmul = 0, max_receptive_field (%d) == max_nVertices (%d) <= 4096, "
                                      "nLevels >= 0, max_Radius (%d) >= 0 and W within 160 KiB", cfg->neighbourhood, cfg->max_receptive_field,
                      cfg->max_nVertices, cfg->max_Radius);
        Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, 0};
        c.nContractions = 0;
        c.max_nVertices = cfg->max_nVertices;
        c.neighbourhood = cfg->neighbourhood;
        c.max_Radius = cfg->max_Radius;
        *out = c;
        return GF_OK;
    }
    if (cfg->neighbourhood) {   // NeuralFingerprint, GCN_1D, GCN_2D (smp_level_neighbourhood.hip): nLevels = 0 is a model
        if (!rule_neighbourhood(cfg))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: neighbourhood = %d (1: NeuralFingerprint, 2: GCN_1D, 3: GCN_2D) needs first_order = steerable_2d = "
                                      "unrestricted = physics = nContractions = custom_matmul = 0, max_receptive_field (%d) == max_nVertices (%d) <= "
                                      "4096, nLevels >= 0, nDepth = 0 in form 1, max_Radius (%d) >= 0 in form 2, nChanels (%d) <= %d and W1_l, W2_l "
                                      "within 160 KiB", cfg->neighbourhood, cfg->max_receptive_field, cfg->max_nVertices, cfg->max_Radius, cfg->nChanels,
                      gf::kNeighbourhoodMaxChanels);
        Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, 0};
        c.nContractions = 0;
        c.max_nVertices = cfg->max_nVertices;
        c.neighbourhood = cfg->neighbourhood;
        c.max_Radius = cfg->neighbourhood == 2 ? cfg->max_Radius : 0;   // (form 3 stores it and never reads it; form 1 has none)
        *out = c;
        return GF_OK;
    }
    if (cfg->nLevels < 1 || cfg->nChanels < 1 || cfg->nFeatures < 1 || cfg->nDepth < 0 || cfg->max_receptive_field < 1)
        GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: bad configuration");
    Config c = {cfg->nLevels, cfg->nChanels, cfg->nFeatures, cfg->nDepth, cfg->max_receptive_field, cfg->has_WL_ordering};
    c.nContractions = cfg->nContractions ? cfg->nContractions : 18;
    c.custom_matmul = cfg->custom_matmul ? 1 : 0;
    c.physics = cfg->physics ? 1 : 0;
    c.nClass = nClass;
    c.max_nVertices = cfg->first_order || cfg->steerable_2d || cfg->unrestricted ? cfg->max_nVertices : 0;
    if (cfg->unrestricted) {   // Unrestricted_SMP_1D, _1D_ver2, _2D (smp_level_unrestricted.hip)
        if (!rule_unrestricted(cfg))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: unrestricted = %d (1: Unrestricted_SMP_1D, 2: _1D_ver2, 3: _2D) needs first_order = "
                                      "steerable_2d = 0, max_receptive_field (%d) == max_nVertices (%d) <= 4096, nContractions = custom_matmul = "
                                      "physics = 0 and a parameter count that fits an int", cfg->unrestricted, cfg->max_receptive_field, cfg->max_nVertices);
        // the handle also carries the restricted sibling whose rows, tables and read-out the form sits on (Config::unrestricted)
        c.unrestricted = cfg->unrestricted;
        c.first_order = cfg->unrestricted == 1 ? 2 : cfg->unrestricted == 2 ? 3 : 0;
        c.steerable_2d = cfg->unrestricted == 3 ? 1 : 0;
        c.nContractions = c.first_order ? 2 : 0;
    } else if (cfg->steerable_2d) {   // SMP_2D, SMP_2D_ver4 (smp_level_2d.hip; a classifier read-out is allowed), SMP_2D_ver5 (smp_level_2d_ver5.hip)
        if (!rule_2d(cfg))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: steerable_2d = %d (1: SMP_2D, 2: SMP_2D_ver4, 5: SMP_2D_ver5) needs first_order = 0, "
                                      "max_receptive_field (%d) == max_nVertices (%d) <= 4096, nContractions = custom_matmul = physics = 0 and, "
                                      "for 5, nChanels (%d) <= 128", cfg->steerable_2d, cfg->max_receptive_field, cfg->max_nVertices, cfg->nChanels);
        if (nClass && cfg->steerable_2d == 5) GF_REFUSE(GF_ERR_UNSUPPORTED, "gf_smp_create_classifier: SMP_2D_ver5 has no `_classification` class");
        c.steerable_2d = cfg->steerable_2d;
        c.nContractions = 0;
    } else if (cfg->first_order >= 2) {   // SMP_1D, SMP_1D_ver2, SMP_1D_ver3 (smp_level_1d.hip); a classifier read-out is allowed
        if (!rule_1d(cfg))
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: first_order = %d (2: SMP_1D, 3: SMP_1D_ver2, 4: SMP_1D_ver3) needs max_receptive_field "
                                      "(%d) == max_nVertices (%d) and nContractions = custom_matmul = physics = 0", cfg->first_order,
                      cfg->max_receptive_field, cfg->max_nVertices);
        c.first_order = cfg->first_order;
        c.nContractions = 2;
    } else if (cfg->first_order) {   // SMP_theta: K_l = [2 C'][C], per-size blocks of max_nVertices entries (Config::first_order)
        if (cfg->nContractions || cfg->custom_matmul || cfg->max_nVertices < cfg->max_receptive_field)
            GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: first_order = 1 needs nContractions = custom_matmul = 0 and max_nVertices (%d) >= "
                                      "max_receptive_field (%d)", cfg->max_nVertices, cfg->max_receptive_field);
        c.first_order = 1;
        c.nContractions = 2;
        if (cfg->physics && entry.kind == ConfigEntry::Tower) c.decay = entry.decay;   // (a CCN_1D tower)
    }
    if (c.nContractions == 4 && c.custom_matmul)   // SMP_gamma: Reshape2D + MatMul on [4 C][C]
        GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: nContractions = 4 (SMP_gamma) applies K_l [4 C][C] by Reshape2D + MatMul: set custom_matmul = 0");
    // (a tower of SMP_gamma_physics / SMP_gamma_pairgraphs: RisiContraction_4, K_l [4 C_{l-1}][C_l], computed at its own halving widths)
    if (c.physics && (c.nDepth != 0 || (c.nContractions != 18 && c.nContractions != 4 && !c.first_order) || c.custom_matmul))
        GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: a physics tower has nDepth 0 (raw features), RisiContraction_18 or _4 and [nK C', C] weights");
    if (!c.per_size() && c.nContractions != 4 && c.nContractions != 10 && c.nContractions != 18 && c.nContractions != 50)
        GF_REFUSE(GF_ERR_INVALID, "gf_smp_create: nContractions = %d (expected 4, 10, 18 or 50)", cfg->nContractions);
    *out = c;
    return GF_OK;
}
#undef GF_REFUSE

}  // namespace gfsmp

namespace gf {

bool model_plan(const gf_smp_model_config *cfg, ModelPlan *p, char *why, size_t nwhy) {
    if (cfg->nTowers < 1 || cfg->nTowers > 2 || cfg->nLevels < 1 || cfg->nChanels < 1 || cfg->max_receptive_field < 1 || cfg->nKept < 0 ||
        cfg->nKept > 18 || cfg->nFeatures[0] < 1 || (cfg->nTowers == 2 && cfg->nFeatures[1] < 1)) {   // (nFeatures: what gf_smp_create refuses of a tower)
        snprintf(why, nwhy, "gf_smp_model_create: bad configuration");
        return false;
    }
    const int nK = cfg->nContractions ? cfg->nContractions : 18;
    if (nK != 18 && nK != 4) {
        snprintf(why, nwhy, "gf_smp_model_create: nContractions = %d (expected 0 or 18: RisiContraction_18, 4: RisiContraction_4)", cfg->nContractions);
        return false;
    }
    if (nK == 4 && cfg->nKept > 0) {
        snprintf(why, nwhy, "gf_smp_model_create: nKept > 0 (RisiContraction_18_dropout) with nContractions = 4: no such model");
        return false;
    }
    const int maxV[2] = {cfg->max_nVertices[0], cfg->max_nVertices[1] ? cfg->max_nVertices[1] : cfg->max_nVertices[0]};
    if (cfg->first_order && (cfg->nContractions || cfg->nKept > 0 || maxV[0] < cfg->max_receptive_field || maxV[1] < cfg->max_receptive_field)) {
        snprintf(why, nwhy, "gf_smp_model_create: first_order = 1 (SMP_theta_physics / _pairgraphs) needs nContractions = nKept = 0 and "
                            "max_nVertices (%d, %d) >= max_receptive_field (%d)", maxV[0], maxV[1], cfg->max_receptive_field);
        return false;
    }
    // CCN_1D (GraphFlow/CCN_1D.h:34-39): always two first-order towers, at least 16 channels, 0 < decay <= 1 (!(..): a NaN is refused too)
    if (cfg->ccn_1d && (cfg->nTowers != 2 || cfg->first_order != 1 || cfg->nChanels < gfsmp::kCcnMinChanels ||
                        !(cfg->nChanels_decay > 0.0 && cfg->nChanels_decay <= 1.0))) {
        snprintf(why, nwhy, "gf_smp_model_create: ccn_1d = 1 (CCN_1D) needs nTowers = 2 (%d), first_order = 1 (%d), nChanels >= 16 (%d) and "
                            "0 < nChanels_decay <= 1 (%g)", cfg->nTowers, cfg->first_order, cfg->nChanels, cfg->nChanels_decay);
        return false;
    }
    p->nK = nK;
    p->nTowers = cfg->nTowers;
    p->maxV[0] = maxV[0];
    p->maxV[1] = maxV[1];
    p->decay = cfg->ccn_1d ? cfg->nChanels_decay : 0.0;
    // the towers: what gf_smp_create is asked for, and what it will make of it (the width rule -- halving, or the decay -- and the blocks)
    gfsmp::Config *tower = p->tower;
    for (int t = 0; t < cfg->nTowers; ++t) {
        gf_smp_config &tc = p->tower_cfg[t];
        tc = gf_smp_config();   // (every field zero)
        tc.nLevels = cfg->nLevels, tc.nChanels = cfg->nChanels, tc.nFeatures = cfg->nFeatures[t], tc.max_receptive_field = cfg->max_receptive_field;
        tc.nContractions = cfg->first_order ? 0 : nK, tc.physics = 1;
        tc.first_order = cfg->first_order ? 1 : 0, tc.max_nVertices = cfg->first_order ? maxV[t] : 0;
        if (gfsmp::resolve_config(&p->tower_cfg[t], {gfsmp::ConfigEntry::Tower, 0, p->decay}, &tower[t], why, nwhy) != GF_OK) return false;
    }
    const int L = cfg->nLevels;
    for (int l = 0; l <= L; ++l) {
        p->lvlC.push_back(tower[0].level_channels(l));
        p->fwidth += p->lvlC.back();
    }
    size_t off = 0;
    // the H matrices come first (one per tower), then the levels, towers interleaved inside a level
    size_t toff[2] = {0, 0};
    for (int t = 0; t < cfg->nTowers; ++t) {
        const size_t nH = tower[t].first_block().n;
        p->segs[t].push_back({off, 0, nH});
        off += nH;
        toff[t] = nH;
    }
    for (int l = 1; l <= L; ++l)
        for (int t = 0; t < cfg->nTowers; ++t) {
            const size_t n = tower[t].level_blocks(l).total();   // (one contiguous segment in either layout)
            p->segs[t].push_back({off, toff[t], n});
            off += n;
            toff[t] += n;
        }
    p->head_off = off;
    // head widths: physics nTotal -> nTotal / 2 -> 1 (:229-238); pairgraphs nTotal -> max(nTotal / 2, 10) -> max(that / 2, 10) -> 1;
    // CCN_1D nTotal -> max(int(ceil(nTotal * decay)), 16) -> max(int(ceil(that * decay)), 16) -> 1 (CCN_1D.h:352-353)
    const int nTotal = cfg->nTowers * p->fwidth;
    p->widths.push_back(nTotal);
    if (p->decay > 0.0) {
        for (int i = 0; i < 2; ++i) {
            const int h = int(std::ceil(p->widths.back() * p->decay));
            p->widths.push_back(h > gfsmp::kCcnMinChanels ? h : gfsmp::kCcnMinChanels);
        }
    } else if (cfg->nTowers == 1) {
        p->widths.push_back(nTotal / 2);
    } else {
        const int h1 = nTotal / 2 > 10 ? nTotal / 2 : 10, h2 = h1 / 2 > 10 ? h1 / 2 : 10;
        p->widths.push_back(h1);
        p->widths.push_back(h2);
    }
    if (p->widths[1] < 1) {
        snprintf(why, nwhy, "gf_smp_model_create: %d feature columns leave no hidden units (the reference uses nTotal / 2)", nTotal);
        return false;
    }
    each_head_block(p->widths, [p](size_t n) { p->head_params += n; });   // (= gf_head_param_count)
    p->n_params = off + p->head_params;
    return true;
}

namespace {
// The count / capacity protocol of the three *_config_param_blocks calls: each(f) calls f(n) for every block in order.  Two walks and no
// allocation: a caller's configuration may have any number of blocks.
template <class Each>
size_t write_offsets(Each each, size_t *offsets, size_t capacity) {
    size_t count = 0;
    each([&count](size_t) { ++count; });
    if (offsets && count && capacity > count) {
        size_t at = 0, i = 0;
        each([&](size_t n) {
            offsets[i++] = at;
            at += n;
        });
        offsets[count] = at;
    }
    return count;
}
size_t config_param_blocks(const gf_smp_config *cfg, const gfsmp::ConfigEntry &entry, size_t *offsets, size_t capacity) {
    gfsmp::Config c;
    char why[640];
    if (gfsmp::resolve_config(cfg, entry, &c, why, sizeof why) != GF_OK) return 0;
    return write_offsets([&c](auto f) { c.each_registered(f); }, offsets, capacity);
}
}  // namespace
}  // namespace gf

extern "C" {
size_t gf_smp_config_param_blocks(const gf_smp_config *cfg, size_t *offsets, size_t capacity) {
    return gf::config_param_blocks(cfg, gfsmp::kHandleEntry, offsets, capacity);
}
size_t gf_smp_classifier_config_param_blocks(const gf_smp_config *cfg, int nClass, size_t *offsets, size_t capacity) {
    return gf::config_param_blocks(cfg, {gfsmp::ConfigEntry::Classifier, nClass, 0.0}, offsets, capacity);
}
size_t gf_smp_model_config_param_blocks(const gf_smp_model_config *cfg, size_t *offsets, size_t capacity) {
    gf::ModelPlan plan;
    char why[512];
    if (!cfg || !gf::model_plan(cfg, &plan, why, sizeof why)) return 0;
    return gf::write_offsets([&plan](auto f) { gf::each_registered(plan, f); }, offsets, capacity);
}
}  // extern "C"
