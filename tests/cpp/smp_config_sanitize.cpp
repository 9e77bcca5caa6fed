// Stand-alone program for the sanitizers: gfsmp::resolve_config (graphflow_amd/csrc/smp_config.cpp) and the block enumeration of
// gfsmp::Config (smp_prep.h) on the grid of tests/test_smp_config_agreement.py -- an accepted configuration per family and form, every
// refusal of the create functions -- and on hostile structs: the resolver shifts and multiplies a caller's fields.  On the way: an accepted
// configuration's blocks add up to param_count at both granularities, and view_params ends where param_count says.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "smp_config.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

// nLevels 2, nChanels 4, nFeatures 4, nDepth 1, max_receptive_field 6, WL ordering; the rest zero
static gf_smp_config base() {
    gf_smp_config c;
    std::memset(&c, 0, sizeof c);
    c.nLevels = 2, c.nChanels = 4, c.nFeatures = 4, c.nDepth = 1, c.max_receptive_field = 6, c.has_WL_ordering = 1;
    return c;
}
static gf_smp_config no_cap() {
    gf_smp_config c = base();
    c.max_nVertices = c.max_receptive_field;
    return c;
}
#define WITH(start, ...) [] { gf_smp_config c = start(); __VA_ARGS__; return c; }()

static gf_status resolve(const gf_smp_config &c, int nClass, gfsmp::Config *out, char *why, size_t nwhy) {
    const gfsmp::ConfigEntry entry = {nClass ? gfsmp::ConfigEntry::Classifier : gfsmp::ConfigEntry::Handle, nClass, 0.0};
    why[0] = 0;
    return gfsmp::resolve_config(&c, entry, out, why, nwhy);
}

// the draw blocks and the level segments must both add up to param_count, and the views must tile the vector
static void check_layout(const gfsmp::Config &c) {
    size_t drawn = c.first_block().n + c.readout_block().n;
    for (int l = 1; l <= c.nLevels; ++l) {
        size_t level = 0;
        c.level_blocks(l).each_draw([&level](const gfsmp::Config::Block &b) {
            CHECK(b.n > 0 && b.div > 0);
            level += b.n;
        });
        CHECK(level == c.level_blocks(l).total());
        drawn += level;
    }
    const size_t n = gfsmp::param_count(c);
    CHECK(drawn == n);
    std::vector<float> p(n + 1, 0.f);
    float *H, *W;
    std::vector<float *> K, b;
    gfsmp::view_params<float>(c, p.data(), &H, &K, &b, &W);
    CHECK(H == p.data() && W + c.readout_block().n == p.data() + n);
    for (int l = 1; l <= c.nLevels; ++l) CHECK(K[l] >= p.data() && K[l] <= W && b[l] >= p.data() && b[l] <= W);
    float *q = p.data();
    gfsmp::uniform_draw(c.first_block(), &q);
    for (int l = 1; l <= c.nLevels; ++l) c.level_blocks(l).each_draw([&q](const gfsmp::Config::Block &blk) { gfsmp::uniform_draw(blk, &q); });
    gfsmp::uniform_draw(c.readout_block(), &q);
    CHECK(q == p.data() + n && p[n] == 0.f);
}

struct Case {
    gf_smp_config cfg;
    int nClass;
    gf_status status;
};

int main() {
    const gf_status OK = GF_OK, INV = GF_ERR_INVALID, UNS = GF_ERR_UNSUPPORTED;
    const std::vector<Case> grid = {
        // accepted: the 18-, 10-, 50- and 4-slice models, an `_18` tower, the field-level families, the neighbourhood forms, the classifiers
        {base(), 0, OK},
        {WITH(base, c.nContractions = 18, c.custom_matmul = 1), 0, OK},
        {WITH(base, c.nContractions = 10, c.custom_matmul = 1), 0, OK},
        {WITH(base, c.nContractions = 50, c.custom_matmul = 1), 0, OK},
        {WITH(base, c.nContractions = 4), 0, OK},
        {WITH(base, c.physics = 1, c.nDepth = 0), 0, OK},
        {WITH(no_cap, c.first_order = 1), 0, OK},
        {WITH(base, c.first_order = 1, c.max_nVertices = 12), 0, OK},
        {WITH(no_cap, c.first_order = 2), 0, OK},
        {WITH(no_cap, c.first_order = 3), 0, OK},
        {WITH(no_cap, c.first_order = 4), 0, OK},
        {WITH(no_cap, c.steerable_2d = 1), 0, OK},
        {WITH(no_cap, c.steerable_2d = 2), 0, OK},
        {WITH(no_cap, c.steerable_2d = 5), 0, OK},
        {WITH(no_cap, c.unrestricted = 1), 0, OK},
        {WITH(no_cap, c.unrestricted = 2), 0, OK},
        {WITH(no_cap, c.unrestricted = 3), 0, OK},
        {WITH(no_cap, c.neighbourhood = 1, c.nDepth = 0), 0, OK},
        {WITH(no_cap, c.neighbourhood = 2, c.max_Radius = 1), 0, OK},
        {WITH(no_cap, c.neighbourhood = 3), 0, OK},
        {WITH(no_cap, c.neighbourhood = 3, c.nLevels = 0), 0, OK},
        {WITH(base, c.nContractions = 10, c.custom_matmul = 1), 3, OK},
        {WITH(base, c.nContractions = 50, c.custom_matmul = 1), 3, OK},
        {WITH(base, c.nContractions = 18, c.custom_matmul = 1), 3, OK},
        {WITH(base, c.nContractions = 4), 3, OK},
        {WITH(no_cap, c.first_order = 2), 3, OK},
        {WITH(no_cap, c.first_order = 3), 3, OK},
        {WITH(no_cap, c.first_order = 4), 3, OK},
        {WITH(no_cap, c.steerable_2d = 1), 3, OK},
        {WITH(no_cap, c.steerable_2d = 2), 3, OK},
        // refused
        {WITH(base, c.nContractions = 7), 0, INV},
        {WITH(base, c.nContractions = 4, c.custom_matmul = 1), 0, INV},
        {WITH(base, c.physics = 1), 0, INV},
        {WITH(base, c.physics = 1, c.nDepth = 0, c.nContractions = 10), 0, INV},
        {WITH(no_cap, c.physics = 1, c.nDepth = 0, c.first_order = 1), 0, INV},
        {WITH(base, c.physics = 1, c.nDepth = 0, c.nContractions = 4), 0, INV},
        {WITH(base, c.nLevels = 0), 0, INV},
        {WITH(base, c.nChanels = 0), 0, INV},
        {WITH(base, c.nDepth = -1), 0, INV},
        {WITH(no_cap, c.neighbourhood = 1), 0, INV},
        {WITH(no_cap, c.neighbourhood = 2, c.first_order = 2), 0, INV},
        {WITH(base, c.unrestricted = 1, c.max_nVertices = 8), 0, INV},
        {WITH(no_cap, c.unrestricted = 4), 0, INV},
        {WITH(base, c.unrestricted = 3, c.nChanels = 65536, c.nLevels = 4, c.max_receptive_field = 4096, c.max_nVertices = 4096), 0, INV},
        {WITH(no_cap, c.steerable_2d = 3), 0, INV},
        {WITH(no_cap, c.steerable_2d = 1, c.first_order = 2), 0, INV},
        {WITH(no_cap, c.steerable_2d = 5, c.nChanels = 129), 0, INV},
        {WITH(base, c.first_order = 2, c.max_nVertices = 8), 0, INV},
        {WITH(no_cap, c.first_order = 3, c.nLevels = 17), 0, INV},
        {WITH(no_cap, c.first_order = 5), 0, INV},
        {WITH(base, c.first_order = 1, c.max_nVertices = 5), 0, INV},
        {WITH(no_cap, c.first_order = 1, c.nContractions = 18), 0, INV},
        {WITH(no_cap, c.first_order = 1), 3, UNS},
        {WITH(no_cap, c.unrestricted = 1), 3, UNS},
        {WITH(no_cap, c.neighbourhood = 2), 3, UNS},
        {WITH(base, c.physics = 1, c.nDepth = 0), 3, INV},
        {base(), 1, INV},
        {WITH(no_cap, c.steerable_2d = 5), 3, UNS},
        {WITH(base, c.nContractions = 7), 3, INV},
        {WITH(base, c.first_order = 2, c.max_nVertices = 8), 3, INV},
    };
    char why[640];
    gfsmp::Config out;
    for (size_t i = 0; i < grid.size(); ++i) {
        const gf_status st = resolve(grid[i].cfg, grid[i].nClass, &out, why, sizeof why);
        if (st != grid[i].status) std::printf("grid entry %zu: status %d, expected %d (%s)\n", i, (int)st, (int)grid[i].status, why);
        CHECK(st == grid[i].status);
        CHECK((st == GF_OK) == (why[0] == 0));
        if (st == GF_OK) check_layout(out);
    }
    // the towers of gf_smp_model_create: the two the plain entry refuses, and CCN_1D's width rule
    const gfsmp::ConfigEntry tower = {gfsmp::ConfigEntry::Tower, 0, 0.0}, ccn = {gfsmp::ConfigEntry::Tower, 0, 0.7};
    const gf_smp_config theta_tower = WITH(no_cap, c.physics = 1, c.nDepth = 0, c.first_order = 1, c.nChanels = 20);
    const gf_smp_config gamma_tower = WITH(base, c.physics = 1, c.nDepth = 0, c.nContractions = 4);
    CHECK(gfsmp::resolve_config(&theta_tower, tower, &out, why, sizeof why) == GF_OK && out.level_channels(2) == 5);
    check_layout(out);
    CHECK(gfsmp::resolve_config(&theta_tower, ccn, &out, why, sizeof why) == GF_OK && out.level_channels(1) == 16 && out.level_channels(2) == 16);
    check_layout(out);
    CHECK(gfsmp::resolve_config(&gamma_tower, tower, &out, why, sizeof why) == GF_OK && out.nContractions == 4);
    check_layout(out);
    CHECK(gfsmp::resolve_config(nullptr, tower, &out, why, sizeof why) == GF_ERR_INVALID);

    // hostile structs: every field of every family at values no caller means.  Whatever the verdict, nothing may overflow on the way to it;
    // what is accepted at a size a test can hold is laid out as well.
    const int hostile[] = {INT_MIN, -1, 0, 31, 4096, 65536, INT_MAX};
    int gf_smp_config::*const fields[] = {&gf_smp_config::nLevels, &gf_smp_config::nChanels, &gf_smp_config::nFeatures, &gf_smp_config::nDepth,
                                          &gf_smp_config::max_receptive_field, &gf_smp_config::max_nVertices, &gf_smp_config::nContractions,
                                          &gf_smp_config::max_Radius};
    std::vector<gf_smp_config> families;
    for (size_t i = 0; i < grid.size(); ++i)
        if (grid[i].status == GF_OK && !grid[i].nClass) families.push_back(grid[i].cfg);
    long accepted = 0, refused = 0;
    for (const gf_smp_config &family : families)
        for (int gf_smp_config::*f : fields)
            for (int v : hostile)
                for (int both = 0; both < 2; ++both) {
                    gf_smp_config c = family;
                    c.*f = v;
                    if (both) c.max_receptive_field = c.max_nVertices = (f == &gf_smp_config::max_receptive_field || f == &gf_smp_config::max_nVertices) ? v : 4096;
                    for (int nClass : {0, 3, INT_MIN}) {
                        const gf_status st = resolve(c, nClass, &out, why, sizeof why);
                        st == GF_OK ? ++accepted : ++refused;
                        if (st == GF_OK && out.nLevels <= 4 && out.nChanels <= 64 && out.nFeatures <= 64 && out.nDepth <= 4 && out.max_nVertices <= 64)
                            check_layout(out);
                    }
                }
    // the four the issue names, outright
    CHECK(resolve(WITH(no_cap, c.first_order = 3, c.nLevels = 31), 0, &out, why, sizeof why) == GF_ERR_INVALID);
    CHECK(resolve(WITH(no_cap, c.steerable_2d = 2, c.nLevels = 31), 0, &out, why, sizeof why) == GF_ERR_INVALID);
    CHECK(resolve(WITH(base, c.unrestricted = 3, c.max_receptive_field = 4096, c.max_nVertices = 4096), 0, &out, why, sizeof why) == GF_ERR_INVALID);   // (2.3e10 s^2 per channel: no int)
    CHECK(resolve(WITH(base, c.unrestricted = 3, c.max_receptive_field = 512, c.max_nVertices = 512), 0, &out, why, sizeof why) == GF_OK);
    CHECK(gfsmp::param_count(out) == (size_t)4 * 8 + 2 * ((size_t)4 * (512ull * 513 * 1025 / 6) + 512ull * 4 + 4) + 4);
    CHECK(resolve(WITH(base, c.unrestricted = 3, c.max_receptive_field = 4096, c.max_nVertices = 4096, c.nChanels = INT_MAX), 0, &out, why, sizeof why) == GF_ERR_INVALID);
    CHECK(resolve(WITH(no_cap, c.unrestricted = 2, c.nFeatures = INT_MAX, c.nDepth = INT_MAX), 0, &out, why, sizeof why) == GF_ERR_INVALID);
    CHECK(resolve(WITH(no_cap, c.neighbourhood = 2, c.nFeatures = INT_MAX, c.nDepth = INT_MAX), 0, &out, why, sizeof why) == GF_ERR_INVALID);
    CHECK(resolve(WITH(no_cap, c.first_order = 4, c.nChanels = INT_MAX), 0, &out, why, sizeof why) == GF_ERR_INVALID);
    CHECK(resolve(WITH(base, c.nLevels = -5, c.nChanels = -5, c.nFeatures = -5), 0, &out, why, sizeof why) == GF_ERR_INVALID);
    CHECK(accepted > 0 && refused > 0);
    std::printf("%ld hostile configurations accepted, %ld refused\n", accepted, refused);
    std::printf(fails ? "FAILED\n" : "PASSED\n");
    return fails ? 1 : 0;
}
