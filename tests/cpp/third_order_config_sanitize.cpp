// Stand-alone program for the sanitizers: the branches gfsmp::resolve_config (graphflow_amd/csrc/smp_config.cpp) has for GCN_3D and
// GRU_GCN_3D (gf_smp_config.neighbourhood = 6, 7), the block enumeration of the Config they become (smp_prep.h) and the LDS plan of the
// third-order pool (smp_config.h: smp_third_lds_bytes, smp_third_max_members) -- accepted configurations, every refusal with a piece of
// its message, and hostile structs: the resolver multiplies a caller's fields.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "smp_config.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static gf_smp_config form(int f, int L, int H, int F, int D, int maxV, int R) {
    gf_smp_config c;
    std::memset(&c, 0, sizeof c);
    c.nLevels = L, c.nChanels = H, c.nFeatures = F, c.nDepth = D, c.max_receptive_field = c.max_nVertices = maxV;
    c.neighbourhood = f, c.max_Radius = R;
    return c;
}

static gf_status resolve(const gf_smp_config &c, int nClass, gfsmp::Config *out, char *why, size_t nwhy) {
    const gfsmp::ConfigEntry entry = {nClass ? gfsmp::ConfigEntry::Classifier : gfsmp::ConfigEntry::Handle, nClass, 0.0};
    why[0] = 0;
    return gfsmp::resolve_config(&c, entry, out, why, nwhy);
}

// the blocks add up to param_count, the views tile the vector, the draws end where param_count says
static void check_layout(const gfsmp::Config &c, size_t expect) {
    const size_t n = gfsmp::param_count(c);
    CHECK(n == expect);
    size_t drawn = c.first_block().n + c.readout_block().n;
    c.shared_blocks().each_draw([&drawn](const gfsmp::Config::Block &b) { drawn += b.n; });
    for (int l = 1; l <= c.nLevels; ++l) c.level_blocks(l).each_draw([&drawn](const gfsmp::Config::Block &b) { drawn += b.n; });
    CHECK(drawn == n);
    std::vector<float> p(n + 1, 0.f);
    float *H, *W, *shared;
    std::vector<float *> K, b;
    gfsmp::view_params<float>(c, p.data(), &H, &K, &b, &W, &shared);
    CHECK(H == p.data() && W + c.readout_block().n == p.data() + n && shared == p.data() + c.first_block().n);
    float *q = p.data();
    gfsmp::uniform_draw(c.first_block(), &q);
    c.shared_blocks().each_draw([&q](const gfsmp::Config::Block &blk) { gfsmp::uniform_draw(blk, &q); });
    for (int l = 1; l <= c.nLevels; ++l) c.level_blocks(l).each_draw([&q](const gfsmp::Config::Block &blk) { gfsmp::uniform_draw(blk, &q); });
    gfsmp::uniform_draw(c.readout_block(), &q);
    CHECK(q == p.data() + n && p[n] == 0.f);
}

int main() {
    char why[640];
    gfsmp::Config out;
    // accepted: both forms at 0, 1 and 3 levels, radius 0 and beyond the levels, 1 and 64 channels, the largest neighbourhood at 64
    for (int f = 6; f <= 7; ++f)
        for (int L : {0, 1, 3})
            for (int H : {1, 5, 64})
                for (int R : {0, 5}) {
                    const gf_smp_config c = form(f, L, H, 4, 1, H == 64 ? 474 : 12, R);
                    CHECK(resolve(c, 0, &out, why, sizeof why) == GF_OK && !why[0]);
                    CHECK(out.neighbourhood == f && out.third_order() && out.gated() == (f == 7) && out.max_Radius == R);
                    for (int l = 1; l <= L; ++l) CHECK(out.nb_radius(l) == (l < R ? l : R));
                    const size_t FD = 8, h = (size_t)H;
                    check_layout(out, f == 6 ? h * FD + (size_t)L * (h * FD + h * h) + h : h * FD + 8 * h * h + h);
                    CHECK(resolve(c, 3, &out, why, sizeof why) == GF_ERR_UNSUPPORTED && std::strstr(why, "GCN_3D / GRU_GCN_3D have no"));
                }
    // the forms that keep their predicates
    for (int f = 1; f <= 5; ++f) {
        const gf_smp_config c = form(f, 2, 8, 4, f == 1 ? 0 : 1, 9, 1);
        CHECK(resolve(c, 0, &out, why, sizeof why) == GF_OK && !out.third_order() && out.gated() == (f >= 4));
    }
    // refused, with a piece of the message
    struct Bad {
        gf_smp_config c;
        const char *text;
    };
    std::vector<Bad> bad;
    for (int f = 6; f <= 7; ++f) {
        gf_smp_config c = form(f, 2, 8, 5, 1, 9, 1);
        c.first_order = 1, bad.push_back({c, "GRU_GCN_3D) needs"});
        c = form(f, 2, 8, 5, 1, 9, 1), c.steerable_2d = 1, bad.push_back({c, "GRU_GCN_3D) needs"});
        c = form(f, 2, 8, 5, 1, 9, 1), c.unrestricted = 1, bad.push_back({c, "GRU_GCN_3D) needs"});
        c = form(f, 2, 8, 5, 1, 9, 1), c.physics = 1, bad.push_back({c, "GRU_GCN_3D) needs"});
        c = form(f, 2, 8, 5, 1, 9, 1), c.custom_matmul = 1, bad.push_back({c, "GRU_GCN_3D) needs"});
        c = form(f, 2, 8, 5, 1, 9, 1), c.nContractions = 18, bad.push_back({c, "GRU_GCN_3D) needs"});
        c = form(f, 2, 8, 5, 1, 9, 1), c.max_receptive_field = 6, bad.push_back({c, "GRU_GCN_3D) needs"});
        bad.push_back({form(f, 2, 8, 5, 1, 9, -1), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, -1, 8, 5, 1, 9, 1), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, 2, 0, 5, 1, 9, 1), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, 2, INT_MIN, 5, 1, 9, 1), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, 2, 8, INT_MAX, INT_MAX, 9, 1), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, 2, 8, 5, 1, INT_MAX, 1), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, 2, 8, 5, 1, 4097, 1), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, INT_MAX, 8, 5, 1, 9, INT_MAX), "GRU_GCN_3D) needs"});
        bad.push_back({form(f, 2, 65, 5, 1, 9, 1), "at most 64 channels"});
        bad.push_back({form(f, 2, INT_MAX, 5, 1, 9, 1), "at most 64 channels"});
        bad.push_back({form(f, 2, 64, 5, 1, 475, 1), "at most 474 vertices"});
        bad.push_back({form(f, 2, 32, 5, 1, 1200, 1), "at most 1046 vertices"});
    }
    for (const Bad &b : bad) {
        CHECK(resolve(b.c, 0, &out, why, sizeof why) == GF_ERR_INVALID);
        if (!std::strstr(why, b.text)) std::printf("FAILED: \"%s\" lacks \"%s\"\n", why, b.text), ++fails;
    }
    // the LDS plan: the largest neighbourhood fits 160 KiB, one more does not; the fixed part at 64 channels is the documented figure
    CHECK(gf::smp_third_lds_bytes(64, 0) == 42272 && gf::smp_third_max_members(64) == 474);
    for (int H = 1; H <= gf::kThirdMaxChanels; ++H) {
        const int m = gf::smp_third_max_members(H);
        CHECK(m >= 3 && gf::smp_third_lds_bytes(H, m) <= 160 * 1024 && gf::smp_third_lds_bytes(H, m + 1) > 160 * 1024);
    }
    std::printf(fails ? "%d checks FAILED\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
