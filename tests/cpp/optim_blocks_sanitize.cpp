// Stand-alone program for the sanitizers: the host-only parameter-block tables -- gf_smp_config_param_blocks, its classifier and model
// siblings (graphflow_amd/csrc/smp_config.cpp) -- over the configurations of Part B of tests/golden/optimisers.npz
// (tests/golden/make_optimiser_golden.py: BLOCK_CASES, in that order), the count / capacity protocol with guard words around the caller's
// buffer, refused and hostile configurations.  Prints one line per class, "<class> <size of every block>", for tests/test_optimisers.py
// to compare with the record.
#include <climits>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "smp_config.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static gf_smp_config zero() {
    gf_smp_config c;
    std::memset(&c, 0, sizeof c);
    return c;
}
// nLevels 2, nFeatures 4, nDepth 1, fields of up to 6 vertices
static gf_smp_config field(int nChanels) {
    gf_smp_config c = zero();
    c.nLevels = 2, c.nChanels = nChanels, c.nFeatures = 4, c.nDepth = 1, c.max_receptive_field = 6, c.has_WL_ordering = 1;
    return c;
}
static gf_smp_config vertex(int nChanels) {
    gf_smp_config c = field(nChanels);
    c.has_WL_ordering = 0, c.max_nVertices = 6;
    return c;
}
#define WITH(start, ...) [] { gf_smp_config c = start; __VA_ARGS__; return c; }()

typedef std::function<size_t(size_t *, size_t)> Table;

// the protocol of one call: count first, nothing written below count + 1, exactly count + 1 entries at or above it
static void show(const char *name, const Table &table, size_t count_expected) {
    const size_t n = table(nullptr, 0);
    CHECK(n > 0);
    const size_t guard = (size_t)0xA5A5A5A5A5A5A5A5ull;
    std::vector<size_t> buf(n + 3, guard);
    CHECK(table(buf.data() + 1, n) == n);
    for (size_t v : buf) CHECK(v == guard);
    CHECK(table(buf.data() + 1, 0) == n && table(nullptr, n + 1) == n);
    CHECK(table(buf.data() + 1, n + 1) == n);
    CHECK(buf[0] == guard && buf[n + 2] == guard && buf[1] == 0 && buf[n + 1] == count_expected);
    std::printf("%s", name);
    for (size_t b = 0; b < n; ++b) {
        CHECK(buf[b + 2] > buf[b + 1]);
        std::printf(" %zu", buf[b + 2] - buf[b + 1]);
    }
    std::printf("\n");
}

static size_t count_of(const gf_smp_config &c, int nClass) {
    gfsmp::Config out;
    char why[640];
    const gfsmp::ConfigEntry entry = {nClass ? gfsmp::ConfigEntry::Classifier : gfsmp::ConfigEntry::Handle, nClass, 0.0};
    return gfsmp::resolve_config(&c, entry, &out, why, sizeof why) == GF_OK ? gfsmp::param_count(out) : 0;
}

static void handle(const char *name, const gf_smp_config &c) {
    show(name, [&c](size_t *o, size_t cap) { return gf_smp_config_param_blocks(&c, o, cap); }, count_of(c, 0));
}

static gf_smp_model_config model(int nTowers, int nChanels, int cap, int F2, int first_order, int maxV2, int ccn, double decay) {
    gf_smp_model_config m;
    std::memset(&m, 0, sizeof m);
    m.nTowers = nTowers, m.nLevels = 2, m.nChanels = nChanels, m.max_receptive_field = cap;
    m.nFeatures[0] = 4, m.nFeatures[1] = F2;
    m.first_order = first_order, m.max_nVertices[0] = first_order ? 6 : 0, m.max_nVertices[1] = maxV2;
    m.ccn_1d = ccn, m.nChanels_decay = decay;
    return m;
}
static void composite(const char *name, const gf_smp_model_config &m) {
    gf::ModelPlan plan;
    char why[512];
    CHECK(gf::model_plan(&m, &plan, why, sizeof why));
    show(name, [&m](size_t *o, size_t cap) { return gf_smp_model_config_param_blocks(&m, o, cap); }, plan.n_params);
}

int main() {
    handle("SMP_omega", WITH(field(4), c.nContractions = 18));
    handle("SMP_theta", WITH(field(4), c.max_receptive_field = 4, c.first_order = 1, c.max_nVertices = 6));
    handle("SMP_1D_ver3", WITH(field(4), c.first_order = 4, c.max_nVertices = 6));
    handle("SMP_2D_ver5", WITH(field(4), c.steerable_2d = 5, c.max_nVertices = 6));
    handle("Unrestricted_SMP_2D", WITH(field(4), c.unrestricted = 3, c.max_nVertices = 6));
    handle("GCN_1D", WITH(vertex(5), c.neighbourhood = 2, c.max_Radius = 1));
    handle("GRU_GCN_1D", WITH(vertex(5), c.neighbourhood = 4, c.max_Radius = 1));
    handle("GCN_1D_Distance", WITH(vertex(5), c.neighbourhood = 2, c.max_Radius = 1, c.distance_channel = 1));
    handle("GCN_1D_Kernel", WITH(vertex(5), c.neighbourhood = 2, c.max_Radius = 1, c.readout = 1));
    handle("GCA_1D", WITH(vertex(5), c.neighbourhood = 2, c.max_Radius = 1, c.readout = 2));
    handle("LCNN", WITH(vertex(5), c.matrix_form = 1, c.nNeighbors = 3, c.nChanels2 = 4, c.nDense = 7));
    handle("GCN_MW", WITH(vertex(5), c.matrix_form = 2));
    handle("CGCN_1D", WITH(vertex(1), c.covariant = 1));
    const gf_smp_config ver6 = WITH(field(4), c.nContractions = 10, c.custom_matmul = 1);
    show("SMP_2D_ver6_classification", [&ver6](size_t *o, size_t cap) { return gf_smp_classifier_config_param_blocks(&ver6, 3, o, cap); }, count_of(ver6, 3));
    composite("SMP_omega_physics", model(1, 4, 6, 0, 0, 0, 0, 0.0));
    composite("SMP_omega_pairgraphs", model(2, 4, 5, 3, 0, 0, 0, 0.0));
    composite("CCN_1D", model(2, 16, 4, 3, 1, 5, 1, 0.7));

    // refusals: no blocks, nothing written
    size_t word = 7;
    const gf_smp_config bad = WITH(field(4), c.nContractions = 7);
    CHECK(gf_smp_config_param_blocks(&bad, &word, 1) == 0 && gf_smp_config_param_blocks(nullptr, &word, 1) == 0 && word == 7);
    CHECK(gf_smp_classifier_config_param_blocks(&ver6, 1, &word, 1) == 0 && gf_smp_classifier_config_param_blocks(&ver6, INT_MIN, &word, 1) == 0);
    gf_smp_model_config three = model(2, 4, 5, 3, 0, 0, 0, 0.0);
    three.nTowers = 3;
    CHECK(gf_smp_model_config_param_blocks(&three, &word, 1) == 0 && gf_smp_model_config_param_blocks(nullptr, &word, 1) == 0 && word == 7);
    // hostile fields: whatever the verdict, the table is either empty or tiles the parameter count
    const int hostile[] = {INT_MIN, -1, 0, 31, 64};   // (sizes a test can hold: the layout arithmetic of a larger accepted one is not this call's)
    int gf_smp_config::*const fields[] = {&gf_smp_config::nChanels, &gf_smp_config::nFeatures, &gf_smp_config::nDepth, &gf_smp_config::max_nVertices};
    const gf_smp_config families[] = {WITH(field(4), c.nContractions = 18), WITH(field(4), c.first_order = 4, c.max_nVertices = 6),
                                      WITH(vertex(5), c.neighbourhood = 2, c.max_Radius = 1, c.distance_channel = 1)};
    long accepted = 0;
    for (const gf_smp_config &family : families)
        for (int gf_smp_config::*f : fields)
            for (int v : hostile) {
                gf_smp_config c = family;
                c.*f = v;
                const size_t n = gf_smp_config_param_blocks(&c, nullptr, 0);
                if (!n || n > 100000) continue;
                std::vector<size_t> off(n + 1);
                CHECK(gf_smp_config_param_blocks(&c, off.data(), n + 1) == n && off[0] == 0 && off[n] == count_of(c, 0));
                ++accepted;
            }
    CHECK(accepted > 0);
    std::printf(fails ? "FAILED\n" : "PASSED\n");
    return fails ? 1 : 0;
}
