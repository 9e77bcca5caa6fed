// Stand-alone program for the sanitizers: what LCNN and GCN_MW (gf_smp_config.matrix_form = 1, 2) add to the host side -- the branch of
// gfsmp::resolve_config (graphflow_amd/csrc/smp_config.cpp), the block enumeration of the Config they become (smp_prep.h) and the host
// preparation (smp_prep.cpp: matrix_form_molecule, build_batch_matrix_form): accepted configurations, every refusal with a piece of its
// message, hostile structs, and the row lists of small batches -- padded, disconnected, one vertex, k > V, the molV == V refusal -- checked
// entry by entry against the order, the sequence and A-hat they were built from.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "smp_config.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static gf_smp_config gcn(int L, int H, int F, int D, int maxV) {
    gf_smp_config c;
    std::memset(&c, 0, sizeof c);
    c.nLevels = L, c.nChanels = H, c.nFeatures = F, c.nDepth = D, c.max_receptive_field = c.max_nVertices = maxV;
    c.matrix_form = 2;
    return c;
}
static gf_smp_config lcnn(int V, int F, int k, int D, int C1, int C2, int nD) {
    gf_smp_config c = gcn(2, C1, F, D, V);
    c.matrix_form = 1, c.nNeighbors = k, c.nChanels2 = C2, c.nDense = nD;
    return c;
}

static gf_status resolve(const gf_smp_config &c, gfsmp::ConfigEntry::Kind kind, gfsmp::Config *out, char *why, size_t nwhy) {
    const gfsmp::ConfigEntry entry = {kind, kind == gfsmp::ConfigEntry::Classifier ? 3 : 0, 0.0};
    why[0] = 0;
    return gfsmp::resolve_config(&c, entry, out, why, nwhy);
}

// the blocks add up to param_count, the views tile the vector, the draws end where param_count says
static void check_layout(const gfsmp::Config &c, size_t expect) {
    const size_t n = gfsmp::param_count(c);
    CHECK(n == expect);
    std::vector<float> p(n + 1, 0.f);
    float *H, *W;
    std::vector<float *> K, b;
    gfsmp::view_params<float>(c, p.data(), &H, &K, &b, &W);
    CHECK(H == p.data() && W + c.readout_block().n == p.data() + n);
    float *q = p.data();
    gfsmp::uniform_draw(c.first_block(), &q);
    for (int l = 1; l <= c.nLevels; ++l) c.level_blocks(l).each_draw([&q](const gfsmp::Config::Block &blk) { gfsmp::uniform_draw(blk, &q); });
    gfsmp::uniform_draw(c.readout_block(), &q);
    CHECK(q == p.data() + n && p[n] == 0.f);
}

struct Mol {
    int V;
    std::vector<int> adj;
    std::vector<double> feat;
};
static Mol molecule(int V, int F, std::initializer_list<std::pair<int, int> > edges, bool one_way = false) {
    Mol m = {V, std::vector<int>((size_t)V * V, 0), std::vector<double>((size_t)V * F, 0.0)};
    for (const std::pair<int, int> &e : edges) {
        m.adj[(size_t)e.first * V + e.second] = 1;
        if (!one_way) m.adj[(size_t)e.second * V + e.first] = 1;
    }
    for (int v = 0; v < V; ++v) m.feat[(size_t)v * F + (v * 3) % F] = 1.0 + 0.25 * (v % 3);
    return m;
}

static void check_batch(const gfsmp::Config &c, const std::vector<Mol> &mols, int expect_bad) {
    std::vector<int> nV, adj;
    std::vector<double> feat;
    for (const Mol &m : mols) {
        nV.push_back(m.V);
        adj.insert(adj.end(), m.adj.begin(), m.adj.end());
        feat.insert(feat.end(), m.feat.begin(), m.feat.end());
    }
    gfsmp::BatchLayout B;
    const int bad = gfsmp::build_batch_matrix_form(c, (int)mols.size(), nV.data(), adj.data(), feat.data(), &B);
    CHECK(bad == expect_bad);
    if (bad >= 0) return;
    const gfsmp::BatchLayout::RowLists &rl = B.rl;
    const int rows = B.mol_first_vertex[mols.size()];
    CHECK((int)rl.ptr.size() == rows + 1 && (int)rl.tptr.size() == rows + 1 && rl.ptr[0] == 0 && rl.tptr[0] == 0);
    CHECK(rl.ptr[rows] == rl.tptr[rows] && (size_t)rl.ptr[rows] == rl.src.size() && rl.src.size() == rl.tsrc.size());
    CHECK(B.x.size() == (size_t)rows * c.fdim() && (int)B.level.size() == c.nLevels + 1 && B.level[0].rows == rows);
    // the transposed list holds every entry of the forward list once, and a row's slots never decrease
    size_t matched = 0;
    for (int r = 0; r < rows; ++r) {
        for (int64_t e = rl.ptr[r]; e < rl.ptr[r + 1]; ++e) {
            CHECK(rl.src[e] >= 0 && rl.src[e] < rows && rl.slot[e] >= 0 && rl.slot[e] < (c.matrix_form == 1 ? c.nNeighbors : 1));
            CHECK(e == rl.ptr[r] || rl.slot[e] >= rl.slot[e - 1]);
            const int u = rl.src[e];
            for (int64_t t = rl.tptr[u]; t < rl.tptr[u + 1]; ++t)
                if (rl.tsrc[t] == r && rl.tslot[t] == rl.slot[e] && rl.tcoef[t] == rl.coef[e]) {
                    ++matched;
                    break;
                }
        }
        for (int64_t t = rl.tptr[r]; t < rl.tptr[r + 1]; ++t) CHECK(t == rl.tptr[r] || rl.tslot[t] >= rl.tslot[t - 1]);
    }
    CHECK(matched == rl.src.size());
    if (c.matrix_form == 1) {   // the per-(row, slot) offsets: every entry between sptr[r k + s] and the next has row r's slot s
        const int k = c.nNeighbors;
        CHECK(rl.sptr.size() == (size_t)rows * k + 1 && rl.tsptr.size() == rl.sptr.size() && rl.sptr[0] == 0 && rl.tsptr[0] == 0);
        for (int r = 0; r < rows; ++r)
            for (int s = 0; s < k; ++s) {
                CHECK(rl.sptr[(size_t)r * k + s] == rl.ptr[r] + s && rl.sptr[(size_t)r * k + s + 1] == rl.ptr[r] + s + 1);
                const int64_t t0 = rl.tsptr[(size_t)r * k + s], t1 = rl.tsptr[(size_t)r * k + s + 1];
                CHECK(t0 >= rl.tptr[r] && t0 <= t1 && t1 <= rl.tptr[r + 1]);
                for (int64_t t = t0; t < t1; ++t) CHECK(rl.tslot[t] == s);
            }
        CHECK(rl.tsptr[(size_t)rows * k] == rl.tptr[rows]);
    } else {
        CHECK(rl.sptr.empty() && rl.tsptr.empty());
    }
    for (size_t m = 0; m < mols.size(); ++m) {
        gfsmp::MatrixFormMolecule M;
        gfsmp::matrix_form_molecule(c, mols[m].V, mols[m].adj.data(), mols[m].feat.data(), &M);
        const int r0 = B.mol_first_vertex[m];
        if (c.matrix_form == 1) {
            const int V = c.max_nVertices, k = c.nNeighbors;
            CHECK((int)M.order.size() == V && (int)M.seq.size() == V * k && B.mol_first_vertex[m + 1] - r0 == V);
            for (int i = 0; i < V; ++i)
                for (int j = 0; j < k; ++j) {
                    const int64_t e = rl.ptr[r0 + i] + j;
                    CHECK(rl.src[e] == r0 + M.seq[(size_t)i * k + j] && rl.slot[e] == j && rl.coef[e] == 1.f);
                    CHECK(M.seq[(size_t)i * k + j] <= mols[m].V && B.rl.seq[((size_t)m * V + i) * k + j] == M.seq[(size_t)i * k + j]);
                }
            for (int v = mols[m].V; v < V; ++v)   // a dummy's row of x is zero
                for (int f = 0; f < c.fdim(); ++f) CHECK(B.x[(size_t)(r0 + v) * c.fdim() + f] == 0.f);
        } else {
            const int V = mols[m].V;
            for (int i = 0; i < V; ++i) {
                int64_t e = rl.ptr[r0 + i];
                double sum = 0.0;
                for (int j = 0; j < V; ++j) {
                    const double a = M.norm_adj[(size_t)i * V + j];
                    sum += a;
                    if (a == 0.0) continue;
                    CHECK(rl.src[e] == r0 + j && rl.coef[e] == (float)a);
                    ++e;
                }
                CHECK(e == rl.ptr[r0 + i + 1] && std::isfinite(sum));
            }
        }
    }
}

int main() {
    char why[640];
    gfsmp::Config out;
    // accepted: GCN_MW at 0, 1, 3 and 64 levels, LCNN at the reference's demo setting, k > V and the widest operands
    for (int L : {0, 1, 3, 64})
        for (int H : {1, 20, 80}) {
            CHECK(resolve(gcn(L, H, 4, 1, 6), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK && !why[0]);
            CHECK(out.matrix_form == 2 && out.top_channels() == H && !out.neighbourhood && !out.gated());
            check_layout(out, (size_t)8 * H + (size_t)L * H * H + H);
        }
    CHECK(resolve(lcnn(6, 4, 5, 3, 16, 8, 128), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK && !why[0]);
    CHECK(out.matrix_form == 1 && out.top_channels() == 128 && out.nNeighbors == 5);
    check_layout(out, 5 * 16 * 16 + 16 + 5 * 16 * 8 + 8 + 128 * 6 * 8 + 128);
    CHECK(resolve(lcnn(4, 4, 6, 2, 5, 10, 9), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    CHECK(resolve(lcnn(16, 4, 1, 0, 65536, 4096, 1), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    // unsupported entries
    for (const gf_smp_config &c : {gcn(1, 20, 4, 1, 6), lcnn(6, 4, 5, 3, 16, 8, 128)}) {
        CHECK(resolve(c, gfsmp::ConfigEntry::Classifier, &out, why, sizeof why) == GF_ERR_UNSUPPORTED && std::strstr(why, "LCNN / GCN_MW have no"));
        CHECK(resolve(c, gfsmp::ConfigEntry::Tower, &out, why, sizeof why) == GF_ERR_UNSUPPORTED && std::strstr(why, "are no towers"));
    }
    // refused, with a piece of the message
    struct Bad {
        gf_smp_config c;
        const char *text;
    };
    std::vector<Bad> bad;
    for (int f = 1; f <= 2; ++f) {
        const gf_smp_config base = f == 1 ? lcnn(6, 4, 5, 3, 16, 8, 128) : gcn(1, 20, 4, 1, 6);
        gf_smp_config c = base;
        c.first_order = 1, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.steerable_2d = 1, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.unrestricted = 1, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.neighbourhood = 2, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.physics = 1, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.custom_matmul = 1, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.nContractions = 18, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.max_receptive_field = 5, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.max_nVertices = c.max_receptive_field = 4097, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.nChanels = 0, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.nChanels = INT_MIN, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.nDepth = -1, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.nLevels = f == 1 ? 3 : 65, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.nLevels = -1, bad.push_back({c, "GCN_MW) needs"});
        c = base, c.nChanels = 65537, bad.push_back({c, "at most 65536"});
        c = base, c.nChanels = INT_MAX, bad.push_back({c, "at most 65536"});
        c = base, c.nFeatures = INT_MAX, c.nDepth = INT_MAX, bad.push_back({c, "at most 65536"});
    }
    gf_smp_config c = lcnn(6, 4, 0, 3, 16, 8, 128);
    bad.push_back({c, "GCN_MW) needs"});
    c = lcnn(6, 4, 5, 3, 16, 0, 128), bad.push_back({c, "GCN_MW) needs"});
    c = lcnn(6, 4, 5, 3, 16, 8, INT_MIN), bad.push_back({c, "GCN_MW) needs"});
    c = lcnn(6, 4, INT_MAX, 3, 16, 8, 128), bad.push_back({c, "at most 65536"});
    c = lcnn(6, 4, 5, 3, 16, INT_MAX, 128), bad.push_back({c, "at most 65536"});
    c = lcnn(4096, 4, 5, 3, 16, 17, 128), bad.push_back({c, "at most 65536"});
    c = lcnn(4096, 4, 5, 3, 16, 16, 65536), bad.push_back({c, "must fit an int"});
    c = gcn(1, 20, 4, 1, 6), c.matrix_form = 3, bad.push_back({c, "GCN_MW) needs"});
    c = gcn(1, 20, 4, 1, 6), c.matrix_form = -1, bad.push_back({c, "GCN_MW) needs"});
    for (const Bad &b : bad) {
        CHECK(resolve(b.c, gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_ERR_INVALID);
        if (!std::strstr(why, b.text)) std::printf("FAILED: \"%s\" lacks \"%s\"\n", why, b.text), ++fails;
    }
    // the host preparation
    const int F = 4;
    const Mol path3 = molecule(3, F, {{0, 1}, {1, 2}}), one = molecule(1, F, {}), ring6 = molecule(6, F, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 0}});
    const Mol split6 = molecule(6, F, {{0, 1}, {1, 2}, {3, 4}, {4, 5}, {3, 5}}), oneway = molecule(5, F, {{0, 1}, {0, 2}, {3, 0}, {4, 0}}, true);
    CHECK(resolve(gcn(2, 8, F, 1, 6), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    check_batch(out, {path3, one, ring6, split6, oneway}, -1);
    std::vector<Mol> many;
    for (int i = 0; i < 70; ++i) many.push_back(i % 3 == 0 ? ring6 : i % 3 == 1 ? one : split6);   // (enough molecules for the worker threads)
    check_batch(out, many, -1);
    CHECK(resolve(lcnn(6, F, 5, 3, 16, 8, 128), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    check_batch(out, {path3, one, ring6, oneway}, -1);
    check_batch(out, {path3, split6, one}, 1);    // a full-size molecule whose fragments hold three vertices each: pads with row 6
    check_batch(out, many, 2);                    // ... the first such molecule is named
    CHECK(resolve(lcnn(8, F, 5, 0, 10, 80, 3), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    check_batch(out, {split6, path3, one, ring6}, -1);   // below full size: real rows with pad entries
    check_batch(out, many, -1);
    CHECK(resolve(lcnn(4, F, 6, 2, 5, 10, 9), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    check_batch(out, {path3, one}, -1);   // k > V
    std::printf(fails ? "%d checks FAILED\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
