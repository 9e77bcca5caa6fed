// Stand-alone program for the sanitizers: what CGCN_1D and CGCN_2D (gf_smp_config.covariant = 1, 2) add to the host side -- the branch of
// gfsmp::resolve_config (graphflow_amd/csrc/smp_config.cpp), the block enumeration of the Config they become (smp_prep.h) and the batch
// (smp_prep.cpp: build_batch_covariant): accepted configurations, every refusal with a piece of its message, hostile structs, and batches
// with V = 1, V = max_nVertices and an isolated vertex, an asymmetric adjacency and a set diagonal entry, checked entry by entry against
// a direct evaluation.
#include <climits>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "smp_config.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static gf_smp_config base(int form, int L, int M, int F, int D) {
    gf_smp_config c;
    std::memset(&c, 0, sizeof c);
    c.nLevels = L, c.nChanels = 1, c.nFeatures = F, c.nDepth = D, c.max_nVertices = M;
    c.covariant = form;
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
    CHECK(n == expect && c.readout_block().n == 0 && c.shared_blocks().total() == 0);
    CHECK(c.top_channels() == c.max_nVertices && c.first_block().n == (size_t)c.fdim() && c.first_block().div == (size_t)c.fdim());
    std::vector<float> p(n + 1, 0.f);
    float *H, *W;
    std::vector<float *> K, b;
    gfsmp::view_params<float>(c, p.data(), &H, &K, &b, &W);
    CHECK(H == p.data() && W == p.data() + n);
    for (int l = 1; l <= c.nLevels; ++l) {
        CHECK(K[l] == p.data() + c.fdim() + (size_t)(l - 1) * c.max_nVertices * c.max_nVertices);
        CHECK(c.level_blocks(l).mat[0].div == (size_t)c.max_nVertices && c.level_blocks(l).nmat == 1);
    }
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
static Mol molecule(int V, int F, std::initializer_list<std::pair<int, int> > edges, double tint) {
    Mol m = {V, std::vector<int>((size_t)V * V, 0), std::vector<double>((size_t)V * F, 0.0)};
    for (const std::pair<int, int> &e : edges) m.adj[(size_t)e.first * V + e.second] = m.adj[(size_t)e.second * V + e.first] = 1;
    for (int v = 0; v < V; ++v) m.feat[(size_t)v * F + (v * 3) % F] = tint + 0.25 * (v % 3);
    return m;
}

// the classes' Floyd-Warshall, written out once more (CGCN_1D.h:156-176)
static std::vector<int> hops_of(const Mol &m) {
    const int V = m.V, far = 1000000000;
    std::vector<int> d((size_t)V * V, 0);
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) {
            d[(size_t)i * V + j] = i == j ? 0 : far;
            if (i != j && m.adj[(size_t)i * V + j] > 0) d[(size_t)i * V + j] = d[(size_t)j * V + i] = 1;
        }
    for (int k = 0; k < V; ++k)
        for (int i = 0; i < V; ++i)
            for (int j = 0; j < V; ++j)
                if (d[(size_t)i * V + k] + d[(size_t)k * V + j] < d[(size_t)i * V + j]) d[(size_t)i * V + j] = d[(size_t)i * V + k] + d[(size_t)k * V + j];
    return d;
}

static void check_batch(const gfsmp::Config &c, const std::vector<Mol> &mols) {
    std::vector<int> nV, adj;
    std::vector<double> feat;
    for (const Mol &m : mols) {
        nV.push_back(m.V);
        adj.insert(adj.end(), m.adj.begin(), m.adj.end());
        feat.insert(feat.end(), m.feat.begin(), m.feat.end());
    }
    gfsmp::BatchLayout B;
    gfsmp::build_batch_covariant(c, (int)mols.size(), nV.data(), adj.data(), feat.data(), &B);
    const int M = c.max_nVertices, FD = c.fdim(), F = c.nFeatures;
    CHECK(B.nMol == (int)mols.size() && B.nb_lists.size() == 1 && (int)B.level.size() == c.nLevels + 1);
    const gfsmp::BatchLayout::NeighbourList &nl = B.nb_lists[0];
    int v0 = 0;
    long long e = 0, t = 0;
    for (size_t k = 0; k < mols.size(); ++k) {
        const Mol &m = mols[k];
        const int V = m.V;
        const std::vector<int> d = hops_of(m);
        CHECK(B.mol_first_vertex[k] == v0 && B.mols[k].V == V);
        for (int v = 0; v < V; ++v) {
            CHECK(B.nb_vertex_mol[(size_t)v0 + v] == (int)k);
            CHECK(nl.ptr[(size_t)v0 + v] == e && nl.tptr[(size_t)v0 + v] == t);
            for (int u = 0; u < V; ++u) {
                if (m.adj[(size_t)u * V + v] > 0) CHECK(e < (long long)nl.idx.size() && nl.idx[(size_t)e++] == v0 + u);
                if (m.adj[(size_t)v * V + u] > 0) CHECK(t < (long long)nl.tidx.size() && nl.tidx[(size_t)t++] == v0 + u);
            }
            for (int i = 0; i < M; ++i) {
                const int want = i < V && d[(size_t)i * V + v] <= 255 ? d[(size_t)i * V + v] : 255;
                CHECK(B.cov_hop[((size_t)v0 + v) * M + i] == want);
            }
            for (int dd = 0; dd <= c.nDepth; ++dd)
                for (int f = 0; f < F; ++f) {
                    double want = 0.0;
                    for (int u = 0; u < V; ++u)
                        if (d[(size_t)u * V + v] == dd) want += m.feat[(size_t)u * F + f];
                    CHECK(B.x[((size_t)v0 + v) * FD + (size_t)dd * F + f] == (float)want);
                }
        }
        v0 += V;
    }
    CHECK(nl.ptr[(size_t)v0] == e && nl.tptr[(size_t)v0] == t && (long long)nl.idx.size() == e && (long long)nl.tidx.size() == t);
    CHECK(B.cov_hop.size() == (size_t)v0 * M && B.x.size() == (size_t)v0 * FD);
    for (int l = 0; l <= c.nLevels; ++l) CHECK(B.level[l].nNodes == v0 && B.level[l].rows == v0);
}

int main() {
    char why[640];
    gfsmp::Config c;
    using Kind = gfsmp::ConfigEntry;
    // ---- accepted ----
    for (int form = 1; form <= 2; ++form) {
        const int shapes[][4] = {{0, 1, 1, 0}, {1, 6, 4, 5}, {3, 29, 5, 2}, {64, 64, 4, 1}, {2, 75, 3, 0}};
        for (const int *s : shapes) {
            gf_smp_config g = base(form, s[0], s[1], s[2], s[3]);
            g.max_receptive_field = -5, g.has_WL_ordering = 7, g.max_Radius = -9;   // (not read)
            CHECK(resolve(g, Kind::Handle, &c, why, sizeof why) == GF_OK);
            CHECK(c.covariant == form && c.nChanels == 1 && c.max_nVertices == s[1] && c.nLevels == s[0] && !c.neighbourhood && !c.has_WL_ordering);
            check_layout(c, (size_t)s[2] * (s[3] + 1) + (size_t)s[0] * s[1] * s[1]);
        }
    }
    CHECK(gf::smp_covariant_lds_bytes(64) <= 160 * 1024 && gf::smp_covariant_lds_bytes(gf::kCovariantMaxVertices) <= 160 * 1024);
    CHECK(gf::smp_covariant_lds_bytes(gf::kCovariantMaxVertices + 1) > 160 * 1024);
    // ---- refused, with a piece of the message ----
    struct Bad {
        gf_smp_config g;
        Kind::Kind kind;
        gf_status st;
        const char *text;
    };
    std::vector<Bad> bad;
    auto with = [](gf_smp_config g, int gf_smp_config::*field, int value) {
        g.*field = value;
        return g;
    };
    const gf_smp_config ok = base(2, 2, 6, 4, 1);
    bad.push_back({with(ok, &gf_smp_config::covariant, 3), Kind::Handle, GF_ERR_INVALID, "covariant = 3"});
    bad.push_back({with(ok, &gf_smp_config::covariant, INT_MIN), Kind::Handle, GF_ERR_INVALID, "the covariant models are"});
    for (int gf_smp_config::*f : {&gf_smp_config::first_order, &gf_smp_config::steerable_2d, &gf_smp_config::unrestricted, &gf_smp_config::neighbourhood,
                                  &gf_smp_config::matrix_form, &gf_smp_config::distance_channel, &gf_smp_config::readout, &gf_smp_config::physics,
                                  &gf_smp_config::nContractions, &gf_smp_config::custom_matmul})
        for (int v : {1, -1, INT_MAX}) bad.push_back({with(ok, f, v), Kind::Handle, GF_ERR_INVALID, "every other form selector 0"});
    for (int v : {0, 2, -1, INT_MAX}) bad.push_back({with(ok, &gf_smp_config::nChanels, v), Kind::Handle, GF_ERR_INVALID, "nChanels = 1"});
    for (int v : {-1, 65, INT_MAX, INT_MIN}) bad.push_back({with(ok, &gf_smp_config::nLevels, v), Kind::Handle, GF_ERR_INVALID, "nLevels in 0 .. 64"});
    for (int v : {0, -3, INT_MIN}) bad.push_back({with(ok, &gf_smp_config::nFeatures, v), Kind::Handle, GF_ERR_INVALID, "nFeatures >= 1"});
    for (int v : {-1, INT_MIN}) bad.push_back({with(ok, &gf_smp_config::nDepth, v), Kind::Handle, GF_ERR_INVALID, "nDepth >= 0"});
    bad.push_back({with(with(ok, &gf_smp_config::nFeatures, INT_MAX), &gf_smp_config::nDepth, INT_MAX), Kind::Handle, GF_ERR_INVALID, "at most 65536"});
    for (int v : {0, -1, 76, 4096, INT_MAX, INT_MIN})
        bad.push_back({with(ok, &gf_smp_config::max_nVertices, v), Kind::Handle, GF_ERR_INVALID, "max_nVertices in 1 .. 75"});
    bad.push_back({ok, Kind::Classifier, GF_ERR_UNSUPPORTED, "CGCN_1D / CGCN_2D have no `_classification` class"});
    bad.push_back({ok, Kind::Tower, GF_ERR_UNSUPPORTED, "are no towers"});
    for (const Bad &b : bad) {
        const gf_status st = resolve(b.g, b.kind, &c, why, sizeof why);
        CHECK(st == b.st);
        if (!std::strstr(why, b.text)) {
            std::printf("FAILED message \"%s\" lacks \"%s\"\n", why, b.text);
            ++fails;
        }
    }
    // ---- hostile structs: every field at an extreme, covariant set ----
    for (int v : {INT_MIN, -1, 0, 1, INT_MAX}) {
        gf_smp_config g;
        int *w = reinterpret_cast<int *>(&g);
        for (size_t i = 0; i < sizeof g / sizeof(int); ++i) w[i] = v;
        g.covariant = 1;
        (void)resolve(g, Kind::Handle, &c, why, sizeof why);
        (void)resolve(g, Kind::Classifier, &c, why, sizeof why);
        (void)resolve(g, Kind::Tower, &c, why, sizeof why);
    }
    // ---- batches ----
    const int F = 4;
    Mol one = molecule(1, F, {}, 1.0);
    Mol full = molecule(6, F, {{0, 1}, {0, 2}, {0, 3}, {3, 4}, {3, 5}}, 0.5);             // V = max_nVertices
    Mol lone = molecule(6, F, {{0, 1}, {1, 2}, {4, 5}}, 0.75);                            // vertex 3 is isolated
    Mol asym = molecule(5, F, {{0, 1}, {0, 2}, {0, 3}, {0, 4}}, 1.5);
    asym.adj[0 * 5 + 1] = 0, asym.adj[3 * 5 + 0] = 0;
    Mol diag = molecule(4, F, {{0, 1}, {0, 2}, {0, 3}}, 2.0);
    diag.adj[1 * 4 + 1] = 1;
    for (int form = 1; form <= 2; ++form)
        for (int L : {0, 2, 4}) {
            gf_smp_config g = base(form, L, 6, F, 2);
            CHECK(resolve(g, Kind::Handle, &c, why, sizeof why) == GF_OK);
            check_batch(c, {one});
            check_batch(c, {full});
            check_batch(c, {one, full, lone, asym, diag, one});
        }
    if (fails) {
        std::printf("%d checks FAILED\n", fails);
        return 1;
    }
    std::printf("PASSED\n");
    return 0;
}
