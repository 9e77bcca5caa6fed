// Stand-alone program for the sanitizers: what GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel and GCA_1D (gf_smp_config.readout = 1, 2) add to
// the host side -- the branch of gfsmp::resolve_config (graphflow_amd/csrc/smp_config.cpp), the block enumeration of the Config they become
// (smp_prep.h) and the pair batch (smp_prep.cpp: interleave_pairs, then build_batch_neighbourhood unchanged): accepted configurations,
// every refusal with a piece of its message, hostile structs, and pair batches -- different sizes, one vertex, disconnected -- checked
// entry by entry against a direct evaluation.
#include <climits>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "smp_config.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

static gf_smp_config base(int form, int readout, int L, int H, int F, int D, int maxV, int R) {
    gf_smp_config c;
    std::memset(&c, 0, sizeof c);
    c.nLevels = L, c.nChanels = H, c.nFeatures = F, c.nDepth = D, c.max_receptive_field = c.max_nVertices = maxV;
    c.neighbourhood = form, c.max_Radius = R, c.readout = readout;
    return c;
}

static gf_status resolve(const gf_smp_config &c, gfsmp::ConfigEntry::Kind kind, gfsmp::Config *out, char *why, size_t nwhy) {
    const gfsmp::ConfigEntry entry = {kind, kind == gfsmp::ConfigEntry::Classifier ? 3 : 0, 0.0};
    why[0] = 0;
    return gfsmp::resolve_config(&c, entry, out, why, nwhy);
}

// the blocks add up to param_count, the views tile the vector, the draws end where param_count says
static void check_layout(const gfsmp::Config &c, size_t expect, size_t readout) {
    const size_t n = gfsmp::param_count(c);
    CHECK(n == expect && c.readout_block().n == readout);
    std::vector<float> p(n + 1, 0.f);
    float *H, *W;
    std::vector<float *> K, b;
    gfsmp::view_params<float>(c, p.data(), &H, &K, &b, &W);
    CHECK(H == p.data() && W + readout == p.data() + n);
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

// hop distances of one graph, directly (breadth first from every vertex)
static std::vector<int> hops_of(const Mol &m) {
    const int V = m.V, far = 1 << 20;
    std::vector<int> d((size_t)V * V, far);
    for (int s = 0; s < V; ++s) {
        std::vector<int> queue(1, s);
        d[(size_t)s * V + s] = 0;
        for (size_t at = 0; at < queue.size(); ++at) {
            const int u = queue[at];
            for (int w = 0; w < V; ++w)
                if ((m.adj[(size_t)u * V + w] > 0 || m.adj[(size_t)w * V + u] > 0) && d[(size_t)s * V + w] == far) {
                    d[(size_t)s * V + w] = d[(size_t)s * V + u] + 1;
                    queue.push_back(w);
                }
        }
    }
    return d;
}

// a batch of pairs through interleave_pairs and build_batch_neighbourhood: graph 2 p is X_p, 2 p + 1 is Y_p, every list entry by entry
static void check_pairs(const gfsmp::Config &c, const std::vector<Mol> &xs, const std::vector<Mol> &ys) {
    const int nPairs = (int)xs.size(), F = c.nFeatures;
    std::vector<int> nv[2], adj[2];
    std::vector<double> feat[2];
    for (int side = 0; side < 2; ++side)
        for (const Mol &m : side ? ys : xs) {
            nv[side].push_back(m.V);
            adj[side].insert(adj[side].end(), m.adj.begin(), m.adj.end());
            feat[side].insert(feat[side].end(), m.feat.begin(), m.feat.end());
        }
    gfsmp::PairBatch pb;
    gfsmp::interleave_pairs(F, nPairs, nv[0].data(), adj[0].data(), feat[0].data(), nv[1].data(), adj[1].data(), feat[1].data(), &pb);
    CHECK((int)pb.nVertices.size() == 2 * nPairs);
    size_t a = 0, f = 0;
    for (int g = 0; g < 2 * nPairs; ++g) {   // plain copies, in the order X_0, Y_0, X_1, ..
        const Mol &m = g & 1 ? ys[(size_t)(g >> 1)] : xs[(size_t)(g >> 1)];
        CHECK(pb.nVertices[(size_t)g] == m.V);
        for (size_t i = 0; i < m.adj.size(); ++i) CHECK(pb.adj[a + i] == m.adj[i]);
        for (size_t i = 0; i < m.feat.size(); ++i) CHECK(pb.feature[f + i] == m.feat[i]);
        a += m.adj.size(), f += m.feat.size();
    }
    CHECK(a == pb.adj.size() && f == pb.feature.size());
    gfsmp::BatchLayout B;
    gfsmp::build_batch_neighbourhood(c, 2 * nPairs, pb.nVertices.data(), pb.adj.data(), pb.feature.data(), &B);
    CHECK(B.nMol == 2 * nPairs && (int)B.mol_first_vertex.size() == 2 * nPairs + 1);
    const int total = B.mol_first_vertex[(size_t)2 * nPairs];
    CHECK((int)B.nb_vertex_mol.size() == total && B.x.size() == (size_t)total * c.fdim());
    for (int g = 0; g < 2 * nPairs; ++g) {
        const Mol &m = g & 1 ? ys[(size_t)(g >> 1)] : xs[(size_t)(g >> 1)];
        const int v0 = B.mol_first_vertex[(size_t)g], V = m.V;
        CHECK(B.mol_first_vertex[(size_t)g + 1] - v0 == V);
        const std::vector<int> d = hops_of(m);
        for (int v = 0; v < V; ++v) {
            CHECK(B.nb_vertex_mol[(size_t)v0 + v] == g);   // pair = g >> 1, side = g & 1
            for (int k = 0; k <= c.nDepth; ++k)            // the shell sums, directly
                for (int col = 0; col < F; ++col) {
                    double sum = 0.0;
                    for (int u = 0; u < V; ++u)
                        if (d[(size_t)u * V + v] == k) sum += m.feat[(size_t)u * F + col];
                    CHECK(B.x[((size_t)v0 + v) * c.fdim() + (size_t)k * F + col] == (float)sum);
                }
            for (int l = 1; l <= c.nLevels; ++l) {         // N_l(v) = {u: dist <= min(l, max_Radius)} in ALL forms of a pair model
                const gfsmp::BatchLayout::NeighbourList &nl = B.nb_lists[(size_t)B.nb_list_of_level[(size_t)l]];
                const int r = l < c.max_Radius ? l : c.max_Radius;
                CHECK(c.nb_radius(l) == r);
                int64_t e = nl.ptr[(size_t)v0 + v], t = nl.tptr[(size_t)v0 + v];
                for (int u = 0; u < V; ++u) {
                    if (d[(size_t)v * V + u] <= r) CHECK(e < nl.ptr[(size_t)v0 + v + 1] && nl.idx[(size_t)e++] == v0 + u);
                    if (d[(size_t)u * V + v] <= r) CHECK(t < nl.tptr[(size_t)v0 + v + 1] && nl.tidx[(size_t)t++] == v0 + u);
                }
                CHECK(e == nl.ptr[(size_t)v0 + v + 1] && t == nl.tptr[(size_t)v0 + v + 1]);   // nothing of another graph
            }
        }
    }
}

int main() {
    char why[640];
    gfsmp::Config out;
    // accepted: the three pair classes and GCA_1D, at 0 and 3 levels and several widths
    for (int form : {2, 3, 6})
        for (int L : {0, 1, 3})
            for (int H : {1, 20, 64}) {
                CHECK(resolve(base(form, 1, L, H, 4, 1, 9, 2), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK && !why[0]);
                CHECK(out.readout == 1 && out.neighbourhood == form && out.top_channels() == 2 * H && out.max_Radius == 2 && !out.distance_channel);
                CHECK(out.nb_radius(3) == 2 && out.nb_radius(1) == 1);   // (form 3 reads max_Radius here)
                check_layout(out, (size_t)8 * H + (size_t)L * (8 * H + (size_t)H * H) + 2 * H, (size_t)2 * H);
            }
    for (int L : {0, 2})
        for (int H : {1, 33, 128}) {
            CHECK(resolve(base(2, 2, L, H, 4, 1, 9, 1), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK && !why[0]);
            CHECK(out.readout == 2 && out.neighbourhood == 2 && out.top_channels() == 0);
            check_layout(out, (size_t)8 * H + (size_t)L * (8 * H + (size_t)H * H), 0);
        }
    CHECK(resolve(base(2, 2, 2, 64, 4, 0, 172, 1), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);   // the Gram kernel's LDS bound, reached
    CHECK(gf::smp_gram_lds_bytes(172, 64) <= 160 * 1024 && gf::smp_gram_lds_bytes(173, 64) > 160 * 1024);
    CHECK(gf::smp_gram_lds_bytes(147, 128) <= 160 * 1024 && gf::smp_gram_lds_bytes(148, 128) > 160 * 1024);
    CHECK(gf::smp_gram_lds_bytes(199, 5) <= 160 * 1024 && gf::smp_gram_lds_bytes(200, 5) > 160 * 1024);
    // a zero tail: the plain forms, unchanged (form 3 alone ignores max_Radius)
    CHECK(resolve(base(3, 0, 3, 8, 4, 1, 9, 1), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK && out.readout == 0);
    CHECK(out.nb_radius(3) == 3 && out.top_channels() == 8);
    check_layout(out, (size_t)8 * 8 + 3 * (8 * 8 + 8 * 8) + 8, 8);
    // unsupported entries
    for (const gf_smp_config &c : {base(2, 1, 2, 8, 4, 1, 9, 1), base(6, 1, 2, 8, 4, 1, 9, 1), base(2, 2, 2, 8, 4, 1, 9, 1)}) {
        CHECK(resolve(c, gfsmp::ConfigEntry::Classifier, &out, why, sizeof why) == GF_ERR_UNSUPPORTED && std::strstr(why, "have no `_classification` class"));
        CHECK(resolve(c, gfsmp::ConfigEntry::Tower, &out, why, sizeof why) == GF_ERR_UNSUPPORTED && std::strstr(why, "are no towers"));
    }
    // refused, with a piece of the message
    struct Bad {
        gf_smp_config c;
        const char *text;
    };
    std::vector<Bad> bad;
    for (int k = 0; k < 4; ++k) {
        const gf_smp_config b0 = k < 3 ? base(k == 0 ? 2 : k == 1 ? 3 : 6, 1, 2, 8, 4, 1, 9, 1) : base(2, 2, 2, 8, 4, 1, 9, 1);
        gf_smp_config c = b0;
        c.first_order = 1, bad.push_back({c, "needs first_order"});
        c = b0, c.steerable_2d = 1, bad.push_back({c, "needs first_order"});
        c = b0, c.unrestricted = 1, bad.push_back({c, "needs first_order"});
        c = b0, c.physics = 1, bad.push_back({c, "needs first_order"});
        c = b0, c.custom_matmul = 1, bad.push_back({c, "needs first_order"});
        c = b0, c.nContractions = 18, bad.push_back({c, "needs first_order"});
        c = b0, c.max_receptive_field = 5, bad.push_back({c, "needs first_order"});
        c = b0, c.max_nVertices = c.max_receptive_field = 4097, bad.push_back({c, "needs first_order"});
        c = b0, c.max_Radius = -1, bad.push_back({c, "max_Radius (-1) >= 0"});
        c = b0, c.max_Radius = INT_MIN, bad.push_back({c, "needs first_order"});
        c = b0, c.nChanels = 0, bad.push_back({c, "needs first_order"});
        c = b0, c.nChanels = INT_MIN, bad.push_back({c, "needs first_order"});
        c = b0, c.nChanels = INT_MAX, bad.push_back({c, k == 2 ? "at most 64" : "needs first_order"});
        c = b0, c.nFeatures = INT_MAX, c.nDepth = INT_MAX, bad.push_back({c, "needs first_order"});
        c = b0, c.nDepth = -1, bad.push_back({c, "needs first_order"});
        c = b0, c.nLevels = -1, bad.push_back({c, "needs first_order"});
        c = b0, c.nLevels = 65, bad.push_back({c, "needs first_order"});
        c = b0, c.distance_channel = 1, bad.push_back({c, "the read-outs are"});
        c = b0, c.matrix_form = 2, bad.push_back({c, "the read-outs are"});
        c = b0, c.readout = 3, bad.push_back({c, "the read-outs are"});
        c = b0, c.readout = -1, bad.push_back({c, "the read-outs are"});
        c = b0, c.readout = INT_MAX, bad.push_back({c, "the read-outs are"});
        c = b0, c.readout = INT_MIN, bad.push_back({c, "the read-outs are"});
        for (int form : {0, 1, 4, 5, 7, 8, -2, INT_MAX}) c = b0, c.neighbourhood = form, bad.push_back({c, "the read-outs are"});
    }
    gf_smp_config c = base(3, 2, 2, 8, 4, 1, 9, 1);   // the Gram read-out sits on form 2 alone
    bad.push_back({c, "the read-outs are"});
    c = base(6, 2, 2, 8, 4, 1, 9, 1), bad.push_back({c, "the read-outs are"});
    c = base(6, 1, 2, 65, 4, 1, 9, 1), bad.push_back({c, "at most 64 channels"});
    c = base(6, 1, 2, 64, 4, 0, 475, 1), bad.push_back({c, "at most 474 vertices"});
    c = base(2, 2, 2, 64, 4, 0, 173, 1), bad.push_back({c, "against 160 KiB"});
    c = base(2, 2, 2, 128, 4, 0, 148, 1), bad.push_back({c, "against 160 KiB"});
    c = base(2, 2, 2, 5, 4, 0, 4096, 1), bad.push_back({c, "against 160 KiB"});
    for (const Bad &b : bad) {
        CHECK(resolve(b.c, gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_ERR_INVALID);
        if (!std::strstr(why, b.text)) std::printf("FAILED: \"%s\" lacks \"%s\"\n", why, b.text), ++fails;
    }
    // the pair batch
    const int F = 4;
    const Mol path3 = molecule(3, F, {{0, 1}, {1, 2}}, 1.0), one = molecule(1, F, {}, 0.5);
    const Mol ring6 = molecule(6, F, {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {5, 0}}, 2.0);
    const Mol split6 = molecule(6, F, {{0, 1}, {1, 2}, {3, 4}, {4, 5}, {3, 5}}, 1.5), lone5 = molecule(5, F, {{0, 1}, {1, 2}, {3, 4}}, 0.75);
    for (int form : {2, 3, 6})
        for (int R : {0, 1, 2}) {
            CHECK(resolve(base(form, 1, 3, 8, F, 2, 6, R), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
            check_pairs(out, {path3, one, ring6, split6, one}, {one, ring6, ring6, lone5, one});
        }
    CHECK(resolve(base(2, 1, 0, 8, F, 0, 6, 1), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    check_pairs(out, {one}, {path3});
    std::vector<Mol> xs, ys;
    for (int i = 0; i < 70; ++i) {   // (enough graphs for the worker threads)
        xs.push_back(i % 3 == 0 ? ring6 : i % 3 == 1 ? one : split6);
        ys.push_back(i % 4 == 0 ? path3 : i % 4 == 1 ? lone5 : i % 4 == 2 ? one : ring6);
    }
    CHECK(resolve(base(3, 1, 3, 8, F, 1, 6, 1), gfsmp::ConfigEntry::Handle, &out, why, sizeof why) == GF_OK);
    check_pairs(out, xs, ys);
    std::printf(fails ? "%d checks FAILED\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
