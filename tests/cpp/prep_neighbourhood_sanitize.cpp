// Stand-alone program for the sanitizers: gfsmp::build_batch_neighbourhood (graphflow_amd/csrc/smp_prep.cpp) on batches of random molecules
// -- one vertex, isolated vertices, directed adjacencies -- for the three forms, with the invariants of its tables checked on the way:
// lists ascending and inside the molecule, form 1 without self loops, the transpose holding exactly the reversed pairs.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "smp_prep.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

int main() {
    std::srand(11);
    for (int form = 1; form <= 3; ++form)
        for (int L = 0; L <= 3; ++L) {
            gfsmp::Config cfg = {L, 6, 3, form == 1 ? 0 : 2, 9, 0};
            cfg.nContractions = 0;
            cfg.max_nVertices = 9;
            cfg.neighbourhood = form;
            cfg.max_Radius = form == 2 ? L / 2 : 0;
            const int nMol = 37;
            std::vector<int> nV(nMol), adj;
            std::vector<double> feat;
            for (int m = 0; m < nMol; ++m) {
                const int V = 1 + std::rand() % 9;
                nV[m] = V;
                for (int i = 0; i < V; ++i)
                    for (int j = 0; j < V; ++j) adj.push_back(i != j && std::rand() % 4 == 0);   // (directed on purpose)
                for (int i = 0; i < V * 3; ++i) feat.push_back((std::rand() % 8) / 8.0);
            }
            gfsmp::BatchLayout B;
            for (int rep = 0; rep < 2; ++rep) gfsmp::build_batch_neighbourhood(cfg, nMol, &nV[0], &adj[0], &feat[0], &B);   // (twice: reused vectors)
            const int total = B.mol_first_vertex[nMol];
            CHECK((int)B.x.size() == total * cfg.fdim());
            CHECK((int)B.nb_list_of_level.size() == L + 1);
            for (int l = 1; l <= L; ++l) CHECK(B.nb_list_of_level[l] >= 0 && B.nb_list_of_level[l] < (int)B.nb_lists.size());
            if (form == 1) CHECK(B.nb_lists.size() == (L ? 1u : 0u));
            for (const gfsmp::BatchLayout::NeighbourList &nl : B.nb_lists) {
                CHECK((int)nl.ptr.size() == total + 1 && (int)nl.tptr.size() == total + 1);
                CHECK(nl.ptr[total] == (int64_t)nl.idx.size() && nl.tptr[total] == (int64_t)nl.tidx.size() && nl.idx.size() == nl.tidx.size());
                std::set<std::pair<int, int> > fwd, rev;
                for (int g = 0; g < total; ++g) {
                    const int m = B.nb_vertex_mol[g], lo = B.mol_first_vertex[m], hi = B.mol_first_vertex[m + 1];
                    for (int64_t e = nl.ptr[g]; e < nl.ptr[g + 1]; ++e) {
                        CHECK(nl.idx[e] >= lo && nl.idx[e] < hi);
                        CHECK(e == nl.ptr[g] || nl.idx[e - 1] < nl.idx[e]);
                        CHECK(form != 1 || nl.idx[e] != g);
                        fwd.insert(std::make_pair(g, nl.idx[e]));
                    }
                    for (int64_t e = nl.tptr[g]; e < nl.tptr[g + 1]; ++e) {
                        CHECK(nl.tidx[e] >= lo && nl.tidx[e] < hi);
                        CHECK(e == nl.tptr[g] || nl.tidx[e - 1] < nl.tidx[e]);
                        rev.insert(std::make_pair(nl.tidx[e], g));
                    }
                }
                CHECK(fwd == rev);
            }
        }
    std::printf(fails ? "FAILED\n" : "PASSED\n");
    return fails ? 1 : 0;
}
