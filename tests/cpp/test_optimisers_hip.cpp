// use_optimiser of the host drop-in classes (graphflow_amd/host: SMP_handle_hip.h's skeleton, SMP_omega_hip.h, SMP_physics_hip.h), driven by
// tests/test_optimisers_gpu.py with the runs of Part C of tests/golden/optimisers.npz: after srand(seed) the constructor, use_optimiser with
// the run's kind, the recorded number of BatchLearn(nBatch, molecule, target, learning_rate) steps.  Prints, as hexadecimal floats, the
// weights before, the pair of every step and the weights after; the test compares them with the record.
//   case <id> <class> <seed> <kind> <learning_rate> <steps> <n> <F>, then n graphs (V, adjacency, features) and n targets
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "SMP_families_hip.h"
#include "SMP_omega_hip.h"
#include "SMP_physics_hip.h"

struct Graph {   // the public fields of the reference's DenseGraph that the classes read
    int nVertices, nFeatures;
    int **adj;
    double **feature;
};

static Graph *read_graph(std::istream &in, int F) {
    Graph *g = new Graph();   // (leaked on purpose)
    in >> g->nVertices;
    g->nFeatures = F;
    g->adj = new int *[g->nVertices];
    g->feature = new double *[g->nVertices];
    for (int i = 0; i < g->nVertices; ++i) {
        g->adj[i] = new int[g->nVertices];
        for (int j = 0; j < g->nVertices; ++j) in >> g->adj[i][j];
    }
    for (int i = 0; i < g->nVertices; ++i) {
        g->feature[i] = new double[F];
        for (int f = 0; f < F; ++f) in >> g->feature[i][f];
    }
    return g;
}

static void print(const char *tag, const std::vector<float> &v) {
    std::printf("%s", tag);
    for (size_t i = 0; i < v.size(); ++i) std::printf(" %a", (double)v[i]);
    std::printf("\n");
}

template <class Net>
static void run(Net &net, int kind, double lr, int steps, std::vector<Graph *> &x, std::vector<double> &t) {
    gf_optim_config oc = {kind, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // (nBatch and the rate come with every BatchLearn; the classes' default constants)
    net.use_optimiser(oc);
    print("params0", net.parameters());
    for (int s = 0; s < steps; ++s) {
        const std::pair<double, double> r = net.BatchLearn((int)x.size(), &x[0], &t[0], lr);
        std::printf("pair %a %a\n", r.first, r.second);
    }
    print("params", net.parameters());
}

int main(int argc, char **argv) {
    if (argc < 2) return 1;
    std::ifstream in(argv[1]);
    if (!in) return 1;
    std::string word, id, cls;
    while (in >> word) {
        if (word != "case") return 4;
        int seed, kind, steps, n, F;
        double lr;
        in >> id >> cls >> seed >> kind >> lr >> steps >> n >> F;
        std::vector<Graph *> x;
        std::vector<double> t(n);
        for (int i = 0; i < n; ++i) x.push_back(read_graph(in, F));
        for (int i = 0; i < n; ++i) in >> t[i];
        std::printf("case %s\n", id.c_str());
        srand((unsigned)seed);
        if (cls == "SMP_omega") {
            SMP_omega_hip net(6, 6, 2, 4, 4, 1);
            run(net, kind, lr, steps, x, t);
        } else if (cls == "GCN_1D") {
            GCN_1D_hip net(2, 6, 4, 5, 1, 1, 0.9);
            run(net, kind, lr, steps, x, t);
        } else if (cls == "SMP_omega_physics") {
            SMP_omega_physics_hip net(6, 6, 2, 4, 4);
            run(net, kind, lr, steps, x, t);
        } else {
            return 3;
        }
        std::fflush(stdout);
    }
    std::printf("DONE\n");
    return 0;
}
