// test_family_dropins_hip.cpp -- driver for the drop-in classes of graphflow_amd/host/SMP_families_hip.h (and the iterative methods of the
// older SMP_omega_hip, SMP_2D_ver6_classification_hip, SMP_omega_physics_hip): tests/test_family_dropins_host.py writes the cases -- class,
// constructor arguments, seed, molecules, targets, what to do -- into a text file and compares what this program prints with the goldens
// and with the Python wrappers.  Nothing is judged here; a number is printed as a hexadecimal float, so no digit is lost on the way.
//
//   test_family_dropins_hip <cases> <directory for checkpoints>
//   case <id> <class> <n> <n constructor integers> <momentum_param> <seed>
//   batch <samples> <nFeatures> <second graph per sample: 0 | 1> <distance matrices: 0 | 1>    then per graph: V, adj [V][V], feature [V][F] (, distance [V][V])
//   targets <count> <values>                                                                  (count 0: the class takes none)
//   steps <nSteps> <learning_rate>                         srand(seed), construct, nSteps x BatchLearn, save_model, a second object after
//                                                          srand(99) + load_model; prints params0, pair per step, params, predict of both
//   init                                                   srand(seed), construct; prints params0
//   checkpoint <count> <weights>                           construct, set_parameters(weights), save_model to <id>.txt; a second object
//                                                          load_model's <id>_reference.txt (written by the test: the real class's own
//                                                          file); prints its parameters as `loaded`
//   fit <kind> <nIterations> <learning_rate> <epsilon>     srand(seed), construct, the iterative BatchLearn (kind 0) or Learn on the first
//                                                          sample (kind 1); prints params0, pair, decisions, rate, params
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "SMP_classification_hip.h"
#include "SMP_families_hip.h"
#include "SMP_omega_hip.h"
#include "SMP_physics_hip.h"

struct Molecule {  // public fields of GraphFlow/DenseGraph.h
    int nVertices, nFeatures;
    int **adj;
    double **feature, **distance;
    Molecule(int V, int F) : nVertices(V), nFeatures(F) {
        adj = new int *[V];
        feature = new double *[V];
        distance = new double *[V];
        for (int i = 0; i < V; ++i) {
            adj[i] = new int[V]();
            feature[i] = new double[F]();
            distance[i] = new double[V]();
        }
    }
};

struct Case {
    std::string id, cls, ckpt;
    std::vector<int> c;
    double momentum;
    int seed, n;
    std::vector<Molecule *> x, y;
    std::vector<double> t;
};

static Molecule *read_graph(std::istream &in, int F, bool dist) {
    int V;
    in >> V;
    Molecule *g = new Molecule(V, F);
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) in >> g->adj[i][j];
    for (int i = 0; i < V; ++i)
        for (int f = 0; f < F; ++f) in >> g->feature[i][f];
    if (dist)
        for (int i = 0; i < V; ++i)
            for (int j = 0; j < V; ++j) in >> g->distance[i][j];
    return g;
}

static void print(const char *what, const std::vector<float> &v) {
    std::printf("%s", what);
    for (size_t i = 0; i < v.size(); ++i) std::printf(" %a", (double)v[i]);
    std::printf("\n");
}

// the three shapes of the public methods
struct Single {
    template <class Net> static std::pair<double, double> step(Net &n, Case &k, double lr) { return n.BatchLearn(k.n, &k.x[0], &k.t[0], lr); }
    template <class Net> static std::pair<double, double> fit(Net &n, Case &k, int kind, int it, double lr, double eps) {
        return kind == 0 ? n.BatchLearn(k.n, &k.x[0], &k.t[0], it, lr, eps) : n.Learn(k.x[0], k.t[0], it, lr, eps);
    }
    template <class Net> static void predict(Net &n, Case &k, int i) { std::printf(" %a", n.Predict(k.x[i])); }
};
struct Pairs {
    template <class Net> static std::pair<double, double> step(Net &n, Case &k, double lr) { return n.BatchLearn(k.n, &k.x[0], &k.y[0], &k.t[0], lr); }
    template <class Net> static std::pair<double, double> fit(Net &n, Case &k, int kind, int it, double lr, double eps) {
        return kind == 0 ? n.BatchLearn(k.n, &k.x[0], &k.y[0], &k.t[0], it, lr, eps) : n.Learn(k.x[0], k.y[0], k.t[0], it, lr, eps);
    }
    template <class Net> static void predict(Net &n, Case &k, int i) { std::printf(" %a", n.Predict(k.x[i], k.y[i])); }
};
struct Gram {
    template <class Net> static std::pair<double, double> step(Net &n, Case &k, double lr) { return n.BatchLearn(k.n, &k.x[0], lr); }
    template <class Net> static std::pair<double, double> fit(Net &n, Case &k, int kind, int it, double lr, double eps) {
        return kind == 0 ? n.BatchLearn(k.n, &k.x[0], it, lr, eps) : n.Learn(k.x[0], it, lr, eps);
    }
    template <class Net> static void predict(Net &n, Case &k, int i) {
        const int V = k.x[i]->nVertices;
        std::vector<double> flat((size_t)V * V);
        std::vector<double *> rows(V);
        for (int r = 0; r < V; ++r) rows[r] = &flat[(size_t)r * V];
        n.Predict(k.x[i], &rows[0]);
        for (size_t j = 0; j < flat.size(); ++j) std::printf(" %a", flat[j]);
    }
};

// the constructor argument lists: N integers, with or without momentum_param behind them
template <class Net, int N, bool M> struct Make;
template <class Net> struct Make<Net, 4, true> { static Net *of(const Case &k) { return new Net(k.c[0], k.c[1], k.c[2], k.c[3], k.momentum); } };
template <class Net> struct Make<Net, 5, true> { static Net *of(const Case &k) { return new Net(k.c[0], k.c[1], k.c[2], k.c[3], k.c[4], k.momentum); } };
template <class Net> struct Make<Net, 6, true> { static Net *of(const Case &k) { return new Net(k.c[0], k.c[1], k.c[2], k.c[3], k.c[4], k.c[5], k.momentum); } };
template <class Net> struct Make<Net, 7, true> { static Net *of(const Case &k) { return new Net(k.c[0], k.c[1], k.c[2], k.c[3], k.c[4], k.c[5], k.c[6], k.momentum); } };
template <class Net> struct Make<Net, 5, false> { static Net *of(const Case &k) { return new Net(k.c[0], k.c[1], k.c[2], k.c[3], k.c[4]); } };
template <class Net> struct Make<Net, 6, false> { static Net *of(const Case &k) { return new Net(k.c[0], k.c[1], k.c[2], k.c[3], k.c[4], k.c[5]); } };

// set_parameters where the class has it (two of the older classes do not; no checkpoint case names them)
template <class Net>
static auto set_weights(Net &n, const std::vector<float> &w, int) -> decltype(n.set_parameters(w), true) {
    n.set_parameters(w);
    return true;
}
template <class Net>
static bool set_weights(Net &, const std::vector<float> &, long) { return false; }

template <class Net, int N, bool M, class Shape>
static int run(Case &k, const std::string &verb, std::istream &in) {
    if ((int)k.c.size() != N) return 2;
    std::srand((unsigned)k.seed);
    Net &net = *Make<Net, N, M>::of(k);   // (leaked on purpose, like the molecules)
    print("params0", net.parameters());
    if (verb == "init") return 0;   // (the constructor's weights alone)
    if (verb == "checkpoint") {   // the class at given weights: save_model; a second object loads the reference's own file
        size_t n;
        in >> n;
        std::vector<float> w(n);
        for (size_t i = 0; i < n; ++i) {
            double v;
            in >> v;
            w[i] = (float)v;
        }
        if (n != net.parameters().size() || !set_weights(net, w, 0)) return 5;
        net.save_model(k.ckpt);
        std::srand(99u);
        Net &second = *Make<Net, N, M>::of(k);
        second.load_model(k.ckpt.substr(0, k.ckpt.size() - 4) + "_reference.txt");
        print("loaded", second.parameters());
        return 0;
    }
    if (verb == "steps") {
        int nSteps;
        double lr;
        in >> nSteps >> lr;
        for (int it = 0; it < nSteps; ++it) {
            const std::pair<double, double> r = Shape::step(net, k, lr);
            std::printf("pair %a %a\n", r.first, r.second);
        }
        print("params", net.parameters());
        net.save_model(k.ckpt);
        std::srand(99u);
        Net &second = *Make<Net, N, M>::of(k);
        second.load_model(k.ckpt);
        std::printf("predict");
        for (int i = 0; i < k.n; ++i) Shape::predict(net, k, i);
        std::printf("\nreloaded");
        for (int i = 0; i < k.n; ++i) Shape::predict(second, k, i);
        std::printf("\n");
        return 0;
    }
    int kind, nIter;
    double lr, eps;
    in >> kind >> nIter >> lr >> eps;
    const std::pair<double, double> r = Shape::fit(net, k, kind, nIter, lr, eps);
    std::printf("pair %a %a\ndecisions", r.first, r.second);
    for (size_t i = 0; i < net.last_decisions.size(); ++i) std::printf(" %d", (int)net.last_decisions[i]);
    std::printf("\nrate %a %d %d %d %d\n", net.last_fit.learning_rate, net.last_fit.iterations, net.last_fit.accepted, net.last_fit.rejected,
                net.last_fit.left_early);
    print("params", net.parameters());
    return 0;
}

#define CLASS(NAME, N, M, SHAPE) \
    if (k.cls == #NAME) return run<NAME##_hip, N, M, SHAPE>(k, verb, in);
static int dispatch(Case &k, const std::string &verb, std::istream &in) {
    CLASS(SMP_theta, 6, false, Single)
    CLASS(SMP_1D, 5, true, Single)
    CLASS(SMP_1D_ver2, 5, true, Single)
    CLASS(SMP_1D_ver3, 5, true, Single)
    CLASS(SMP_1D_classification, 6, true, Single)
    CLASS(SMP_1D_ver3_classification, 6, true, Single)
    CLASS(SMP_2D, 5, true, Single)
    CLASS(SMP_2D_ver4, 5, true, Single)
    CLASS(SMP_2D_ver5, 5, true, Single)
    CLASS(SMP_2D_classification, 6, true, Single)
    CLASS(SMP_2D_ver4_classification, 6, true, Single)
    CLASS(Unrestricted_SMP_1D, 5, true, Single)
    CLASS(Unrestricted_SMP_1D_ver2, 5, true, Single)
    CLASS(Unrestricted_SMP_2D, 5, true, Single)
    CLASS(NeuralFingerprint, 4, true, Single)
    CLASS(GCN_1D, 6, true, Single)
    CLASS(GCN_2D, 6, true, Single)
    CLASS(GCN_3D, 6, true, Single)
    CLASS(GRU_GCN_1D, 6, true, Single)
    CLASS(GRU_GCN_2D, 6, true, Single)
    CLASS(GRU_GCN_3D, 6, true, Single)
    CLASS(GCN_1D_Distance, 6, true, Single)
    CLASS(GCN_2D_Distance, 6, true, Single)
    CLASS(GCN_3D_Distance, 6, true, Single)
    CLASS(GCN_1D_Kernel, 6, true, Pairs)
    CLASS(GCN_2D_Kernel, 6, true, Pairs)
    CLASS(GCN_3D_Kernel, 6, true, Pairs)
    CLASS(GCA_1D, 6, true, Gram)
    CLASS(LCNN, 7, true, Single)
    CLASS(GCN_MW, 5, true, Single)
    CLASS(CGCN_1D, 4, true, Single)
    CLASS(CGCN_2D, 4, true, Single)
    // the older classes: their two iterative methods
    CLASS(SMP_omega, 6, false, Single)
    CLASS(SMP_2D_ver6_classification, 6, true, Single)
    CLASS(SMP_omega_physics, 5, false, Single)
    return 3;
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    std::ifstream in(argv[1]);
    if (!in) return 1;
    std::string word;
    Case k;
    while (in >> word) {
        if (word == "case") {
            k = Case();
            int n;
            in >> k.id >> k.cls >> n;
            k.c.resize(n);
            for (int i = 0; i < n; ++i) in >> k.c[i];
            in >> k.momentum >> k.seed;
            k.ckpt = std::string(argv[2]) + "/" + k.id + ".txt";
        } else if (word == "batch") {
            int F, second, dist;
            in >> k.n >> F >> second >> dist;
            for (int i = 0; i < k.n; ++i) k.x.push_back(read_graph(in, F, dist != 0));
            for (int i = 0; second && i < k.n; ++i) k.y.push_back(read_graph(in, F, false));
        } else if (word == "targets") {
            int n;
            in >> n;
            k.t.resize(n ? n : 1);
            for (int i = 0; i < n; ++i) in >> k.t[i];
        } else if (word == "steps" || word == "fit" || word == "init" || word == "checkpoint") {
            std::printf("case %s\n", k.id.c_str());
            const int st = dispatch(k, word, in);
            if (st) {
                std::fprintf(stderr, "case %s: class %s with %d constructor integers is not known here (%d)\n", k.id.c_str(), k.cls.c_str(), (int)k.c.size(), st);
                return st;
            }
            std::fflush(stdout);
        } else {
            return 4;
        }
    }
    std::printf("DONE\n");
    return 0;
}
