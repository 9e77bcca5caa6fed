// test_SMP_classification_hip.cpp -- the classification drop-ins, driven like the reference's tests/test_SMP_2D_ver6_classification.cpp: its
// four hand-built molecules (CH4, NH3, H2O, C2H4; one-hot C,H,N,O features; label = number of atoms), nClass 11, nLevels 1, nChanels 10,
// nDepth 5, max_nVertices 10, momentum 0.9, learning rate 1e-3, 1000 epochs of BatchLearn, then Predict.
// Known answers: the REAL reference classes, constructed after srand(17), report for the first three BatchLearn calls the (before, after)
// sums of log-probabilities below and predict 5, 4, 3, 6 after the 1000 epochs (tests/golden/make_classification_golden.py ->
// smp_classification.npz, v6_train / v7_train).  The same seed must give the same initial weights and the same trajectory here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "SMP_classification_hip.h"

struct Molecule {  // public fields of GraphFlow/DenseGraph.h
    int nVertices, nFeatures;
    int **adj;
    double **feature;
    Molecule(int V, int F) : nVertices(V), nFeatures(F) {
        adj = new int *[V];
        feature = new double *[V];
        for (int i = 0; i < V; ++i) {
            adj[i] = new int[V]();
            feature[i] = new double[F]();
        }
    }
};

static Molecule *build(const char *labels, int nEdges, const int (*edges)[2]) {
    const int V = (int)std::strlen(labels);
    Molecule *m = new Molecule(V, 4);
    for (int e = 0; e < nEdges; ++e) m->adj[edges[e][0]][edges[e][1]] = m->adj[edges[e][1]][edges[e][0]] = 1;
    for (int v = 0; v < V; ++v) m->feature[v][std::strchr("CHNO", labels[v]) - "CHNO"] = 1.0;
    return m;
}

static int close_to(const char *what, double got, double ref, double tol) {
    const double rel = std::fabs(got - ref) / std::fmax(1.0, std::fabs(ref));
    std::printf("%-36s %-14.8f reference %-14.8f rel %.2e %s\n", what, got, ref, rel, rel <= tol ? "" : "  <-- FAIL");
    return rel > tol;
}

template <class Net>
static int drive(const char *name, Molecule **mol, double *target, const double (*ref)[2], const std::string &ckpt) {
    int bad = 0;
    srand(17);
    Net train(11, 10, 1, 10, 4, 5, 0.9);
    for (int it = 0; it < 3; ++it) {
        std::pair<double, double> r = train.BatchLearn(4, mol, target, 1e-3);
        char what[96];
        std::snprintf(what, sizeof what, "%s BatchLearn %d before", name, it);
        bad |= close_to(what, r.first, ref[it][0], 5e-5);
        std::snprintf(what, sizeof what, "%s BatchLearn %d after", name, it);
        bad |= close_to(what, r.second, ref[it][1], 5e-5);
        bad |= !(r.first <= 0.0 && r.second <= 0.0);   // sums of log-probabilities
    }
    std::pair<double, double> last;
    for (int epoch = 3; epoch < 1000; ++epoch) last = train.BatchLearn(4, mol, target, 1e-3);
    std::printf("%s after 1000 epochs: loss %.6f -> %.6f\n", name, last.first, last.second);
    bad |= !(last.second > -0.05);
    train.save_model(ckpt);
    srand(99);
    Net test(11, 10, 1, 10, 4, 5, 0.9);
    test.load_model(ckpt);
    for (int i = 0; i < 4; ++i) {
        const double a = train.Predict(mol[i]), b = test.Predict(mol[i]);
        std::printf("%s target %g Predict %g (loaded model %g)\n", name, target[i], a, b);
        bad |= a != target[i] || b != target[i];
    }
    bad |= (int)train.Feature(mol[0]).size() != 10;
    bad |= close_to("getLoss of the loaded model", test.getLoss(4, mol, target), train.getLoss(4, mol, target), 1e-4);   // 6 printed digits
    // the checkpoint holds param_count numbers: H [10][24], K_1 [10][nK 10], b_1 [10], W [11][10]
    size_t count = 0;
    if (FILE *f = std::fopen(ckpt.c_str(), "r")) {
        double v;
        while (std::fscanf(f, "%lf", &v) == 1) ++count;
        std::fclose(f);
    }
    bad |= count != train.parameters().size();
    return bad;
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    static const int e1[][2] = {{0, 1}, {0, 2}, {0, 3}, {0, 4}}, e2[][2] = {{0, 1}, {0, 2}, {0, 3}}, e3[][2] = {{0, 1}, {0, 2}},
                     e4[][2] = {{0, 1}, {0, 2}, {0, 3}, {3, 4}, {3, 5}};
    Molecule *mol[4] = {build("CHHHH", 4, e1), build("NHHH", 3, e2), build("OHH", 2, e3), build("CHHCHH", 5, e4)};
    double target[4];
    for (int i = 0; i < 4; ++i) target[i] = mol[i]->nVertices;
    static const double ref6[3][2] = {{-9.61412754, -9.59751021}, {-9.59751021, -9.56610351}, {-9.56610351, -9.52163867}};
    static const double ref7[3][2] = {{-9.59646200, -9.57951857}, {-9.57951857, -9.54746907}, {-9.54746907, -9.50203433}};
    int bad = drive<SMP_2D_ver6_classification_hip>("ver6", mol, target, ref6, dir + "/gf_classification_v6.dat");
    bad |= drive<SMP_2D_ver7_classification_hip>("ver7", mol, target, ref7, dir + "/gf_classification_v7.dat");
    std::printf(bad ? "FAILED\n" : "PASSED\n");
    return bad;
}
