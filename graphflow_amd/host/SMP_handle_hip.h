// SMP_handle_hip.h -- the shared skeleton of the drop-in classes for every model the library runs on ONE gf_smp handle
// (SMP_families_hip.h holds the classes; SMP_omega_hip.h, SMP_classification_hip.h and SMP_physics_hip.h are older and stand alone).
//
//   reference (every model header)                                here
//   constructor: weights_initialization() from rand()             gf_smp_*uniform_init_host after the caller's srand: the same weights
//   getLoss(nBatch, DenseGraph**, target)                         one device forward over the batch, the losses added in double in order
//   BatchLearn(nBatch, molecule, target, lr)                      loss before, summed gradients, sgd->Learn(lr, nBatch), loss after
//   BatchLearn(nBatch, molecule, target, nIterations, lr, eps)    gf_smp_fit_host, kind 0: the class's loop, comparison for comparison
//   Learn(molecule, target, nIterations, lr, eps)                 gf_smp_fit_host, kind 1
//   Predict / Feature                                             forward only (a classifier's Predict is the arg-max label as a double)
//   save_model / load_model                                       byte-compatible text checkpoints
//   -                                                             parameters() / gradients() / set_parameters(): flat views in
//                                                                 registration order; last_fit / last_decisions: what the last
//                                                                 iterative call did, iteration by iteration (gf_smp_fit's log)
//
// Three shapes of the public methods: SMP_single_hip (one graph per sample and a target), SMP_pairs_hip (GCN_*D_Kernel: two graphs per
// sample), SMP_gram_hip (GCA_1D: no target; Predict fills a V x V matrix).  The molecule type is a template parameter of the methods:
// anything with the public fields of the reference's DenseGraph (nVertices, nFeatures, int **adj, double **feature, and for the
// distance models double **distance) works, DenseGraph itself included.  Plain C++11, no HIP.  No CPU fallback: every call ends in
// libgf_hip.so and aborts with the library's message if the device path fails (the reference aborts on assert).
#ifndef GF_SMP_HANDLE_HIP_H_INCLUDED
#define GF_SMP_HANDLE_HIP_H_INCLUDED

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "gf_runtime.h"

namespace gfhost {

// molecule->distance when the molecule type has one (DenseGraph does), NULL otherwise
template <class Graph>
auto distance_of(const Graph *g, int) -> decltype(&g->distance[0][0], (double **)0) { return g->distance; }
template <class Graph>
double **distance_of(const Graph *, long) { return NULL; }

// a gf_smp_config with every field zero: the classes set the fields of their family by name
inline gf_smp_config zero_config() {
    gf_smp_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    return cfg;
}

// DenseGraph** -> the flat batch of gf_smp_prepare*: vertex counts, adjacency / feature (/ distance) matrices back to back
struct FlatBatch {
    std::vector<int> nV, adj;
    std::vector<double> feature, distance;
    template <class Graph>
    void fill(const char *who, int nBatch, Graph **molecule, int max_nVertices, int nFeatures, bool with_distance) {
        nV.resize(nBatch);
        adj.clear();
        feature.clear();
        distance.clear();
        for (int m = 0; m < nBatch; ++m) {
            const Graph *g = molecule[m];
            if (g->nVertices > max_nVertices || g->nFeatures != nFeatures) {
                std::fprintf(stderr, "%s: molecule %d has %d vertices / %d features (model: <= %d / %d)\n", who, m, g->nVertices, g->nFeatures,
                             max_nVertices, nFeatures);
                std::abort();
            }
            nV[m] = g->nVertices;
            double **dist = with_distance ? distance_of(g, 0) : NULL;
            if (with_distance && !dist) {
                std::fprintf(stderr, "%s: the model needs a molecule type with a `distance` matrix\n", who);
                std::abort();
            }
            for (int i = 0; i < g->nVertices; ++i) {
                adj.insert(adj.end(), g->adj[i], g->adj[i] + g->nVertices);
                feature.insert(feature.end(), g->feature[i], g->feature[i] + nFeatures);
                if (dist) distance.insert(distance.end(), dist[i], dist[i] + g->nVertices);
            }
        }
    }
};

}  // namespace gfhost

class SMP_handle_hip : public gfhost::FitLog {
public:
    ~SMP_handle_hip() { gf_smp_destroy(net); }

    void save_model(std::string filename) { must(gf_smp_save_model(net, NULL, filename.c_str()), "gf_smp_save_model"); }
    void load_model(std::string filename) { must(gf_smp_load_model(net, NULL, filename.c_str()), "gf_smp_load_model"); }

    // flat views of sgd->params[i]->value / ->gradient in registration order
    std::vector<float> parameters() {
        std::vector<float> p(gf_smp_param_count(net));
        must(gf_smp_parameters_download(net, &p[0], NULL), "gf_smp_parameters_download");
        return p;
    }
    std::vector<float> gradients() {
        std::vector<float> g(gf_smp_param_count(net));
        must(gf_smp_parameters_download(net, NULL, &g[0]), "gf_smp_parameters_download");
        return g;
    }
    void set_parameters(const std::vector<float> &p) { must(gf_smp_parameters_upload(net, &p[0]), "gf_smp_parameters_upload"); }
    // sgd = new SGD / Momentum / Adam / AdaMax / AdaDelta(...) in place of the class's own (gfhost::OptimiserChoice); starts from zero state
    void use_optimiser(const gf_optim_config &config) {
        choice.optim = config;
        choice.chosen = true;
        must(gf_smp_adam_reset(net), "gf_smp_adam_reset");
    }

    int nClass, max_nVertices, nFeatures;   // (last_fit / last_decisions of the last iterative call: gfhost::FitLog)
    double momentum;

protected:
    // nClass >= 2: a classifier handle.  use_momentum: sgd = new Momentum(momentum_param), else Adam.
    SMP_handle_hip(const char *name, const gf_smp_config &cfg, int nClass, bool use_momentum, double momentum_param)
        : nClass(nClass), max_nVertices(cfg.max_nVertices ? cfg.max_nVertices : cfg.max_receptive_field), nFeatures(cfg.nFeatures),
          momentum(momentum_param), name(name), cfg(cfg), use_momentum(use_momentum), net(NULL) {
        gf_ctx *ctx = gfhost::default_context();
        must(nClass ? gf_smp_create_classifier(ctx, &cfg, nClass, &net) : gf_smp_create(ctx, &cfg, &net), "gf_smp_create");
        std::vector<float> w(gf_smp_param_count(net));   // weights_initialization()
        must(nClass ? gf_smp_classifier_uniform_init_host(&cfg, nClass, &w[0]) : gf_smp_uniform_init_host(&cfg, &w[0]), "gf_smp_uniform_init_host");
        must(gf_smp_parameters_upload(net, &w[0]), "gf_smp_parameters_upload");
    }

    template <class Graph>
    void bind(int nBatch, Graph **molecule) {
        x.fill(name, nBatch, molecule, max_nVertices, nFeatures, cfg.distance_channel != 0);
        if (cfg.distance_channel)
            must(gf_smp_prepare_distance(net, nBatch, &x.nV[0], &x.adj[0], &x.feature[0], &x.distance[0]), "gf_smp_prepare_distance");
        else
            must(gf_smp_prepare(net, nBatch, &x.nV[0], &x.adj[0], &x.feature[0]), "gf_smp_prepare");
    }
    template <class Graph>
    void bind_pairs(int nBatch, Graph **molecule_X, Graph **molecule_Y) {
        x.fill(name, nBatch, molecule_X, max_nVertices, nFeatures, false);
        y.fill(name, nBatch, molecule_Y, max_nVertices, nFeatures, false);
        must(gf_smp_prepare_pairs(net, nBatch, &x.nV[0], &x.adj[0], &x.feature[0], &y.nV[0], &y.adj[0], &y.feature[0]), "gf_smp_prepare_pairs");
    }

    // the bound batch forwarded: the sum of its losses (target NULL: the Gram auto-encoder)
    double forward_loss(int nBatch, const double *target) {
        std::vector<double> loss(nBatch);
        must(gf_smp_forward_host_samples(net, target, NULL, &loss[0], NULL), "gf_smp_forward_host_samples");
        double total = 0.0;
        for (int i = 0; i < nBatch; ++i) total += loss[i];
        return total;
    }
    // BatchLearn(nBatch, ..., learning_rate) on the bound batch
    std::pair<double, double> learn_once(int nBatch, const double *target, double learning_rate) {
        std::pair<double, double> ret;
        ret.first = forward_loss(nBatch, target);
        must(gf_smp_backward(net, NULL, NULL, 0), "gf_smp_backward");
        if (choice.chosen) {
            const gf_optim_config oc = choice.step_config(learning_rate, nBatch);
            must(gf_smp_optimiser_step(net, NULL, NULL, &oc), "gf_smp_optimiser_step");
        } else if (use_momentum) {
            must(gf_smp_momentum_step(net, NULL, NULL, learning_rate, nBatch, momentum), "gf_smp_momentum_step");
        } else {
            must(gf_smp_adam_step(net, NULL, NULL, learning_rate, nBatch), "gf_smp_adam_step");
        }
        ret.second = forward_loss(nBatch, target);
        return ret;
    }
    // the two iterative calls on the bound batch (kind 0: BatchLearn, 1: Learn)
    std::pair<double, double> fit(int kind, const double *target, int nIterations, double learning_rate, double epsilon) {
        return gfhost::fit_host(gf_smp_fit_host, "gf_smp_fit_host", net, target, kind, choice.chosen ? choice.optim.kind : use_momentum ? 1 : 0,
                                nIterations, learning_rate, epsilon, choice.chosen ? choice.optim.gamma : momentum, this);
    }
    double predict_one() {
        double y = 0.0;
        must(gf_smp_forward_host_samples(net, NULL, &y, NULL, NULL), "gf_smp_forward_host_samples");
        return y;
    }
    std::vector<double> feature_one() {
        std::vector<double> f(gf_smp_feature_width(net));
        must(gf_smp_forward_host_samples(net, NULL, NULL, NULL, &f[0]), "gf_smp_forward_host_samples");
        return f;
    }
    void must(gf_status st, const char *what) {
        if (st != GF_OK) gfhost::die(gfhost::default_context(), what, st);
    }

    const char *name;
    gf_smp_config cfg;
    bool use_momentum;
    gf_smp *net;
    gfhost::FlatBatch x, y;
    gfhost::OptimiserChoice choice;

private:
    SMP_handle_hip(const SMP_handle_hip &);
    SMP_handle_hip &operator=(const SMP_handle_hip &);
};

// one graph per sample and a target: the regression models, their classifiers (target = the label as a double), the distance models
class SMP_single_hip : public SMP_handle_hip {
public:
    template <class Graph>
    double getLoss(int nBatch, Graph **molecule, double *target) {
        bind(nBatch, molecule);
        return forward_loss(nBatch, target);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule, double *target, double learning_rate) {
        bind(nBatch, molecule);
        return learn_once(nBatch, target, learning_rate);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule, double *target, int nIterations, double learning_rate, double epsilon) {
        bind(nBatch, molecule);
        return fit(0, target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    std::pair<double, double> Learn(Graph *molecule, double target, int nIterations, double learning_rate, double epsilon) {
        bind(1, &molecule);
        return fit(1, &target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    double Predict(Graph *molecule) {
        bind(1, &molecule);
        return predict_one();
    }
    template <class Graph>
    std::vector<double> Feature(Graph *molecule) {
        bind(1, &molecule);
        return feature_one();
    }

protected:
    SMP_single_hip(const char *name, const gf_smp_config &cfg, int nClass, bool use_momentum, double momentum_param)
        : SMP_handle_hip(name, cfg, nClass, use_momentum, momentum_param) {}
};

// two graphs per sample (GCN_1D_Kernel.h:291-432 and its siblings)
class SMP_pairs_hip : public SMP_handle_hip {
public:
    template <class Graph>
    double getLoss(int nBatch, Graph **molecule_X, Graph **molecule_Y, double *target) {
        bind_pairs(nBatch, molecule_X, molecule_Y);
        return forward_loss(nBatch, target);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule_X, Graph **molecule_Y, double *target, double learning_rate) {
        bind_pairs(nBatch, molecule_X, molecule_Y);
        return learn_once(nBatch, target, learning_rate);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule_X, Graph **molecule_Y, double *target, int nIterations, double learning_rate,
                                         double epsilon) {
        bind_pairs(nBatch, molecule_X, molecule_Y);
        return fit(0, target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    std::pair<double, double> Learn(Graph *molecule_X, Graph *molecule_Y, double target, int nIterations, double learning_rate, double epsilon) {
        bind_pairs(1, &molecule_X, &molecule_Y);
        return fit(1, &target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    double Predict(Graph *molecule_X, Graph *molecule_Y) {
        bind_pairs(1, &molecule_X, &molecule_Y);
        return predict_one();
    }
    template <class Graph>
    std::vector<double> Feature(Graph *molecule_X, Graph *molecule_Y) {
        bind_pairs(1, &molecule_X, &molecule_Y);
        return feature_one();
    }

protected:
    SMP_pairs_hip(const char *name, const gf_smp_config &cfg, double momentum_param) : SMP_handle_hip(name, cfg, 0, true, momentum_param) {}
};

// no target: the auto-encoder (GCA_1D.h:303-445); Predict fills mat[V][V] with the Gram matrix
class SMP_gram_hip : public SMP_handle_hip {
public:
    template <class Graph>
    double getLoss(int nBatch, Graph **molecule) {
        bind(nBatch, molecule);
        return forward_loss(nBatch, NULL);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule, double learning_rate) {
        bind(nBatch, molecule);
        return learn_once(nBatch, NULL, learning_rate);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule, int nIterations, double learning_rate, double epsilon) {
        bind(nBatch, molecule);
        return fit(0, NULL, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    std::pair<double, double> Learn(Graph *molecule, int nIterations, double learning_rate, double epsilon) {
        bind(1, &molecule);
        return fit(1, NULL, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    void Predict(Graph *molecule, double **mat) {
        bind(1, &molecule);
        forward_loss(1, NULL);
        const int V = molecule->nVertices;
        std::vector<double> flat((size_t)V * V);
        must(gf_smp_gram_host(net, &flat[0]), "gf_smp_gram_host");
        for (int i = 0; i < V; ++i)
            for (int j = 0; j < V; ++j) mat[i][j] = flat[(size_t)i * V + j];
    }

protected:
    SMP_gram_hip(const char *name, const gf_smp_config &cfg, double momentum_param) : SMP_handle_hip(name, cfg, 0, true, momentum_param) {}
};

#endif
