// SMP_classification_hip.h -- drop-ins for the public API of the reference's classification models SMP_2D_ver6_classification /
// SMP_2D_ver7_classification (GraphFlow/SMP_2D_ver6_classification.h:30-950 and its ver7 sibling) on top of the classifier handle of the
// C ABI (gf_smp_create_classifier, include/gf_hip.h).
//
//   reference                                                     here
//   SMP_2D_ver6_classification(nClass, max_nVertices, nLevels,    same arguments, nClass first (:32, :46); the constructor draws the
//       nChanels, nFeatures, nDepth, momentum_param[, wl])        initial weights from rand() exactly as :256-259 does
//   BatchLearn(nBatch, DenseGraph**, target, lr)       :577       one device pass over the batch: loss before, summed gradients,
//                                                                 Momentum::Learn(lr, nBatch), loss after
//   getLoss                                            :566       the SUM of LogLoss values = sum of log p[label], at most 0 (the
//                                                                 reference's sign: BatchLearn's pair rises towards 0 while it learns)
//   Predict                                            :699       the arg-max label (lowest index on a tie), as a double
//   Feature                                            :715       graph_feature
//   save_model / load_model                            :764       byte-compatible text checkpoints: H, (K_l, b_l)..., W[nClass][C]
//
// target[i] is the label as a double (the reference's (int)target).  The molecule type is a template parameter of the methods, as in
// SMP_omega_hip.h.  No CPU fallback: every call ends in libgf_hip.so and aborts with the library's message if the device path fails.
#ifndef GF_SMP_CLASSIFICATION_HIP_H_INCLUDED
#define GF_SMP_CLASSIFICATION_HIP_H_INCLUDED

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "gf_runtime.h"

class SMP_classification_hip : public gfhost::FitLog {   // (last_fit / last_decisions of the last iterative call)
protected:
    SMP_classification_hip(int nClass, int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, double momentum_param,
                           bool has_WL_ordering, int nContractions)
        : nClass(nClass), max_nVertices(max_nVertices), nLevels(nLevels), nChanels(nChanels), nFeatures(nFeatures), nDepth(nDepth),
          momentum(momentum_param), net(NULL) {
        gf_smp_config cfg = {nLevels, nChanels, nFeatures, nDepth, max_nVertices, has_WL_ordering ? 1 : 0, nContractions, 1};
        must(gf_smp_create_classifier(gfhost::default_context(), &cfg, nClass, &net), "gf_smp_create_classifier");
        std::vector<float> w(gf_smp_param_count(net));
        must(gf_smp_classifier_uniform_init_host(&cfg, nClass, &w[0]), "gf_smp_classifier_uniform_init_host");
        must(gf_smp_parameters_upload(net, &w[0]), "gf_smp_parameters_upload");
    }

public:
    ~SMP_classification_hip() { gf_smp_destroy(net); }

    template <class Graph>
    double getLoss(int nBatch, Graph **molecule, double *target) {
        bind(nBatch, molecule);
        return forward_loss(nBatch, target);
    }

    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule, double *target, double learning_rate) {
        std::pair<double, double> ret;
        ret.first = getLoss(nBatch, molecule, target);  // leaves the batch bound and forwarded
        must(gf_smp_backward(net, NULL, NULL, 0), "gf_smp_backward");
        if (choice.chosen) {
            const gf_optim_config oc = choice.step_config(learning_rate, nBatch);
            must(gf_smp_optimiser_step(net, NULL, NULL, &oc), "gf_smp_optimiser_step");
        } else {
            must(gf_smp_momentum_step(net, NULL, NULL, learning_rate, nBatch, momentum), "gf_smp_momentum_step");
        }
        ret.second = forward_loss(nBatch, target);
        return ret;
    }

    // the two iterative calls (SMP_2D_ver6_classification.h:604-697): the class's loops on LogLoss values, inside the library
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
        double label = 0.0;
        must(gf_smp_forward_host(net, NULL, &label, NULL, NULL), "gf_smp_forward_host");
        return label;
    }

    template <class Graph>
    std::vector<double> Feature(Graph *molecule) {
        bind(1, &molecule);
        std::vector<double> f(nChanels);
        must(gf_smp_forward_host(net, NULL, NULL, NULL, &f[0]), "gf_smp_forward_host");
        return f;
    }

    void save_model(std::string filename) { must(gf_smp_save_model(net, NULL, filename.c_str()), "gf_smp_save_model"); }
    void load_model(std::string filename) { must(gf_smp_load_model(net, NULL, filename.c_str()), "gf_smp_load_model"); }
    // sgd = new SGD / Momentum / Adam / AdaMax / AdaDelta(...) in place of the class's Momentum (gfhost::OptimiserChoice); starts from zero state
    void use_optimiser(const gf_optim_config &config) {
        choice.optim = config;
        choice.chosen = true;
        must(gf_smp_adam_reset(net), "gf_smp_adam_reset");
    }

    // flat view of sgd->params[i]->value in registration order (H, K_1, b_1, ..., W)
    std::vector<float> parameters() {
        std::vector<float> p(gf_smp_param_count(net));
        must(gf_smp_parameters_download(net, &p[0], NULL), "gf_smp_parameters_download");
        return p;
    }

    int nClass, max_nVertices, nLevels, nChanels, nFeatures, nDepth;

private:
    double forward_loss(int nBatch, double *target) {
        std::vector<double> loss(nBatch);
        must(gf_smp_forward_host(net, target, NULL, &loss[0], NULL), "gf_smp_forward_host");
        double total = 0.0;
        for (int i = 0; i < nBatch; ++i) total += loss[i];
        return total;
    }
    // DenseGraph** -> the flat batch of gf_smp_prepare (host graph preparation + index upload)
    template <class Graph>
    void bind(int nBatch, Graph **molecule) {
        nV.resize(nBatch);
        adj.clear();
        feature.clear();
        for (int m = 0; m < nBatch; ++m) {
            const Graph *g = molecule[m];
            if (g->nVertices > max_nVertices || g->nFeatures != nFeatures) {
                std::fprintf(stderr, "SMP_classification_hip: molecule %d has %d vertices / %d features (model: <= %d / %d)\n", m, g->nVertices,
                             g->nFeatures, max_nVertices, nFeatures);
                std::abort();
            }
            nV[m] = g->nVertices;
            for (int i = 0; i < g->nVertices; ++i) {
                adj.insert(adj.end(), g->adj[i], g->adj[i] + g->nVertices);
                feature.insert(feature.end(), g->feature[i], g->feature[i] + nFeatures);
            }
        }
        must(gf_smp_prepare(net, nBatch, &nV[0], &adj[0], &feature[0]), "gf_smp_prepare");
    }
    std::pair<double, double> fit(int kind, const double *target, int nIterations, double learning_rate, double epsilon) {
        return gfhost::fit_host(gf_smp_fit_host, "gf_smp_fit_host", net, target, kind, choice.chosen ? choice.optim.kind : 1, nIterations, learning_rate,
                                epsilon, choice.chosen ? choice.optim.gamma : momentum, this);
    }
    void must(gf_status st, const char *what) {
        if (st != GF_OK) gfhost::die(gfhost::default_context(), what, st);
    }
    double momentum;
    gfhost::OptimiserChoice choice;
    gf_smp *net;
    std::vector<int> nV, adj;
    std::vector<double> feature;
};

// RisiContraction_10 levels (SMP_2D_ver6_classification.h:136-143)
class SMP_2D_ver6_classification_hip : public SMP_classification_hip {
public:
    SMP_2D_ver6_classification_hip(int nClass, int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, double momentum_param,
                                   bool has_WL_ordering = true)
        : SMP_classification_hip(nClass, max_nVertices, nLevels, nChanels, nFeatures, nDepth, momentum_param, has_WL_ordering, 10) {}
};
// RisiContraction_50 levels (SMP_2D_ver7_classification.h:136-143)
class SMP_2D_ver7_classification_hip : public SMP_classification_hip {
public:
    SMP_2D_ver7_classification_hip(int nClass, int max_nVertices, int nLevels, int nChanels, int nFeatures, int nDepth, double momentum_param,
                                   bool has_WL_ordering = true)
        : SMP_classification_hip(nClass, max_nVertices, nLevels, nChanels, nFeatures, nDepth, momentum_param, has_WL_ordering, 50) {}
};

#endif
