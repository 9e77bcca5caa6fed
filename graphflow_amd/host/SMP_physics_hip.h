// SMP_physics_hip.h -- drop-ins for the `_physics` and `_pairgraphs` model classes of the reference on top of gf_smp_model_*
// (include/gf_hip.h):
//   SMP_omega_physics_hip(max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures)      GraphFlow/SMP_omega_physics.h:31
//   SMP_beta_physics_hip(max_nVertices, nLevels, nChanels, nFeatures)                              GraphFlow/SMP_beta_physics.h:31
//   SMP_omega_pairgraphs_hip(max_nV_1, max_nV_2, max_rf, nLevels, nChanels, nFeatures_1, _2)       GraphFlow/SMP_omega_pairgraphs.h:81
//   SMP_beta_pairgraphs_hip(max_nV_1, max_nV_2, nLevels, nChanels, nFeatures_1, _2)                GraphFlow/SMP_beta_pairgraphs.h:81
//   SMP_sigma_pairgraphs_hip(..., nKept) + setMode / setTrainMode / setTestMode                    GraphFlow/SMP_sigma_pairgraphs.h:81,139
//   SMP_gamma_physics_hip([use_coulomb,] max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures)
//                                                                                                  GraphFlow/SMP_gamma_physics.h:31,47
//   SMP_gamma_pairgraphs_hip(max_nV_1, max_nV_2, max_rf, nLevels, nChanels, nFeatures_1, _2)       GraphFlow/SMP_gamma_pairgraphs.h
//   SMP_theta_physics_hip(max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures)        GraphFlow/SMP_theta_physics.h
//   SMP_theta_pairgraphs_hip(max_nV_1, max_nV_2, max_rf, nLevels, nChanels, nFeatures_1, _2)       GraphFlow/SMP_theta_pairgraphs.h
//   CCN_1D_hip(max_nV_1, max_nV_2, max_rf, nLevels, nChanels, nFeatures_1, _2, nChanels_decay)     GraphFlow/CCN_1D.h:34
// with the reference's public training / inference methods: BatchLearn, Threaded_BatchLearn, getLoss, Predict,
// Threaded_Predict, init_multi_threads (accepted, nothing to do: a batch is one device pass), save_model / load_model (the
// text format of SMP_omega_physics.h:927-949: every parameter value in registration order).  The constructors draw the initial
// weights from rand() exactly as weights_initialization does: the same srand() starts from the reference's model.
// The molecule type is a template parameter (any type with DenseGraph's public nVertices / nFeatures / adj / feature).
// No CPU fallback: every call ends in libgf_hip.so and aborts with the library's message if the device path fails.
#ifndef GF_SMP_PHYSICS_HIP_H_INCLUDED
#define GF_SMP_PHYSICS_HIP_H_INCLUDED

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "gf_runtime.h"

class SMP_model_hip : public gfhost::FitLog {   // (last_fit / last_decisions of the last iterative call)
protected:
    // nContractions: 18 (RisiContraction_18 / _18_dropout towers) or 4 (the `_gamma` models: RisiContraction_4, K_l [4 C_{l-1}][C_l]);
    // 0 with first_order = 1: the first-order towers of the `_theta` models, and with ccn_1d and nChanels_decay those of CCN_1D
    SMP_model_hip(int nTowers, int maxV1, int maxV2, int max_rf, int nLevels, int nChanels, int F1, int F2, int nKept, int nContractions = 18,
                  int first_order = 0, double nChanels_decay = 0.0, bool ccn_1d = false)
        : net(NULL), towers(nTowers) {
        maxV[0] = maxV1;
        maxV[1] = maxV2;
        nF[0] = F1;
        nF[1] = F2;
        gf_smp_model_config cfg = {nTowers, nLevels, nChanels, max_rf, {F1, F2}, nKept, nContractions};
        if (first_order) {
            cfg.first_order = first_order;
            cfg.max_nVertices[0] = maxV1;
            cfg.max_nVertices[1] = maxV2;
        }
        cfg.ccn_1d = ccn_1d ? 1 : 0;
        cfg.nChanels_decay = nChanels_decay;
        must(gf_smp_model_create(gfhost::default_context(), &cfg, &net), "gf_smp_model_create");
        std::vector<float> w(gf_smp_model_param_count(net));
        must(gf_smp_model_uniform_init_host(net, &w[0]), "gf_smp_model_uniform_init_host");  // weights_initialization()
        must(gf_smp_model_parameters_upload(net, &w[0]), "gf_smp_model_parameters_upload");
    }

public:
    ~SMP_model_hip() { gf_smp_model_destroy(net); }
    void init_multi_threads(int) {}
    void setMode(bool train) { must(gf_smp_model_set_mode(net, train ? 1 : 0), "gf_smp_model_set_mode"); }
    void setTrainMode() { setMode(true); }
    void setTestMode() { setMode(false); }
    // sgd = new SGD / Momentum / Adam / AdaMax / AdaDelta(...) in place of the class's Adam (gfhost::OptimiserChoice).  Before the first
    // step: the composite handle keeps the kind of its first step (optimiser 1, Momentum, has no iterative call here).
    void use_optimiser(const gf_optim_config &config) {
        choice.optim = config;
        choice.chosen = true;
    }

    void save_model(std::string filename) {
        std::vector<float> p = parameters();
        FILE *f = std::fopen(filename.c_str(), "w");
        if (!f) die("save_model: cannot open file");
        for (size_t i = 0; i < p.size(); ++i) std::fprintf(f, "%g ", (double)p[i]);
        std::fclose(f);
    }
    void load_model(std::string filename) {
        std::vector<float> p(gf_smp_model_param_count(net));
        FILE *f = std::fopen(filename.c_str(), "r");
        if (!f) die("load_model: cannot open file");
        double v;
        size_t got = 0;
        while (got < p.size() && std::fscanf(f, "%lf", &v) == 1) p[got++] = (float)v;
        std::fclose(f);
        if (got != p.size()) die("load_model: the file holds fewer values than the model has parameters");
        must(gf_smp_model_parameters_upload(net, &p[0]), "gf_smp_model_parameters_upload");
    }
    std::vector<float> parameters() {
        std::vector<float> p(gf_smp_model_param_count(net));
        must(gf_smp_model_parameters_download(net, &p[0], NULL), "gf_smp_model_parameters_download");
        return p;
    }
    std::vector<float> gradients() {
        std::vector<float> g(gf_smp_model_param_count(net));
        must(gf_smp_model_parameters_download(net, NULL, &g[0]), "gf_smp_model_parameters_download");
        return g;
    }

protected:
    template <class Graph>
    void pack(int t, int nBatch, Graph **molecule) {
        nV[t].resize(nBatch);
        adj[t].clear();
        feature[t].clear();
        for (int m = 0; m < nBatch; ++m) {
            const Graph *g = molecule[m];
            if (g->nVertices > maxV[t] || g->nFeatures != nF[t]) die("a molecule exceeds max_nVertices or has the wrong feature count");
            nV[t][m] = g->nVertices;
            for (int i = 0; i < g->nVertices; ++i) {
                adj[t].insert(adj[t].end(), g->adj[i], g->adj[i] + g->nVertices);
                feature[t].insert(feature[t].end(), g->feature[i], g->feature[i] + nF[t]);
            }
        }
    }
    void prepare(int nBatch) {
        must(gf_smp_model_prepare(net, nBatch, &nV[0][0], &adj[0][0], &feature[0][0], towers == 2 ? &nV[1][0] : NULL,
                                  towers == 2 ? &adj[1][0] : NULL, towers == 2 ? &feature[1][0] : NULL),
             "gf_smp_model_prepare");
    }
    double loss_of_batch(int nBatch, double *target) {
        std::vector<double> loss(nBatch);
        must(gf_smp_model_forward_host(net, target, NULL, &loss[0]), "gf_smp_model_forward_host");
        double total = 0.0;
        for (int i = 0; i < nBatch; ++i) total += loss[i];
        return total;
    }
    std::pair<double, double> learn(int nBatch, double *target, double learning_rate, bool with_losses) {
        std::pair<double, double> ret(0.0, 0.0);
        if (with_losses)
            ret.first = loss_of_batch(nBatch, target);  // getLoss (its forward draws dropout masks too, as the reference's does)
        must(gf_smp_model_forward_host(net, target, NULL, NULL), "gf_smp_model_forward_host");
        must(gf_smp_model_backward(net, NULL, NULL, 0), "gf_smp_model_backward");
        if (choice.chosen) {
            const gf_optim_config oc = choice.step_config(learning_rate, nBatch);
            must(gf_smp_model_optimiser_step(net, NULL, NULL, &oc), "gf_smp_model_optimiser_step");
        } else {
            must(gf_smp_model_adam_step(net, learning_rate, nBatch), "gf_smp_model_adam_step");
        }
        if (with_losses) ret.second = loss_of_batch(nBatch, target);
        return ret;
    }
    void predict_batch(int nBatch, double *predict) { must(gf_smp_model_forward_host(net, NULL, predict, NULL), "gf_smp_model_forward_host"); }
    // the two iterative calls on the prepared batch (SMP_omega_physics.h:730-825): kind 0 BatchLearn, 1 Learn; Adam (gf_smp_model_fit_host).
    // With RisiContraction_18_dropout in the towers (SMP_sigma_pairgraphs_hip, train mode) this is NOT the class's loop draw for draw: the
    // class evaluates the loss with one set of slice masks and draws fresh ones for the forward its reverse sweep starts from; here the
    // reverse sweep starts from the forward that evaluated the loss (one draw per iteration where the class has two).
    std::pair<double, double> fit(int kind, const double *target, int nIterations, double learning_rate, double epsilon) {
        return gfhost::fit_host(gf_smp_model_fit_host, "gf_smp_model_fit_host", net, target, kind, choice.chosen ? choice.optim.kind : 0, nIterations,
                                learning_rate, epsilon, 0.0, this);
    }
    void must(gf_status st, const char *what) {
        if (st != GF_OK) gfhost::die(gfhost::default_context(), what, st);
    }
    void die(const char *msg) {
        std::fprintf(stderr, "SMP_model_hip: %s\n", msg);
        std::abort();
    }
    gf_smp_model *net;
    gfhost::OptimiserChoice choice;
    int towers, maxV[2], nF[2];
    std::vector<int> nV[2], adj[2];
    std::vector<double> feature[2];
};

// one tower: SMP_omega_physics (SMP_omega_physics.h:607-925)
class SMP_omega_physics_hip : public SMP_model_hip {
public:
    SMP_omega_physics_hip(int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures)
        : SMP_model_hip(1, max_nVertices, 0, max_receptive_field, nLevels, nChanels, nFeatures, 0, 0) {}

protected:
    struct gamma_wiring {};
    SMP_omega_physics_hip(gamma_wiring, int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures)
        : SMP_model_hip(1, max_nVertices, 0, max_receptive_field, nLevels, nChanels, nFeatures, 0, 0, 4) {}
    struct theta_wiring {};
    SMP_omega_physics_hip(theta_wiring, int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures)
        : SMP_model_hip(1, max_nVertices, 0, max_receptive_field, nLevels, nChanels, nFeatures, 0, 0, 0, 1) {}

public:
    template <class Graph>
    double getLoss(int nBatch, Graph **molecule, double *target) {
        pack(0, nBatch, molecule);
        prepare(nBatch);
        return loss_of_batch(nBatch, target);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule, double *target, double learning_rate) {
        pack(0, nBatch, molecule);
        prepare(nBatch);
        return learn(nBatch, target, learning_rate, true);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule, double *target, int nIterations, double learning_rate, double epsilon) {
        pack(0, nBatch, molecule);
        prepare(nBatch);
        return fit(0, target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    std::pair<double, double> Learn(Graph *molecule, double target, int nIterations, double learning_rate, double epsilon) {
        pack(0, 1, &molecule);
        prepare(1);
        return fit(1, &target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    void Threaded_BatchLearn(int nBatch, Graph **molecule, double *target, double learning_rate) {
        pack(0, nBatch, molecule);
        prepare(nBatch);
        learn(nBatch, target, learning_rate, false);
    }
    template <class Graph>
    void Threaded_Predict(int nBatch, Graph **molecule, double *predict) {
        pack(0, nBatch, molecule);
        prepare(nBatch);
        predict_batch(nBatch, predict);
    }
    template <class Graph>
    double Predict(Graph *molecule) {
        double y = 0.0;
        Threaded_Predict(1, &molecule, &y);
        return y;
    }
};

class SMP_beta_physics_hip : public SMP_omega_physics_hip {  // no receptive-field cap (SMP_beta_physics.h:31)
public:
    SMP_beta_physics_hip(int max_nVertices, int nLevels, int nChanels, int nFeatures)
        : SMP_omega_physics_hip(max_nVertices, max_nVertices, nLevels, nChanels, nFeatures) {}
};

// two towers: SMP_omega_pairgraphs (SMP_omega_pairgraphs.h:732-1080)
class SMP_omega_pairgraphs_hip : public SMP_model_hip {
public:
    SMP_omega_pairgraphs_hip(int max_nVertices_1, int max_nVertices_2, int max_receptive_field, int nLevels, int nChanels,
                             int nFeatures_1, int nFeatures_2, int nKept = 0)
        : SMP_model_hip(2, max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1, nFeatures_2, nKept) {}

protected:
    struct gamma_wiring {};
    SMP_omega_pairgraphs_hip(gamma_wiring, int max_nVertices_1, int max_nVertices_2, int max_receptive_field, int nLevels, int nChanels,
                             int nFeatures_1, int nFeatures_2)
        : SMP_model_hip(2, max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1, nFeatures_2, 0, 4) {}
    // first-order towers; ccn_1d: CCN_1D's width rule, head and feature normalisation at nChanels_decay
    struct theta_wiring {};
    SMP_omega_pairgraphs_hip(theta_wiring, int max_nVertices_1, int max_nVertices_2, int max_receptive_field, int nLevels, int nChanels,
                             int nFeatures_1, int nFeatures_2, double nChanels_decay = 0.0, bool ccn_1d = false)
        : SMP_model_hip(2, max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1, nFeatures_2, 0, 0, 1,
                        nChanels_decay, ccn_1d) {}

public:
    template <class Graph>
    double getLoss(int nBatch, Graph **molecule_1, Graph **molecule_2, double *target) {
        bind(nBatch, molecule_1, molecule_2);
        return loss_of_batch(nBatch, target);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule_1, Graph **molecule_2, double *target, double learning_rate) {
        bind(nBatch, molecule_1, molecule_2);
        return learn(nBatch, target, learning_rate, true);
    }
    template <class Graph>
    std::pair<double, double> BatchLearn(int nBatch, Graph **molecule_1, Graph **molecule_2, double *target, int nIterations, double learning_rate,
                                         double epsilon) {
        bind(nBatch, molecule_1, molecule_2);
        return fit(0, target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    std::pair<double, double> Learn(Graph *molecule_1, Graph *molecule_2, double target, int nIterations, double learning_rate, double epsilon) {
        bind(1, &molecule_1, &molecule_2);
        return fit(1, &target, nIterations, learning_rate, epsilon);
    }
    template <class Graph>
    void Threaded_BatchLearn(int nBatch, Graph **molecule_1, Graph **molecule_2, double *target, double learning_rate) {
        bind(nBatch, molecule_1, molecule_2);
        learn(nBatch, target, learning_rate, false);
    }
    template <class Graph>
    void Threaded_Predict(int nBatch, Graph **molecule_1, Graph **molecule_2, double *predict) {
        bind(nBatch, molecule_1, molecule_2);
        predict_batch(nBatch, predict);
    }
    template <class Graph>
    double Predict(Graph *molecule_1, Graph *molecule_2) {
        double y = 0.0;
        Threaded_Predict(1, &molecule_1, &molecule_2, &y);
        return y;
    }

private:
    template <class Graph>
    void bind(int nBatch, Graph **m1, Graph **m2) {
        pack(0, nBatch, m1);
        pack(1, nBatch, m2);
        prepare(nBatch);
    }
};

class SMP_beta_pairgraphs_hip : public SMP_omega_pairgraphs_hip {
public:
    SMP_beta_pairgraphs_hip(int max_nVertices_1, int max_nVertices_2, int nLevels, int nChanels, int nFeatures_1, int nFeatures_2)
        : SMP_omega_pairgraphs_hip(max_nVertices_1, max_nVertices_2, max_nVertices_1 > max_nVertices_2 ? max_nVertices_1 : max_nVertices_2,
                                   nLevels, nChanels, nFeatures_1, nFeatures_2) {}
};

// RisiContraction_18_dropout inside the towers (SMP_sigma_pairgraphs.h:81): nKept of the 18 slices in train mode.  Its iterative
// BatchLearn / Learn draw the slice masks once per iteration, not twice as the class does (SMP_model_hip::fit says how).
class SMP_sigma_pairgraphs_hip : public SMP_omega_pairgraphs_hip {
public:
    SMP_sigma_pairgraphs_hip(int max_nVertices_1, int max_nVertices_2, int max_receptive_field, int nLevels, int nChanels,
                             int nFeatures_1, int nFeatures_2, int nKept)
        : SMP_omega_pairgraphs_hip(max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1, nFeatures_2, nKept) {}
};

// SMP_gamma_physics (GraphFlow/SMP_gamma_physics.h): SMP_omega_physics with RisiContraction_4 and K_l [4 C_{l-1}][C_l], no reduced
// adjacency.  The use_coulomb constructor builds the same model: the reference stores the flag and never reads it.
class SMP_gamma_physics_hip : public SMP_omega_physics_hip {
public:
    SMP_gamma_physics_hip(int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures)
        : SMP_omega_physics_hip(gamma_wiring(), max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures) {}
    SMP_gamma_physics_hip(bool use_coulomb, int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures)
        : SMP_omega_physics_hip(gamma_wiring(), max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures) {
        (void)use_coulomb;
    }
};

// SMP_gamma_pairgraphs (GraphFlow/SMP_gamma_pairgraphs.h): SMP_omega_pairgraphs with RisiContraction_4 towers
class SMP_gamma_pairgraphs_hip : public SMP_omega_pairgraphs_hip {
public:
    SMP_gamma_pairgraphs_hip(int max_nVertices_1, int max_nVertices_2, int max_receptive_field, int nLevels, int nChanels, int nFeatures_1,
                             int nFeatures_2)
        : SMP_omega_pairgraphs_hip(gamma_wiring(), max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1,
                                   nFeatures_2) {}
};

// SMP_theta_physics (GraphFlow/SMP_theta_physics.h): one first-order tower (SMP_theta's level, K_l [2 C_{l-1}][C_l], per-size lambda1,
// lambda2, b), channels halving per level, every level read out, the one-hidden-layer head
class SMP_theta_physics_hip : public SMP_omega_physics_hip {
public:
    SMP_theta_physics_hip(int max_nVertices, int max_receptive_field, int nLevels, int nChanels, int nFeatures)
        : SMP_omega_physics_hip(theta_wiring(), max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures) {}
};

// SMP_theta_pairgraphs (GraphFlow/SMP_theta_pairgraphs.h): two such towers and the two-hidden-layer head
class SMP_theta_pairgraphs_hip : public SMP_omega_pairgraphs_hip {
public:
    SMP_theta_pairgraphs_hip(int max_nVertices_1, int max_nVertices_2, int max_receptive_field, int nLevels, int nChanels, int nFeatures_1,
                             int nFeatures_2)
        : SMP_omega_pairgraphs_hip(theta_wiring(), max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1,
                                   nFeatures_2) {}
};

// CCN_1D (GraphFlow/CCN_1D.h): SMP_theta_pairgraphs with widths and head sized by nChanels_decay (at least 16 channels), feature rows
// divided by their L1 norm.  What the class asserts (nChanels >= 16, 0 < nChanels_decay <= 1, the cap within both vertex limits) the
// library refuses, and the constructor aborts with its message.
class CCN_1D_hip : public SMP_omega_pairgraphs_hip {
public:
    CCN_1D_hip(int max_nVertices_1, int max_nVertices_2, int max_receptive_field, int nLevels, int nChanels, int nFeatures_1, int nFeatures_2,
               double nChanels_decay)
        : SMP_omega_pairgraphs_hip(theta_wiring(), max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1,
                                   nFeatures_2, nChanels_decay, true) {}
};

#endif
