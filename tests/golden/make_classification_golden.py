#!/usr/bin/env python3
"""Generate tests/golden/smp_classification.npz from the REAL reference classifiers
(GraphFlow/SMP_2D_ver6_classification.h, GraphFlow/SMP_2D_ver7_classification.h).

Run in the build container only (needs the reference tree):   python tests/golden/make_classification_golden.py
A small driver (below) that includes the reference header is compiled, once per model, into a temporary directory outside the
repository and fed through stdin / stdout.  Only data is recorded: inputs, and the reference's graph feature, scores
(predict->value), probabilities (LogLoss::probability), loss (LogLoss::value = log p[label], at most 0), parameter gradients and
Predict label; the weights the constructor draws after srand(seed), a three-step BatchLearn (Momentum) trajectory on the four
toy molecules and the labels Predict returns after the reference demo's 1000 epochs.
Inputs are float32-representable so the fp32 device path and the fp64 checkers see identical numbers.

The read-out weights W are scaled so that max |score| <= 2 in the ordinary cases (asserted): the tests' gradient bound rests on
it.  One SATURATED case per model scales W until the gap max(score) - score[label] lies in (150, 600): an fp32 probability is
0 there, the reference's fp64 loss is still finite.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import er_graph, f32exact, synthetic_molecule, toy_molecules  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "/root/reference")
NK = {6: 10, 7: 50}

DRIVER = r"""
#include <cstdio>
#include <vector>
#if VER == 6
#include "SMP_2D_ver6_classification.h"
typedef SMP_2D_ver6_classification Net;
#else
#include "SMP_2D_ver7_classification.h"
typedef SMP_2D_ver7_classification Net;
#endif

static DenseGraph *read_graph(int F) {
    int V;
    if (scanf("%d", &V) != 1) return NULL;
    DenseGraph *g = new DenseGraph(V, F);
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) scanf("%d", &g->adj[i][j]);
    for (int i = 0; i < V; ++i)
        for (int f = 0; f < F; ++f) scanf("%lf", &g->feature[i][f]);
    return g;
}
static void print_params(Net &net, bool gradient) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j)
            printf("%.17g ", gradient ? net.sgd->params[i]->gradient[j] : net.sgd->params[i]->value[j]);
    printf("\n");
}

// Objects are leaked on purpose: the model's and the executor's destructors free the same memory.
int main() {
    char mode[16];
    int nClass, maxV, L, C, F, D, wl;
    if (scanf("%15s %d %d %d %d %d %d %d", mode, &nClass, &maxV, &L, &C, &F, &D, &wl) != 8) return 1;
    if (mode[0] == 'r') {   // run: one molecule, given parameters -> feature, scores, probabilities, loss, gradients, Predict
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        Net &net = *new Net(nClass, maxV, L, C, F, D, 0.9, wl != 0);
        for (size_t i = 0; i < net.sgd->params.size(); ++i)
            for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
        net.complete_computation_graph(g);
        net.target->value[0] = target;
        net.graph->forward();
        net.graph->backward();
        for (int f = 0; f < C; ++f) printf("%.17g ", net.graph_feature->value[f]);
        printf("\n");
        for (int c = 0; c < nClass; ++c) printf("%.17g ", net.predict->value[c]);
        printf("\n");
        for (int c = 0; c < nClass; ++c) printf("%.17g ", net.logl->probability[c]);
        printf("\n%.17g\n", net.logl->getLoss());
        print_params(net, true);
        printf("%.17g\n", net.Predict(g));
        return 0;
    }
    // learn: srand(seed), the constructor's weights, nIter x BatchLearn(nMol, molecules, targets, lr) recorded, then BatchLearn up to
    // nEpochs in all and Predict on every molecule
    int seed, nIter, nEpochs, nMol;
    double lr;
    scanf("%d %d %d %lf %d", &seed, &nIter, &nEpochs, &lr, &nMol);
    std::vector<DenseGraph *> mol(nMol);
    std::vector<double> tgt(nMol);
    for (int m = 0; m < nMol; ++m) mol[m] = read_graph(F);
    for (int m = 0; m < nMol; ++m) scanf("%lf", &tgt[m]);
    srand((unsigned)seed);
    Net &net = *new Net(nClass, maxV, L, C, F, D, 0.9, wl != 0);
    print_params(net, false);
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(nMol, &mol[0], &tgt[0], lr);
        printf("%.17g %.17g ", r.first, r.second);
    }
    printf("\n");
    print_params(net, false);
    std::pair<double, double> last(0, 0);
    for (int it = nIter; it < nEpochs; ++it) last = net.BatchLearn(nMol, &mol[0], &tgt[0], lr);
    printf("%.17g %.17g\n", last.first, last.second);
    for (int m = 0; m < nMol; ++m) printf("%.17g ", net.Predict(mol[m]));
    printf("\n");
    return 0;
}
"""


def class_params(nK, nClass, C, F, D, L, seed):
    """Random float32-exact parameters in registration order: H[C, F(D+1)], (K_l[C, nK C], b_l[C]) x L, W[nClass, C]."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-1, 1, C * F * (D + 1)) / np.sqrt(F * (D + 1))]
    for _ in range(L):
        parts.append(rng.uniform(-1, 1, nK * C * C) / np.sqrt(nK * C))
        parts.append(rng.uniform(-0.1, 0.1, C))
    parts.append(rng.uniform(-1, 1, nClass * C) / np.sqrt(C))
    return f32exact(np.concatenate(parts))


def graph_text(adj, feat):
    V = len(adj)
    return "%d\n%s\n%s\n" % (V, " ".join(str(int(x)) for x in np.asarray(adj).ravel()),
                             " ".join("%.17g" % x for x in np.asarray(feat, dtype=np.float64).ravel()))


def run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def cases():
    """(tag, adj, feature, label, (nClass, L, C, D, wl, maxV), saturated)"""
    out = []
    for name, adj, feat, tgt in toy_molecules():   # the reference test's molecules and hyper-parameters: label = atom count
        out.append(("toy_" + name, adj, feat, int(tgt), (11, 1, 10, 5, 1, 10), False))
    for seed, nV, L, C, wl in ((401, 9, 2, 6, 1), (402, 12, 3, 4, 0), (403, 11, 2, 5, 0), (404, 10, 3, 4, 1)):
        adj, feat, _ = synthetic_molecule(seed, nV)
        out.append(("syn%d_L%d_wl%d" % (nV, L, wl), adj, feat, nV % 7, (7, L, C, 2, wl, nV), False))
    adj, feat = er_graph(20, 0.15, 4, 5)
    out.append(("er20_L2", adj, feat, 3, (5, 2, 4, 2, 1, 20), False))
    name, adj, feat, tgt = toy_molecules()[0]
    out.append(("saturated_" + name, adj, feat, None, (11, 1, 4, 5, 1, 10), True))   # (label: the lowest score, chosen below)
    return out


def run_case(exe, adj, feat, label, cfg, params):
    nClass, L, C, D, wl, maxV = cfg
    F = feat.shape[1]
    text = "run %d %d %d %d %d %d %d\n" % (nClass, maxV, L, C, F, D, wl) + graph_text(adj, feat) + "%d\n" % label
    text += " ".join("%.17g" % x for x in params) + "\n"
    lines = run(exe, text)
    rec = {"graph_feature": np.array(lines[0].split(), dtype=np.float64), "scores": np.array(lines[1].split(), dtype=np.float64),
           "probability": np.array(lines[2].split(), dtype=np.float64), "loss": np.array([float(lines[3])]),
           "grads": np.array(lines[4].split(), dtype=np.float64), "label": np.array([int(float(lines[5]))], dtype=np.int32)}
    assert rec["grads"].size == params.size and rec["scores"].size == nClass, (rec["grads"].size, params.size)
    return rec


def main():
    if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", "SMP_2D_ver6_classification.h")):
        sys.exit("reference not found at %s" % REF_ROOT)
    out, tags = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for ver in (6, 7):
            src, exe = os.path.join(tmp, "cls_driver.cpp"), os.path.join(tmp, "cls_driver_v%d" % ver)
            with open(src, "w") as f:
                f.write(DRIVER)
            subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-DVER=%d" % ver, "-I", os.path.join(REF_ROOT, "GraphFlow"),
                                   "-o", exe, src])
            nK = NK[ver]
            # the four toy molecules share ONE parameter vector (recorded once: at RisiContraction_50's 50 x 10 x 10 weights four copies
            # would be a quarter of the file), its W scaled by the largest score over the four
            toys = [c for c in cases() if c[0].startswith("toy_")]
            nClass, L, C, D, wl, maxV = toys[0][4]
            toy_params = class_params(nK, nClass, C, toys[0][2].shape[1], D, L, 900 + 20 * ver)
            zmax = max(np.abs(run_case(exe, adj, feat, label, cfg, toy_params)["scores"]).max() for _, adj, feat, label, cfg, _ in toys)
            toy_params[-nClass * C:] = f32exact(toy_params[-nClass * C:] * (1.5 / zmax))
            toy_first = "v%d_%s" % (ver, toys[0][0])
            for i, (tag, adj, feat, label, cfg, saturated) in enumerate(cases()):
                nClass, L, C, D, wl, maxV = cfg
                F = feat.shape[1]
                nW = nClass * C
                if tag.startswith("toy_"):
                    params = toy_params
                else:
                    params = class_params(nK, nClass, C, F, D, L, 900 + 20 * ver + i)
                    # the scores are linear in W: one run to see them, then W scaled (and rounded to float32) and the recorded run
                    probe = run_case(exe, adj, feat, 0 if label is None else label, cfg, params)
                    z = probe["scores"]
                    if saturated:
                        label = int(np.argmin(z))
                        factor = 300.0 / (z.max() - z[label])
                    else:
                        factor = 1.5 / np.abs(z).max()
                    params[-nW:] = f32exact(params[-nW:] * factor)
                rec = run_case(exe, adj, feat, label, cfg, params)
                z = rec["scores"]
                if saturated:
                    gap = z.max() - z[label]
                    assert 150.0 < gap < 600.0, gap
                    assert np.float32(np.exp(np.float32(-gap))) == 0 and np.isfinite(rec["loss"][0]) and abs(rec["loss"][0] + gap) < 5.0
                else:
                    assert np.abs(z).max() <= 2.0, np.abs(z).max()
                p = "v%d_%s" % (ver, tag)
                out[p + "__adj"], out[p + "__feature"] = adj.astype(np.int32), feat
                out[p + "__target"] = np.array([label], dtype=np.int32)
                out[p + "__cfg"] = np.array([nClass, L, C, D, wl, maxV, nK, 1 if saturated else 0], dtype=np.int32)
                if tag.startswith("toy_") and p != toy_first:
                    out[p + "__params_from"] = np.array(toy_first)   # (the tag whose __params these are)
                else:
                    out[p + "__params"] = params.astype(np.float32)
                for k, v in rec.items():
                    out[p + "__" + k] = v
                tags.append(p)
            # the reference demo (tests/test_SMP_2D_ver6_classification.cpp): four toy molecules as one batch, from the constructor's
            # weights after srand(seed); three recorded BatchLearn steps, 1000 epochs in all, then Predict
            mols = toy_molecules()
            nClass, L, C, D, maxV, seed, nIter, nEpochs, lr = 11, 1, 10, 5, 10, 17, 3, 1000, 1e-3
            F = mols[0][2].shape[1]
            text = "learn %d %d %d %d %d %d 1\n%d %d %d %.17g %d\n" % (nClass, maxV, L, C, F, D, seed, nIter, nEpochs, lr, len(mols))
            text += "".join(graph_text(adj, feat) for _, adj, feat, _ in mols)
            text += " ".join("%d" % int(t) for *_, t in mols) + "\n"
            lines = run(exe, text)
            p = "v%d_train" % ver
            out[p + "__cfg"] = np.array([nClass, L, C, D, maxV, seed, nIter, nEpochs, nK], dtype=np.int32)
            out[p + "__lr"] = np.array([lr, 0.9])
            out[p + "__targets"] = np.array([int(t) for *_, t in mols], dtype=np.int32)
            out[p + "__params0"] = np.array(lines[0].split(), dtype=np.float64).astype(np.float32)   # (what an fp32 model starts from)
            out[p + "__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
            out[p + "__params"] = np.array(lines[2].split(), dtype=np.float64).astype(np.float32)
            out[p + "__last_losses"] = np.array(lines[3].split(), dtype=np.float64)
            out[p + "__labels_trained"] = np.array([int(float(x)) for x in lines[4].split()], dtype=np.int32)
    out["tags"] = np.array(tags)
    path = os.path.join(HERE, "smp_classification.npz")
    np.savez_compressed(path, **out)
    print("wrote smp_classification.npz: %d cases + two BatchLearn trajectories, %d bytes" % (len(tags), os.path.getsize(path)))
    for ver in (6, 7):
        print("ver%d: losses %s, after %d epochs %s, Predict %s" % (ver, out["v%d_train__losses" % ver].ravel(), 1000,
                                                                  out["v%d_train__last_losses" % ver], out["v%d_train__labels_trained" % ver]))


if __name__ == "__main__":
    main()
