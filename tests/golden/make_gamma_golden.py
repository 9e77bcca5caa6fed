#!/usr/bin/env python3
"""Generate tests/golden/smp_gamma.npz from the REAL reference SMP_gamma (GraphFlow/SMP_gamma.h).

Run in the build container only (needs the reference tree):   python tests/golden/make_gamma_golden.py
A small driver (below) that includes SMP_gamma.h from the reference is compiled into a temporary directory outside the
repository and fed through stdin / stdout.  Only data is recorded: inputs, and the reference's prediction, graph feature,
loss and parameter gradients; a three-step BatchLearn (Adam) trajectory; the weights weights_initialization() draws after
srand(seed).  Inputs are float32-representable so the fp32 device path and the fp64 checkers see identical numbers.
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

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "SMP_gamma.h"

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

// Objects are leaked on purpose: the model's and the executor's destructors free the same memory.
int main() {
    char mode[16];
    int maxV, L, C, F, D, wl;
    if (scanf("%15s %d %d %d %d %d %d", mode, &maxV, &L, &C, &F, &D, &wl) != 7) return 1;
    if (mode[0] == 'r') {   // run: one molecule, given parameters -> feature, prediction, loss, gradients
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        SMP_gamma &net = *new SMP_gamma(maxV, L, C, F, D, wl != 0);
        for (size_t i = 0; i < net.sgd->params.size(); ++i)
            for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
        net.complete_computation_graph(g);
        net.target->value[0] = target;
        net.graph->forward();
        net.graph->backward();
        for (int f = 0; f < C; ++f) printf("%.17g ", net.graph_feature->value[f]);
        printf("\n%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
        for (size_t i = 0; i < net.sgd->params.size(); ++i)
            for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", net.sgd->params[i]->gradient[j]);
        printf("\n");
        return 0;
    }
    // learn: srand(seed), the constructor's weights, nIter x BatchLearn(nMol, molecules, targets, lr)
    int seed, nIter, nMol;
    double lr;
    scanf("%d %d %lf %d", &seed, &nIter, &lr, &nMol);
    std::vector<DenseGraph *> mol(nMol);
    std::vector<double> tgt(nMol);
    for (int m = 0; m < nMol; ++m) mol[m] = read_graph(F);
    for (int m = 0; m < nMol; ++m) scanf("%lf", &tgt[m]);
    srand((unsigned)seed);
    SMP_gamma &net = *new SMP_gamma(maxV, L, C, F, D, wl != 0);
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", net.sgd->params[i]->value[j]);
    printf("\n");
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(nMol, &mol[0], &tgt[0], lr);
        printf("%.17g %.17g ", r.first, r.second);
    }
    printf("\n");
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", net.sgd->params[i]->value[j]);
    printf("\n");
    return 0;
}
"""


def gamma_params(C, F, D, L, seed):
    """Random float32-exact parameters in SMP_gamma's registration order: H[C, F(D+1)], (K_l[4C, C], b_l[C]) x L, W[C]."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-1, 1, C * F * (D + 1)) / np.sqrt(F * (D + 1))]
    for _ in range(L):
        parts.append(rng.uniform(-1, 1, 4 * C * C) / np.sqrt(4 * C))
        parts.append(rng.uniform(-0.1, 0.1, C))
    parts.append(rng.uniform(-1, 1, C) / np.sqrt(C))
    return f32exact(np.concatenate(parts))


def graph_text(adj, feat):
    V = len(adj)
    return "%d\n%s\n%s\n" % (V, " ".join(str(int(x)) for x in np.asarray(adj).ravel()),
                             " ".join("%.17g" % x for x in np.asarray(feat, dtype=np.float64).ravel()))


def run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def cases():
    """(tag, adj, feature, target, (L, C, D, wl))"""
    out = []
    for name, adj, feat, tgt in toy_molecules():   # the four hand-built molecules of the reference's SMP tests
        out.append(("toy_" + name, adj, feat, tgt, (2, 6, 3, 1)))
    for seed, nV, L, C, wl in ((301, 9, 2, 6, 1), (302, 14, 3, 5, 1), (303, 12, 3, 4, 0), (304, 17, 4, 4, 1)):
        adj, feat, tgt = synthetic_molecule(seed, nV)
        out.append(("syn%d_L%d" % (nV, L), adj, feat, tgt, (L, C, 2, wl)))
    adj, feat = er_graph(20, 0.15, 4, 5)
    out.append(("er20_L4", adj, feat, 2.5, (4, 4, 2, 1)))
    return out


def main():
    hdr = os.path.join(REF_ROOT, "GraphFlow", "SMP_gamma.h")
    if not os.path.exists(hdr):
        sys.exit("reference not found at %s" % REF_ROOT)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "gamma_driver.cpp"), os.path.join(tmp, "gamma_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for i, (tag, adj, feat, tgt, (L, C, D, wl)) in enumerate(cases()):
            V, F = feat.shape
            params = gamma_params(C, F, D, L, 700 + i)
            maxV = max(V, 10)   # (the toy molecules' max_nVertices in the reference's tests; no field is capped either way)
            text = "run %d %d %d %d %d %d\n" % (maxV, L, C, F, D, wl) + graph_text(adj, feat) + "%.17g\n" % tgt
            text += " ".join("%.17g" % x for x in params) + "\n"
            lines = run(exe, text)
            g = np.array(lines[0].split(), dtype=np.float64)
            pred, loss = (float(x) for x in lines[1].split())
            grads = np.array(lines[2].split(), dtype=np.float64)
            assert grads.size == params.size, (grads.size, params.size)
            p = "gamma_" + tag
            out[p + "__adj"], out[p + "__feature"], out[p + "__target"] = adj.astype(np.int32), feat, np.array([tgt], dtype=np.float64)
            out[p + "__cfg"] = np.array([L, C, D, wl, maxV], dtype=np.int32)
            out[p + "__params"] = params.astype(np.float32)
            out[p + "__graph_feature"], out[p + "__predict"], out[p + "__loss"], out[p + "__grads"] = g, np.array([pred]), np.array([loss]), grads
            tags.append(tag)
        # three BatchLearn steps on the four toy molecules as one batch, from the constructor's weights after srand(13)
        mols = toy_molecules()
        L, C, D, seed, nIter, lr = 2, 6, 3, 13, 3, 1e-3
        F = mols[0][2].shape[1]
        maxV = max(len(m[1]) for m in mols)
        text = "learn %d %d %d %d %d 1\n%d %d %.17g %d\n" % (maxV, L, C, F, D, seed, nIter, lr, len(mols))
        text += "".join(graph_text(adj, feat) for _, adj, feat, _ in mols)
        text += " ".join("%.17g" % t for *_, t in mols) + "\n"
        lines = run(exe, text)
        out["train__cfg"] = np.array([L, C, D, maxV, seed, nIter], dtype=np.int32)
        out["train__lr"] = np.array([lr])
        out["train__targets"] = np.array([t for *_, t in mols], dtype=np.float64)
        out["train__params0"] = np.array(lines[0].split(), dtype=np.float64)
        out["train__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
        out["train__params"] = np.array(lines[2].split(), dtype=np.float64)
    out["tags"] = np.array(tags)
    np.savez_compressed(os.path.join(HERE, "smp_gamma.npz"), **out)
    print("wrote smp_gamma.npz: %d cases + a %d-step BatchLearn trajectory" % (len(tags), nIter))


if __name__ == "__main__":
    main()
