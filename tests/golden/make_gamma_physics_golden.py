#!/usr/bin/env python3
"""Generate tests/golden/smp_gamma_physics.npz from the REAL reference SMP_gamma_physics / SMP_gamma_pairgraphs
(GraphFlow/SMP_gamma_physics.h, GraphFlow/SMP_gamma_pairgraphs.h).

Run in the build container only (needs the reference tree):   python tests/golden/make_gamma_physics_golden.py
As make_gamma_golden.py: a small driver that includes the two headers is compiled into a temporary directory outside the
repository and fed through stdin / stdout.  Only data is recorded.  Per case: inputs (float32-exact), parameters, the receptive
fields ([L+1][V][cap+1], slot 0 = size, as gf_smp_prepare_molecule_host writes them), the concatenated feature row, predict,
loss and every parameter gradient.  Per class: the weights weights_initialization() draws after srand(seed) and a three-step
BatchLearn (Adam) loss trajectory on the toy molecules of the reference's test programs.
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
#include "SMP_gamma_physics.h"
#include "SMP_gamma_pairgraphs.h"

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

template <class Lv>
static void print_phi(Lv **level, int L, int V) {
    for (int l = 0; l <= L; ++l)
        for (int v = 0; v < V; ++v) {
            printf("%d ", (int)level[l]->phi[v].size());
            for (size_t i = 0; i < level[l]->phi[v].size(); ++i) printf("%d ", level[l]->phi[v][i]);
        }
    printf("\n");
}

template <class Net>
static void print_run(Net &net) {
    for (int f = 0; f < net.graph_feature->size; ++f) printf("%.17g ", net.graph_feature->value[f]);
    printf("\n%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", net.sgd->params[i]->gradient[j]);
    printf("\n");
}

template <class Net>
static void print_params(Net &net) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", net.sgd->params[i]->value[j]);
    printf("\n");
}

template <class Net>
static void read_params(Net &net) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
}

// Objects are leaked on purpose: the models' and the executors' destructors free the same memory.
int main() {
    char mode[16];
    int towers, maxV1, maxV2, cap, L, C, F1, F2;
    if (scanf("%15s %d %d %d %d %d %d %d %d", mode, &towers, &maxV1, &maxV2, &cap, &L, &C, &F1, &F2) != 9) return 1;
    if (mode[0] == 'r') {   // run: one sample, given parameters -> fields, feature row, prediction, loss, gradients
        DenseGraph *g1 = read_graph(F1), *g2 = towers == 2 ? read_graph(F2) : NULL;
        double target;
        scanf("%lf", &target);
        if (towers == 1) {
            SMP_gamma_physics &net = *new SMP_gamma_physics(maxV1, cap, L, C, F1);
            read_params(net);
            net.complete_computation_graph(g1);
            net.target->value[0] = target;
            net.graph->forward();
            net.graph->backward();
            print_phi(net.level, L, g1->nVertices);
            print_run(net);
        } else {
            SMP_gamma_pairgraphs &net = *new SMP_gamma_pairgraphs(maxV1, maxV2, cap, L, C, F1, F2);
            read_params(net);
            net.complete_computation_graph(g1, g2);
            net.target->value[0] = target;
            net.graph->forward();
            net.graph->backward();
            print_phi(net.level_1, L, g1->nVertices);
            print_phi(net.level_2, L, g2->nVertices);
            print_run(net);
        }
        return 0;
    }
    // learn: srand(seed), the constructor's weights, nIter x BatchLearn(nMol, molecules, targets, lr)
    int seed, nIter, nMol;
    double lr;
    scanf("%d %d %lf %d", &seed, &nIter, &lr, &nMol);
    std::vector<DenseGraph *> m1(nMol), m2(nMol);
    std::vector<double> tgt(nMol);
    for (int m = 0; m < nMol; ++m) m1[m] = read_graph(F1);
    if (towers == 2)
        for (int m = 0; m < nMol; ++m) m2[m] = read_graph(F2);
    for (int m = 0; m < nMol; ++m) scanf("%lf", &tgt[m]);
    srand((unsigned)seed);
    if (towers == 1) {
        SMP_gamma_physics &net = *new SMP_gamma_physics(maxV1, cap, L, C, F1);
        print_params(net);
        for (int it = 0; it < nIter; ++it) {
            std::pair<double, double> r = net.BatchLearn(nMol, &m1[0], &tgt[0], lr);
            printf("%.17g %.17g ", r.first, r.second);
        }
        printf("\n");
        print_params(net);
    } else {
        SMP_gamma_pairgraphs &net = *new SMP_gamma_pairgraphs(maxV1, maxV2, cap, L, C, F1, F2);
        print_params(net);
        for (int it = 0; it < nIter; ++it) {
            std::pair<double, double> r = net.BatchLearn(nMol, &m1[0], &m2[0], &tgt[0], lr);
            printf("%.17g %.17g ", r.first, r.second);
        }
        printf("\n");
        print_params(net);
    }
    return 0;
}
"""


def channels(C, L):
    return [max(1, C >> l) for l in range(L + 1)]


def tower_params(C, F, L):
    """H[C, F], then (K_l[4 C_{l-1}, C_l], b_l[C_l]) for l = 1..L."""
    c = channels(C, L)
    return C * F + sum(4 * c[l - 1] * c[l] + c[l] for l in range(1, L + 1))


def model_params(towers, C, L, F1, F2):
    w = sum(channels(C, L))
    if towers == 1:
        nh = w // 2
        return tower_params(C, F1, L) + nh * w + nh
    nTot = 2 * w
    h1 = max(nTot // 2, 10)
    h2 = max(h1 // 2, 10)
    return tower_params(C, F1, L) + tower_params(C, F2, L) + h1 * nTot + h2 * h1 + h2


def graph_text(adj, feat):
    V = len(adj)
    return "%d\n%s\n%s\n" % (V, " ".join(str(int(x)) for x in np.asarray(adj).ravel()),
                             " ".join("%.17g" % x for x in np.asarray(feat, dtype=np.float64).ravel()))


def run(exe, text):
    return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def parse_phi(line, L, V, cap):
    vals = [int(x) for x in line.split()]
    phi = np.full((L + 1, V, cap + 1), -1, dtype=np.int32)
    k = 0
    for l in range(L + 1):
        for v in range(V):
            n = vals[k]
            phi[l, v, 0] = n
            phi[l, v, 1:1 + n] = vals[k + 1:k + 1 + n]
            k += 1 + n
    assert k == len(vals)
    return phi


def cases():
    """(tag, towers, (adj, feat), (adj2, feat2) or None, target, L, C, cap)"""
    g12 = synthetic_molecule(5, 12)
    g9 = synthetic_molecule(6, 9)
    g17 = synthetic_molecule(9, 17)
    er40 = er_graph(40, 0.1, 5, 41)
    er10 = er_graph(10, 0.3, 3, 42)
    return [
        ("phys_ref_c16", 1, g12[:2], None, g12[2], 3, 16, 4),       # the reference test program's configuration
        ("phys_c10", 1, g17[:2], None, g17[2], 3, 10, 8),           # widths 10 / 5 / 2 / 1
        ("phys_big40", 1, er40, None, 7.5, 3, 8, 40),              # fields of 33 - 40 positions
        ("pair_ref_c16", 2, g12[:2], g9[:2], g12[2], 3, 16, 6),     # the reference test program's configuration
        ("pair_c10_f53", 2, g17[:2], er10, 4.0, 3, 10, 6),          # odd widths, nFeatures 5 and 3
    ]


def main():
    for h in ("SMP_gamma_physics.h", "SMP_gamma_pairgraphs.h"):
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %s" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(9404)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "gamma_physics_driver.cpp"), os.path.join(tmp, "gamma_physics_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        for tag, towers, ga, gb, tgt, L, C, cap in cases():
            V1, F1 = ga[1].shape
            V2, F2 = gb[1].shape if gb else (0, 0)
            maxV1, maxV2 = max(V1, 10), max(V2, 10)
            params = f32exact(rng.uniform(-0.3, 0.3, model_params(towers, C, L, F1, F2)))
            text = "run %d %d %d %d %d %d %d %d\n" % (towers, maxV1, maxV2, cap, L, C, F1, F2) + graph_text(*ga)
            if gb:
                text += graph_text(*gb)
            text += "%.17g\n" % tgt + " ".join("%.17g" % x for x in params) + "\n"
            lines = run(exe, text)
            p = "gphys_" + tag
            out[p + "__phi"] = parse_phi(lines[0], L, V1, cap)
            if gb:
                out[p + "__phi2"] = parse_phi(lines[1], L, V2, cap)
                lines = lines[1:]
            g = np.array(lines[1].split(), dtype=np.float64)
            pred, loss = (float(x) for x in lines[2].split())
            grads = np.array(lines[3].split(), dtype=np.float64)
            assert grads.size == params.size, (tag, grads.size, params.size)
            assert g.size == towers * sum(channels(C, L)), (tag, g.size)
            out[p + "__adj"], out[p + "__feature"] = ga[0].astype(np.int32), ga[1]
            if gb:
                out[p + "__adj2"], out[p + "__feature2"] = gb[0].astype(np.int32), gb[1]
            out[p + "__target"] = np.array([tgt], dtype=np.float64)
            out[p + "__cfg"] = np.array([towers, L, C, cap, maxV1, maxV2], dtype=np.int32)
            out[p + "__params"] = params.astype(np.float32)
            out[p + "__graph_feature"], out[p + "__predict"], out[p + "__loss"] = g, np.array([pred]), np.array([loss])
            out[p + "__grads"] = grads.astype(np.float32)   # (fp32 keeps the file small; tests compare at 1e-5)
            print("%-14s fields up to %d positions, %d parameters, predict %.6g" % (tag, int(out[p + "__phi"][..., 0].max()), params.size, pred))
        # three BatchLearn steps on the toy molecules of the reference's test programs, from the weights the constructors draw after
        # srand(7): physics C = 16, L = 3, cap 4 on the four molecules; pairgraphs cap 6 on all 16 ordered pairs (target = difference
        # of the atom counts)
        mols = [(a, f) for _, a, f, _ in toy_molecules()]
        tg = [t for *_, t in toy_molecules()]
        L, C, maxV, seed, nIter, lr = 3, 16, 10, 7, 3, 1e-3
        for name, towers, cap, m1, m2, t in (("trainphys", 1, 4, mols, None, tg),
                                             ("trainpair", 2, 6, [mols[i] for i in range(4) for j in range(4)],
                                              [mols[j] for i in range(4) for j in range(4)], [tg[i] - tg[j] for i in range(4) for j in range(4)])):
            text = "learn %d %d %d %d %d %d 4 4\n%d %d %.17g %d\n" % (towers, maxV, maxV, cap, L, C, seed, nIter, lr, len(m1))
            text += "".join(graph_text(a, f) for a, f in m1)
            if m2:
                text += "".join(graph_text(a, f) for a, f in m2)
            text += " ".join("%.17g" % x for x in t) + "\n"
            lines = run(exe, text)
            out[name + "__cfg"] = np.array([towers, L, C, cap, maxV, seed, nIter], dtype=np.int32)
            out[name + "__lr"] = np.array([lr])
            out[name + "__targets"] = np.array(t, dtype=np.float64)
            out[name + "__params0"] = np.array(lines[0].split(), dtype=np.float64).astype(np.float32)   # (what the fp32 model holds)
            out[name + "__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
            assert out[name + "__params0"].size == model_params(towers, C, L, 4, 4)
            print("%s: losses %s" % (name, out[name + "__losses"].ravel().tolist()))
    path = os.path.join(HERE, "smp_gamma_physics.npz")
    np.savez_compressed(path, **out)
    print("wrote smp_gamma_physics.npz: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
