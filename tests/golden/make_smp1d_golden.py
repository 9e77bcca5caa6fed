#!/usr/bin/env python3
"""Generate tests/golden/smp_1d.npz from the REAL reference classes SMP_1D, SMP_1D_ver2, SMP_1D_ver3, SMP_1D_classification and
SMP_1D_ver3_classification (GraphFlow/SMP_1D*.h).

Run where the reference tree is available:   python tests/golden/make_smp1d_golden.py
A small driver (below) that only includes the five reference headers is compiled into a temporary directory outside the repository and
fed through stdin / stdout.  Only data is recorded: the inputs, the receptive fields per level, the reference's graph feature,
prediction (scores, probabilities and arg-max label for the classifiers), loss and parameter gradients, the weights
weights_initialization() draws after srand(seed) for each of the five classes, and a three-step BatchLearn (Momentum) trajectory of
SMP_1D_ver3.  Inputs are float32-representable so the fp32 device path and the fp64 checkers see identical numbers.

Every fixture passes two asserts here: the read-out's worst-case fp32 rounding stays under half of the suite's 1e-5, and no
pre-activation (level 0, the levels, the read-out's column sums) lies within 1e-3 max|z| of zero, so that fp32 cannot take the other
branch of a LeakyReLU -- which at the slope 0 of SMP_1D_ver2 / ver3 would switch a gradient off.  Parameters are redrawn until the
second holds; the smallest margin kept is printed.  A pre-activation that is EXACTLY zero is not counted: at slope 0 whole columns of
a field are switched off, their sums (the read-out's column sums, the S of the level above) are sums of exact zeros in fp32 as in fp64,
and both formats take the same branch there -- provided the switched-off values themselves keep the margin, which is what is asserted.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "/root/reference")
HEADERS = ("SMP_1D.h", "SMP_1D_ver2.h", "SMP_1D_ver3.h", "SMP_1D_classification.h", "SMP_1D_ver3_classification.h")
MARGIN = 1e-3      # smallest |z| / max |z| a fixture may hold
MOMENTUM = 0.9

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
// (every one of the five headers defines a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_SMP_1D
#include "SMP_1D.h"
#undef INF
#define INF INF_of_SMP_1D_ver2
#include "SMP_1D_ver2.h"
#undef INF
#define INF INF_of_SMP_1D_ver3
#include "SMP_1D_ver3.h"
#undef INF
#define INF INF_of_SMP_1D_classification
#include "SMP_1D_classification.h"
#undef INF
#define INF INF_of_SMP_1D_ver3_classification
#include "SMP_1D_ver3_classification.h"
#undef INF

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

static double zmin = 1e300, zmax = 0.0;
static void margins(const double *z, int n) {
    for (int i = 0; i < n; ++i) {
        const double a = fabs(z[i]);
        if (a == 0.0) continue;   // a sum of switched-off activations (slope 0): exactly zero in fp32 as well, the same branch in both
        if (a < zmin) zmin = a;
        if (a > zmax) zmax = a;
    }
}

template <class Net>
static void print_params(Net &net, bool grads) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", grads ? net.sgd->params[i]->gradient[j] : net.sgd->params[i]->value[j]);
    printf("\n");
}

template <class Net>
static void run_common(Net &net, DenseGraph *g, double target, int L) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
    net.complete_computation_graph(g);
    net.target->value[0] = target;
    net.graph->forward();
    net.graph->backward();
    const int V = g->nVertices;
    for (int l = 0; l <= L; ++l)
        for (int v = 0; v < V; ++v) {
            printf("%d ", (int)net.level[l]->phi[v].size());
            for (size_t i = 0; i < net.level[l]->phi[v].size(); ++i) printf("%d ", net.level[l]->phi[v][i]);
            if (l == 0) margins(net.level[0]->f_transpose[v]->value, net.level[0]->f_transpose[v]->size);
            else margins(net.level[l]->add[v]->value, net.level[l]->add[v]->size);
            if (l == L) margins(net.shrinked[v]->value, net.shrinked[v]->size);
        }
    printf("\n");
    for (int f = 0; f < net.graph_feature->size; ++f) printf("%.17g ", net.graph_feature->value[f]);
    printf("\n");
}

template <class Net>
static void run_regression(Net &net, DenseGraph *g, double target, int L) {
    run_common(net, g, target, L);
    printf("%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
    print_params(net, true);
    printf("%.17g %.17g\n", zmin, zmax);
}

template <class Net>
static void run_classifier(Net &net, DenseGraph *g, double target, int L, int nClass) {
    run_common(net, g, target, L);
    for (int c = 0; c < nClass; ++c) printf("%.17g ", net.predict->value[c]);
    printf("\n");
    for (int c = 0; c < nClass; ++c) printf("%.17g ", net.logl->probability[c]);
    printf("\n%.17g\n", net.logl->getLoss());
    print_params(net, true);
    printf("%.17g %.17g\n", zmin, zmax);
    printf("%.17g\n", net.Predict(g));
}

template <class Net>
static void learn(Net &net, int nIter, int nMol, DenseGraph **m, double *tgt, double lr) {
    print_params(net, false);
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(nMol, m, tgt, lr);
        printf("%.17g %.17g ", r.first, r.second);
    }
    printf("\n");
    print_params(net, false);
}

// kind 1: SMP_1D, 2: SMP_1D_ver2, 3: SMP_1D_ver3, 4: SMP_1D_classification, 5: SMP_1D_ver3_classification.  Objects are leaked on
// purpose: the models' and the executors' destructors free the same memory.
int main() {
    char mode[16];
    int kind, nClass, maxV, L, C, F, D, wl;
    double mom;
    if (scanf("%15s %d %d %d %d %d %d %d %d %lf", mode, &kind, &nClass, &maxV, &L, &C, &F, &D, &wl, &mom) != 10) return 1;
    if (mode[0] == 'r') {   // run: one sample, given parameters
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        if (kind == 1) run_regression(*new SMP_1D(maxV, L, C, F, D, mom, wl != 0), g, target, L);
        else if (kind == 2) run_regression(*new SMP_1D_ver2(maxV, L, C, F, D, mom, wl != 0), g, target, L);
        else if (kind == 3) run_regression(*new SMP_1D_ver3(maxV, L, C, F, D, mom, wl != 0), g, target, L);
        else if (kind == 4) run_classifier(*new SMP_1D_classification(nClass, maxV, L, C, F, D, mom, wl != 0), g, target, L, nClass);
        else run_classifier(*new SMP_1D_ver3_classification(nClass, maxV, L, C, F, D, mom, wl != 0), g, target, L, nClass);
        return 0;
    }
    // learn: srand(seed), the constructor's weights, nIter x BatchLearn(nMol, molecules, targets, lr)  (nIter 0: the weights only)
    int seed, nIter, nMol;
    double lr;
    scanf("%d %d %lf %d", &seed, &nIter, &lr, &nMol);
    std::vector<DenseGraph *> m(nMol);
    std::vector<double> tgt(nMol);
    for (int i = 0; i < nMol; ++i) m[i] = read_graph(F);
    for (int i = 0; i < nMol; ++i) scanf("%lf", &tgt[i]);
    srand((unsigned)seed);
    if (kind == 1) learn(*new SMP_1D(maxV, L, C, F, D, mom, wl != 0), nIter, nMol, &m[0], &tgt[0], lr);
    else if (kind == 2) learn(*new SMP_1D_ver2(maxV, L, C, F, D, mom, wl != 0), nIter, nMol, &m[0], &tgt[0], lr);
    else if (kind == 3) learn(*new SMP_1D_ver3(maxV, L, C, F, D, mom, wl != 0), nIter, nMol, &m[0], &tgt[0], lr);
    else if (kind == 4) learn(*new SMP_1D_classification(nClass, maxV, L, C, F, D, mom, wl != 0), nIter, nMol, &m[0], &tgt[0], lr);
    else learn(*new SMP_1D_ver3_classification(nClass, maxV, L, C, F, D, mom, wl != 0), nIter, nMol, &m[0], &tgt[0], lr);
    return 0;
}
"""


def channels(version, C, L):
    """channel count per level: constant for SMP_1D (version 1), doubling for SMP_1D_ver2 / ver3"""
    return [C if version == 1 else C << l for l in range(L + 1)]


def smp1d_blocks(version, C, FD, L, maxV, nClass=0):
    """[(block name, size)] in registration order: H; per level (lambda1_s, lambda2_s, b_s[C_l]) for s = 1..maxV, then for version 3
    K_eye[C_{l-1}, C_{l-1}] and K_one[C_{l-1}, C_{l-1}]; W[C_L] or, for a classifier, W[nClass, C_L]."""
    c = channels(version, C, L)
    out = [("H", C * FD)]
    for l in range(1, L + 1):
        for s in range(1, maxV + 1):
            out += [("lam1_%d_%d" % (l, s), 1), ("lam2_%d_%d" % (l, s), 1), ("b_%d_%d" % (l, s), c[l])]
        if version == 3:
            out += [("Keye_%d" % l, c[l - 1] * c[l - 1]), ("Kone_%d" % l, c[l - 1] * c[l - 1])]
    out.append(("W", max(nClass, 1) * c[L]))
    return out


def random_params(blocks, rng, nClass=0):
    """float32-exact parameters, scaled by fan-in as the SMP_theta fixtures are: lambda2_s multiplies a sum over the s positions, the
    matrices have about sqrt(n) inputs per output, the read-out weights C_L."""
    parts = []
    for name, n in blocks:
        if name.startswith("lam"):
            size = int(name.rsplit("_", 1)[1]) if name.startswith("lam2") else 1
            parts.append(rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n) / (2.0 * size))
        elif name.startswith("b_"):
            # (bounded away from zero: at slope 0 a position whose inputs are all switched off has z = b exactly)
            parts.append(rng.uniform(0.05, 0.15, n) * rng.choice([-1.0, 1.0], n))
        elif name == "W":
            parts.append(rng.uniform(-1, 1, n) / np.sqrt(n / max(nClass, 1)))
        else:
            parts.append(rng.uniform(-1, 1, n) / np.sqrt(np.sqrt(n)))
    return f32exact(np.concatenate(parts))


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


def cycle_molecule(V=4, F=4):
    """a ring: every vertex has the same field size at every level -- V vertices share one lambda_s, which tells the multiplicities
    j, j (j + 1) (j + 2) / 6 and 1 apart"""
    adj = np.zeros((V, V), dtype=np.int32)
    for v in range(V):
        adj[v, (v + 1) % V] = adj[(v + 1) % V, v] = 1
    feat = np.zeros((V, F))
    feat[np.arange(V), np.arange(V) % F] = 1.0
    feat[0, 1] = 0.5
    return adj, feat, float(V)


def star_molecule(deg, F=4):
    adj = np.zeros((deg + 1, deg + 1), dtype=np.int32)
    adj[0, 1:] = adj[1:, 0] = 1
    feat = np.zeros((deg + 1, F))
    feat[0, 0] = 1.0
    feat[1:, 1] = 1.0
    feat[2, 2] = 0.5   # (leaves that differ: their WL ranks do too)
    return adj, feat, float(deg + 1)


def molecules():
    """(name, adj, feature, target, wl): the four toy molecules, the 4-cycle, the 5-leaf star, a 12-vertex synthetic molecule twice"""
    out = [(n, a, f, t, 1) for n, a, f, t in toy_molecules()]
    out.append(("cycle4",) + cycle_molecule() + (1,))
    out.append(("star5",) + star_molecule(5) + (1,))
    a, f, t = synthetic_molecule(5, 12)
    out.append(("syn12", a, f, t, 1))
    out.append(("syn12_nowl", a, f, t, 0))
    return out


VERSION_CHANNELS = {1: (4, 3, 5), 2: (4, 3), 3: (4, 3)}   # 3: a float2 at columns 2, 3 would straddle the halves; 5: one float per lane
L_ALL, D_ALL, MAXV = 2, 1, 12
N_CLASS = 5


def head(kind, nClass, maxV, L, C, F, D, wl):
    return "%d %d %d %d %d %d %d %d %.17g\n" % (kind, nClass, maxV, L, C, F, D, wl, MOMENTUM)


def record(exe, rng, kind, version, nClass, adj, feat, tgt, L, C, D, wl, maxV):
    """one fixture: parameters are redrawn until the pre-activation margin holds"""
    V, F = feat.shape
    blocks = smp1d_blocks(version, C, F * (D + 1), L, maxV, nClass)
    CL = channels(version, C, L)[L]
    for attempt in range(2000):
        params = random_params(blocks, rng, nClass)
        text = "run " + head(kind, nClass, maxV, L, C, F, D, wl) + graph_text(adj, feat) + "%.17g\n" % tgt
        text += " ".join("%.17g" % x for x in params) + "\n"
        lines = run(exe, text)
        rec = {"phi": parse_phi(lines[0], L, V, maxV), "graph_feature": np.array(lines[1].split(), dtype=np.float64)}
        if nClass:
            rec["scores"] = np.array(lines[2].split(), dtype=np.float64)
            rec["probability"] = np.array(lines[3].split(), dtype=np.float64)
            rec["loss"] = np.array([float(lines[4])])
            rec["grads"] = np.array(lines[5].split(), dtype=np.float64)
            zmin, zmax = (float(x) for x in lines[6].split())
            rec["label"] = np.array([int(float(lines[7]))], dtype=np.int32)
            out_scale = max(1.0, np.abs(rec["scores"]).max())
            worst = np.abs(params[-nClass * CL:].reshape(nClass, CL) * rec["graph_feature"][None, :]).sum(1).max()
        else:
            pred, loss = (float(x) for x in lines[2].split())
            rec["predict"], rec["loss"] = np.array([pred]), np.array([loss])
            rec["grads"] = np.array(lines[3].split(), dtype=np.float64)
            zmin, zmax = (float(x) for x in lines[4].split())
            out_scale = max(1.0, abs(pred))
            worst = np.abs(rec["graph_feature"] * params[-CL:]).sum()
        assert rec["grads"].size == params.size and rec["graph_feature"].size == CL, (rec["grads"].size, params.size)
        if zmin < MARGIN * zmax or worst * 2.0 ** -24 * CL > 5e-6 * out_scale:
            continue
        rec.update(adj=adj.astype(np.int32), feature=feat, target=np.array([tgt], dtype=np.float64), params=params.astype(np.float32),
                   cfg=np.array([version, L, C, D, wl, maxV, nClass], dtype=np.int32), margin=np.array([zmin / zmax]))
        return rec, attempt
    raise AssertionError("no draw with a pre-activation margin of %g" % MARGIN)


def main():
    for h in HEADERS:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %s" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(1901)
    worst_margin = 1.0
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "smp1d_driver.cpp"), os.path.join(tmp, "smp1d_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for version in (1, 2, 3):
            for C in VERSION_CHANNELS[version]:
                for name, adj, feat, tgt, wl in molecules():
                    rec, tries = record(exe, rng, version, version, 0, adj, feat, tgt, L_ALL, C, D_ALL, wl, MAXV)
                    tag = "v%d_%s_c%d" % (version, name, C)
                    for k, v in rec.items():
                        out["%s__%s" % (tag, k)] = v
                    tags.append(tag)
                    worst_margin = min(worst_margin, float(rec["margin"][0]))
                    print("%-22s %4d parameters, predict %10.6g, margin %.3g (%d redraws)" % (tag, rec["params"].size, rec["predict"][0],
                                                                                           rec["margin"][0], tries))
        out["tags"] = np.array(tags)
        # both classifiers at nClass = 5 on the 12-vertex molecule, the label in the middle of the range
        ctags = []
        adj, feat, _ = synthetic_molecule(5, 12)
        for kind, version in ((4, 1), (5, 3)):
            for C in (4, 3):
                rec, tries = record(exe, rng, kind, version, N_CLASS, adj, feat, 2.0, L_ALL, C, D_ALL, 1, MAXV)
                tag = "cls_v%d_syn12_c%d" % (version, C)
                for k, v in rec.items():
                    out["%s__%s" % (tag, k)] = v
                ctags.append(tag)
                worst_margin = min(worst_margin, float(rec["margin"][0]))
                print("%-22s %4d parameters, label %d, loss %.6g, margin %.3g (%d redraws)" % (tag, rec["params"].size, rec["label"][0],
                                                                                              rec["loss"][0], rec["margin"][0], tries))
        out["class_tags"] = np.array(ctags)
        # the weights each of the five constructors draws after srand(seed)
        tm = toy_molecules()
        mol_text = "".join(graph_text(a, f) for _, a, f, _ in tm) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        L, C, D, maxV, seed = 2, 3, 1, 6, 29
        for kind, version, nClass in ((1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 1, N_CLASS), (5, 3, N_CLASS)):
            lines = run(exe, "learn " + head(kind, nClass, maxV, L, C, 4, D, 1) + "%d 0 0 %d\n" % (seed, len(tm)) + mol_text)
            p = "init_k%d__" % kind
            out[p + "cfg"] = np.array([version, L, C, D, 1, maxV, nClass, seed], dtype=np.int32)
            out[p + "params0"] = np.array(lines[0].split(), dtype=np.float64)
            assert out[p + "params0"].size == sum(n for _, n in smp1d_blocks(version, C, 4 * (D + 1), L, maxV, nClass))
        # three BatchLearn (Momentum) steps of SMP_1D_ver3 on the four toy molecules as one batch, after srand(13)
        L, C, D, maxV, seed, nIter, lr = 2, 4, 1, 6, 13, 3, 1e-3
        lines = run(exe, "learn " + head(3, 0, maxV, L, C, 4, D, 1) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm)) + mol_text)
        out["train__cfg"] = np.array([3, L, C, D, 1, maxV, 0, seed, nIter], dtype=np.int32)
        out["train__lr"] = np.array([lr])
        out["train__momentum"] = np.array([MOMENTUM])
        out["train__targets"] = np.array([t for *_, t in tm], dtype=np.float64)
        out["train__params0"] = np.array(lines[0].split(), dtype=np.float64)
        out["train__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
        out["train__params"] = np.array(lines[2].split(), dtype=np.float64)
    assert worst_margin >= MARGIN
    np.savez_compressed(os.path.join(HERE, "smp_1d.npz"), **out)
    print("wrote smp_1d.npz: %d regression cases, %d classifier cases, five initial-weight records, a %d-step Momentum trajectory; "
          "smallest pre-activation margin %.3g of max |z|" % (len(tags), len(ctags), nIter, worst_margin))


if __name__ == "__main__":
    main()
