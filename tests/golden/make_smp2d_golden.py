#!/usr/bin/env python3
"""Generate tests/golden/smp_2d.npz from the REAL reference classes SMP_2D, SMP_2D_ver4, SMP_2D_classification and
SMP_2D_ver4_classification (GraphFlow/SMP_2D*.h).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_smp2d_golden.py
A small driver (below) that only includes the four reference headers is compiled into a temporary directory outside the repository and
fed through stdin / stdout.  Only data is recorded: the inputs, the receptive fields per level, the reference's graph feature,
prediction (scores, probabilities and arg-max label for the classifiers), loss and parameter gradients, for CH4 at nLevels = 2 the level
activations and reduced adjacencies, the weights weights_initialization() draws after srand(seed) for each of the four classes, and a
three-step BatchLearn (Momentum) trajectory of SMP_2D_ver4.  Inputs are float32-representable so the fp32 device path and the fp64
checkers see identical numbers.

Every fixture passes two asserts here: the read-out's worst-case fp32 rounding stays under half of the suite's 1e-5, and no
pre-activation (level 0, the levels, the read-out's sums) lies within 1e-3 max|z| of zero, so that fp32 cannot take the other branch of
a LeakyReLU.  Parameters are redrawn until the second holds (random_params says how they are drawn so that it can); the smallest
margin kept is printed.  A pre-activation that is EXACTLY zero
is not counted (as in make_smp1d_golden.py): both formats take the same branch there.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")   # the reference tree (the directory that holds GraphFlow/)
HEADERS = ("SMP_2D.h", "SMP_2D_ver4.h", "SMP_2D_classification.h", "SMP_2D_ver4_classification.h")
MARGIN = 1e-3      # smallest |z| / max |z| a fixture may hold
MOMENTUM = 0.9

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
// (every one of the four headers defines a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_SMP_2D
#include "SMP_2D.h"
#undef INF
#define INF INF_of_SMP_2D_ver4
#include "SMP_2D_ver4.h"
#undef INF
#define INF INF_of_SMP_2D_classification
#include "SMP_2D_classification.h"
#undef INF
#define INF INF_of_SMP_2D_ver4_classification
#include "SMP_2D_ver4_classification.h"
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
        if (a == 0.0) continue;
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
            if (l == 0) margins(net.level[0]->f_reshape[v]->value, net.level[0]->f_reshape[v]->size);
            else margins(net.level[l]->add[v]->value, net.level[l]->add[v]->size);
            if (l == L) margins(net.shrinked[v]->value, net.shrinked[v]->size);
        }
    printf("\n");
    for (int f = 0; f < net.graph_feature->size; ++f) printf("%.17g ", net.graph_feature->value[f]);
    printf("\n");
    for (int l = 0; l <= L; ++l)   // the activations f_l[v], [s][s][C_l] row-major, back to back
        for (int v = 0; v < V; ++v)
            for (int i = 0; i < net.level[l]->f[v]->size; ++i) printf("%.17g ", net.level[l]->f[v]->value[i]);
    printf("\n");
    for (int l = 1; l <= L; ++l)   // the reduced adjacencies, [s][s]
        for (int v = 0; v < V; ++v)
            for (int i = 0; i < net.level[l]->adj[v]->size; ++i) printf("%.17g ", net.level[l]->adj[v]->value[i]);
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
    printf("%.17g\n", (double)net.Predict(g));
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

// kind 1: SMP_2D, 2: SMP_2D_ver4, 3: SMP_2D_classification, 4: SMP_2D_ver4_classification.  Objects are leaked on purpose: the models'
// and the executors' destructors free the same memory.
int main() {
    char mode[16];
    int kind, nClass, maxV, L, C, F, D, wl;
    double mom;
    if (scanf("%15s %d %d %d %d %d %d %d %d %lf", mode, &kind, &nClass, &maxV, &L, &C, &F, &D, &wl, &mom) != 10) return 1;
    if (mode[0] == 'r') {   // run: one sample, given parameters
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        if (kind == 1) run_regression(*new SMP_2D(maxV, L, C, F, D, mom, wl != 0), g, target, L);
        else if (kind == 2) run_regression(*new SMP_2D_ver4(maxV, L, C, F, D, mom, wl != 0), g, target, L);
        else if (kind == 3) run_classifier(*new SMP_2D_classification(nClass, maxV, L, C, F, D, mom, wl != 0), g, target, L, nClass);
        else run_classifier(*new SMP_2D_ver4_classification(nClass, maxV, L, C, F, D, mom, wl != 0), g, target, L, nClass);
        return 0;
    }
    // learn: srand(seed), the constructor's weights_initialization(), nIter x BatchLearn(nMol, molecules, targets, lr)  (nIter 0: the weights only)
    int seed, nIter, nMol;
    double lr;
    scanf("%d %d %lf %d", &seed, &nIter, &lr, &nMol);
    std::vector<DenseGraph *> m(nMol);
    std::vector<double> tgt(nMol);
    for (int i = 0; i < nMol; ++i) m[i] = read_graph(F);
    for (int i = 0; i < nMol; ++i) scanf("%lf", &tgt[i]);
    srand((unsigned)seed);
#define GF_LEARN(T, ...) { T &net = *new T(__VA_ARGS__); learn(net, nIter, nMol, &m[0], &tgt[0], lr); }
    if (kind == 1) GF_LEARN(SMP_2D, maxV, L, C, F, D, mom, wl != 0)
    else if (kind == 2) GF_LEARN(SMP_2D_ver4, maxV, L, C, F, D, mom, wl != 0)
    else if (kind == 3) GF_LEARN(SMP_2D_classification, nClass, maxV, L, C, F, D, mom, wl != 0)
    else GF_LEARN(SMP_2D_ver4_classification, nClass, maxV, L, C, F, D, mom, wl != 0)
    return 0;
}
"""


def channels(form, C, L):
    """channel count per level: constant for SMP_2D (form 1), doubling for SMP_2D_ver4 (form 2)"""
    return [C if form == 1 else C << l for l in range(L + 1)]


def smp2d_blocks(form, C, FD, L, maxV, nClass=0):
    """[(block name, size)] in registration order: H; per level (lambda1_s[C_{l-1}], lambda2_s[C_{l-1}], b_s[C_l]) for s = 1..maxV, then
    scalar_l[C_{l-1}]; W[C_L] or, for a classifier, W[nClass, C_L]."""
    c = channels(form, C, L)
    out = [("H", C * FD)]
    for l in range(1, L + 1):
        for s in range(1, maxV + 1):
            out += [("lam1_%d_%d" % (l, s), c[l - 1]), ("lam2_%d_%d" % (l, s), c[l - 1]), ("b_%d_%d" % (l, s), c[l])]
        out.append(("scalar_%d" % l, c[l - 1]))
    out.append(("W", max(nClass, 1) * c[L]))
    return out


def random_params(form, C, FD, L, maxV, rng, nClass=0):
    """float32-exact parameters in registration order, drawn so that the margin CAN hold.  A field of 12 vertices has 144 C_l
    pre-activations per vertex and level and the read-out sums 144 of them: independent draws never keep all of them 1e-3 max|z| away
    from zero.  So every channel of every level gets one sign: with sigma the sign of a channel of the level below (H's rows have one
    sign each, the WL features are >= 0), scalar_l has sigma's sign, lambda1_s and lambda2_s one sign per channel for all sizes, and b_s
    the sign of lambda * sigma -- every term of z pulls the same way and |z| >= |b|.  A negative channel is drawn 100 times larger, so
    that behind the 0.01 slope both kinds of activation lie in +-[0.2, 1]: the sums over 4 .. 144 positions then stay within three
    decades.  W has the graph feature's sign per channel (times one sign per class): the read-out's dot product does not cancel."""
    c = channels(form, C, L)

    def signs(n):
        return rng.choice([-1.0, 1.0], n)

    def big(sg):   # 100 for the channels whose pre-activations are negative
        return np.where(sg > 0, 1.0, 100.0)

    sigma = signs(C)
    parts = [(sigma * big(sigma))[:, None] * rng.uniform(0.2, 0.21, (C, FD))]
    for l in range(1, L + 1):
        cp = c[l - 1]
        s1 = signs(cp)
        s2 = s1 if form == 1 else signs(cp)
        t1, t2 = s1 * sigma, s2 * sigma
        for size in range(1, maxV + 1):
            k = 1.0 if form == 1 else 2.0
            parts.append(s1 * big(t1) * k * rng.uniform(0.03, 0.05, cp))
            parts.append(s2 * big(t2) * k * rng.uniform(0.03, 0.05, cp) / size)
            tb = t1 if form == 1 else np.concatenate([t1, t2])
            parts.append(tb * big(tb) * rng.uniform(0.25, 0.4, c[l]))
        parts.append(sigma * rng.uniform(0.2, 0.5, cp))
        sigma = t1 if form == 1 else np.concatenate([t1, t2])
    rows = max(nClass, 1)
    parts.append(signs(rows)[:, None] * sigma[None, :] * rng.uniform(0.5, 1.0, (rows, c[L])) / (100.0 * c[L]))
    return f32exact(np.concatenate([np.ravel(x) for x in parts]))


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


def molecules():
    """(name, adj, feature, target, wl): the four toy molecules (CH4: four vertices of one field size at level 1, five at level 2) and one
    12-vertex synthetic molecule, with and without the WL ordering"""
    out = [(n, a, f, t, 1) for n, a, f, t in toy_molecules()]
    a, f, t = synthetic_molecule(5, 12)
    out.append(("syn12", a, f, t, 1))
    out.append(("syn12nowl", a, f, t, 0))
    return out


CONFIGS = ((5, 2), (10, 2), (8, 3))   # (C, nLevels): lane vectors of 1, 2 and 4 floats
D_ALL, MAXV = 1, 14                   # (max_nVertices above the largest molecule: unused per-size blocks, whose gradients stay zero)
N_CLASS = 5
ACTIVATIONS_OF = "CH4"


def head(kind, nClass, maxV, L, C, F, D, wl):
    return "%d %d %d %d %d %d %d %d %.17g\n" % (kind, nClass, maxV, L, C, F, D, wl, MOMENTUM)


def record(exe, rng, kind, form, nClass, adj, feat, tgt, L, C, D, wl, maxV, activations):
    """one fixture: parameters are redrawn until the pre-activation margin holds"""
    V, F = feat.shape
    blocks = smp2d_blocks(form, C, F * (D + 1), L, maxV, nClass)
    CL = channels(form, C, L)[L]
    for attempt in range(2000):
        params = random_params(form, C, F * (D + 1), L, maxV, rng, nClass)
        assert params.size == sum(n for _, n in blocks)
        text = "run " + head(kind, nClass, maxV, L, C, F, D, wl) + graph_text(adj, feat) + "%.17g\n" % tgt
        text += " ".join("%.17g" % x for x in params) + "\n"
        lines = run(exe, text)
        rec = {"phi": parse_phi(lines[0], L, V, maxV), "graph_feature": np.array(lines[1].split(), dtype=np.float64)}
        if activations:
            rec["activations"] = np.array(lines[2].split(), dtype=np.float64)
            rec["adjacency"] = np.array(lines[3].split(), dtype=np.float64)
        lines = lines[4:]
        if nClass:
            rec["scores"] = np.array(lines[0].split(), dtype=np.float64)
            rec["probability"] = np.array(lines[1].split(), dtype=np.float64)
            rec["loss"] = np.array([float(lines[2])])
            rec["grads"] = np.array(lines[3].split(), dtype=np.float64)
            zmin, zmax = (float(x) for x in lines[4].split())
            rec["label"] = np.array([int(float(lines[5]))], dtype=np.int32)
            out_scale = max(1.0, np.abs(rec["scores"]).max())
            worst = np.abs(params[-nClass * CL:].reshape(nClass, CL) * rec["graph_feature"][None, :]).sum(1).max()
        else:
            pred, loss = (float(x) for x in lines[0].split())
            rec["predict"], rec["loss"] = np.array([pred]), np.array([loss])
            rec["grads"] = np.array(lines[1].split(), dtype=np.float64)
            zmin, zmax = (float(x) for x in lines[2].split())
            out_scale = max(1.0, abs(pred))
            worst = np.abs(rec["graph_feature"] * params[-CL:]).sum()
        assert rec["grads"].size == params.size and rec["graph_feature"].size == CL, (rec["grads"].size, params.size)
        if zmin < MARGIN * zmax or worst * 2.0 ** -24 * CL > 5e-6 * out_scale:
            continue
        rec.update(adj=adj.astype(np.int32), feature=feat, target=np.array([tgt], dtype=np.float64), params=params.astype(np.float32),
                   cfg=np.array([form, L, C, D, wl, maxV, nClass], dtype=np.int32), margin=np.array([zmin / zmax]))
        return rec, attempt
    raise AssertionError("no draw with a pre-activation margin of %g" % MARGIN)


def main():
    for h in HEADERS:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(2204)
    worst_margin = 1.0
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "smp2d_driver.cpp"), os.path.join(tmp, "smp2d_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for form in (1, 2):
            for C, L in CONFIGS:
                for name, adj, feat, tgt, wl in molecules():
                    rec, tries = record(exe, rng, form, form, 0, adj, feat, tgt, L, C, D_ALL, wl, MAXV, name == ACTIVATIONS_OF and L == 2)
                    tag = "f%d_%s_c%d" % (form, name, C)
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
        for kind, form in ((3, 1), (4, 2)):
            for C in (5, 8):
                rec, tries = record(exe, rng, kind, form, N_CLASS, adj, feat, 2.0, 2, C, D_ALL, 1, MAXV, False)
                tag = "cls_f%d_syn12_c%d" % (form, C)
                for k, v in rec.items():
                    out["%s__%s" % (tag, k)] = v
                ctags.append(tag)
                worst_margin = min(worst_margin, float(rec["margin"][0]))
                print("%-22s %4d parameters, label %d, loss %.6g, margin %.3g (%d redraws)" % (tag, rec["params"].size, rec["label"][0],
                                                                                              rec["loss"][0], rec["margin"][0], tries))
        out["class_tags"] = np.array(ctags)
        # the weights each constructor's weights_initialization() draws after srand(seed)
        tm = toy_molecules()
        mol_text = "".join(graph_text(a, f) for _, a, f, _ in tm) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        L, C, D, maxV, seed = 2, 3, 1, 6, 31
        for kind, form, nClass in ((1, 1, 0), (2, 2, 0), (3, 1, N_CLASS), (4, 2, N_CLASS)):
            lines = run(exe, "learn " + head(kind, nClass, maxV, L, C, 4, D, 1) + "%d 0 0 %d\n" % (seed, len(tm)) + mol_text)
            p = "init_k%d__" % kind
            out[p + "cfg"] = np.array([form, L, C, D, 1, maxV, nClass, seed], dtype=np.int32)
            out[p + "params0"] = np.array(lines[0].split(), dtype=np.float64)
            assert out[p + "params0"].size == sum(n for _, n in smp2d_blocks(form, C, 4 * (D + 1), L, maxV, nClass))
        # three BatchLearn (Momentum) steps of SMP_2D_ver4 on the four toy molecules as one batch, after srand(17)
        L, C, D, maxV, seed, nIter, lr = 2, 4, 1, 6, 17, 3, 1e-3
        lines = run(exe, "learn " + head(2, 0, maxV, L, C, 4, D, 1) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm)) + mol_text)
        out["train__cfg"] = np.array([2, L, C, D, 1, maxV, 0, seed, nIter], dtype=np.int32)
        out["train__lr"] = np.array([lr])
        out["train__momentum"] = np.array([MOMENTUM])
        out["train__targets"] = np.array([t for *_, t in tm], dtype=np.float64)
        out["train__params0"] = np.array(lines[0].split(), dtype=np.float64)
        out["train__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
        out["train__params"] = np.array(lines[2].split(), dtype=np.float64)
    assert worst_margin >= MARGIN
    np.savez_compressed(os.path.join(HERE, "smp_2d.npz"), **out)
    print("wrote smp_2d.npz: %d regression cases, %d classifier cases, four initial-weight records, a %d-step Momentum trajectory; "
          "smallest pre-activation margin %.3g of max |z|" % (len(tags), len(ctags), nIter, worst_margin))


if __name__ == "__main__":
    main()
