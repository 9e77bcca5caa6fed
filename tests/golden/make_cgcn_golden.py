#!/usr/bin/env python3
"""Generate tests/golden/smp_cgcn.npz from the REAL reference classes CGCN_1D and CGCN_2D (GraphFlow/CGCN_1D.h, CGCN_2D.h, with
VertexRepresentation.h, RisiLayer1D.h, RisiLayer2D.h, MatVecMul.h, Masking.h, LeakyReLU.h, SumVectors.h and SumComponents.h behind them).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_cgcn_golden.py
A small driver (below) that only includes the two reference headers is compiled into a temporary directory outside the repository and fed
through stdin / stdout.  It ends with _exit: the classes' destructors delete members that level 0 never allocated.  Only data is recorded:
per case and class the inputs, N(v) and the masks as the class filled them, graph feature, prediction, loss and the parameter gradients in
registration order, for one small case every h_l[v]; the weights each class draws after srand(seed); a three-step BatchLearn (Momentum
0.9) trajectory per class (L = 2, the 2D class L = 1); one save_model file per class.  Inputs are float32-representable.

The weights of the forward and gradient cases are drawn here, not by uniform_init (whose weights shrink a 2D network by roughly the square
per level): multiples of 1/64, mostly positive, every F_l scaled by the power of two that brings max |h_l| into [0.5, 1).  Every fixture
passes three asserts: the in-mask activations of the case span at most three decades; every in-mask pre-activation lies at least 1e-3
max|z| from zero; a numpy float32 evaluation of tests/cgcn_ref.py meets the fp64 class within HALF of the suite's tolerance
(field_suite.TOL, tests/util.py: rel_err) on every recorded quantity, the gradient block by block.  A draw that fails is drawn again; no
case is excused."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import cgcn_ref as cref  # noqa: E402
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402
from make_neighbourhood_golden import graph_text, isolated_molecule  # noqa: E402
from util import rel_err  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")   # the reference tree (the directory that holds GraphFlow/)
HEADERS = ("CGCN_1D.h", "CGCN_2D.h")
MOMENTUM = 0.9
HALF_TOL = 0.5e-5   # half of field_suite.TOL
GAP = 1e-3          # of max|z|, every in-mask pre-activation
DECADES = 1e3       # in-mask activations: largest over smallest

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include <string>
#include <unistd.h>
// (both headers define a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_CGCN_1D
#include "CGCN_1D.h"
#undef INF
#define INF INF_of_CGCN_2D
#include "CGCN_2D.h"
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

template <class Net>
static void print_params(Net &net, bool grads) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", grads ? net.sgd->params[i]->gradient[j] : net.sgd->params[i]->value[j]);
    printf("\n");
}
template <class Net>
static void read_params(Net &net) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
}

template <class Net>
static void run_one(Net &net, DenseGraph *g, double target, int L, int M, const char *save_to) {
    read_params(net);
    net.complete_computation_graph(g);
    net.target->value[0] = target;
    net.graph->forward();
    net.graph->backward();
    const int V = g->nVertices;
    if (L >= 1)   // N(v) as the class filled it (the members of neighbor[v], by pointer; the same at every level)
        for (int v = 0; v < V; ++v) {
            printf("%d ", (int)net.level[1]->neighbor[v]->vectors.size());
            for (size_t i = 0; i < net.level[1]->neighbor[v]->vectors.size(); ++i)
                for (int u = 0; u < V; ++u)
                    if (net.level[1]->neighbor[v]->vectors[i] == net.level[0]->representation[u]) printf("%d ", u);
        }
    printf("\n");
    for (int l = 0; l <= L; ++l)
        for (int v = 0; v < V; ++v)
            for (int u = 0; u < M; ++u) printf("%d ", net.level[l]->receptive_field[v]->value[u] != 0.0 ? 1 : 0);
    printf("\n");
    for (int l = 0; l <= L; ++l)
        for (int v = 0; v < V; ++v)
            for (int i = 0; i < M; ++i) printf("%.17g ", net.level[l]->representation[v]->value[i]);
    printf("\n");
    for (int i = 0; i < M; ++i) printf("%.17g ", net.sum_representations->value[i]);
    printf("\n");
    printf("%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
    print_params(net, true);
    if (save_to[0]) net.save_model(std::string(save_to));
}

template <class Net>
static void learn(Net &net, int nIter, int n, DenseGraph **x, double *tgt, double lr) {
    print_params(net, false);
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(n, x, tgt, lr);
        printf("%.17g %.17g ", r.first, r.second);
    }
    printf("\n");
    print_params(net, false);
}

// form 1: CGCN_1D, 2: CGCN_2D.  argv[1] (optional): where `run` saves.  Ends with _exit: no destructor runs.
int main(int argc, char **argv) {
    char mode[16];
    int form, M, L, F, D;
    double mom;
    if (scanf("%15s %d %d %d %d %d %lf", mode, &form, &M, &L, &F, &D, &mom) != 7) return 1;
    const char *save_to = argc > 1 ? argv[1] : "";
    if (mode[0] == 'r') {   // run: one molecule, given parameters
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        if (form == 1) run_one(*new CGCN_1D(L, M, F, D, mom), g, target, L, M, save_to);
        else run_one(*new CGCN_2D(L, M, F, D, mom), g, target, L, M, save_to);
    } else {   // learn: srand(seed), the constructor's weights_initialization(), nIter x BatchLearn  (nIter 0: the weights only)
        int seed, nIter, n;
        double lr;
        scanf("%d %d %lf %d", &seed, &nIter, &lr, &n);
        std::vector<DenseGraph *> x(n);
        std::vector<double> tgt(n);
        for (int i = 0; i < n; ++i) x[i] = read_graph(F);
        for (int i = 0; i < n; ++i) scanf("%lf", &tgt[i]);
        srand((unsigned)seed);
        if (form == 1) learn(*new CGCN_1D(L, M, F, D, mom), nIter, n, &x[0], &tgt[0], lr);
        else learn(*new CGCN_2D(L, M, F, D, mom), nIter, n, &x[0], &tgt[0], lr);
    }
    fflush(stdout);
    _exit(0);
}
"""


def run(exe, text, *args):
    return subprocess.run([exe, *args], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def cases():
    """(name, adj, feature, target, nLevels, max_nVertices, nDepth): the cases the issue lists, each at the smallest shape that can still go wrong"""
    tm = toy_molecules()
    toys = {n: (a, f) for n, a, f, _ in tm}
    out = [("toy_" + n, a, f, float(t), 1, 6, 5) for n, a, f, t in tm]   # tests/test_CGCN_2D.cpp's constants
    one = (np.zeros((1, 1), dtype=np.int32), np.array([[1.0, 0.5, 0.0, 0.25]]))
    two = (np.array([[0, 1], [1, 0]], dtype=np.int32), np.array([[1.0, 0.0, 0.5, 0.0], [0.0, 1.0, 0.0, 0.25]]))
    diag = np.array(toys["NH3"][0], dtype=np.int32)
    diag[1, 1] = 1   # (vertex 1 is its own neighbour)
    asym = np.array(toys["CH4"][0], dtype=np.int32)
    asym[0, 1] = 0
    asym[3, 0] = 0
    syn = synthetic_molecule(5, 12)
    iso = isolated_molecule()
    out += [("one", one[0], one[1], 1.5, 2, 3, 1),
            ("two", two[0], two[1], -0.5, 2, 4, 1),
            ("full",) + toys["CH4"] + (2.0, 2, 5, 2),                      # V = max_nVertices
            ("isolated", iso[0], iso[1], 3.0, 2, 7, 2),                     # a vertex with no neighbour
            ("diagonal", diag, toys["NH3"][1], 1.0, 2, 5, 1),
            ("asymmetric", asym, toys["CH4"][1], 0.75, 2, 6, 1),
            ("saturated",) + toys["CH4"] + (1.25, 4, 5, 1),                 # L above the diameter
            ("L0",) + toys["C2H4"] + (2.5, 0, 6, 2),
            ("syn12", syn[0], np.ascontiguousarray(syn[1][:, :4] + 0.5 * syn[1][:, 4:5]), 4.0, 3, 16, 2)]
    return out


def draw_params(form, adj, feat, L, M, D, rng):
    """float32-exact parameters: multiples of 1/64, mostly positive; F_l times the power of two that brings max |h_l| into [0.5, 1)"""
    FD = feat.shape[1] * (D + 1)
    p = np.zeros(cref.n_params(FD, L, M))
    p[:FD] = rng.integers(16, 65, FD) / 64.0 * np.where(rng.random(FD) < 0.15, -1.0, 1.0)
    for l in range(1, L + 1):
        F = rng.integers(16, 65, M * M) / 64.0 * np.where(rng.random(M * M) < 0.15, -1.0, 1.0)
        lo, hi = FD + (l - 1) * M * M, FD + l * M * M
        p[lo:hi] = F
        top = np.abs(cref.run(form, adj, feat, 0.0, p[:hi], l, M, D)["h"][l]).max()
        if top > 0:
            p[lo:hi] = F * 2.0 ** (-np.floor(np.log2(top)) - 1)
    return f32exact(p)


def conditions(form, adj, feat, params, L, M, D):
    """(the spread of the in-mask activations, the smallest pre-activation gap)"""
    r = cref.run(form, adj, feat, 0.0, params, L, M, D)
    a = np.abs(r["h"][r["masks"] > 0])
    a = a[a > 0]
    return (a.max() / a.min() if a.size else 1.0), cref.min_preactivation_gap(form, adj, feat, params, L, M, D)


def record(exe, form, adj, feat, tgt, params, L, M, D, save_to=None):
    V, F = feat.shape
    text = "run %d %d %d %d %d %.17g\n" % (form, M, L, F, D, MOMENTUM) + graph_text(adj, feat) + "%.17g\n" % tgt
    text += " ".join("%.17g" % x for x in params) + "\n"
    lines = run(exe, text, *([save_to] if save_to else []))
    vals, N, k = [int(x) for x in lines[0].split()], [], 0
    for v in range(V if L >= 1 else 0):
        N.append(vals[k + 1:k + 1 + vals[k]])
        k += 1 + vals[k]
    assert k == len(vals)
    pred, loss = (float(x) for x in lines[4].split())
    rec = {"lists": cref.lists_flat(N), "masks": np.array(lines[1].split(), dtype=np.uint8).reshape(L + 1, V, M),
           "activations": np.array(lines[2].split(), dtype=np.float64).reshape(L + 1, V, M),
           "feature_out": np.array(lines[3].split(), dtype=np.float64), "result": np.array([pred, loss, tgt]),
           "grads": np.array(lines[5].split(), dtype=np.float64), "adj": np.asarray(adj, dtype=np.int32), "feature": feat,
           "cfg": np.array([form, L, M, D], dtype=np.int32), "params": params.astype(np.float32)}
    assert rec["grads"].size == params.size and rec["feature_out"].size == M
    if L >= 1:
        assert N == cref.neighbours(adj), "the class's neighbours are not the restatement's"
    assert np.array_equal(rec["masks"], cref.masks(adj, L, M).astype(np.uint8)), "the class's masks are not the restatement's"
    return rec


def blockwise(x, ref, blocks):
    errs, off = [], 0
    for _, n in blocks:
        errs.append(rel_err(x[off:off + n], ref[off:off + n]))
        off += n
    return max(errs)


def fp32_error(rec, form, adj, feat, tgt, params, L, M, D):
    """the largest rel_err of a float32 evaluation of the restatement against the class's fp64 numbers, the gradient block by block"""
    r = cref.run(form, adj, feat, tgt, params, L, M, D, dtype=np.float32)
    return max(rel_err(r["h"], rec["activations"]), rel_err(r["feature"], rec["feature_out"]), rel_err([r["predict"]], rec["result"][:1]),
               rel_err([r["loss"]], rec["result"][1:2]),
               blockwise(r["grads"].astype(np.float64), rec["grads"], cref.blocks(feat.shape[1] * (D + 1), L, M)))


def main():
    for h in HEADERS:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(2917)
    worst, smallest, widest = 0.0, np.inf, 0.0
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "cgcn_driver.cpp"), os.path.join(tmp, "cgcn_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for form in (1, 2):
            for name, adj, feat, tgt, L, M, D in cases():
                feat, draws = f32exact(feat), 0
                while True:
                    draws += 1
                    assert draws <= 400, name
                    params = draw_params(form, adj, feat, L, M, D, rng)
                    spread, gap = conditions(form, adj, feat, params, L, M, D)
                    if spread > DECADES or gap < GAP:
                        continue
                    rec = record(exe, form, adj, feat, tgt, params, L, M, D)
                    e = fp32_error(rec, form, adj, feat, tgt, params, L, M, D)
                    # the class against the fp64 restatement, while both are at hand
                    r64 = cref.run(form, adj, feat, tgt, params, L, M, D)
                    assert rel_err(r64["h"], rec["activations"]) <= 1e-12 and rel_err(r64["grads"], rec["grads"]) <= 1e-12, name
                    if e <= HALF_TOL:
                        break
                tag = "c%d_%s" % (form, name)
                if name != "toy_CH4":   # (every h_l[v] for the small case)
                    del rec["activations"]
                for k, v in rec.items():
                    out["%s__%s" % (tag, k)] = v
                tags.append(tag)
                worst, smallest, widest = max(worst, e), min(smallest, gap), max(widest, spread)
                print("%-18s %5d parameters (draw %d), predict %10.6g, activations within a factor %.3g, smallest gap %.3g, fp32 restatement "
                      "within %.3g" % (tag, params.size, draws, rec["result"][0], spread, gap, e), flush=True)
        out["tags"] = np.array(tags)
        # one save_model file per class, on its first case at the case's parameters
        ck = os.path.join(tmp, "model.txt")
        for form in (1, 2):
            name, adj, feat, tgt, L, M, D = cases()[0]
            tag = "c%d_%s" % (form, name)
            record(exe, form, adj, f32exact(feat), tgt, out[tag + "__params"].astype(np.float64), L, M, D, save_to=ck)
            with open(ck, "rb") as f:
                out["checkpoint_c%d__text" % form] = np.frombuffer(f.read(), dtype=np.uint8)
            out["checkpoint_c%d__tag" % form] = np.array(tag)
            os.remove(ck)
        # the weights each constructor's weights_initialization() draws after srand(seed), and three BatchLearn (Momentum) steps per class on
        # the four toy molecules; lr = 0.1 unless the loss rises at a step, then half of it, and so on
        tm = toy_molecules()
        mols = [(a, f32exact(f)) for _, a, f, _ in tm]
        targets = np.array([0.25 * t for *_, t in tm], dtype=np.float64)
        M, D, nIter, seed = 6, 1, 3, 23
        text = "".join(graph_text(*m) for m in mols) + " ".join("%.17g" % t for t in targets) + "\n"
        for form, L in ((1, 2), (2, 1)):   # (a 2D network of two levels is identically zero on the toy molecules: every H has one neighbour)
            lr = 0.1
            while True:
                lines = run(exe, "learn %d %d %d %d %d %.17g\n" % (form, M, L, 4, D, MOMENTUM) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(mols)) + text)
                losses = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
                p0 = np.array(lines[0].split(), dtype=np.float64)
                if (losses[:, 1] <= losses[:, 0]).all():
                    break
                lr *= 0.5
                assert lr > 1e-4
            ref_losses, ref_p = cref.momentum_steps(form, mols, targets, p0, L, M, D, nIter, lr, MOMENTUM)
            assert np.abs(ref_losses - losses).max() <= 1e-9 * max(1.0, np.abs(losses).max())
            assert np.abs(ref_p - np.array(lines[2].split(), dtype=np.float64)).max() <= 1e-9
            p = "train_c%d__" % form
            out[p + "cfg"] = np.array([form, L, M, D, seed, nIter], dtype=np.int32)
            out[p + "lr"] = np.array([lr])
            out[p + "momentum"] = np.array([MOMENTUM])
            out[p + "targets"] = targets
            out[p + "params0"] = p0
            out[p + "losses"] = losses
            out[p + "params"] = np.array(lines[2].split(), dtype=np.float64)
            assert p0.size == cref.n_params(4 * (D + 1), L, M)
            print("form %d: seed %d, three BatchLearn steps at lr %g, losses %s" % (form, seed, lr, losses.ravel()))
    assert worst <= HALF_TOL and smallest >= GAP and widest <= DECADES
    np.savez_compressed(os.path.join(HERE, "smp_cgcn.npz"), **out)
    print("wrote smp_cgcn.npz: %d cases, two checkpoints, two %d-step Momentum trajectories with their initial weights; in-mask activations "
          "within a factor %.3g, smallest pre-activation gap %.3g of max|z|; the fp32 restatement within %.3g of the classes everywhere"
          % (len(tags), nIter, widest, smallest, worst))


if __name__ == "__main__":
    main()
