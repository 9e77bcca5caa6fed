#!/usr/bin/env python3
"""Generate tests/golden/smp_matrix_form.npz from the REAL reference classes LCNN and GCN_MW (GraphFlow/LCNN.h, GCN_MW.h, with Conv1D.h,
ShuffleMatrix.h and DenseGraph.h behind them).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_matrix_form_golden.py
A small driver (below) that only includes the two reference headers is compiled into a temporary directory outside the repository and
fed through stdin / stdout.  Only data is recorded: per case the inputs, the class's order and sequence (LCNN) or A-hat (GCN_MW), for the
small cases the activations, the graph feature, prediction, loss and every parameter gradient; the weights each class draws after
srand(seed); a three-step BatchLearn (Momentum 0.9) trajectory per class; one save_model file.  Inputs are float32-representable.

LeakyReLU has a kink at 0: parameters are drawn so that no pre-activation lies within MARGIN = 1e-3 of max|z| of zero, in every case and
at every step of the trajectories (a case with a few thousand pre-activations would never pass a draw: the wide cases are shallow); a
draw that fails is drawn again (the next numbers of the generator, the next seed of a trajectory).
Then every fixture passes this assert: a numpy float32 evaluation of tests/matrix_form_ref.py meets the fp64 class within HALF of the
suite's tolerance (field_suite.TOL, tests/util.py: rel_err) on every recorded quantity, the gradient block by block.  A fixture that
cannot is drawn with smaller parameters (the scale is halved); the tolerance does not move.  The four demo molecules of a class share
one parameter vector, so that a batch of them has the sum of their gradients.  LCNN keeps its histogram in nVertices (nDepth + 1) doubles
per vertex: every LCNN case has nFeatures <= nVertices."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import matrix_form_ref as mref  # noqa: E402
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402
from make_gru_gcn_golden import disconnected_molecule  # noqa: E402
from make_neighbourhood_golden import directed_molecule, graph_text, isolated_molecule  # noqa: E402
from util import rel_err  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")   # the reference tree (the directory that holds GraphFlow/)
HEADERS = ("LCNN.h", "GCN_MW.h", "Conv1D.h", "ShuffleMatrix.h", "DenseGraph.h")
MOMENTUM = 0.9
HALF_TOL = 0.5e-5   # half of field_suite.TOL
MARGIN = 1e-3

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include <string>
// (both headers define a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_LCNN
#include "LCNN.h"
#undef INF
#define INF INF_of_GCN_MW
#include "GCN_MW.h"
#undef INF

static DenseGraph *read_graph(int F) {
    int V;
    if (scanf("%d", &V) != 1) return NULL;
    DenseGraph *g = new DenseGraph(V, F);
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) scanf("%d", &g->adj[i][j]);
    for (int i = 0; i < V; ++i)
        for (int f = 0; f < F; ++f) scanf("%lf", &g->feature[i][f]);
    g->create_norm_adj();
    return g;
}

static void print_values(const char *sep, const double *v, int n) {
    for (int i = 0; i < n; ++i) printf("%.17g ", v[i]);
    printf("%s", sep);
}

template <class Net>
static void print_params(Net &net, bool grads) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        print_values("", grads ? net.sgd->params[i]->gradient : net.sgd->params[i]->value, net.sgd->params[i]->size);
    printf("\n");
}

template <class Net>
static void read_params(Net &net) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
}

// line 1: the structure, line 2: the activations, then feature, (predict, loss), gradients
static void run(LCNN &net, DenseGraph *g, double target, const char *save_to) {
    read_params(net);
    net.complete_computation_graph(g);
    net.target->value[0] = target;
    net.graph->forward();
    net.graph->backward();
    for (int i = 0; i < net.nVertices; ++i) printf("%d ", net.order[i]);
    for (int i = 0; i < net.sequence->size; ++i) printf("%d ", (int)net.sequence->value[i]);
    printf("\n");
    print_values("", net.firstReLU->value, net.firstReLU->size);
    print_values("\n", net.secondConv->value, net.secondConv->size);
    print_values("\n", net.denseLayer->value, net.denseLayer->size);
    printf("%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
    print_params(net, true);
    if (save_to[0]) net.save_model(std::string(save_to));
}

static void run(GCN_MW &net, DenseGraph *g, double target, const char *save_to) {
    read_params(net);
    net.complete_computation_graph(g);
    net.target->value[0] = target;
    net.graph->forward();
    net.graph->backward();
    print_values("\n", g->norm_adj->value, g->norm_adj->size);
    for (int l = 0; l <= net.nLevels; ++l) print_values("", net.level[l]->hidden->value, net.level[l]->hidden->size);
    printf("\n");
    print_values("\n", net.final_feature->value, net.final_feature->size);
    printf("%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
    print_params(net, true);
    if (save_to[0]) net.save_model(std::string(save_to));
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

// kind 1: LCNN(V, F, k, D, C1, C2, nDense), 2: GCN_MW(L, V, F, H, D) -- the seven numbers a .. g.  Objects are leaked on purpose.
// argv[1] (optional): where `run` saves the model.
int main(int argc, char **argv) {
    char mode[16];
    int kind, a, b, c, d, e, f, g;
    double mom;
    if (scanf("%15s %d %d %d %d %d %d %d %d %lf", mode, &kind, &a, &b, &c, &d, &e, &f, &g, &mom) != 10) return 1;
    const int F = kind == 1 ? b : c;
    if (mode[0] == 'r') {   // run: one sample, given parameters
        DenseGraph *gr = read_graph(F);
        double target;
        scanf("%lf", &target);
        const char *save_to = argc > 1 ? argv[1] : "";
        if (kind == 1) run(*new LCNN(a, b, c, d, e, f, g, mom), gr, target, save_to);
        else run(*new GCN_MW(a, b, c, d, e, mom), gr, target, save_to);
        return 0;
    }
    // learn: srand(seed), the constructor's weights_initialization(), nIter x BatchLearn(nMol, molecules, targets, lr)
    int seed, nIter, nMol;
    double lr;
    scanf("%d %d %lf %d", &seed, &nIter, &lr, &nMol);
    std::vector<DenseGraph *> m(nMol);
    std::vector<double> tgt(nMol);
    for (int i = 0; i < nMol; ++i) m[i] = read_graph(F);
    for (int i = 0; i < nMol; ++i) scanf("%lf", &tgt[i]);
    srand((unsigned)seed);
    if (kind == 1) learn(*new LCNN(a, b, c, d, e, f, g, mom), nIter, nMol, &m[0], &tgt[0], lr);
    else learn(*new GCN_MW(a, b, c, d, e, mom), nIter, nMol, &m[0], &tgt[0], lr);
    return 0;
}
"""

LCNN_DEMO = (6, 5, 3, 16, 8, 128)   # (V, k, D, C1, C2, nDense) of the reference's tests/test_LCNN.cpp
GCN_DEMO = (1, 20, 1)               # (L, H, D) of tests/test_GCN_MW.cpp


def run(exe, text, *args):
    return subprocess.run([exe, *args], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def head(kind, cfg, F, maxV):
    if kind == "lcnn":
        V, k, D, C1, C2, nD = cfg
        nums = (1, V, F, k, D, C1, C2, nD)
    else:
        L, H, D = cfg
        nums = (2, L, maxV, F, H, D, 0, 0)
    return " ".join(str(n) for n in nums) + " %.17g\n" % MOMENTUM


def cases(kind):
    """(name, adj, feature, target, cfg).  The first four are the reference's demo settings and share one parameter vector."""
    toys = [(n, a, f, t) for n, a, f, t in toy_molecules()]
    one = (np.zeros((1, 1), dtype=np.int32), np.array([[1.0, 0.5, 0.0, 0.25]]), 1.0)
    by = {n: (a, f, t) for n, a, f, t in toys}
    if kind == "gcn_mw":   # cfg = (L, H, D): L in {0, 1, 2, 3}, output widths 8, 10, 20, 64 and 80
        return [(n, a, f, t, GCN_DEMO) for n, a, f, t in toys] + [
            ("C2H4_L0",) + by["C2H4"] + ((0, 10, 2),),
            ("CH4_L3",) + by["CH4"] + ((3, 8, 0),),
            ("single",) + one + ((1, 5, 2),),
            ("disconnected",) + disconnected_molecule() + ((3, 64, 0),),
            ("directed",) + directed_molecule() + ((1, 10, 1),),
            ("isolated",) + isolated_molecule() + ((2, 9, 1),),
            ("syn9",) + synthetic_molecule(3, 9) + ((1, 80, 0),),
            ("syn29",) + synthetic_molecule(7, 29) + ((1, 8, 2),)]
    # cfg = (V, k, D, C1, C2, nDense): k F' and k C1 off the K tile (k = 3, F' = 5), widths 8, 10, 64 and 80, one vertex, a disconnected
    # molecule below full size (real rows with pad entries), k > V, a full-size molecule without pads (C2H4 at V = 6)
    return [(n, a, f, t, LCNN_DEMO) for n, a, f, t in toys] + [
        ("single",) + one + ((4, 3, 1, 10, 8, 5),),
        ("disconnected",) + disconnected_molecule() + ((8, 5, 0, 10, 80, 3),),
        ("H2O_k_above_V",) + by["H2O"] + ((4, 6, 2, 5, 10, 9),),
        ("isolated",) + isolated_molecule() + ((7, 4, 1, 64, 8, 16),),
        ("syn9_k3",) + synthetic_molecule(3, 9) + ((10, 3, 0, 7, 64, 6),),
        ("syn12",) + synthetic_molecule(5, 12) + ((12, 10, 1, 64, 10, 7),)]


def random_params(kind, cfg, F, rng, scale):
    """float32-exact parameters in registration order: multiples of 1/64 in [-1, 1] times `scale`; the biases keep the full range so that
    no pre-activation of an all-zero row sits at the kink"""
    return f32exact(np.concatenate([rng.integers(-64, 65, n) / 64.0 * (1.0 if name in ("b1", "b2") else scale)
                                    for name, n in mref.blocks(kind, cfg, F)]))


def record(exe, kind, cfg, params, adj, feat, tgt, save_to=None):
    V, F = feat.shape
    text = "run " + head(kind, cfg, F, V) + graph_text(adj, feat) + "%.17g\n" % tgt + " ".join("%.17g" % x for x in params) + "\n"
    lines = run(exe, text, *([save_to] if save_to else []))
    pred, loss = (float(x) for x in lines[3].split())
    rec = {"structure": np.array(lines[0].split(), dtype=np.float64), "activations": np.array(lines[1].split(), dtype=np.float64),
           "graph_feature": np.array(lines[2].split(), dtype=np.float64), "result": np.array([pred, loss, tgt]),
           "grads": np.array(lines[4].split(), dtype=np.float64), "adj": np.asarray(adj, dtype=np.int32), "feature": feat,
           "cfg": np.array(cfg, dtype=np.int32), "params": params.astype(np.float32)}
    assert rec["grads"].size == params.size
    return rec


def restated(kind, r):
    """(structure, activations) of a restatement's run in the driver's layout"""
    if kind == "lcnn":
        return np.concatenate([r["order"], r["seq"].ravel()]).astype(np.float64), np.concatenate([r["a1"].ravel(), r["c2"].ravel()])
    return r["norm_adj"].ravel(), np.concatenate([h.ravel() for h in r["activations"]])


def fp32_error(kind, cfg, rec, adj, feat, tgt, params):
    """the largest rel_err of a float32 evaluation of the restatement against the class's fp64 numbers, the gradient block by block"""
    r = mref.run(kind, cfg, adj, feat, tgt, params, dtype=np.float32)
    errs = [rel_err(restated(kind, r)[1], rec["activations"]), rel_err(r["graph_feature"], rec["graph_feature"]),
            rel_err([r["predict"]], rec["result"][:1]), rel_err([r["loss"]], rec["result"][1:2])]
    off = 0
    for _, n in mref.blocks(kind, cfg, feat.shape[1]):
        errs.append(rel_err(r["grads"][off:off + n], rec["grads"][off:off + n]))
        off += n
    return max(errs)


def main():
    for h in HEADERS:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(4129)
    worst, smallest = 0.0, np.inf
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "matrix_form_driver.cpp"), os.path.join(tmp, "matrix_form_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for kind in ("lcnn", "gcn_mw"):
            todo = cases(kind)
            groups = [todo[:4]] + [[c] for c in todo[4:]]   # (the demo molecules share their parameters)
            for group in groups:
                cfg, F = group[0][4], group[0][2].shape[1]
                scale, draws = 1.0, 0
                while True:
                    params = random_params(kind, cfg, F, rng, scale)
                    draws += 1
                    assert draws <= 4000, group[0][0]
                    if min(mref.run(kind, cfg, a, f32exact(f), t, params)["margin"] for _, a, f, t, _ in group) < MARGIN:
                        continue   # (the margin condition: drawn again)
                    recs = [record(exe, kind, cfg, params, a, f32exact(f), t) for _, a, f, t, _ in group]
                    e = max(fp32_error(kind, cfg, rec, a, f32exact(f), t, params) for rec, (_, a, f, t, _) in zip(recs, group))
                    if e <= HALF_TOL:
                        break
                    scale *= 0.5
                    assert scale > 1e-3, (group[0][0], e)
                for rec, (name, adj, feat, tgt, _) in zip(recs, group):
                    r = mref.run(kind, cfg, adj, f32exact(feat), tgt, params)
                    structure = restated(kind, r)[0]
                    assert rel_err(structure, rec["structure"]) <= (0 if kind == "lcnn" else 1e-15), "the class's structure is not the restatement's"
                    tag = "%s_%s" % (kind, name)
                    if rec["activations"].size > 2000:   # (the activations of the small cases)
                        del rec["activations"]
                    for k, v in rec.items():
                        out["%s__%s" % (tag, k)] = v
                    tags.append(tag)
                    worst, smallest = max(worst, e), min(smallest, r["margin"])
                    print("%-24s %6d parameters (scale %g, draw %d), predict %10.6g, margin %.3g, fp32 restatement within %.3g"
                          % (tag, params.size, scale, draws, rec["result"][0], r["margin"], e), flush=True)
        out["tags"] = np.array(tags)
        # one save_model file: GCN_MW on CH4 at the case's parameters
        name, adj, feat, tgt, cfg = cases("gcn_mw")[0]
        ck = os.path.join(tmp, "model.txt")
        record(exe, "gcn_mw", cfg, out["gcn_mw_CH4__params"].astype(np.float64), adj, f32exact(feat), tgt, save_to=ck)
        with open(ck, "rb") as f:
            out["checkpoint__text"] = np.frombuffer(f.read(), dtype=np.uint8)
        out["checkpoint__tag"] = np.array("gcn_mw_CH4")
        # the weights each constructor's weights_initialization() draws after srand(seed), and three BatchLearn (Momentum) steps per class on
        # the four toy molecules as one batch at the demo settings: lr = 0.1 unless the loss rises at a step, then half of it, and so on; the
        # seed is the first from 23 on whose every step satisfies the margin condition
        tm = toy_molecules()
        mols = [(a, f32exact(f)) for _, a, f, _ in tm]
        mol_text = "".join(graph_text(a, f) for a, f in mols) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        targets = np.array([t for *_, t in tm], dtype=np.float64)
        nIter = 3
        for kind, cfg in (("lcnn", LCNN_DEMO), ("gcn_mw", GCN_DEMO)):
            seed, lr = 23, 0.1
            while True:
                lines = run(exe, "learn " + head(kind, cfg, 4, 6) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm)) + mol_text)
                losses = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
                p0 = np.array(lines[0].split(), dtype=np.float64)
                if not (losses[:, 1] <= losses[:, 0]).all():
                    lr *= 0.5
                    assert lr > 1e-4
                    continue
                rl, rp, small = mref.momentum_steps(kind, cfg, mols, targets, p0, nIter, lr, MOMENTUM)
                if small >= MARGIN:
                    break
                seed, lr = seed + 1, 0.1
                assert seed < 4000
            final = np.array(lines[2].split(), dtype=np.float64)
            assert rel_err(rl, losses) <= 1e-9 and rel_err(rp, final) <= 1e-9, "the restatement's trajectory is not the class's"
            p = "train_%s__" % kind
            out[p + "cfg"] = np.array(cfg, dtype=np.int32)
            out[p + "seed"] = np.array([seed, nIter, 6], dtype=np.int32)
            out[p + "lr"] = np.array([lr])
            out[p + "momentum"] = np.array([MOMENTUM])
            out[p + "targets"] = targets
            out[p + "params0"] = p0
            out[p + "losses"] = losses
            out[p + "params"] = final
            assert p0.size == sum(n for _, n in mref.blocks(kind, cfg, 4))
            smallest = min(smallest, small)
            print("%s: seed %d, three BatchLearn steps at lr %g, smallest margin %.3g, losses %s" % (kind, seed, lr, small, losses.ravel()))
    assert worst <= HALF_TOL and smallest >= MARGIN
    np.savez_compressed(os.path.join(HERE, "smp_matrix_form.npz"), **out)
    print("wrote smp_matrix_form.npz: %d cases, one checkpoint, two %d-step Momentum trajectories with their initial weights; smallest "
          "margin kept %.3g of max|z|; the fp32 restatement within %.3g of the classes everywhere" % (len(tags), nIter, smallest, worst))


if __name__ == "__main__":
    main()
