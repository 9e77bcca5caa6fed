#!/usr/bin/env python3
"""Generate tests/golden/smp_third_order.npz from the REAL reference classes GCN_3D and GRU_GCN_3D (GraphFlow/GCN_3D.h, GRU_GCN_3D.h,
with RisiLayer3D.h and KMax.h behind them).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_third_order_golden.py
A small driver (below) that only includes the two reference headers is compiled into a temporary directory outside the repository and
fed through stdin / stdout.  Only data is recorded: per case the inputs, the neighbourhoods N_l(v) as the class filled them, the
reference's graph feature, prediction, loss and parameter gradients, for the small cases every h_l[v]; the weights each class draws after
srand(seed); a three-step BatchLearn (Momentum 0.9) trajectory per form; one save_model file.  Inputs are float32-representable.

KMax keeps the H largest of H^3 triple products: a discrete choice.  Within a symmetry class of RisiLayer3D the choice changes nothing;
between classes it is a kink, so every fixture is drawn with a margin, as make_ccn1d_golden.py draws pre-activation margins: at every
(vertex, level) with three members or more, of every case and of every step of the trajectories, the classes that hold the top H entries
and the first class below differ pairwise-adjacently by at least third_order_ref.GAP = 1e-5 of max|T| in fp64 -- ten times the float32
evaluation error of the closed form.  A draw that fails is drawn again (the next numbers of the generator, the next seed of a
trajectory); the smallest gap kept is printed.  Then every fixture passes this assert: a numpy float32 evaluation of
tests/third_order_ref.py, selection included, meets the fp64 class within HALF of the suite's tolerance (field_suite.TOL, tests/util.py:
rel_err) on every recorded quantity, the gradient block by block.  A fixture that cannot is drawn with smaller parameters (the scale is
halved); the tolerance does not move.  The class costs H^3 m^3 per vertex: 64 channels on at most 9 vertices, 29 vertices at 16."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import third_order_ref as tref  # noqa: E402
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402
from make_gru_gcn_golden import disconnected_molecule  # noqa: E402
from make_neighbourhood_golden import graph_text, isolated_molecule, parse_lists  # noqa: E402
from make_smp1d_golden import cycle_molecule, star_molecule  # noqa: E402
from util import rel_err  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")   # the reference tree (the directory that holds GraphFlow/)
HEADERS = ("GCN_3D.h", "GRU_GCN_3D.h", "RisiLayer3D.h", "KMax.h")
MOMENTUM = 0.9
HALF_TOL = 0.5e-5   # half of field_suite.TOL

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include <string>
// (both headers define a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_GCN_3D
#include "GCN_3D.h"
#undef INF
#define INF INF_of_GRU_GCN_3D
#include "GRU_GCN_3D.h"
#undef INF

static Vector *feature_of(GCN_3D &net) { return net.final_feature; }
static Vector *feature_of(GRU_GCN_3D &net) { return net.graph_feature; }

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
static void run(Net &net, DenseGraph *g, double target, int L, const char *save_to) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
    net.complete_computation_graph(g);
    net.target->value[0] = target;
    net.graph->forward();
    net.graph->backward();
    const int V = g->nVertices;
    for (int l = 1; l <= L; ++l)   // N_l(v) as the class filled it: the members of neighbor[v], by pointer
        for (int v = 0; v < V; ++v) {
            printf("%d ", (int)net.level[l]->neighbor[v]->vectors.size());
            for (size_t i = 0; i < net.level[l]->neighbor[v]->vectors.size(); ++i)
                for (int u = 0; u < V; ++u)
                    if (net.level[l]->neighbor[v]->vectors[i] == net.level[l - 1]->hidden[u]) printf("%d ", u);
        }
    printf("\n");
    for (int l = 0; l <= L; ++l)   // h_l[v], back to back
        for (int v = 0; v < V; ++v)
            for (int i = 0; i < net.level[l]->hidden[v]->size; ++i) printf("%.17g ", net.level[l]->hidden[v]->value[i]);
    printf("\n");
    for (int f = 0; f < feature_of(net)->size; ++f) printf("%.17g ", feature_of(net)->value[f]);
    printf("\n");
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

// form 6: GCN_3D, 7: GRU_GCN_3D.  Objects are leaked on purpose.  argv[1] (optional): where `run` saves the model.
int main(int argc, char **argv) {
    char mode[16];
    int form, maxV, L, H, F, D, R;
    double mom;
    if (scanf("%15s %d %d %d %d %d %d %d %lf", mode, &form, &maxV, &L, &H, &F, &D, &R, &mom) != 9) return 1;
    if (mode[0] == 'r') {   // run: one sample, given parameters
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        const char *save_to = argc > 1 ? argv[1] : "";
        if (form == 6) run(*new GCN_3D(L, maxV, F, H, D, R, mom), g, target, L, save_to);
        else run(*new GRU_GCN_3D(L, maxV, F, H, D, R, mom), g, target, L, save_to);
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
    if (form == 6) learn(*new GCN_3D(L, maxV, F, H, D, R, mom), nIter, nMol, &m[0], &tgt[0], lr);
    else learn(*new GRU_GCN_3D(L, maxV, F, H, D, R, mom), nIter, nMol, &m[0], &tgt[0], lr);
    return 0;
}
"""


def random_params(form, H, FD, L, rng, scale=1.0):
    """float32-exact parameters in registration order: multiples of 1/64 in [-1, 1] times `scale`"""
    return f32exact(np.concatenate([rng.integers(-64, 65, n) / 64.0 * scale for _, n in tref.blocks(form, H, FD, L)]))


def run(exe, text, *args):
    return subprocess.run([exe, *args], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def cases(form):
    """(name, adj, feature, target, nLevels, H, nDepth, max_Radius): the cases of make_gru_gcn_golden.py; 64 channels on the 9-vertex
    molecule only, the 29-vertex one at 16 and 8"""
    toys = {n: (a, f, t) for n, a, f, t in toy_molecules()}
    one = (np.zeros((1, 1), dtype=np.int32), np.array([[1.0, 0.5, 0.0, 0.25]]), 1.0)
    wide = {6: (64, 33, 16), 7: (32, 9, 8)}[form]
    return [("CH4",) + toys["CH4"] + (3, 5, 2, 1),
            ("NH3",) + toys["NH3"] + (1, 9, 0, 2),
            ("H2O",) + toys["H2O"] + (3, 16, 2, 5),
            ("C2H4_L0",) + toys["C2H4"] + (0, 17, 2, 1),
            ("C2H4",) + toys["C2H4"] + (3, 8, 0, 2),
            ("single",) + one + (1, 1, 2, 1),
            ("single_deep",) + one + (3, 5, 0, 0),
            ("isolated",) + isolated_molecule() + (3, 8, 2, 2),
            ("disconnected",) + disconnected_molecule() + (3, 9, 0, 5),
            ("cycle6",) + cycle_molecule(6) + (3, 16, 2, 2),
            ("star8_r0",) + star_molecule(8) + (3, 5, 0, 0),     # (radius 0: every neighbourhood is the vertex itself, n = 0)
            ("star8_far",) + star_molecule(8) + (3, 17, 2, 5),   # (a radius beyond the diameter 2: min(3, 5) = 3)
            ("syn9",) + synthetic_molecule(3, 9) + (1, wide[0], 0, 1),
            ("syn12",) + synthetic_molecule(5, 12) + (3, wide[1], 0, 2),
            ("syn29",) + synthetic_molecule(7, 29) + (3, wide[2], 2, 2),
            ("syn12_L0",) + synthetic_molecule(5, 12) + (0, 16, 2, 1)]


def head(form, maxV, L, H, F, D, R):
    return "%d %d %d %d %d %d %d %.17g\n" % (form, maxV, L, H, F, D, R, MOMENTUM)


def record(exe, params, form, adj, feat, tgt, L, H, D, R, save_to=None):
    V, F = feat.shape
    text = "run " + head(form, V, L, H, F, D, R) + graph_text(adj, feat) + "%.17g\n" % tgt
    text += " ".join("%.17g" % x for x in params) + "\n"
    lines = run(exe, text, *([save_to] if save_to else []))
    N = parse_lists(lines[0], L, V)
    pred, loss = (float(x) for x in lines[3].split())
    rec = {"lists": tref.lists_flat(N, L), "activations": np.array(lines[1].split(), dtype=np.float64),
           "graph_feature": np.array(lines[2].split(), dtype=np.float64), "result": np.array([pred, loss, tgt]),
           "grads": np.array(lines[4].split(), dtype=np.float64), "adj": adj.astype(np.int32), "feature": feat,
           "cfg": np.array([form, L, H, D, R, V], dtype=np.int32), "params": params.astype(np.float32)}
    assert rec["grads"].size == params.size and rec["graph_feature"].size == H
    assert N == tref.neighbourhoods(adj, L, R), "the class's neighbourhoods are not the restatement's"
    return rec, N


def fp32_error(rec, N, form, adj, feat, tgt, params, L, H, D, R):
    """the largest rel_err of a float32 evaluation of the restatement against the class's fp64 numbers, the gradient block by block"""
    r = tref.run(form, adj, feat, tgt, params, L, H, D, R, nbh=N, dtype=np.float32)
    errs = [rel_err(tref.activations(r), rec["activations"]), rel_err(r["graph_feature"], rec["graph_feature"]),
            rel_err([r["predict"]], rec["result"][:1]), rel_err([r["loss"]], rec["result"][1:2])]
    off = 0
    for _, n in tref.blocks(form, H, feat.shape[1] * (D + 1), L):
        errs.append(rel_err(r["grads"][off:off + n], rec["grads"][off:off + n]))
        off += n
    return max(errs)


def main():
    for h in HEADERS:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(2417)
    worst, smallest = 0.0, np.inf
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "third_order_driver.cpp"), os.path.join(tmp, "third_order_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for form in (6, 7):
            for name, adj, feat, tgt, L, H, D, R in cases(form):
                feat = f32exact(feat)
                FD, scale, draws = feat.shape[1] * (D + 1), 1.0, 0
                while True:
                    params = random_params(form, H, FD, L, rng, scale)
                    draws += 1
                    assert draws <= 200, name
                    gap = tref.run(form, adj, feat, tgt, params, L, H, D, R)["gap"]
                    if gap < tref.GAP:   # (the gap condition: drawn again)
                        continue
                    rec, N = record(exe, params, form, adj, feat, tgt, L, H, D, R)
                    e = fp32_error(rec, N, form, adj, feat, tgt, params, L, H, D, R)
                    if e <= HALF_TOL:
                        break
                    scale *= 0.5
                    assert scale > 1e-3, (name, e)
                tag = "n%d_%s" % (form, name)
                if len(adj) > 9 or H > 17:   # (every h_l[v] for the small cases)
                    del rec["activations"]
                for k, v in rec.items():
                    out["%s__%s" % (tag, k)] = v
                tags.append(tag)
                worst, smallest = max(worst, e), min(smallest, gap)
                print("%-18s %5d parameters (scale %g, draw %d), predict %10.6g, smallest gap %.3g, fp32 restatement within %.3g"
                      % (tag, params.size, scale, draws, rec["result"][0], gap, e), flush=True)
        out["tags"] = np.array(tags)
        # one save_model file: GCN_3D on CH4 at the case's parameters
        name, adj, feat, tgt, L, H, D, R = cases(6)[0]
        ck = os.path.join(tmp, "model.txt")
        record(exe, out["n6_CH4__params"].astype(np.float64), 6, adj, f32exact(feat), tgt, L, H, D, R, save_to=ck)
        with open(ck, "rb") as f:
            out["checkpoint__text"] = np.frombuffer(f.read(), dtype=np.uint8)
        out["checkpoint__tag"] = np.array("n6_CH4")
        # the weights each constructor's weights_initialization() draws after srand(seed), and three BatchLearn (Momentum) steps per form on
        # the four toy molecules as one batch: lr = 0.1 unless the loss rises at a step, then half of it, and so on; the seed is the first
        # from 23 on whose every step satisfies the gap condition
        tm = toy_molecules()
        mols = [(a, f32exact(f)) for _, a, f, _ in tm]
        mol_text = "".join(graph_text(a, f) for a, f in mols) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        targets = np.array([t for *_, t in tm], dtype=np.float64)
        maxV, nIter = 6, 3
        for form, L, H, D, R in ((6, 3, 6, 1, 2), (7, 2, 5, 1, 2)):
            seed, lr = 23, 0.1
            while True:
                lines = run(exe, "learn " + head(form, maxV, L, H, 4, D, R) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm)) + mol_text)
                losses = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
                p0 = np.array(lines[0].split(), dtype=np.float64)
                if not (losses[:, 1] <= losses[:, 0]).all():
                    lr *= 0.5
                    assert lr > 1e-4
                    continue
                gap = tref.momentum_steps(form, mols, targets, p0, L, H, D, R, nIter, lr, MOMENTUM)[2]
                if gap >= tref.GAP:
                    break
                seed, lr = seed + 1, 0.1
                assert seed < 200
            p = "train_n%d__" % form
            out[p + "cfg"] = np.array([form, L, H, D, R, maxV, seed, nIter], dtype=np.int32)
            out[p + "lr"] = np.array([lr])
            out[p + "momentum"] = np.array([MOMENTUM])
            out[p + "targets"] = targets
            out[p + "params0"] = p0
            out[p + "losses"] = losses
            out[p + "params"] = np.array(lines[2].split(), dtype=np.float64)
            assert p0.size == tref.n_params(form, H, 4 * (D + 1), L)
            smallest = min(smallest, gap)
            print("form %d: seed %d, three BatchLearn steps at lr %g, smallest gap %.3g, losses %s" % (form, seed, lr, gap, losses.ravel()))
    assert worst <= HALF_TOL and smallest >= tref.GAP
    np.savez_compressed(os.path.join(HERE, "smp_third_order.npz"), **out)
    print("wrote smp_third_order.npz: %d cases, one checkpoint, two %d-step Momentum trajectories with their initial weights; smallest gap "
          "kept %.3g of max|T|; the fp32 restatement within %.3g of the classes everywhere" % (len(tags), nIter, smallest, worst))


if __name__ == "__main__":
    main()
