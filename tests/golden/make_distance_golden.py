#!/usr/bin/env python3
"""Generate tests/golden/smp_distance.npz from the REAL reference classes GCN_1D_Distance, GCN_2D_Distance and GCN_3D_Distance
(GraphFlow/GCN_1D_Distance.h, GCN_2D_Distance.h, GCN_3D_Distance.h, with Sort.h, RisiLayer2D.h, RisiLayer3D.h and KMax.h behind them).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_distance_golden.py
A small driver (below) that only includes the three reference headers is compiled into a temporary directory outside the repository and
fed through stdin / stdout.  Only data is recorded: per case the inputs (adjacency, features, the distance matrix), the neighbourhoods
N_l(v) as the class filled them, the reference's final feature [2 H], prediction, loss and parameter gradients in registration order, for
CH4 every h_l[v] of both channels; the weights each class draws after srand(seed); a three-step BatchLearn (Momentum 0.9) trajectory per
class; one save_model file.  Inputs are float32-representable; distances are real-valued (pairwise distances of random points rounded to
1/16), one case has an asymmetric matrix (which pins the column convention), one has tied and negative entries.

Every fixture passes two asserts, as its siblings': a numpy float32 evaluation of tests/distance_ref.py meets the fp64 class within HALF
of the suite's tolerance (field_suite.TOL, tests/util.py: rel_err) on every recorded quantity, the gradient block by block; and for the 3D
class the classes of RisiLayer3D around the KMax cut differ by at least third_order_ref.GAP = 1e-5 max|T| in both channels, at every step
of the trajectory too.  A draw that fails is drawn again or with smaller parameters (the scale is halved); no case is excused."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import distance_ref as dref  # noqa: E402
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402
from make_neighbourhood_golden import graph_text, isolated_molecule, parse_lists  # noqa: E402
from make_smp1d_golden import cycle_molecule  # noqa: E402
from third_order_ref import GAP  # noqa: E402
from util import rel_err  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")   # the reference tree (the directory that holds GraphFlow/)
HEADERS = ("GCN_1D_Distance.h", "GCN_2D_Distance.h", "GCN_3D_Distance.h", "Sort.h")
FORMS = (2, 3, 6)   # the neighbourhood form of GCN_1D_Distance, GCN_2D_Distance, GCN_3D_Distance
MOMENTUM = 0.9
HALF_TOL = 0.5e-5   # half of field_suite.TOL

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include <string>
// (every header defines a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_GCN_1D_Distance
#include "GCN_1D_Distance.h"
#undef INF
#define INF INF_of_GCN_2D_Distance
#include "GCN_2D_Distance.h"
#undef INF
#define INF INF_of_GCN_3D_Distance
#include "GCN_3D_Distance.h"
#undef INF

static DenseGraph *read_graph(int F) {
    int V;
    if (scanf("%d", &V) != 1) return NULL;
    DenseGraph *g = new DenseGraph(V, F);
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) scanf("%d", &g->adj[i][j]);
    for (int i = 0; i < V; ++i)
        for (int f = 0; f < F; ++f) scanf("%lf", &g->feature[i][f]);
    for (int i = 0; i < V; ++i)
        for (int j = 0; j < V; ++j) scanf("%lf", &g->distance[i][j]);
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
    for (int l = 1; l <= L; ++l)   // N_l(v) as the class filled it: the members of the vertex channel's neighbor[v], by pointer
        for (int v = 0; v < V; ++v) {
            printf("%d ", (int)net.chanel_vertex[l]->neighbor[v]->vectors.size());
            for (size_t i = 0; i < net.chanel_vertex[l]->neighbor[v]->vectors.size(); ++i)
                for (int u = 0; u < V; ++u)
                    if (net.chanel_vertex[l]->neighbor[v]->vectors[i] == net.chanel_vertex[l - 1]->hidden[u]) printf("%d ", u);
        }
    printf("\n");
    for (int l = 0; l <= L; ++l)   // [h^v_l[v] | h^d_l[v]], back to back
        for (int v = 0; v < V; ++v) {
            for (int i = 0; i < net.chanel_vertex[l]->hidden[v]->size; ++i) printf("%.17g ", net.chanel_vertex[l]->hidden[v]->value[i]);
            for (int i = 0; i < net.chanel_distance[l]->hidden[v]->size; ++i) printf("%.17g ", net.chanel_distance[l]->hidden[v]->value[i]);
        }
    printf("\n");
    for (int f = 0; f < net.final->size; ++f) printf("%.17g ", net.final->value[f]);
    printf("\n");
    printf("%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
    print_params(net, true);
    for (int v = 0; v < V; ++v)   // the sorted rows the distance channel read
        for (int i = 0; i < net.distance_sorted[v]->size; ++i) printf("%.17g ", net.distance_sorted[v]->value[i]);
    printf("\n");
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

// form 2: GCN_1D_Distance, 3: GCN_2D_Distance, 6: GCN_3D_Distance.  Objects are leaked on purpose.  argv[1] (optional): where `run` saves.
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
        if (form == 2) run(*new GCN_1D_Distance(L, maxV, F, H, D, R, mom), g, target, L, save_to);
        else if (form == 3) run(*new GCN_2D_Distance(L, maxV, F, H, D, R, mom), g, target, L, save_to);
        else run(*new GCN_3D_Distance(L, maxV, F, H, D, R, mom), g, target, L, save_to);
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
    if (form == 2) learn(*new GCN_1D_Distance(L, maxV, F, H, D, R, mom), nIter, nMol, &m[0], &tgt[0], lr);
    else if (form == 3) learn(*new GCN_2D_Distance(L, maxV, F, H, D, R, mom), nIter, nMol, &m[0], &tgt[0], lr);
    else learn(*new GCN_3D_Distance(L, maxV, F, H, D, R, mom), nIter, nMol, &m[0], &tgt[0], lr);
    return 0;
}
"""


def point_distances(V, rng, asymmetric=False):
    """pairwise distances of V random points in the cube [0, 3]^3, rounded to 1/16 (float32-exact); asymmetric: the upper triangle moved"""
    p = rng.uniform(0.0, 3.0, (V, 3))
    d = np.round(np.linalg.norm(p[:, None, :] - p[None, :, :], axis=2) * 16) / 16
    if asymmetric:
        d = d + np.triu(np.round(rng.uniform(0.25, 1.5, (V, V)) * 16) / 16, 1)
        assert not np.array_equal(d, d.T)
    return d


def tied_negative_distances(V):
    """ties, negative entries (they sort in front of the zeros of the diagonal and of the padding) and a non-zero diagonal entry"""
    d = np.full((V, V), 1.0)
    d[np.arange(V), np.arange(V)] = 0.0
    d[0, 1] = d[1, 0] = -0.5
    d[0, V - 1] = -0.5
    d[V - 1, V - 1] = 0.25
    d[1, V - 1] = d[V - 1, 1] = 1.0
    return d


def random_params(form, H, FD, M, L, rng, scale=1.0):
    """float32-exact parameters in registration order: multiples of 1/64 in [-1, 1] times `scale`; W2 of form 3 is divided by H (its
    aggregate is a sum over pairs of members)"""
    parts = []
    for name, n in dref.blocks(H, FD, M, L):
        w = rng.integers(-64, 65, n) / 64.0 * scale
        if name.startswith("W2") and form == 3:
            w = w / H
        parts.append(w)
    return f32exact(np.concatenate(parts))


def mol_text(adj, feat, dist):
    return graph_text(adj, feat) + " ".join("%.17g" % x for x in np.asarray(dist, dtype=np.float64).ravel()) + "\n"


def run(exe, text, *args):
    return subprocess.run([exe, *args], input=text, capture_output=True, text=True, check=True).stdout.split("\n")


def cases(form, rng):
    """(name, adj, feature, distance, target, nLevels, H, nDepth, max_Radius, max_nVertices): the cases the issue lists, each at the
    smallest shape that can still go wrong; the 3D class costs H^3 m^3 per vertex and channel, so its widths stay small"""
    toys = {n: (a, f, t) for n, a, f, t in toy_molecules()}
    one = (np.zeros((1, 1), dtype=np.int32), np.array([[1.0, 0.5, 0.0, 0.25]]), 1.0)
    syn = synthetic_molecule(5, 12)
    wide = 8 if form == 6 else 33

    def with_d(mol, dist=None, **kw):
        adj, feat, t = mol
        return (adj, feat, point_distances(len(adj), rng, **kw) if dist is None else dist, t)

    iso, cyc = isolated_molecule(), cycle_molecule(6)
    return [("CH4",) + with_d(toys["CH4"]) + (3, 5, 2, 1, 5),
            ("single",) + with_d(one) + (2, 5, 1, 1, 1),
            ("isolated",) + with_d(iso) + (3, 8, 2, 2, 6),
            ("cycle6",) + with_d(cyc) + (3, 16 if form != 6 else 9, 1, 2, 6),
            ("syn12_L0",) + with_d(syn) + (0, 17, 2, 1, 12),
            ("syn12",) + with_d(syn) + (3, wide, 0, 2, 12),
            ("NH3_padded",) + with_d(toys["NH3"]) + (2, 9, 1, 5, 7),            # V = 4 < M = 7: three zeros sort among the values
            ("CH4_asymmetric",) + with_d(toys["CH4"], asymmetric=True) + (2, 6, 0, 1, 6),
            ("H2O_tied_negative",) + with_d(toys["H2O"], tied_negative_distances(3)) + (3, 7, 2, 0, 5)]


def head(form, maxV, L, H, F, D, R):
    return "%d %d %d %d %d %d %d %.17g\n" % (form, maxV, L, H, F, D, R, MOMENTUM)


def record(exe, params, form, adj, feat, dist, tgt, L, H, D, R, M, save_to=None):
    V, F = feat.shape
    text = "run " + head(form, M, L, H, F, D, R) + mol_text(adj, feat, dist) + "%.17g\n" % tgt
    text += " ".join("%.17g" % x for x in params) + "\n"
    lines = run(exe, text, *([save_to] if save_to else []))
    N = parse_lists(lines[0], L, V)
    pred, loss = (float(x) for x in lines[3].split())
    rec = {"lists": dref.lists_flat(N, L), "activations": np.array(lines[1].split(), dtype=np.float64),
           "final_feature": np.array(lines[2].split(), dtype=np.float64), "result": np.array([pred, loss, tgt]),
           "grads": np.array(lines[4].split(), dtype=np.float64), "x_d": np.array(lines[5].split(), dtype=np.float64).reshape(V, M),
           "adj": adj.astype(np.int32), "feature": feat, "distance": np.asarray(dist, dtype=np.float64),
           "cfg": np.array([form, L, H, D, R, V, M], dtype=np.int32), "params": params.astype(np.float32)}
    assert rec["grads"].size == params.size and rec["final_feature"].size == 2 * H
    assert N == dref.neighbourhoods(adj, L, R), "the class's neighbourhoods are not the restatement's"
    return rec


def fp32_error(rec, form, adj, feat, dist, tgt, params, L, H, D, R, M):
    """the largest rel_err of a float32 evaluation of the restatement against the class's fp64 numbers, the gradient block by block"""
    r = dref.run(form, adj, feat, dist, tgt, params, L, H, D, M, R, dtype=np.float32)
    assert np.array_equal(r["x_d"].astype(np.float64), rec["x_d"])   # (fp32-exact inputs: the sorted rows agree exactly)
    errs = [rel_err(dref.activations(r), rec["activations"]), rel_err(r["final_feature"], rec["final_feature"]),
            rel_err([r["predict"]], rec["result"][:1]), rel_err([r["loss"]], rec["result"][1:2])]
    off = 0
    for _, n in dref.blocks(H, feat.shape[1] * (D + 1), M, L):
        errs.append(rel_err(r["grads"][off:off + n], rec["grads"][off:off + n]))
        off += n
    return max(errs)


def main():
    for h in HEADERS:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(2429)
    worst, smallest = 0.0, np.inf
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "distance_driver.cpp"), os.path.join(tmp, "distance_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for form in FORMS:
            for name, adj, feat, dist, tgt, L, H, D, R, M in cases(form, rng):
                feat, dist = f32exact(feat), f32exact(dist)
                FD, scale, draws = feat.shape[1] * (D + 1), 1.0, 0
                while True:
                    params = random_params(form, H, FD, M, L, rng, scale)
                    draws += 1
                    assert draws <= 200, name
                    gap = dref.run(form, adj, feat, dist, tgt, params, L, H, D, M, R)["gap"]
                    if gap < GAP:   # (the gap condition of the 3D class, both channels: drawn again)
                        continue
                    rec = record(exe, params, form, adj, feat, dist, tgt, L, H, D, R, M)
                    e = fp32_error(rec, form, adj, feat, dist, tgt, params, L, H, D, R, M)
                    if e <= HALF_TOL:
                        break
                    scale *= 0.5
                    assert scale > 1e-3, (name, e)
                tag = "n%d_%s" % (form, name)
                if name != "CH4":   # (every h_l[v] of both channels for CH4)
                    del rec["activations"]
                for k, v in rec.items():
                    out["%s__%s" % (tag, k)] = v
                tags.append(tag)
                worst, smallest = max(worst, e), min(smallest, gap)
                print("%-24s %5d parameters (scale %g, draw %d), predict %10.6g, smallest gap %.3g, fp32 restatement within %.3g"
                      % (tag, params.size, scale, draws, rec["result"][0], gap, e), flush=True)
        out["tags"] = np.array(tags)
        # one save_model file: GCN_2D_Distance on CH4 at the case's parameters (the file's order is not the registration order)
        name, adj, feat, dist, tgt, L, H, D, R, M = cases(3, np.random.default_rng(0))[0]
        ck = os.path.join(tmp, "model.txt")
        record(exe, out["n3_CH4__params"].astype(np.float64), 3, adj, f32exact(feat), out["n3_CH4__distance"], tgt, L, H, D, R, M, save_to=ck)
        with open(ck, "rb") as f:
            out["checkpoint__text"] = np.frombuffer(f.read(), dtype=np.uint8)
        out["checkpoint__tag"] = np.array("n3_CH4")
        # the weights each constructor's weights_initialization() draws after srand(seed), and three BatchLearn (Momentum) steps per class on
        # the four toy molecules as one batch: lr = 0.1 unless the loss rises at a step, then half of it, and so on; the seed is the first
        # from 23 on whose every step satisfies the gap condition
        tm = toy_molecules()
        mols = [(a, f32exact(f), f32exact(point_distances(len(a), rng))) for _, a, f, _ in tm]
        text = "".join(mol_text(a, f, d) for a, f, d in mols) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        targets = np.array([t for *_, t in tm], dtype=np.float64)
        maxV, nIter = 7, 3   # (one more than the largest molecule: every row is padded)
        for i, (a, f, d) in enumerate(mols):
            out["train__distance_%d" % i] = d
        for form, L, H, D, R in ((2, 3, 6, 1, 2), (3, 2, 5, 1, 1), (6, 2, 5, 1, 2)):
            seed, lr = 23, 0.1
            while True:
                lines = run(exe, "learn " + head(form, maxV, L, H, 4, D, R) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm)) + text)
                losses = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
                p0 = np.array(lines[0].split(), dtype=np.float64)
                if not (losses[:, 1] <= losses[:, 0]).all():
                    lr *= 0.5
                    assert lr > 1e-4
                    continue
                ref_losses, ref_p, gap = dref.momentum_steps(form, mols, targets, p0, L, H, D, maxV, R, nIter, lr, MOMENTUM)
                if gap >= GAP:
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
            assert p0.size == dref.n_params(H, 4 * (D + 1), maxV, L)
            smallest = min(smallest, gap)
            print("form %d: seed %d, three BatchLearn steps at lr %g, smallest gap %.3g, losses %s" % (form, seed, lr, gap, losses.ravel()))
    assert worst <= HALF_TOL and smallest >= GAP
    np.savez_compressed(os.path.join(HERE, "smp_distance.npz"), **out)
    print("wrote smp_distance.npz: %d cases, one checkpoint, three %d-step Momentum trajectories with their initial weights; smallest gap "
          "kept %.3g of max|T|; the fp32 restatement within %.3g of the classes everywhere" % (len(tags), nIter, smallest, worst))


if __name__ == "__main__":
    main()
