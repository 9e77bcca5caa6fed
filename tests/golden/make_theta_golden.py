#!/usr/bin/env python3
"""Generate tests/golden/smp_theta.npz and smp_theta_physics.npz from the REAL reference classes SMP_theta, SMP_theta_physics and
SMP_theta_pairgraphs (GraphFlow/SMP_theta.h, SMP_theta_physics.h, SMP_theta_pairgraphs.h).

Run where the reference tree is available:   python tests/golden/make_theta_golden.py
A small driver (below) that includes the reference headers is compiled into a temporary directory outside the repository and fed
through stdin / stdout.  Only data is recorded: the inputs, the receptive fields per level, the reference's prediction, graph
feature, loss and parameter gradients, the weights weights_initialization() draws after srand(seed), and a three-step BatchLearn
(Adam) trajectory.  Inputs are float32-representable so the fp32 device path and the fp64 checkers see identical numbers.
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

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "SMP_theta.h"
#include "SMP_theta_physics.h"
#include "SMP_theta_pairgraphs.h"

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

template <class Net>
static void run_one(Net &net, DenseGraph *g, double target, int L) {
    read_params(net);
    net.complete_computation_graph(g);
    net.target->value[0] = target;
    net.graph->forward();
    net.graph->backward();
    print_phi(net.level, L, g->nVertices);
    print_run(net);
}

template <class Net>
static void learn(Net &net, int nIter, int nMol, DenseGraph **m, double *tgt, double lr) {
    print_params(net);
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(nMol, m, tgt, lr);
        printf("%.17g %.17g ", r.first, r.second);
    }
    printf("\n");
    print_params(net);
}

// towers 0: SMP_theta, 1: SMP_theta_physics, 2: SMP_theta_pairgraphs.  Objects are leaked on purpose: the models' and the executors'
// destructors free the same memory.
int main() {
    char mode[16];
    int towers, maxV1, maxV2, cap, L, C, F1, F2, D, wl;
    if (scanf("%15s %d %d %d %d %d %d %d %d %d %d", mode, &towers, &maxV1, &maxV2, &cap, &L, &C, &F1, &F2, &D, &wl) != 11) return 1;
    if (mode[0] == 'r') {   // run: one sample, given parameters -> fields, feature row, prediction, loss, gradients
        DenseGraph *g1 = read_graph(F1), *g2 = towers == 2 ? read_graph(F2) : NULL;
        double target;
        scanf("%lf", &target);
        if (towers == 0) {
            run_one(*new SMP_theta(maxV1, cap, L, C, F1, D, wl != 0), g1, target, L);
        } else if (towers == 1) {
            run_one(*new SMP_theta_physics(maxV1, cap, L, C, F1), g1, target, L);
        } else {
            SMP_theta_pairgraphs &net = *new SMP_theta_pairgraphs(maxV1, maxV2, cap, L, C, F1, F2);
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
    if (towers == 0) {
        learn(*new SMP_theta(maxV1, cap, L, C, F1, D, wl != 0), nIter, nMol, &m1[0], &tgt[0], lr);
    } else if (towers == 1) {
        learn(*new SMP_theta_physics(maxV1, cap, L, C, F1), nIter, nMol, &m1[0], &tgt[0], lr);
    } else {
        SMP_theta_pairgraphs &net = *new SMP_theta_pairgraphs(maxV1, maxV2, cap, L, C, F1, F2);
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


def channels(C, L, tower):
    return [max(1, C >> l) if tower else C for l in range(L + 1)]


def theta_blocks(C, FD, L, maxV, tower=False, name=""):
    """[(block name, size)] of one SMP_theta body in registration order (SMP_theta.h:254-264): H; per level (lambda1_s, lambda2_s,
    b_s[C_l]) for s = 1..maxV, then K_l[2 C_{l-1}, C_l]; W[C] unless a tower."""
    c = channels(C, L, tower)
    out = [(name + "H", C * FD)]
    for l in range(1, L + 1):
        for s in range(1, maxV + 1):
            out += [("%slam1_%d_%d" % (name, l, s), 1), ("%slam2_%d_%d" % (name, l, s), 1), ("%sb_%d_%d" % (name, l, s), c[l])]
        out.append(("%sK_%d" % (name, l), 2 * c[l - 1] * c[l]))
    if not tower:
        out.append(("W", C))
    return out


def model_blocks(towers, C, L, F, maxV):
    """Registration order of SMP_theta (towers 0), SMP_theta_physics (1: H, levels, W1, W2) and SMP_theta_pairgraphs (2: H_1, H_2, the
    levels with the towers interleaved, W1, W2, W3)."""
    if towers == 0:
        return theta_blocks(C, F[0], L, maxV[0])
    w = sum(channels(C, L, True))
    t = [theta_blocks(C, F[i], L, maxV[i], True, "t%d_" % (i + 1)) for i in range(towers)]
    out = [b[0] for b in t]
    per = [maxV[i] * 3 + 1 for i in range(towers)]
    for l in range(L):
        for i in range(towers):
            out += t[i][1 + l * per[i]:1 + (l + 1) * per[i]]
    if towers == 1:
        nh = w // 2
        return out + [("W1", nh * w), ("W2", nh)]
    nTot = 2 * w
    h1 = max(nTot // 2, 10)
    h2 = max(h1 // 2, 10)
    return out + [("W1", h1 * nTot), ("W2", h2 * h1), ("W3", h2)]


def random_params(blocks, rng):
    """float32-exact parameters.  The per-size scalars let both halves of K_l contribute alike; the matrices are scaled by
    their fan-in (a block of n = rows x columns elements with comparable sides has about sqrt(n) inputs per output), so that activations stay
    of order one through the levels and the prediction -- an inner product of the graph feature -- is not a difference of large numbers
    that fp32 cannot resolve to the suite's 1e-5."""
    parts = []
    for name, n in blocks:
        if "lam" in name:   # (lambda2_s multiplies a sum over the s positions of the field: scaled by 1 / s)
            size = int(name.rsplit("_", 1)[1]) if "lam2" in name else 1
            parts.append(rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n) / (2.0 * size))
        elif "b_" in name:
            parts.append(rng.uniform(-0.1, 0.1, n))
        elif name in ("W", "W2", "W3") and not name.startswith("t"):
            parts.append(rng.uniform(-1, 1, n) / np.sqrt(n))
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


def path_molecule(V, F=4):
    """V atoms in a chain (V = 1: a single atom, whose fields hold one position at every level)"""
    adj = np.zeros((V, V), dtype=np.int32)
    for v in range(V - 1):
        adj[v, v + 1] = adj[v + 1, v] = 1
    feat = np.zeros((V, F))
    feat[np.arange(V), np.arange(V) % F] = 1.0
    return adj, feat, float(V)


def star_molecule(deg, F=4):
    adj = np.zeros((deg + 1, deg + 1), dtype=np.int32)
    adj[0, 1:] = adj[1:, 0] = 1
    feat = np.zeros((deg + 1, F))
    feat[0, 0] = 1.0
    feat[1:, 1] = 1.0
    feat[2, 2] = 0.5   # (leaves that differ: their WL ranks do too)
    return adj, feat, float(deg + 1)


def small_molecules():
    """1, 2, 5 and 9 vertices: an atom, a bond, CH4 of the reference's tests, a synthetic 9-atom molecule (4 features each)"""
    ch4 = toy_molecules()[0]
    a9, f9, t9 = synthetic_molecule(6, 9)
    return [("v1",) + path_molecule(1), ("v2",) + path_molecule(2), ("v5", ch4[1], ch4[2], ch4[3]), ("v9", a9, f9[:, :4] + f9[:, 4:5] * 0.5, t9)]


def theta_cases():
    """(tag, adj, feature, target, (L, C, D, wl, cap, maxV))"""
    out = []
    for name, adj, feat, tgt in small_molecules():
        V = len(adj)
        for C, wl in ((8, 1), (10, 0), (1, 1)):
            out.append(("%s_c%d" % (name, C), adj, feat, tgt, (2, C, 2, wl, 10, 10)))   # no cap
    adj, feat, tgt = star_molecule(5)
    out.append(("star5_cap4", adj, feat, tgt, (2, 8, 1, 1, 4, 6)))      # the cap drops the centre's whole hop-1 shell at level 1
    out.append(("star5_cap4_nowl", adj, feat, tgt, (2, 10, 1, 0, 4, 6)))
    adj, feat, tgt = synthetic_molecule(5, 12)
    out.append(("syn12_cap6_L3", adj, feat, tgt, (3, 8, 2, 1, 6, 12)))
    return out


def tower_cases():
    """(tag, towers, (adj, feat), (adj2, feat2) or None, target, L, C, cap)"""
    g12 = synthetic_molecule(5, 12)
    g9 = synthetic_molecule(6, 9)
    return [
        ("phys_c16", 1, g12[:2], None, g12[2], 2, 16, 6),     # widths 16 / 8 / 4
        ("phys_c10", 1, g9[:2], None, g9[2], 2, 10, 9),       # widths 10 / 5 / 2, no cap
        ("pair_c16", 2, g12[:2], g9[:2], g12[2], 2, 16, 6),
    ]


def head(towers, maxV1, maxV2, cap, L, C, F1, F2, D, wl):
    return "%d %d %d %d %d %d %d %d %d %d\n" % (towers, maxV1, maxV2, cap, L, C, F1, F2, D, wl)


def main():
    for h in ("SMP_theta.h", "SMP_theta_physics.h", "SMP_theta_pairgraphs.h"):
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %s" % REF_ROOT)
    out, pout = {}, {}
    rng = np.random.default_rng(7311)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "theta_driver.cpp"), os.path.join(tmp, "theta_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for tag, adj, feat, tgt, (L, C, D, wl, cap, maxV) in theta_cases():
            V, F = feat.shape
            params = random_params(model_blocks(0, C, L, [F * (D + 1)], [maxV]), rng)
            text = "run " + head(0, maxV, 0, cap, L, C, F, 0, D, wl) + graph_text(adj, feat) + "%.17g\n" % tgt
            text += " ".join("%.17g" % x for x in params) + "\n"
            lines = run(exe, text)
            p = "theta_" + tag
            out[p + "__phi"] = parse_phi(lines[0], L, V, cap)
            g = np.array(lines[1].split(), dtype=np.float64)
            pred, loss = (float(x) for x in lines[2].split())
            grads = np.array(lines[3].split(), dtype=np.float64)
            assert grads.size == params.size and g.size == C, (tag, grads.size, params.size)
            # the fixture is one fp32 can resolve: the worst-case rounding of the read-out's inner product stays below half of the suite's 1e-5
            assert np.abs(g * params[-C:]).sum() * 2.0 ** -24 * C <= 5e-6 * max(1.0, abs(pred)), (tag, pred)
            out[p + "__adj"], out[p + "__feature"], out[p + "__target"] = adj.astype(np.int32), feat, np.array([tgt], dtype=np.float64)
            out[p + "__cfg"] = np.array([L, C, D, wl, cap, maxV], dtype=np.int32)
            out[p + "__params"] = params.astype(np.float32)
            out[p + "__graph_feature"], out[p + "__predict"], out[p + "__loss"], out[p + "__grads"] = g, np.array([pred]), np.array([loss]), grads
            tags.append(tag)
            print("%-18s fields up to %d positions, %d parameters, predict %.6g" % (tag, int(out[p + "__phi"][..., 0].max()), params.size, pred))
        out["tags"] = np.array(tags)
        # three BatchLearn steps on the four small molecules as one batch, from the constructor's weights after srand(13)
        mols = small_molecules()
        L, C, D, cap, maxV, seed, nIter, lr = 2, 8, 2, 10, 10, 13, 3, 1e-3
        text = "learn " + head(0, maxV, 0, cap, L, C, 4, 0, D, 1) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(mols))
        text += "".join(graph_text(a, f) for _, a, f, _ in mols) + " ".join("%.17g" % t for *_, t in mols) + "\n"
        lines = run(exe, text)
        out["train__cfg"] = np.array([L, C, D, cap, maxV, seed, nIter], dtype=np.int32)
        out["train__lr"] = np.array([lr])
        out["train__targets"] = np.array([t for *_, t in mols], dtype=np.float64)
        out["train__params0"] = np.array(lines[0].split(), dtype=np.float64)
        out["train__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
        out["train__params"] = np.array(lines[2].split(), dtype=np.float64)

        ptags = []
        for tag, towers, ga, gb, tgt, L, C, cap in tower_cases():
            V1, F1 = ga[1].shape
            V2, F2 = gb[1].shape if gb else (0, 0)
            maxV1, maxV2 = max(V1, 10), max(V2, 10)
            params = random_params(model_blocks(towers, C, L, [F1, F2], [maxV1, maxV2]), rng)
            text = "run " + head(towers, maxV1, maxV2, cap, L, C, F1, F2, 0, 0) + graph_text(*ga)
            if gb:
                text += graph_text(*gb)
            text += "%.17g\n" % tgt + " ".join("%.17g" % x for x in params) + "\n"
            lines = run(exe, text)
            p = "tphys_" + tag
            pout[p + "__phi"] = parse_phi(lines[0], L, V1, cap)
            if gb:
                pout[p + "__phi2"] = parse_phi(lines[1], L, V2, cap)
                lines = lines[1:]
            g = np.array(lines[1].split(), dtype=np.float64)
            pred, loss = (float(x) for x in lines[2].split())
            grads = np.array(lines[3].split(), dtype=np.float64)
            assert grads.size == params.size, (tag, grads.size, params.size)
            assert g.size == towers * sum(channels(C, L, True)), (tag, g.size)
            pout[p + "__adj"], pout[p + "__feature"] = ga[0].astype(np.int32), ga[1]
            if gb:
                pout[p + "__adj2"], pout[p + "__feature2"] = gb[0].astype(np.int32), gb[1]
            pout[p + "__target"] = np.array([tgt], dtype=np.float64)
            pout[p + "__cfg"] = np.array([towers, L, C, cap, maxV1, maxV2], dtype=np.int32)
            pout[p + "__params"] = params.astype(np.float32)
            pout[p + "__graph_feature"], pout[p + "__predict"], pout[p + "__loss"] = g, np.array([pred]), np.array([loss])
            pout[p + "__grads"] = grads
            ptags.append(tag)
            print("%-18s %d parameters, predict %.6g" % (tag, params.size, pred))
        pout["tags"] = np.array(ptags)
        # three BatchLearn steps of SMP_theta_physics on the four toy molecules of the reference's tests, after srand(7)
        tm = toy_molecules()
        L, C, cap, maxV, seed, nIter, lr = 2, 16, 4, 10, 7, 3, 1e-3
        text = "learn " + head(1, maxV, 0, cap, L, C, 4, 0, 0, 0) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm))
        text += "".join(graph_text(a, f) for _, a, f, _ in tm) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        lines = run(exe, text)
        pout["train__cfg"] = np.array([1, L, C, cap, maxV, seed, nIter], dtype=np.int32)
        pout["train__lr"] = np.array([lr])
        pout["train__targets"] = np.array([t for *_, t in tm], dtype=np.float64)
        pout["train__params0"] = np.array(lines[0].split(), dtype=np.float64)
        pout["train__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
        pout["train__params"] = np.array(lines[2].split(), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "smp_theta.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "smp_theta_physics.npz"), **pout)
    print("wrote smp_theta.npz (%d cases) and smp_theta_physics.npz (%d cases), each with a %d-step BatchLearn trajectory" % (len(tags), len(ptags), nIter))


if __name__ == "__main__":
    main()
