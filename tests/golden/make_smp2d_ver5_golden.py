#!/usr/bin/env python3
"""Generate tests/golden/smp_2d_ver5.npz from the REAL reference class SMP_2D_ver5 (GraphFlow/SMP_2D_ver5.h).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_smp2d_ver5_golden.py
As make_smp2d_golden.py (whose helpers this file uses): a small driver that only includes the reference header is compiled into a
temporary directory outside the repository and fed through stdin / stdout.  Only data is recorded: the inputs, the receptive fields per
level, the reference's graph feature, prediction, loss and parameter gradients, for CH4 at nLevels = 2 the level activations and reduced
adjacencies, the weights weights_initialization() draws after srand(seed), and a three-step BatchLearn (Momentum) trajectory on the four
toy molecules.  Inputs are float32-representable.

Every fixture passes the two asserts of make_smp2d_golden.py: the read-out's worst-case fp32 rounding stays under half of the suite's
1e-5, and no pre-activation lies within MARGIN = 1e-3 max|z| of zero.  Parameters are redrawn until the second holds (random_params says
how they are drawn so that it can); the smallest margin kept is printed.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import f32exact, toy_molecules  # noqa: E402
from make_smp2d_golden import (ACTIVATIONS_OF, CONFIGS, D_ALL, MARGIN, MAXV, MOMENTUM, graph_text, molecules, parse_phi,  # noqa: E402
                               run)

REF_ROOT = os.environ.get("GF_REFERENCE", "")   # the reference tree (the directory that holds GraphFlow/)
HEADER = "SMP_2D_ver5.h"
FORM = 5

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
#include "SMP_2D_ver5.h"

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

static void print_params(SMP_2D_ver5 &net, bool grads) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", grads ? net.sgd->params[i]->gradient[j] : net.sgd->params[i]->value[j]);
    printf("\n");
}

// Objects are leaked on purpose: the model's and the executor's destructors free the same memory.
int main() {
    char mode[16];
    int maxV, L, C, F, D, wl;
    double mom;
    if (scanf("%15s %d %d %d %d %d %d %lf", mode, &maxV, &L, &C, &F, &D, &wl, &mom) != 8) return 1;
    if (mode[0] == 'r') {   // run: one sample, given parameters
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        SMP_2D_ver5 &net = *new SMP_2D_ver5(maxV, L, C, F, D, mom, wl != 0);
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
        for (int l = 0; l <= L; ++l)   // the activations f_l[v], [s][s][C] row-major, back to back
            for (int v = 0; v < V; ++v)
                for (int i = 0; i < net.level[l]->f[v]->size; ++i) printf("%.17g ", net.level[l]->f[v]->value[i]);
        printf("\n");
        for (int l = 1; l <= L; ++l)   // the reduced adjacencies, [s][s]
            for (int v = 0; v < V; ++v)
                for (int i = 0; i < net.level[l]->adj[v]->size; ++i) printf("%.17g ", net.level[l]->adj[v]->value[i]);
        printf("\n");
        printf("%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
        print_params(net, true);
        printf("%.17g %.17g\n", zmin, zmax);
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
    SMP_2D_ver5 &net = *new SMP_2D_ver5(maxV, L, C, F, D, mom, wl != 0);
    print_params(net, false);
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(nMol, &m[0], &tgt[0], lr);
        printf("%.17g %.17g ", r.first, r.second);
    }
    printf("\n");
    print_params(net, false);
    return 0;
}
"""


def smp2d_ver5_blocks(C, FD, L, maxV):
    """[(block name, size)] in registration order (SMP_2D_ver5.h:233-244): H; per level (lambda1_s[C], lambda2_s[C], b_s[C]) for
    s = 1..maxV, then K_l[C, 2C] (row = output channel, columns [eye half | one half]), then scalar_l[C]; W[C]."""
    out = [("H", C * FD)]
    for l in range(1, L + 1):
        for s in range(1, maxV + 1):
            out += [("lam1_%d_%d" % (l, s), C), ("lam2_%d_%d" % (l, s), C), ("b_%d_%d" % (l, s), C)]
        out += [("K_%d" % l, 2 * C * C), ("scalar_%d" % l, C)]
    out.append(("W", C))
    return out


def random_params(C, FD, L, maxV, rng):
    """float32-exact parameters in registration order, drawn so that the margin CAN hold: the one-sign-per-channel recipe of
    make_smp2d_golden.random_params carried through K_l.  With sigma the sign of a channel of the level below (H's rows have one sign
    each, the WL features are >= 0), scalar_l has sigma's sign, lambda1_s and lambda2_s one sign per channel for all sizes, so the
    concatenated channel d has the sign sg[d] = sign(lambda1) sigma on the eye half and sign(lambda2) sigma on the one half.  Every
    output channel c' draws a sign tau[c']: sign K[c'][d] = tau[c'] sg[d] and sign b_s[c'] = tau[c'] -- every term of z pulls the same
    way and |z| >= |b|.  A negative channel's K row and bias are drawn 100 times larger, so that behind the 0.01 slope both kinds of
    activation lie in comparable ranges.  W has the graph feature's sign per channel: the read-out's dot product does not cancel."""

    def signs(n):
        return rng.choice([-1.0, 1.0], n)

    def big(sg):   # 100 for the channels whose pre-activations are negative
        return np.where(sg > 0, 1.0, 100.0)

    sigma = signs(C)
    parts = [(sigma * big(sigma))[:, None] * rng.uniform(0.2, 0.21, (C, FD))]
    for l in range(1, L + 1):
        s1, s2, tau = signs(C), signs(C), signs(C)
        sg = np.concatenate([s1 * sigma, s2 * sigma])
        for size in range(1, maxV + 1):
            parts.append(s1 * 2.0 * rng.uniform(0.03, 0.05, C))
            parts.append(s2 * 2.0 * rng.uniform(0.03, 0.05, C) / size)
            parts.append(tau * big(tau) * rng.uniform(0.25, 0.4, C))
        parts.append((tau * big(tau))[:, None] * sg[None, :] * rng.uniform(0.5, 1.0, (C, 2 * C)) / (2.0 * C))
        parts.append(sigma * rng.uniform(0.2, 0.5, C))
        sigma = tau
    parts.append(signs(1)[0] * sigma * rng.uniform(0.5, 1.0, C) / (100.0 * C))
    return f32exact(np.concatenate([np.ravel(x) for x in parts]))


def head(maxV, L, C, F, D, wl):
    return "%d %d %d %d %d %d %.17g\n" % (maxV, L, C, F, D, wl, MOMENTUM)


def record(exe, rng, adj, feat, tgt, L, C, D, wl, maxV, activations):
    """one fixture: parameters are redrawn until the pre-activation margin holds"""
    V, F = feat.shape
    blocks = smp2d_ver5_blocks(C, F * (D + 1), L, maxV)
    for attempt in range(2000):
        params = random_params(C, F * (D + 1), L, maxV, rng)
        assert params.size == sum(n for _, n in blocks)
        text = "run " + head(maxV, L, C, F, D, wl) + graph_text(adj, feat) + "%.17g\n" % tgt
        text += " ".join("%.17g" % x for x in params) + "\n"
        lines = run(exe, text)
        rec = {"phi": parse_phi(lines[0], L, V, maxV), "graph_feature": np.array(lines[1].split(), dtype=np.float64)}
        if activations:
            rec["activations"] = np.array(lines[2].split(), dtype=np.float64)
            rec["adjacency"] = np.array(lines[3].split(), dtype=np.float64)
        pred, loss = (float(x) for x in lines[4].split())
        rec["predict"], rec["loss"] = np.array([pred]), np.array([loss])
        rec["grads"] = np.array(lines[5].split(), dtype=np.float64)
        zmin, zmax = (float(x) for x in lines[6].split())
        worst = np.abs(rec["graph_feature"] * params[-C:]).sum()
        assert rec["grads"].size == params.size and rec["graph_feature"].size == C, (rec["grads"].size, params.size)
        if zmin < MARGIN * zmax or worst * 2.0 ** -24 * C > 5e-6 * max(1.0, abs(pred)):
            continue
        rec.update(adj=adj.astype(np.int32), feature=feat, target=np.array([tgt], dtype=np.float64), params=params.astype(np.float32),
                   cfg=np.array([FORM, L, C, D, wl, maxV, 0], dtype=np.int32), margin=np.array([zmin / zmax]))
        return rec, attempt
    raise AssertionError("no draw with a pre-activation margin of %g" % MARGIN)


def main():
    if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", HEADER)):
        sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(2205)
    worst_margin = 1.0
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "smp2d_ver5_driver.cpp"), os.path.join(tmp, "smp2d_ver5_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for C, L in CONFIGS:
            for name, adj, feat, tgt, wl in molecules():
                rec, tries = record(exe, rng, adj, feat, tgt, L, C, D_ALL, wl, MAXV, name == ACTIVATIONS_OF and L == 2)
                tag = "f5_%s_c%d" % (name, C)
                for k, v in rec.items():
                    out["%s__%s" % (tag, k)] = v
                tags.append(tag)
                worst_margin = min(worst_margin, float(rec["margin"][0]))
                print("%-22s %4d parameters, predict %10.6g, margin %.3g (%d redraws)" % (tag, rec["params"].size, rec["predict"][0],
                                                                                       rec["margin"][0], tries))
        out["tags"] = np.array(tags)
        # the weights the constructor's weights_initialization() draws after srand(seed)
        tm = toy_molecules()
        mol_text = "".join(graph_text(a, f) for _, a, f, _ in tm) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        L, C, D, maxV, seed = 2, 3, 1, 6, 31
        lines = run(exe, "learn " + head(maxV, L, C, 4, D, 1) + "%d 0 0 %d\n" % (seed, len(tm)) + mol_text)
        out["init__cfg"] = np.array([FORM, L, C, D, 1, maxV, 0, seed], dtype=np.int32)
        out["init__params0"] = np.array(lines[0].split(), dtype=np.float64)
        assert out["init__params0"].size == sum(n for _, n in smp2d_ver5_blocks(C, 4 * (D + 1), L, maxV))
        # three BatchLearn (Momentum) steps on the four toy molecules as one batch, after srand(17)
        L, C, D, maxV, seed, nIter, lr = 2, 4, 1, 6, 17, 3, 1e-3
        lines = run(exe, "learn " + head(maxV, L, C, 4, D, 1) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm)) + mol_text)
        out["train__cfg"] = np.array([FORM, L, C, D, 1, maxV, 0, seed, nIter], dtype=np.int32)
        out["train__lr"] = np.array([lr])
        out["train__momentum"] = np.array([MOMENTUM])
        out["train__targets"] = np.array([t for *_, t in tm], dtype=np.float64)
        out["train__params0"] = np.array(lines[0].split(), dtype=np.float64)
        out["train__losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
        out["train__params"] = np.array(lines[2].split(), dtype=np.float64)
    assert worst_margin >= MARGIN
    np.savez_compressed(os.path.join(HERE, "smp_2d_ver5.npz"), **out)
    print("wrote smp_2d_ver5.npz: %d regression cases, one initial-weight record, a %d-step Momentum trajectory; smallest pre-activation "
          "margin %.3g of max |z|" % (len(tags), nIter, worst_margin))


if __name__ == "__main__":
    main()
