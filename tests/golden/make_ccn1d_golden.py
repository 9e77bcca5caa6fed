#!/usr/bin/env python3
"""Generate tests/golden/ccn_1d.npz, ccn_1d_demo.npz and ccn_1d_checkpoint.dat from the REAL reference class CCN_1D (GraphFlow/CCN_1D.h).

Run where the reference tree is available:   python tests/golden/make_ccn1d_golden.py
A small driver (below) that includes the reference header is compiled into a temporary directory outside the repository and fed through
stdin / stdout.  Only data is recorded: the inputs, the receptive fields per level of both towers, the reference's graph feature,
prediction, loss and parameter gradients, the weights weights_initialization() draws after srand(seed), a three-step BatchLearn (Adam)
trajectory with the Predict values afterwards, and the text checkpoint the real class's save_model writes after those steps (with the
Predict values of a second network that load_model'ed it).  Inputs are float32-representable so the fp32 device path and the fp64
checkers see identical numbers.

Two properties are enforced on every fixture, as in make_smp2d_golden.py: fp32 can resolve the prediction to the suite's 1e-5, and no
pre-activation (level 0, the levels, the read-outs' column sums, the two hidden layers) lies within MARGIN = 1e-3 max|z| of zero, so that
fp32 cannot take the other branch of a LeakyReLU.  random_params says how the parameters are drawn so that the second can hold; they are
redrawn until it does, and the smallest margin kept is printed.

What runs at the demo's settings (tests/test_CCN_1D.cpp: 10 / 10 vertices, cap 6, 16 channels, decay 0.5) has a file of its own,
ccn_1d_demo.npz, so that no committed file reaches 1 MiB: the L = 7 case (a 256 -> 128 -> 64 head, 51 000 parameters), the L = 3
trajectory (train__*) and the loss pairs of three steps at L = 7 (train7__*)."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402
from make_theta_golden import graph_text, parse_phi, run, star_molecule  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "/root/reference")
MARGIN = 1e-3      # smallest |z| / max |z| a fixture may hold
NEG = 20.0         # a channel whose pre-activations are negative is drawn this much larger (its activations: 0.2 of a positive one's)
MIN_CHANELS = 16   # CCN_1D_MINIMUM_NUMBER_OF_CHANELS

DRIVER = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "CCN_1D.h"

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
        if (a < zmin) zmin = a;
        if (a > zmax) zmax = a;
    }
}

static void print_tower(CCN_1D::Level **level, ShrinkMatrix ***shrinked, int L, int V) {
    for (int l = 0; l <= L; ++l)
        for (int v = 0; v < V; ++v) {
            printf("%d ", (int)level[l]->phi[v].size());
            for (size_t i = 0; i < level[l]->phi[v].size(); ++i) printf("%d ", level[l]->phi[v][i]);
            if (l == 0) margins(level[0]->f_transpose[v]->value, level[0]->f_transpose[v]->size);
            else margins(level[l]->add[v]->value, level[l]->add[v]->size);
            margins(shrinked[l][v]->value, shrinked[l][v]->size);
        }
    printf("\n");
}

static void print_params(CCN_1D &net, bool grads) {
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) printf("%.17g ", grads ? net.sgd->params[i]->gradient[j] : net.sgd->params[i]->value[j]);
    printf("\n");
}

// The networks are leaked on purpose: the model's and the executor's destructors free the same memory.
int main() {
    char mode[16], ckpt[512];
    int maxV1, maxV2, cap, L, C, F1, F2;
    double decay;
    if (scanf("%15s %d %d %d %d %d %d %d %lf", mode, &maxV1, &maxV2, &cap, &L, &C, &F1, &F2, &decay) != 9) return 1;
    if (mode[0] == 'r') {   // run: one pair, given parameters -> fields, feature row, prediction, loss, gradients, margins
        DenseGraph *g1 = read_graph(F1), *g2 = read_graph(F2);
        double target;
        scanf("%lf", &target);
        CCN_1D &net = *new CCN_1D(maxV1, maxV2, cap, L, C, F1, F2, decay);
        for (size_t i = 0; i < net.sgd->params.size(); ++i)
            for (int j = 0; j < net.sgd->params[i]->size; ++j) scanf("%lf", &net.sgd->params[i]->value[j]);
        net.complete_computation_graph(g1, g2);
        net.target->value[0] = target;
        net.graph->forward();
        net.graph->backward();
        print_tower(net.level_1, net.shrinked_1, L, g1->nVertices);
        print_tower(net.level_2, net.shrinked_2, L, g2->nVertices);
        margins(net.hidden_1->value, net.hidden_1->size);
        margins(net.hidden_2->value, net.hidden_2->size);
        for (int f = 0; f < net.graph_feature->size; ++f) printf("%.17g ", net.graph_feature->value[f]);
        printf("\n%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
        print_params(net, true);
        double worst = 0.0;   // sum of |terms| of the last inner product: what fp32 has to resolve the prediction against
        for (int j = 0; j < net.W3->size; ++j) worst += fabs(net.hidden_relu_2->value[j] * net.W3->value[j]);
        printf("%.17g %.17g %.17g\n", zmin, zmax, worst);
        return 0;
    }
    // learn: srand(seed), the constructor's weights, nIter x BatchLearn, Predict of every pair, save_model, load_model into a second
    // network, its Predict of every pair
    int seed, nIter, nMol;
    double lr;
    scanf("%d %d %lf %d %511s", &seed, &nIter, &lr, &nMol, ckpt);
    std::vector<DenseGraph *> m1(nMol), m2(nMol);
    std::vector<double> tgt(nMol);
    for (int m = 0; m < nMol; ++m) m1[m] = read_graph(F1);
    for (int m = 0; m < nMol; ++m) m2[m] = read_graph(F2);
    for (int m = 0; m < nMol; ++m) scanf("%lf", &tgt[m]);
    srand((unsigned)seed);
    CCN_1D &net = *new CCN_1D(maxV1, maxV2, cap, L, C, F1, F2, decay);
    print_params(net, false);
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(nMol, &m1[0], &m2[0], &tgt[0], lr);
        printf("%.17g %.17g ", r.first, r.second);
    }
    printf("\n");
    print_params(net, false);
    for (int m = 0; m < nMol; ++m) printf("%.17g ", net.Predict(m1[m], m2[m]));
    printf("\n");
    net.save_model(std::string(ckpt));
    CCN_1D &second = *new CCN_1D(maxV1, maxV2, cap, L, C, F1, F2, decay);
    second.load_model(std::string(ckpt));
    for (int m = 0; m < nMol; ++m) printf("%.17g ", second.Predict(m1[m], m2[m]));
    printf("\n");
    return 0;
}
"""


def channels(C, L, decay):
    """CCN_1D.h:200, :217, the product in double as the class writes it"""
    c = [C]
    for _ in range(L):
        c.append(max(int(math.ceil(c[-1] * decay)), MIN_CHANELS))
    return c


def head_widths(C, L, decay):
    """nTotal, nHidden_1, nHidden_2 (CCN_1D.h:343-353)"""
    n = 2 * sum(channels(C, L, decay))
    h1 = max(int(math.ceil(n * decay)), MIN_CHANELS)
    return n, h1, max(int(math.ceil(h1 * decay)), MIN_CHANELS)


def tower_blocks(t, C, F, L, maxV, decay):
    """[H], then per level [(lambda1_s, lambda2_s, b_s[C_l]) for s = 1..maxV, K_l[2 C_{l-1}, C_l]] of tower t (1 or 2)"""
    c = channels(C, L, decay)
    out = [[("t%d_H" % t, C * F)]]
    for l in range(1, L + 1):
        lv = []
        for s in range(1, maxV + 1):
            lv += [("t%d_lam1_%d_%d" % (t, l, s), 1), ("t%d_lam2_%d_%d" % (t, l, s), 1), ("t%d_b_%d_%d" % (t, l, s), c[l])]
        lv.append(("t%d_K_%d" % (t, l), 2 * c[l - 1] * c[l]))
        out.append(lv)
    return out


def model_blocks(C, L, F, maxV, decay):
    """Registration order of CCN_1D (CCN_1D.h:381-403): H_1, H_2; for l = 1..L tower 1's max_nVertices_1 size entries and K1_l, then
    tower 2's max_nVertices_2 entries and K2_l; W1, W2, W3."""
    t = [tower_blocks(i + 1, C, F[i], L, maxV[i], decay) for i in range(2)]
    out = t[0][0] + t[1][0]
    for l in range(1, L + 1):
        out += t[0][l] + t[1][l]
    n, h1, h2 = head_widths(C, L, decay)
    return out + [("W1", h1 * n), ("W2", h2 * h1), ("W3", h2)]


def random_params(C, L, F, maxV, decay, colsign, rng):
    """float32-exact parameters in registration order, drawn so that the margin CAN hold: a 12-vertex tower has thousands of
    pre-activations, and independent draws never keep all of them 1e-3 max|z| away from zero.  So every channel of every level gets one
    sign.  With colsign the sign of each feature column (the inputs' columns have one sign each) H's rows have one sign sigma each; at a
    level lambda1 and lambda2 have one sign for all sizes, K_top / K_bot the sign lambda * sigma_in * tau_out and b_s the sign tau_out:
    every term of z pulls the same way and |z| >= |b|.  The head's two layers and W3 follow the same rule, so the prediction does not
    cancel either.  A negative channel is drawn NEG times larger: behind the 0.01 slope its activations are 0.2 of a positive one's."""
    c = channels(C, L, decay)

    def signs(n):
        return rng.choice([-1.0, 1.0], n)

    def big(sg):
        return np.where(sg > 0, 1.0, NEG)

    sigma = [signs(C), signs(C)]
    tower = []
    for t in range(2):
        parts = [[(sigma[t] * big(sigma[t]))[:, None] * colsign[t][None, :] * rng.uniform(0.3, 0.6, (C, F[t]))]]
        sg = sigma[t]
        feat_signs = [sg]
        for l in range(1, L + 1):
            cp, cl = c[l - 1], c[l]
            s1, s2, tau = signs(1)[0], signs(1)[0], signs(cl)
            lv = []
            for size in range(1, maxV[t] + 1):
                lv += [np.array([s1 * rng.uniform(0.5, 1.0)]), np.array([s2 * rng.uniform(0.5, 1.0) / size]), tau * big(tau) * rng.uniform(0.25, 0.4, cl)]
            for sl in (s1, s2):   # K_top, then K_bot: [2 C_{l-1}][C_l]
                lv.append(sl * sg[:, None] * (tau * big(tau))[None, :] * rng.uniform(0.5, 1.0, (cp, cl)) / (10.0 * cp))
            parts.append(lv)
            sg = tau
            feat_signs.append(sg)
        tower.append((parts, feat_signs))
    out = tower[0][0][0] + tower[1][0][0]
    for l in range(1, L + 1):
        out += tower[0][0][l] + tower[1][0][l]
    xs = np.concatenate([tower[t][1][l] for l in range(L + 1) for t in range(2)])   # the sign of every column of the feature row
    n, h1, h2 = head_widths(C, L, decay)
    assert xs.size == n
    for width in (h1, h2):
        rho = signs(width)
        out.append((rho * big(rho))[:, None] * xs[None, :] * rng.uniform(0.5, 1.0, (width, xs.size)) / (4.0 * xs.size))
        xs = rho
    out.append(signs(1)[0] * xs * rng.uniform(0.5, 1.0, h2) * 16.0 / h2)
    return f32exact(np.concatenate([np.ravel(x) for x in out]))


def fractional(feat, rng):
    """one-hot rows -> rows of eighths with two or three entries, so that the L1 normalisation changes them"""
    V, F = feat.shape
    out = feat * rng.integers(2, 9, (V, 1)) / 8.0
    out[np.arange(V), (np.argmax(feat, axis=1) + 1) % F] += rng.integers(1, 8, V) / 8.0
    even = np.arange(0, V, 2)
    out[even, (np.argmax(feat[even], axis=1) + 2) % F] += 0.375
    return f32exact(out)


def pair_cases():
    """(file, tag, (adj1, feat1), (adj2, feat2), target, (maxV1, maxV2, cap, L, C, decay))"""
    toy = {n: (a, f, t) for n, a, f, t in toy_molecules()}
    ch4, c2h4, nh3, h2o = toy["CH4"], toy["C2H4"], toy["NH3"], toy["H2O"]
    rng = np.random.default_rng(1301)
    out = [
        # the demo's settings (tests/test_CCN_1D.cpp): 10 / 10 vertices, cap 6, 16 channels, decay 0.5
        ("demo", "toy_L7", c2h4[:2], ch4[:2], c2h4[2] - ch4[2], (10, 10, 6, 7, 16, 0.5)),
        ("main", "toy_L3", nh3[:2], c2h4[:2], nh3[2] - c2h4[2], (10, 10, 6, 3, 16, 0.5)),
    ]
    # the asymmetric pair: widths 27 -> 22 -> 18 -> 16 (lane vectors 1, 2 and 4), the cap of 5 bites on both graphs, rows that the
    # normalisation changes
    a12, f12, t12 = synthetic_molecule(5, 12)
    a8, f8, t8 = synthetic_molecule(6, 8)
    out.append(("main", "asym_c27", (a12, fractional(f12, rng)), (a8, fractional(f8[:, :3] + f8[:, 3:4] + f8[:, 4:5], rng)), t12 - t8,
                (12, 8, 5, 3, 27, 0.8)))
    out.append(("main", "decay1", h2o[:2], nh3[:2], h2o[2] - nh3[2], (5, 5, 4, 1, 16, 1.0)))   # constant widths, a 64 -> 64 -> 64 head
    sa, sf, st = star_molecule(5)
    out.append(("main", "star5_cap4", (sa, sf), h2o[:2], st - h2o[2], (6, 6, 4, 2, 16, 0.5)))   # level 1: the centre's children lie outside its field
    # negative entries: the third column is negative on every vertex (the norm sums |x|, not x), rows of different norms
    neg = f32exact(np.array([[0.5, 0.25, -0.75, 0.0], [0.0, 1.0, -0.125, 0.375], [1.5, 0.0, -0.5, 0.0]]))
    out.append(("main", "negative", (h2o[0], neg), (ch4[0], fractional(ch4[1], rng)), 1.0, (5, 5, 5, 1, 16, 0.5)))
    return out


def head(maxV1, maxV2, cap, L, C, F1, F2, decay):
    return "%d %d %d %d %d %d %d %.17g\n" % (maxV1, maxV2, cap, L, C, F1, F2, decay)


def column_signs(feat):
    sg = np.sign(feat)
    assert all(len(set(col[col != 0])) <= 1 for col in sg.T), "a feature column with both signs"
    return np.where(sg.min(axis=0) < 0, -1.0, 1.0)


def record(exe, rng, ga, gb, tgt, maxV1, maxV2, cap, L, C, decay):
    """one fixture: parameters are redrawn until the pre-activation margin holds"""
    (V1, F1), (V2, F2) = ga[1].shape, gb[1].shape
    blocks = model_blocks(C, L, [F1, F2], [maxV1, maxV2], decay)
    n, _, h2 = head_widths(C, L, decay)
    for attempt in range(200):
        params = random_params(C, L, [F1, F2], [maxV1, maxV2], decay, [column_signs(ga[1]), column_signs(gb[1])], rng)
        assert params.size == sum(sz for _, sz in blocks)
        text = "run " + head(maxV1, maxV2, cap, L, C, F1, F2, decay) + graph_text(*ga) + graph_text(*gb) + "%.17g\n" % tgt
        text += " ".join("%.17g" % x for x in params) + "\n"
        lines = run(exe, text)
        g = np.array(lines[2].split(), dtype=np.float64)
        pred, loss = (float(x) for x in lines[3].split())
        grads = np.array(lines[4].split(), dtype=np.float64)
        zmin, zmax, worst = (float(x) for x in lines[5].split())
        assert grads.size == params.size and g.size == n, (grads.size, params.size, g.size, n)
        # (the worst-case fp32 rounding of the head's last inner product stays below half of the suite's 1e-5)
        if zmin < MARGIN * zmax or worst * 2.0 ** -24 * h2 > 5e-6 * max(1.0, abs(pred)):
            continue
        return attempt, {
            "phi": parse_phi(lines[0], L, V1, cap), "phi2": parse_phi(lines[1], L, V2, cap), "graph_feature": g, "predict": np.array([pred]),
            "loss": np.array([loss]), "grads": grads, "params": params.astype(np.float32), "margin": np.array([zmin / zmax]),
            "adj": ga[0].astype(np.int32), "feature": np.asarray(ga[1], dtype=np.float64), "adj2": gb[0].astype(np.int32),
            "feature2": np.asarray(gb[1], dtype=np.float64), "target": np.array([tgt], dtype=np.float64),
            "cfg": np.array([maxV1, maxV2, cap, L, C], dtype=np.int32), "decay": np.array([decay])}
    raise AssertionError("no draw with a pre-activation margin of %g" % MARGIN)


def demo_pairs():
    """the 16 pairs of the four toy molecules, target = difference of the atom counts (tests/test_CCN_1D.cpp)"""
    tm = toy_molecules()
    return [(a[1:3], b[1:3], a[3] - b[3]) for a in tm for b in tm]


def learn(exe, ckpt, L, seed, nIter, lr):
    pairs = demo_pairs()
    text = "learn " + head(10, 10, 6, L, 16, 4, 4, 0.5) + "%d %d %.17g %d %s\n" % (seed, nIter, lr, len(pairs), ckpt)
    text += "".join(graph_text(*a) for a, _, _ in pairs) + "".join(graph_text(*b) for _, b, _ in pairs)
    text += " ".join("%.17g" % t for *_, t in pairs) + "\n"
    lines = run(exe, text)
    return {"cfg": np.array([10, 10, 6, L, 16, seed, nIter], dtype=np.int32), "decay": np.array([0.5]), "lr": np.array([lr]),
            "targets": np.array([t for *_, t in pairs], dtype=np.float64), "params0": np.array(lines[0].split(), dtype=np.float32),
            "losses": np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2), "params": np.array(lines[2].split(), dtype=np.float64),
            "predict": np.array(lines[3].split(), dtype=np.float64), "checkpoint_predict": np.array(lines[4].split(), dtype=np.float64)}


def main():
    if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", "CCN_1D.h")):
        sys.exit("reference not found at %s" % REF_ROOT)
    files = {"main": {}, "demo": {}}
    tags = {"main": [], "demo": []}
    rng = np.random.default_rng(4201)
    worst = 1.0
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ccn1d_driver.cpp"), os.path.join(tmp, "ccn1d_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        for which, tag, ga, gb, tgt, (maxV1, maxV2, cap, L, C, decay) in pair_cases():
            tries, rec = record(exe, rng, ga, gb, tgt, maxV1, maxV2, cap, L, C, decay)
            for k, v in rec.items():
                files[which]["ccn_%s__%s" % (tag, k)] = v
            tags[which].append(tag)
            worst = min(worst, float(rec["margin"][0]))
            print("%-12s widths %s head %s, %6d parameters, predict %10.6g, margin %.3g (%d redraws)"
                  % (tag, channels(C, L, decay), head_widths(C, L, decay), rec["params"].size, rec["predict"][0], rec["margin"][0], tries))
        # three BatchLearn steps on the 16 toy pairs from the constructor's weights after srand(11): the whole trajectory at L = 3, with
        # the real class's checkpoint; at the demo's L = 7 the loss pairs only (the constants of tests/cpp/test_CCN_1D_hip.cpp)
        ckpt = os.path.join(tmp, "ccn_1d_checkpoint.dat")
        for k, v in learn(exe, ckpt, 3, 11, 3, 1e-3).items():
            files["demo"]["train__" + k] = v
        with open(ckpt) as f:
            text = f.read()
        with open(os.path.join(HERE, "ccn_1d_checkpoint.dat"), "w") as f:
            f.write(text)
        demo = learn(exe, os.path.join(tmp, "demo.dat"), 7, 11, 3, 1e-3)
        for k in ("cfg", "decay", "lr", "targets", "losses", "predict"):
            files["demo"]["train7__" + k] = demo[k]
        files["demo"]["train7__n_params"] = np.array([demo["params"].size])
        print("demo losses (before, after) x 3: " + " ".join("%.10f" % x for x in demo["losses"].ravel()))
    assert worst >= MARGIN
    for which, name in (("main", "ccn_1d.npz"), ("demo", "ccn_1d_demo.npz")):
        files[which]["tags"] = np.array(tags[which])
        np.savez_compressed(os.path.join(HERE, name), **files[which])
        print("wrote %s: %d cases, %d bytes" % (name, len(tags[which]), os.path.getsize(os.path.join(HERE, name))))
    print("smallest pre-activation margin %.3g of max |z|" % worst)


if __name__ == "__main__":
    main()
