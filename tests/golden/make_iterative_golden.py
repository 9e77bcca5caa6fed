#!/usr/bin/env python3
"""Generate tests/golden/smp_iterative.npz from the REAL reference classes: the two iterative training calls every model header has,
BatchLearn(nBatch, molecule, target, nIterations, learning_rate, epsilon) (kind 0) and Learn(molecule, target, nIterations, learning_rate,
epsilon) (kind 1), on one class per loss and optimiser kind:

    SMP_omega (Adam), GCN_1D (Momentum), SMP_2D_ver6_classification (LogLoss: values <= 0), SMP_omega_physics (composite, Adam),
    GCN_1D_Kernel (pairs of graphs), GCA_1D (no target).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_iterative_golden.py
A small driver (below) that only includes the six reference headers is compiled into a temporary directory outside the repository and fed
through stdin / stdout.  Only data is recorded: per run the inputs, the seed, the weights the constructor draws after srand(seed), the pair
the class's call returns, its final value[], and per iteration the loss and the decision.

The classes do not show what happens inside their loops.  The driver therefore runs every case twice from the same seed: once through the
class's own call, and once as the same loop spelled out on the class's public members (graph, sgd, the loss object; the single-step
BatchLearn for kind 0) with a cache of value[] of its own, printing the loss and the decision of every iteration.  It refuses (exit 2)
unless both leave the same pair and the same value[], bit for bit: the printed sequence is then the class's.

Runs per class, as far as the class can produce them (see below): kind 0 with at least one kept and one restored step; kind 0 at a rate so
large that it leaves through learning_rate < 1e-6; kind 1 ending by error < epsilon, by the immediate return, and by exhausting nIterations
with a restored step among them.

Condition, asserted here and not a tolerance to tune: every comparison a recorded loop makes -- loss against the one to beat, error against
epsilon -- has a gap |a - b| / max(|b|, 1) >= 1e-3.  The device's fp32 loss may be 5e-5 off the fp64 class (field_suite's bound after a
step), so no fp32 evaluation can flip a decision, with 20x room.  Per (class, run) the seed, momentum_param, rate, epsilon and iteration
count are drawn -- SEEDS, MOMENTA and the grids below, in order -- until the reference alone satisfies this; what gave the run is recorded
with it (`seed`, `momentum`, `lr`, `eps`), and how many candidates were tried (`tried`).  Two runs may stay missing, and main() asserts
that exactly those do (MAY_BE_MISSING says why): the Adam classes cannot leave through learning_rate < 1e-6 with such a gap."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import toy_molecules  # noqa: E402
from make_neighbourhood_golden import graph_text  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")
GAP = 1e-3
SEEDS = (23, 1, 2, 3, 5, 7, 11, 13, 17, 19, 29, 31)   # tried in this order, per (class, run); the one that gives the run is recorded with it
MOMENTA = (0.9, 0.99, 0.5)                           # momentum_param of the Momentum classes, likewise (the Adam classes take none)
ADAM = ("SMP_omega", "SMP_omega_physics")
# what may stay missing, and why (main() asserts that nothing else does, over every seed, momentum and grid point above):
#   the Adam classes cannot leave through learning_rate < 1e-6 with a gap: that exit needs some twenty restored steps in a row whose
#   losses each rise by the gap, down to a rate of 2e-6; Adam's step is normalised, so at such a rate it moves the weights by about the
#   rate itself and the loss by far less than 1e-3.  (Momentum's velocity, which a restore does not touch, can carry it.)
MAY_BE_MISSING = ("SMP_omega/batch_leave", "SMP_omega_physics/batch_leave")
MAX_LOSS = 100.0   # no recorded loss beyond this many times (1 + |first loss|): a step further out says nothing more, fp32 activations stay far from
                   # their range, and a classifier's samples stay clear of LOG_ZERO
ACCEPT, REJECT, REJECT_LEAVE, LEAVE = 1, 2, 3, 4   # graphflow_amd/csrc/smp_fit_policy.h

# class -> (index in the driver, constructor integers).  max_nVertices 6 = C2H4, 4 features (one-hot C, H, N, O)
CLASSES = {
    "SMP_omega": (0, (6, 6, 2, 4, 4, 1)),                     # max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures, nDepth
    "GCN_1D": (1, (2, 6, 4, 5, 1, 1)),                        # nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius
    "SMP_2D_ver6_classification": (2, (3, 6, 2, 4, 4, 1)),    # nClass, max_nVertices, nLevels, nChanels, nFeatures, nDepth
    "SMP_omega_physics": (3, (6, 6, 2, 4, 4, 0)),             # max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures, -
    "GCN_1D_Kernel": (4, (2, 6, 4, 5, 1, 1)),
    "GCA_1D": (5, (2, 6, 4, 5, 1, 1)),
}

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <string>
#include <algorithm>
// (four of the headers define a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_SMP_omega
#include "SMP_omega.h"
#undef INF
#define INF INF_of_GCN_1D
#include "GCN_1D.h"
#undef INF
#define INF INF_of_SMP_2D_ver6_classification
#include "SMP_2D_ver6_classification.h"
#undef INF
#define INF INF_of_SMP_omega_physics
#include "SMP_omega_physics.h"
#undef INF
#define INF INF_of_GCN_1D_Kernel
#include "GCN_1D_Kernel.h"
#undef INF
#define INF INF_of_GCA_1D
#include "GCA_1D.h"
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

struct Batch {
    int n;
    std::vector<DenseGraph *> x, y;
    std::vector<double> t;
};

// what differs between the classes: the argument lists of their calls and the name of the loss object
template <class Net>
struct Plain {   // SMP_omega, GCN_1D, SMP_omega_physics
    static std::pair<double, double> batch(Net &n, Batch &b, int it, double lr, double eps) { return n.BatchLearn(b.n, &b.x[0], &b.t[0], it, lr, eps); }
    static std::pair<double, double> one(Net &n, Batch &b, int it, double lr, double eps) { return n.Learn(b.x[0], b.t[0], it, lr, eps); }
    static std::pair<double, double> step(Net &n, Batch &b, double lr) { return n.BatchLearn(b.n, &b.x[0], &b.t[0], lr); }
    static void bind(Net &n, Batch &b) { n.complete_computation_graph(b.x[0]); n.target->value[0] = b.t[0]; }
    static double loss(Net &n) { return n.sql->getLoss(); }
};
struct Classes : Plain<SMP_2D_ver6_classification> {
    static double loss(SMP_2D_ver6_classification &n) { return n.logl->getLoss(); }
};
struct Pairs {
    typedef GCN_1D_Kernel Net;
    static std::pair<double, double> batch(Net &n, Batch &b, int it, double lr, double eps) { return n.BatchLearn(b.n, &b.x[0], &b.y[0], &b.t[0], it, lr, eps); }
    static std::pair<double, double> one(Net &n, Batch &b, int it, double lr, double eps) { return n.Learn(b.x[0], b.y[0], b.t[0], it, lr, eps); }
    static std::pair<double, double> step(Net &n, Batch &b, double lr) { return n.BatchLearn(b.n, &b.x[0], &b.y[0], &b.t[0], lr); }
    static void bind(Net &n, Batch &b) { n.complete_computation_graph(b.x[0], b.y[0]); n.target->value[0] = b.t[0]; }
    static double loss(Net &n) { return n.sql->getLoss(); }
};
struct NoTarget {
    typedef GCA_1D Net;
    static std::pair<double, double> batch(Net &n, Batch &b, int it, double lr, double eps) { return n.BatchLearn(b.n, &b.x[0], it, lr, eps); }
    static std::pair<double, double> one(Net &n, Batch &b, int it, double lr, double eps) { return n.Learn(b.x[0], it, lr, eps); }
    static std::pair<double, double> step(Net &n, Batch &b, double lr) { return n.BatchLearn(b.n, &b.x[0], lr); }
    static void bind(Net &n, Batch &b) { n.complete_computation_graph(b.x[0]); }
    static double loss(Net &n) { return n.sql->getLoss(); }
};

template <class Net>
static std::vector<double> values(Net &net) {
    std::vector<double> v;
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) v.push_back(net.sgd->params[i]->value[j]);
    return v;
}
template <class Net>
static void set_values(Net &net, const std::vector<double> &v) {
    size_t k = 0;
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) net.sgd->params[i]->value[j] = v[k++];
}
static void print(const std::vector<double> &v) {
    for (size_t i = 0; i < v.size(); ++i) printf("%.17g ", v[i]);
    printf("\n");
}

// the loops of the classes (SMP_omega.h:827-922), spelled out on public members, with the loss and the decision of every iteration
template <class A, class Net>
static std::pair<double, double> spelled_out(Net &net, Batch &b, int kind, int nIter, double lr, double eps) {
    std::vector<double> cache = values(net);
    std::pair<double, double> ret;
    if (kind == 0) {
        bool have = false;
        for (int iter = 0; iter < nIter; ++iter) {
            std::pair<double, double> r = A::step(net, b, lr);   // (loss before, one step at lr, loss after)
            if (!have) ret.first = ret.second = r.first;
            have = true;
            const double loss = r.second;
            if (loss > ret.second) {
                set_values(net, cache);
                lr *= 0.5;
                printf("%.17g %d\n", loss, lr < 1e-6 ? 3 : 2);
                if (lr < 1e-6) break;
            } else {
                printf("%.17g 1\n", loss);
                ret.second = loss;
                cache = values(net);
            }
        }
        if (!have) {   // nIterations = 0: the loss alone
            std::pair<double, double> r = A::step(net, b, 0.0);
            ret.first = ret.second = r.first;
        }
    } else {
        A::bind(net, b);
        net.graph->forward();
        double best = A::loss(net);
        ret.first = ret.second = best;
        if (!(best < eps)) {
            for (int iter = 0; iter < nIter; ++iter) {
                net.graph->forward();
                net.graph->backward();
                net.sgd->Learn(lr);
                net.graph->forward();
                const double error = A::loss(net);
                if (error < eps) {
                    printf("%.17g 4\n", error);
                    break;
                }
                if (error >= best) {
                    set_values(net, cache);
                    lr = std::max(lr * 0.5, 1e-6);
                    printf("%.17g 2\n", error);
                } else {
                    printf("%.17g 1\n", error);
                    best = error;
                    cache = values(net);
                }
            }
            ret.second = best;
        }
    }
    printf("end %.17g\n", lr);
    return ret;
}

template <class A, class Net>
static int both(Net &net, Net &again, Batch &b, int kind, int nIter, double lr, double eps) {
    print(values(net));
    if (values(net) != values(again)) return 3;   // (the same seed: the same weights)
    std::pair<double, double> r = kind == 0 ? A::batch(net, b, nIter, lr, eps) : A::one(net, b, nIter, lr, eps);
    printf("%.17g %.17g\n", r.first, r.second);
    print(values(net));
    std::pair<double, double> q = spelled_out<A>(again, b, kind, nIter, lr, eps);
    if (memcmp(&r, &q, sizeof r) != 0 || values(net) != values(again)) {
        fprintf(stderr, "the loop spelled out does not reproduce the class: (%.17g, %.17g) against (%.17g, %.17g)\n", q.first, q.second, r.first, r.second);
        return 2;
    }
    return 0;
}

// Objects are leaked on purpose.
int main() {
    int cls, seed, c[6], n, kind, nIter;
    double mom, lr, eps;
    if (scanf("%d %d %d %d %d %d %d %d %lf %d", &cls, &seed, &c[0], &c[1], &c[2], &c[3], &c[4], &c[5], &mom, &n) != 10) return 1;
    const int F = cls == 0 || cls == 2 || cls == 3 ? c[4] : c[2];
    Batch b;
    b.n = n;
    for (int i = 0; i < n; ++i) b.x.push_back(read_graph(F));
    if (cls == 4)
        for (int i = 0; i < n; ++i) b.y.push_back(read_graph(F));
    b.t.resize(n);
    if (cls != 5)
        for (int i = 0; i < n; ++i) scanf("%lf", &b.t[i]);
    if (scanf("%d %d %lf %lf", &kind, &nIter, &lr, &eps) != 4) return 1;
#define TWICE(Net, args) srand((unsigned)seed); Net &net = *new Net args; srand((unsigned)seed); Net &again = *new Net args
    if (cls == 0) { TWICE(SMP_omega, (c[0], c[1], c[2], c[3], c[4], c[5])); return both<Plain<SMP_omega> >(net, again, b, kind, nIter, lr, eps); }
    if (cls == 1) { TWICE(GCN_1D, (c[0], c[1], c[2], c[3], c[4], c[5], mom)); return both<Plain<GCN_1D> >(net, again, b, kind, nIter, lr, eps); }
    if (cls == 2) { TWICE(SMP_2D_ver6_classification, (c[0], c[1], c[2], c[3], c[4], c[5], mom)); return both<Classes>(net, again, b, kind, nIter, lr, eps); }
    if (cls == 3) { TWICE(SMP_omega_physics, (c[0], c[1], c[2], c[3], c[4])); return both<Plain<SMP_omega_physics> >(net, again, b, kind, nIter, lr, eps); }
    if (cls == 4) { TWICE(GCN_1D_Kernel, (c[0], c[1], c[2], c[3], c[4], c[5], mom)); return both<Pairs>(net, again, b, kind, nIter, lr, eps); }
    if (cls == 5) { TWICE(GCA_1D, (c[0], c[1], c[2], c[3], c[4], c[5], mom)); return both<NoTarget>(net, again, b, kind, nIter, lr, eps); }
    return 1;
}
"""


def gap(a, b):
    return abs(a - b) / max(abs(b), 1.0)


def replay(kind, first, losses, lr, eps):
    """the decision rule restated (smp_fit_policy.h): (decisions, second, final rate, smallest gap of any comparison made)"""
    second, dec, g = first, [], np.inf
    if kind == 1:
        g = min(g, gap(first, eps))
        if first < eps:
            return dec, second, lr, g
    for loss in losses:
        if kind == 0:
            g = min(g, gap(loss, second))
            if loss > second:
                lr *= 0.5
                dec.append(REJECT_LEAVE if lr < 1e-6 else REJECT)
                if lr < 1e-6:
                    break
            else:
                second = loss
                dec.append(ACCEPT)
        else:
            g = min(g, gap(loss, eps))
            if loss < eps:
                dec.append(LEAVE)
                break
            g = min(g, gap(loss, second))
            if loss >= second:
                lr = max(lr * 0.5, 1e-6)
                dec.append(REJECT)
            else:
                second = loss
                dec.append(ACCEPT)
    return dec, second, lr, g


def batch_of(name, kind):
    """(x graphs, y graphs or None, targets or None): kind 0 the four toy molecules, kind 1 the first of them; the classifier's labels are
    the molecule's index modulo 3, a pair's partner is the next molecule, its target the sum of the two atom counts"""
    tm = toy_molecules()
    x = [(a, f) for _, a, f, _ in tm]
    t = [tg for *_, tg in tm]
    y = None
    if name == "SMP_2D_ver6_classification":
        t = [float(i % 3) for i in range(len(tm))]
    if name == "GCN_1D_Kernel":
        y = x[1:] + x[:1]
        t = [a + b for a, b in zip(t, t[1:] + t[:1])]
    if name == "GCA_1D":
        t = None
    n = len(x) if kind == 0 else 1
    return x[:n], (y[:n] if y else None), (t[:n] if t else None)


def run_case(exe, name, kind, nIter, lr, eps, seed, momentum):
    cls, ctor = CLASSES[name]
    x, y, t = batch_of(name, kind)
    text = "%d %d %s %.17g %d\n" % (cls, seed, " ".join(str(v) for v in ctor), momentum, len(x))
    text += "".join(graph_text(a, f) for a, f in x)
    if y:
        text += "".join(graph_text(a, f) for a, f in y)
    if t:
        text += " ".join("%.17g" % v for v in t) + "\n"
    text += "%d %d %.17g %.17g\n" % (kind, nIter, lr, eps)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    if "nan" in r.stdout or "inf" in r.stdout:   # (a rate at which the class itself overflows: not a candidate)
        return None, 0.0
    assert r.returncode == 0, (name, kind, nIter, lr, eps, r.returncode, r.stderr[-500:])
    lines = r.stdout.strip().split("\n")
    params0 = np.array(lines[0].split(), dtype=np.float64)
    pair = np.array(lines[1].split(), dtype=np.float64)
    params = np.array(lines[2].split(), dtype=np.float64)
    assert lines[-1].startswith("end ")
    final_lr = float(lines[-1].split()[1])
    rows = [ln.split() for ln in lines[3:-1]]
    losses = np.array([float(r_[0]) for r_ in rows], dtype=np.float64)
    dec = [int(r_[1]) for r_ in rows]
    d2, second, lr2, g = replay(kind, pair[0], losses, lr, eps)
    assert d2 == dec and second == pair[1] and lr2 == final_lr, (name, kind, dec, d2)
    if losses.size and np.abs(losses).max() > MAX_LOSS * (1.0 + abs(pair[0])):
        return None, 0.0
    return {"params0": params0, "pair": pair, "params": params, "losses": losses, "decisions": np.array(dec, dtype=np.uint8),
            "final_lr": np.array([final_lr]), "cfg": np.array([kind, nIter], dtype=np.int32), "lr": np.array([lr]), "eps": np.array([eps]),
            "targets": np.array(t if t else [], dtype=np.float64), "seed": np.array([seed], dtype=np.int32),
            "momentum": np.array([momentum])}, g


RATES = (0.5, 0.25, 0.1, 0.05, 0.02, 0.01, 1.0, 2.0, 4.0, 0.005, 8.0, 16.0)


RUN_NAMES = ("batch_mixed", "batch_leave", "learn_epsilon", "learn_immediate", "learn_exhaust")


def scenarios(first):
    """run -> (kind, candidates (nIter, lr, eps), what the recorded loop must show); `first` = the loss of the first sample at the seed's
    weights (kind 1's starting point: the epsilons are placed around it)"""
    away = abs(first) + 1.0
    return {
        "batch_mixed": (0, [(6, lr, 0.0) for lr in RATES], lambda d: ACCEPT in d and REJECT in d),
        "batch_leave": (0, [(40, lr, 0.0) for lr in (64.0, 16.0, 4.0, 1.0, 256.0, 1024.0)], lambda d: d and d[-1] == REJECT_LEAVE),
        "learn_epsilon": (1, [(8, lr, first - f * abs(first)) for f in (0.5, 0.25, 0.75, 0.1, 0.9, 0.05, 0.02, 0.01, 0.005) for lr in RATES],
                          lambda d: d and d[-1] == LEAVE),
        "learn_immediate": (1, [(4, 0.1, first + away)], lambda d: not d),
        "learn_exhaust": (1, [(5, lr, first - 2 * away) for lr in (1.0, 0.5, 2.0, 4.0, 0.25, 8.0, 0.1)], lambda d: len(d) == 5 and REJECT in d),
    }


def main():
    for name in CLASSES:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", name + ".h")):
            sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out, missing, worst = {}, [], np.inf
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "iterative_driver.cpp"), os.path.join(tmp, "iterative_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        for name, (cls, ctor) in CLASSES.items():
            for run in RUN_NAMES:
                found, tried = None, 0
                for seed in SEEDS:
                    for momentum in (MOMENTA[:1] if name in ADAM else MOMENTA):
                        probe = run_case(exe, name, 1, 0, 0.1, -1e300, seed, momentum)[0]
                        if probe is None:   # (the class overflows on the plain loss at these weights: not a candidate)
                            continue
                        first = probe["pair"][0]
                        kind, candidates, wanted = scenarios(first)[run]
                        for nIter, lr, eps in candidates:
                            rec, g = run_case(exe, name, kind, nIter, lr, eps, seed, momentum)
                            tried += 1
                            if rec is not None and g >= GAP and wanted(list(rec["decisions"])):
                                found = (rec, g, lr, eps)
                                break
                        if found:
                            break
                    if found:
                        break
                out["%s__%s__tried" % (name, run)] = np.array([tried], dtype=np.int32)
                if not found:
                    missing.append("%s/%s" % (name, run))
                    print("%-28s %-16s none of %d candidates (%d seeds) gives it with every gap >= %g" % (name, run, tried, len(SEEDS), GAP))
                    continue
                rec, g, lr, eps = found
                worst = min(worst, g)
                for k, v in rec.items():
                    out["%s__%s__%s" % (name, run, k)] = v
                print("%-28s %-16s seed %-3d momentum %-5g lr %-6g eps %-10.4g pair (%.6g, %.6g) decisions %s smallest gap %.3g" %
                      (name, run, rec["seed"][0], rec["momentum"][0], lr, eps, rec["pair"][0], rec["pair"][1], "".join(str(d) for d in rec["decisions"]), g),
                      "largest |loss| %.4g" % (np.abs(rec["losses"]).max() if rec["losses"].size else 0))
            out[name + "__ctor"] = np.array(ctor, dtype=np.int32)
    assert sorted(missing) == sorted(MAY_BE_MISSING), missing
    assert worst >= GAP
    out["classes"] = np.array(list(CLASSES))
    out["missing"] = np.array(missing)
    np.savez_compressed(os.path.join(HERE, "smp_iterative.npz"), **out)
    print("wrote smp_iterative.npz: %d runs, smallest gap of any comparison %.3g; missing: %s" %
          (sum(1 for k in out if k.endswith("__pair")), worst, ", ".join(missing) or "none"))


if __name__ == "__main__":
    main()
