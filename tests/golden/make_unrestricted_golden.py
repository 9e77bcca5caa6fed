#!/usr/bin/env python3
"""Generate tests/golden/smp_unrestricted.npz from the REAL reference classes Unrestricted_SMP_1D, Unrestricted_SMP_1D_ver2 and
Unrestricted_SMP_2D (GraphFlow/Unrestricted_SMP_*.h).

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_unrestricted_golden.py
A small driver (below) that only includes the three reference headers is compiled into a temporary directory outside the repository and
fed through stdin / stdout.  Only data is recorded: the inputs, the receptive fields per level, the reference's graph feature,
prediction, loss and parameter gradients (the parameters once per form and shape: the molecules share them), for CH4 at nLevels = 2 the level activations (form 3: and the reduced adjacencies), the weights
weights_initialization() draws after srand(seed) for each of the three classes, and a three-step BatchLearn (Momentum) trajectory of
Unrestricted_SMP_2D and of Unrestricted_SMP_1D_ver2.  Inputs are float32-representable so the fp32 device path and the fp64 checkers see
identical numbers.

Every fixture passes two asserts here: the read-out's worst-case fp32 rounding stays under half of the suite's 1e-5, and no
pre-activation (level 0, the levels, the read-out's sums) lies within 1e-3 max|z| of zero, so that fp32 cannot take the other branch of
a LeakyReLU.  Parameters are redrawn until the second holds (random_params says how they are drawn so that it can); the smallest
margin kept is printed.  A pre-activation that is EXACTLY zero is not counted (as in make_smp1d_golden.py): both formats take the same
branch there.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import f32exact, synthetic_molecule, toy_molecules  # noqa: E402
from make_smp1d_golden import cycle_molecule, star_molecule  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")   # the reference tree (the directory that holds GraphFlow/)
HEADERS = ("Unrestricted_SMP_1D.h", "Unrestricted_SMP_1D_ver2.h", "Unrestricted_SMP_2D.h")
MARGIN = 1e-3      # smallest |z| / max |z| a fixture may hold
MOMENTUM = 0.9

DRIVER = r"""
#include <cstdio>
#include <cmath>
#include <vector>
// (every one of the three headers defines a global `const int INF`: one name each, so that they fit into one translation unit)
#define INF INF_of_Unrestricted_SMP_1D
#include "Unrestricted_SMP_1D.h"
#undef INF
#define INF INF_of_Unrestricted_SMP_1D_ver2
#include "Unrestricted_SMP_1D_ver2.h"
#undef INF
#define INF INF_of_Unrestricted_SMP_2D
#include "Unrestricted_SMP_2D.h"
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

static double *level0_of(Unrestricted_SMP_1D &net, int v, int *n) { *n = net.level[0]->f_transpose[v]->size; return net.level[0]->f_transpose[v]->value; }
static double *level0_of(Unrestricted_SMP_1D_ver2 &net, int v, int *n) { *n = net.level[0]->f_transpose[v]->size; return net.level[0]->f_transpose[v]->value; }
static double *level0_of(Unrestricted_SMP_2D &net, int v, int *n) { *n = net.level[0]->f_reshape[v]->size; return net.level[0]->f_reshape[v]->value; }
static void adjacencies(Unrestricted_SMP_1D &, int, int) {}
static void adjacencies(Unrestricted_SMP_1D_ver2 &, int, int) {}
static void adjacencies(Unrestricted_SMP_2D &net, int L, int V) {
    for (int l = 1; l <= L; ++l)   // the reduced adjacencies, [s][s]
        for (int v = 0; v < V; ++v)
            for (int i = 0; i < net.level[l]->adj[v]->size; ++i) printf("%.17g ", net.level[l]->adj[v]->value[i]);
}

template <class Net>
static void run(Net &net, DenseGraph *g, double target, int L) {
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
            if (l == 0) {
                int n;
                double *z = level0_of(net, v, &n);
                margins(z, n);
            } else {
                margins(net.level[l]->add[v]->value, net.level[l]->add[v]->size);
            }
            if (l == L) margins(net.shrinked[v]->value, net.shrinked[v]->size);
        }
    printf("\n");
    for (int f = 0; f < net.graph_feature->size; ++f) printf("%.17g ", net.graph_feature->value[f]);
    printf("\n");
    for (int l = 0; l <= L; ++l)   // the activations f_l[v], row-major, back to back
        for (int v = 0; v < V; ++v)
            for (int i = 0; i < net.level[l]->f[v]->size; ++i) printf("%.17g ", net.level[l]->f[v]->value[i]);
    printf("\n");
    adjacencies(net, L, V);
    printf("\n");
    printf("%.17g %.17g\n", net.predict->value[0], net.sql->getLoss());
    print_params(net, true);
    printf("%.17g %.17g\n", zmin, zmax);
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

// form 1: Unrestricted_SMP_1D, 2: Unrestricted_SMP_1D_ver2, 3: Unrestricted_SMP_2D.  Objects are leaked on purpose: the models' and the
// executors' destructors free the same memory.
int main() {
    char mode[16];
    int form, maxV, L, C, F, D, wl;
    double mom;
    if (scanf("%15s %d %d %d %d %d %d %d %lf", mode, &form, &maxV, &L, &C, &F, &D, &wl, &mom) != 9) return 1;
    if (mode[0] == 'r') {   // run: one sample, given parameters
        DenseGraph *g = read_graph(F);
        double target;
        scanf("%lf", &target);
        if (form == 1) run(*new Unrestricted_SMP_1D(maxV, L, C, F, D, mom, wl != 0), g, target, L);
        else if (form == 2) run(*new Unrestricted_SMP_1D_ver2(maxV, L, C, F, D, mom, wl != 0), g, target, L);
        else run(*new Unrestricted_SMP_2D(maxV, L, C, F, D, mom, wl != 0), g, target, L);
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
#define GF_LEARN(T) { T &net = *new T(maxV, L, C, F, D, mom, wl != 0); learn(net, nIter, nMol, &m[0], &tgt[0], lr); }
    if (form == 1) GF_LEARN(Unrestricted_SMP_1D)
    else if (form == 2) GF_LEARN(Unrestricted_SMP_1D_ver2)
    else GF_LEARN(Unrestricted_SMP_2D)
    return 0;
}
"""


def channels(form, C, L):
    """channel count per level: doubling for Unrestricted_SMP_1D_ver2 (form 2), constant otherwise"""
    return [C << l if form == 2 else C for l in range(L + 1)]


def unrestricted_blocks(form, C, FD, L, maxV):
    """[(block name, size)] in registration order: H; per level for s = 1..maxV (W_s [s, s] | W1_s, W2_s [s, s] | W_s [s, s, C], then
    b_s[C_l]), form 3: then scalar_l[C]; W[C_L]."""
    c = channels(form, C, L)
    out = [("H", C * FD)]
    for l in range(1, L + 1):
        for s in range(1, maxV + 1):
            if form == 2:
                out += [("W1_%d_%d" % (l, s), s * s), ("W2_%d_%d" % (l, s), s * s)]
            else:
                out.append(("W_%d_%d" % (l, s), s * s * (c[l - 1] if form == 3 else 1)))
            out.append(("b_%d_%d" % (l, s), c[l]))
        if form == 3:
            out.append(("scalar_%d" % l, c[l - 1]))
    out.append(("W", c[L]))
    return out


def random_params(form, C, FD, L, maxV, rng):
    """float32-exact parameters in registration order, drawn so that the margin CAN hold.  A field of 12 vertices has up to 144 C
    pre-activations per vertex and level, each a sum over the field: independent draws never keep all of them 1e-3 max|z| away from
    zero.  So every channel of every level gets one sign, as in make_smp2d_golden.py: with sigma the sign of a channel of the level below
    (H's rows have one sign each, the WL features are >= 0), a filter has one sign -- per channel in form 3, per filter in forms 1 and 2,
    whose W_s has no channel index -- scalar_l has sigma's sign and b_s the sign of filter * sigma: every term of z pulls the same way and
    |z| >= |b|.  Behind the 0.01 slope a negative channel is drawn larger (H, b and in form 3 W_s; not at slope 0, where it is switched
    off), so that both kinds of activation stay within three decades.  The draws are multiples of 1/32 (the filters': of 1/8) before scaling: the file stays small."""
    c = channels(form, C, L)
    slope0 = form == 2

    def signs(n):
        return rng.choice([-1.0, 1.0], n)

    def q(lo, hi, shape, step=1):   # lo / 32 .. hi / 32
        return (lo + step * rng.integers(0, (hi - lo) // step + 1, shape)) / 32.0

    def big(sg):   # the channels whose pre-activations are negative
        return np.ones_like(sg) if slope0 else np.where(sg > 0, 1.0, 40.0)

    sigma = signs(C)
    if slope0:   # (a switched-off channel stays off: keep most of level 0 alive, and W1_s positive below, so that gradients reach H)
        sigma[:(C + 1) // 2] = 1.0
        rng.shuffle(sigma)
    parts = [(sigma * big(sigma))[:, None] * q(6, 8, (C, FD))]
    for l in range(1, L + 1):
        cp = c[l - 1]
        if form == 3:
            s1 = signs(cp)
            t = s1 * sigma
            for size in range(1, maxV + 1):
                parts.append((s1 * big(t))[None, None, :] * q(16, 32, (size, size, cp), 4) / (4.0 * size))
                parts.append(t * big(t) * q(8, 13, cp))
            parts.append(sigma * q(8, 16, cp))
        else:
            s1 = np.ones(1) if slope0 else signs(1)
            s2 = signs(1)
            t = s1 * sigma if form == 1 else np.concatenate([s1 * sigma, s2 * sigma])
            for size in range(1, maxV + 1):
                parts.append(s1 * q(16, 32, (size, size), 4) / (2.0 * size))
                if form == 2:
                    parts.append(s2 * q(16, 32, (size, size), 4) / (2.0 * size))
                parts.append(t * big(t) * q(8, 13, c[l]))
        sigma = t
    parts.append(sigma * q(16, 32, c[L]) / (100.0 * c[L]))
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
    """(name, adj, feature, target, wl): the four toy molecules (CH4: four vertices of one field size at level 1, five at level 2), the
    4-cycle, the 5-leaf star and one 12-vertex synthetic molecule, with and without the WL ordering"""
    out = [(n, a, f, t, 1) for n, a, f, t in toy_molecules()]
    out.append(("cycle4",) + cycle_molecule() + (1,))
    out.append(("star5",) + star_molecule(5) + (1,))
    a, f, t = synthetic_molecule(5, 12)
    out.append(("syn12", a, f, t, 1))
    out.append(("syn12nowl", a, f, t, 0))
    return out


CONFIGS = {1: ((5, 2), (4, 3), (3, 2)), 2: ((5, 2), (4, 3), (3, 2)), 3: ((5, 2), (4, 3), (8, 3))}   # (C, nLevels) per form
D_ALL, MAXV = 1, 14                   # (max_nVertices above the largest molecule: unused per-size blocks, whose gradients stay zero)
ACTIVATIONS_OF = "CH4"


def head(form, maxV, L, C, F, D, wl):
    return "%d %d %d %d %d %d %d %.17g\n" % (form, maxV, L, C, F, D, wl, MOMENTUM)


def record(exe, params, form, adj, feat, tgt, L, C, D, wl, maxV, activations):
    """one fixture at the given parameters, or None where a margin fails"""
    V, F = feat.shape
    CL = channels(form, C, L)[L]
    text = "run " + head(form, maxV, L, C, F, D, wl) + graph_text(adj, feat) + "%.17g\n" % tgt
    text += " ".join("%.17g" % x for x in params) + "\n"
    lines = run(exe, text)
    rec = {"phi": parse_phi(lines[0], L, V, maxV), "graph_feature": np.array(lines[1].split(), dtype=np.float64)}
    if activations:
        rec["activations"] = np.array(lines[2].split(), dtype=np.float64)
        if form == 3:
            rec["adjacency"] = np.array(lines[3].split(), dtype=np.float64)
    pred, loss = (float(x) for x in lines[4].split())
    rec["grads"] = np.array(lines[5].split(), dtype=np.float64)
    zmin, zmax = (float(x) for x in lines[6].split())
    rec["result"] = np.array([pred, loss, tgt, zmin / zmax])   # prediction, loss, target, the margin kept
    out_scale = max(1.0, abs(pred))
    worst = np.abs(rec["graph_feature"] * params[-CL:]).sum()
    assert rec["grads"].size == params.size and rec["graph_feature"].size == CL, (rec["grads"].size, params.size)
    if zmin < MARGIN * zmax or worst * 2.0 ** -24 * CL > 5e-6 * out_scale:
        return None
    rec.update(adj=adj.astype(np.int32), feature=feat, cfg=np.array([form, L, C, D, wl, maxV], dtype=np.int32))
    return rec


def record_shape(exe, rng, form, C, L, F):
    """the fixtures of one (form, C, nLevels, feature width): ONE parameter vector for all its molecules (the file stays small),
    redrawn until the margins of every molecule hold"""
    mols = [m for m in molecules() if m[2].shape[1] == F]
    for attempt in range(2000):
        params = random_params(form, C, F * (D_ALL + 1), L, MAXV, rng)
        assert params.size == sum(n for _, n in unrestricted_blocks(form, C, F * (D_ALL + 1), L, MAXV))
        recs = []
        for name, adj, feat, tgt, wl in mols:
            rec = record(exe, params, form, adj, feat, tgt, L, C, D_ALL, wl, MAXV, name == ACTIVATIONS_OF and L == 2)
            if rec is None:
                break
            recs.append((name, rec))
        if len(recs) == len(mols):
            return params.astype(np.float32), recs, attempt
    raise AssertionError("no draw with a pre-activation margin of %g" % MARGIN)


def main():
    for h in HEADERS:
        if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", h)):
            sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    rng = np.random.default_rng(2312)
    worst_margin = 1.0
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "unrestricted_driver.cpp"), os.path.join(tmp, "unrestricted_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), "-o", exe, src])
        tags = []
        for form in (1, 2, 3):
            for C, L in CONFIGS[form]:
                for F in sorted({m[2].shape[1] for m in molecules()}):
                  params, recs, tries = record_shape(exe, rng, form, C, L, F)
                  out["u%d_c%d_f%d__params" % (form, C, F)] = params   # (shared by the molecules of the shape)
                  for name, rec in recs:
                      tag = "u%d_%s_c%d" % (form, name, C)
                      for k, v in rec.items():
                          out["%s__%s" % (tag, k)] = v
                      tags.append(tag)
                      worst_margin = min(worst_margin, float(rec["result"][3]))
                      print("%-22s %5d parameters, predict %10.6g, margin %.3g (%d redraws)" % (tag, params.size, rec["result"][0],
                                                                                             rec["result"][3], tries))
        out["tags"] = np.array(tags)
        # the weights each constructor's weights_initialization() draws after srand(seed)
        tm = toy_molecules()
        mol_text = "".join(graph_text(a, f) for _, a, f, _ in tm) + " ".join("%.17g" % t for *_, t in tm) + "\n"
        L, C, D, maxV, seed = 2, 3, 1, 6, 31
        for form in (1, 2, 3):
            lines = run(exe, "learn " + head(form, maxV, L, C, 4, D, 1) + "%d 0 0 %d\n" % (seed, len(tm)) + mol_text)
            p = "init_u%d__" % form
            out[p + "cfg"] = np.array([form, L, C, D, 1, maxV, seed], dtype=np.int32)
            out[p + "params0"] = np.array(lines[0].split(), dtype=np.float64)
            assert out[p + "params0"].size == sum(n for _, n in unrestricted_blocks(form, C, 4 * (D + 1), L, maxV))
        # three BatchLearn (Momentum) steps of Unrestricted_SMP_2D and of Unrestricted_SMP_1D_ver2 on the four toy molecules as one batch
        L, C, D, maxV, seed, nIter, lr = 2, 4, 1, 6, 17, 3, 1e-3
        for form in (3, 2):
            lines = run(exe, "learn " + head(form, maxV, L, C, 4, D, 1) + "%d %d %.17g %d\n" % (seed, nIter, lr, len(tm)) + mol_text)
            p = "train_u%d__" % form
            out[p + "cfg"] = np.array([form, L, C, D, 1, maxV, seed, nIter], dtype=np.int32)
            out[p + "lr"] = np.array([lr])
            out[p + "momentum"] = np.array([MOMENTUM])
            out[p + "targets"] = np.array([t for *_, t in tm], dtype=np.float64)
            out[p + "params0"] = np.array(lines[0].split(), dtype=np.float64)
            out[p + "losses"] = np.array(lines[1].split(), dtype=np.float64).reshape(nIter, 2)
            out[p + "params"] = np.array(lines[2].split(), dtype=np.float64)
    assert worst_margin >= MARGIN
    np.savez_compressed(os.path.join(HERE, "smp_unrestricted.npz"), **out)
    print("wrote smp_unrestricted.npz: %d cases, three initial-weight records, two %d-step Momentum trajectories; smallest pre-activation "
          "margin %.3g of max |z|" % (len(tags), nIter, worst_margin))


if __name__ == "__main__":
    main()
