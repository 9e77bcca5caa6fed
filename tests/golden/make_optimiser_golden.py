#!/usr/bin/env python3
"""Generate tests/golden/optimisers.npz from the REAL reference classes SGD, AdaMax, AdaDelta, L1Regularization and L2Regularization
(GraphFlow/SGD.h, AdaMax.h, AdaDelta.h, L1Regularization.h, L2Regularization.h) and from the model classes' own sgd->params.

Run where the reference tree is available:   GF_REFERENCE=<reference tree> python tests/golden/make_optimiser_golden.py
The drivers below include only reference headers, are compiled into a temporary directory outside the repository and talk through
stdin / stdout (hexadecimal floats).  Only data is recorded.

Part A -- the operators on synthetic blocks.  Block sizes BLOCKS; parameters and six gradient sets drawn as fp32-representable doubles
(part_a_inputs: the tests draw the same ones, `a_checksum` pins them); nBatch = 7, so g = gradient / nBatch is inexact.  Six steps of
each class; after every step the parameters, every state array, infinity_norm and beta1_t.  Three AdaMax cases: `adamax` (plain),
`adamax_zero` (block ZERO_BLOCK's gradient zero on every step) and `adamax_zero1` (on step 1 only).  The regularisers see fresh
parameters at every step (with 0, +-5e-9, +-2e-8 among them), run forward() and REG_TIMES backward() calls on that step's gradient; the
value and the gradient are recorded.  Per-element arrays are recorded at the indices `a_index`: every element of the blocks up to 255
elements, and a sample of the two large blocks that holds their first and last elements and both sides of every 256-element boundary
it meets -- the elements are independent given the block's norm, which is recorded for every block, so the sample leaves no property of
the reference out and keeps the file small.

Part B -- block tables: for one configuration of each handle family (BLOCK_CASES) the sizes of sgd->params[i] of the real class.

Part C -- trajectories: SMP_omega, GCN_1D, SMP_2D_ver6_classification, SMP_omega_physics at make_iterative_golden's toy sizes, four
steps of the single-step BatchLearn spelled out on the class's public members with an SGD / AdaMax / AdaDelta built over the class's
own sgd->params: per step the loss before and after, the final weights, the largest single-step |dp| (`step_max`).  The driver refuses
(exit 3) a run whose first step has a block with an all-zero gradient: AdaMax divides 0 by 0 there."""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from inputs import toy_molecules  # noqa: E402
from make_neighbourhood_golden import graph_text  # noqa: E402

REF_ROOT = os.environ.get("GF_REFERENCE", "")

# ---- Part A ----------------------------------------------------------------------------------------------------------------------------
BLOCKS = (1, 3, 64, 65, 255, 1025, 40000)
N_BATCH, N_STEPS = 7, 6
A_LR = {"sgd": 0.05, "adamax": 0.002, "adamax_zero": 0.002, "adamax_zero1": 0.002, "adadelta": 0.0}
A_KIND = {"sgd": 2, "adamax": 3, "adamax_zero": 3, "adamax_zero1": 3, "adadelta": 4}
ZERO_BLOCK = 4                 # the 255-element block
REG_LAMBDA, REG_TIMES = 0.01, 7
L1_SPECIALS = (0.0, 5e-9, -5e-9, 2e-8, -2e-8)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def f32_doubles(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def part_a_inputs():
    """(params [n], grads [N_STEPS][n], reg_params [N_STEPS][n]): fp32-representable doubles"""
    n = int(sum(BLOCKS))
    rng = np.random.default_rng(20260)
    params = f32_doubles(rng.uniform(-1.0, 1.0, n))
    grads = f32_doubles(rng.uniform(-1.0, 1.0, (N_STEPS, n)) * 2.0 ** rng.integers(-6, 3, (N_STEPS, n)))
    reg = f32_doubles(rng.uniform(-1.0, 1.0, (N_STEPS, n)))
    for s in range(N_STEPS):   # the specials at the start of the 65-element block and in the middle of the large one
        for at in (int(offsets_of(BLOCKS)[3]), int(offsets_of(BLOCKS)[6]) + 20001 + s):
            reg[s, at:at + len(L1_SPECIALS)] = f32_doubles(L1_SPECIALS)
    return params, grads, reg


def case_grads(case, grads):
    g = grads.copy()
    off = offsets_of(BLOCKS)
    if case == "adamax_zero":
        g[:, off[ZERO_BLOCK]:off[ZERO_BLOCK + 1]] = 0.0
    if case == "adamax_zero1":
        g[0, off[ZERO_BLOCK]:off[ZERO_BLOCK + 1]] = 0.0
    return g


def a_index():
    off = offsets_of(BLOCKS)
    keep = [np.arange(off[b], off[b + 1]) for b in range(len(BLOCKS)) if BLOCKS[b] <= 255]
    for b in range(len(BLOCKS)):
        if BLOCKS[b] > 255:
            lo, hi = int(off[b]), int(off[b + 1])
            edge = [i for i in range(lo, hi) if i % 256 in (0, 255)]
            pick = edge if len(edge) <= 16 else edge[:8] + edge[-8:] + edge[8:-8:max(1, (len(edge) - 16) // 24)]
            pick = [lo, lo + 1, hi - 2, hi - 1] + pick
            if hi - lo > 30000:   # (where part_a_inputs puts the regulariser's special values)
                pick += list(range(lo + 20001, lo + 20012))
            keep.append(np.array(sorted(set(pick)), dtype=np.int64))
    return np.concatenate(keep)


A_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include "SGD.h"
#include "AdaMax.h"
#include "AdaDelta.h"
#include "L1Regularization.h"
#include "L2Regularization.h"

static std::vector<Vector *> blocks;
static void read_into(bool gradient) {
    for (size_t b = 0; b < blocks.size(); ++b)
        for (int j = 0; j < blocks[b]->size; ++j)
            if (scanf("%la", gradient ? &blocks[b]->gradient[j] : &blocks[b]->value[j]) != 1) exit(1);
}
static void print(const char *tag, const std::vector<Vector *> &v, bool gradient) {
    printf("%s", tag);
    for (size_t b = 0; b < v.size(); ++b)
        for (int j = 0; j < v[b]->size; ++j) printf(" %a", gradient ? v[b]->gradient[j] : v[b]->value[j]);
    printf("\n");
}
int main() {
    int kind, nBlocks, nBatch, nSteps, times;
    double lr, lambda;
    if (scanf("%d %d %d %d %la %la %d", &kind, &nBlocks, &nBatch, &nSteps, &lr, &lambda, &times) != 7) return 1;
    for (int b = 0; b < nBlocks; ++b) {
        int size;
        if (scanf("%d", &size) != 1) return 1;
        blocks.push_back(new Vector(size));
    }
    SGD sgd;
    AdaMax adamax;
    AdaDelta adadelta;
    L1Regularization l1(lambda);
    L2Regularization l2(lambda);
    for (int b = 0; b < nBlocks; ++b) {
        if (kind == 2) sgd.add(blocks[b]);
        if (kind == 3) adamax.add(blocks[b]);
        if (kind == 4) adadelta.add(blocks[b]);
        if (kind == 11) l1.add(blocks[b]);
        if (kind == 12) l2.add(blocks[b]);
    }
    if (kind < 10) read_into(false);
    for (int s = 0; s < nSteps; ++s) {
        if (kind > 10) read_into(false);
        read_into(true);
        if (kind == 2) sgd.Learn(lr, nBatch);
        if (kind == 3) adamax.Learn(lr, nBatch);
        if (kind == 4) adadelta.Learn(lr, nBatch);
        if (kind < 10) print("p", blocks, false);
        if (kind == 3) {
            print("s0", adamax.first_order, false);
            printf("norms");
            for (int b = 0; b < nBlocks; ++b) printf(" %a", adamax.infinity_norm[b]);
            printf("\nbeta1_t %a\n", adamax.beta1_t);
        }
        if (kind == 4) {
            print("s0", adadelta.expected_g, false);
            print("s1", adadelta.expected_deltax, false);
        }
        if (kind == 11) {
            l1.forward();
            for (int t = 0; t < times; ++t) l1.backward();
            printf("value %a\n", l1.getLoss());
        }
        if (kind == 12) {
            l2.forward();
            for (int t = 0; t < times; ++t) l2.backward();
            printf("value %a\n", l2.getLoss());
        }
        if (kind > 10) print("g", blocks, true);
    }
    return 0;
}
"""


def hexes(a):
    return " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel())


def parse(line, tag):
    tok = line.split()
    assert tok[0] == tag, (tok[0], tag)
    return np.array([float.fromhex(t) for t in tok[1:]], dtype=np.float64)


def run_part_a(exe, out):
    params, grads, reg = part_a_inputs()
    idx = a_index()
    out["a_index"] = idx
    out["a_blocks"] = np.array(BLOCKS, dtype=np.int64)
    out["a_checksum"] = np.array([params.sum(), grads.sum(), reg.sum()])
    head = "%d %d %d %d %s %s %d\n%s\n"
    for case, kind in A_KIND.items():
        g = case_grads(case, grads)
        text = head % (kind, len(BLOCKS), N_BATCH, N_STEPS, float(A_LR[case]).hex(), float(0.0).hex(), 0, " ".join(str(b) for b in BLOCKS))
        text += hexes(params) + "\n" + "".join(hexes(g[s]) + "\n" for s in range(N_STEPS))
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        rec = {"p": [], "s0": [], "s1": [], "norms": [], "beta1_t": []}
        for ln in lines:
            tag = ln.split(" ", 1)[0]
            v = parse(ln, tag)
            rec[tag].append(v if tag in ("norms", "beta1_t") else v[idx])
        for tag, rows in rec.items():
            if rows:
                assert len(rows) == N_STEPS
                out["a_%s__%s" % (case, tag)] = np.array(rows)
    for name, kind in (("l1", 11), ("l2", 12)):
        text = head % (kind, len(BLOCKS), N_BATCH, N_STEPS, float(0.0).hex(), float(REG_LAMBDA).hex(), REG_TIMES, " ".join(str(b) for b in BLOCKS))
        text += "".join(hexes(reg[s]) + "\n" + hexes(grads[s]) + "\n" for s in range(N_STEPS))
        lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
        out["a_%s__value" % name] = np.array([parse(ln, "value")[0] for ln in lines[0::2]])
        out["a_%s__g" % name] = np.array([parse(ln, "g")[idx] for ln in lines[1::2]])


# ---- Part B ----------------------------------------------------------------------------------------------------------------------------
# class -> (constructor arguments in the class's order, how the library is asked: (entry, arguments)).  entry "handle": the fields of
# gf_smp_config by name; "classifier": the same and nClass; "model": the arguments of graphflow_amd.smp.SMPModel.config.
BLOCK_CASES = {
    "SMP_omega": ("6, 6, 2, 4, 4, 1", ("handle", dict(nLevels=2, nChanels=4, nFeatures=4, nDepth=1, max_receptive_field=6, has_WL_ordering=1, nContractions=18))),
    "SMP_theta": ("6, 4, 2, 4, 4, 1", ("handle", dict(nLevels=2, nChanels=4, nFeatures=4, nDepth=1, max_receptive_field=4, has_WL_ordering=1, first_order=1, max_nVertices=6))),
    "SMP_1D_ver3": ("6, 2, 4, 4, 1, 0.9", ("handle", dict(nLevels=2, nChanels=4, nFeatures=4, nDepth=1, max_receptive_field=6, has_WL_ordering=1, first_order=4, max_nVertices=6))),
    "SMP_2D_ver5": ("6, 2, 4, 4, 1, 0.9", ("handle", dict(nLevels=2, nChanels=4, nFeatures=4, nDepth=1, max_receptive_field=6, has_WL_ordering=1, steerable_2d=5, max_nVertices=6))),
    "Unrestricted_SMP_2D": ("6, 2, 4, 4, 1, 0.9", ("handle", dict(nLevels=2, nChanels=4, nFeatures=4, nDepth=1, max_receptive_field=6, has_WL_ordering=1, unrestricted=3, max_nVertices=6))),
    "GCN_1D": ("2, 6, 4, 5, 1, 1, 0.9", ("handle", dict(nLevels=2, nChanels=5, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, neighbourhood=2, max_Radius=1))),
    "GRU_GCN_1D": ("2, 6, 4, 5, 1, 1, 0.9", ("handle", dict(nLevels=2, nChanels=5, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, neighbourhood=4, max_Radius=1))),
    "GCN_1D_Distance": ("2, 6, 4, 5, 1, 1, 0.9", ("handle", dict(nLevels=2, nChanels=5, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, neighbourhood=2, max_Radius=1, distance_channel=1))),
    "GCN_1D_Kernel": ("2, 6, 4, 5, 1, 1, 0.9", ("handle", dict(nLevels=2, nChanels=5, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, neighbourhood=2, max_Radius=1, readout=1))),
    "GCA_1D": ("2, 6, 4, 5, 1, 1, 0.9", ("handle", dict(nLevels=2, nChanels=5, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, neighbourhood=2, max_Radius=1, readout=2))),
    "LCNN": ("6, 4, 3, 1, 5, 4, 7, 0.9", ("handle", dict(nLevels=2, nChanels=5, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, matrix_form=1, nNeighbors=3, nChanels2=4, nDense=7))),
    "GCN_MW": ("2, 6, 4, 5, 1, 0.9", ("handle", dict(nLevels=2, nChanels=5, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, matrix_form=2))),
    "CGCN_1D": ("2, 6, 4, 1, 0.9", ("handle", dict(nLevels=2, nChanels=1, nFeatures=4, nDepth=1, max_receptive_field=6, max_nVertices=6, covariant=1))),
    "SMP_2D_ver6_classification": ("3, 6, 2, 4, 4, 1, 0.9", ("classifier", dict(nLevels=2, nChanels=4, nFeatures=4, nDepth=1, max_receptive_field=6, has_WL_ordering=1, nContractions=10, custom_matmul=1), 3)),
    "SMP_omega_physics": ("6, 6, 2, 4, 4", ("model", dict(nLevels=2, nChanels=4, max_receptive_field=6, nFeatures=4))),
    "SMP_omega_pairgraphs": ("6, 5, 5, 2, 4, 4, 3", ("model", dict(nLevels=2, nChanels=4, max_receptive_field=5, nFeatures=[4, 3]))),
    "CCN_1D": ("6, 5, 4, 2, 16, 4, 3, 0.7", ("model", dict(nLevels=2, nChanels=16, max_receptive_field=4, nFeatures=[4, 3], first_order=True, max_nVertices=[6, 5], ccn_1d=True,
                                                           nChanels_decay=0.7))),
}

B_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include GF_HEADER
int main() {
    GF_CLASS &net = *new GF_CLASS(GF_ARGS);   // (leaked on purpose)
    for (size_t i = 0; i < net.sgd->params.size(); ++i) printf("%d ", net.sgd->params[i]->size);
    printf("\n");
    return 0;
}
"""


def compile_driver(tmp, name, text, defines=()):
    src, exe = os.path.join(tmp, name + ".cpp"), os.path.join(tmp, name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-pthread", "-w", "-I", os.path.join(REF_ROOT, "GraphFlow"), *defines, "-o", exe, src])
    return exe


def run_part_b(tmp, out):
    def one(name):
        exe = compile_driver(tmp, "blocks_" + name, B_DRIVER, ['-DGF_HEADER="%s.h"' % name, "-DGF_CLASS=" + name, "-DGF_ARGS=" + BLOCK_CASES[name][0]])
        sizes = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
        return name, np.array(sizes, dtype=np.int64)
    with ThreadPoolExecutor(8) as pool:
        for name, sizes in pool.map(one, BLOCK_CASES):
            out["b_%s__sizes" % name] = sizes
            print("%-28s %3d blocks, %6d parameters" % (name, sizes.size, sizes.sum()))
    out["b_classes"] = np.array(list(BLOCK_CASES))


# ---- Part C ----------------------------------------------------------------------------------------------------------------------------
# class -> (constructor arguments, the three calls of the class's gradient sum, the loss object)
TRAJ_CLASSES = {
    "SMP_omega": ("6, 6, 2, 4, 4, 1", "net.sum_gradients->reset_sum_gradients()", "net.sum_gradients->cache_gradients()", "net.sum_gradients->get_sum_gradients()"),
    "GCN_1D": ("2, 6, 4, 5, 1, 1, 0.9", "net.init_sum_gradients()", "net.update_sum_gradients()", "net.get_sum_gradients()"),
    "SMP_2D_ver6_classification": ("3, 6, 2, 4, 4, 1, 0.9", "net.sum_gradients->reset_sum_gradients()", "net.sum_gradients->cache_gradients()",
                                   "net.sum_gradients->get_sum_gradients()"),
    "SMP_omega_physics": ("6, 6, 2, 4, 4", "net.sum_gradients->reset_sum_gradients()", "net.sum_gradients->cache_gradients()", "net.sum_gradients->get_sum_gradients()"),
}
TRAJ_STEPS = 4
TRAJ_LR = {"sgd": (0.02, 0.005, 0.001, 0.0002, 0.00005), "adamax": (0.005,), "adadelta": (0.0,)}   # tried in this order
MAX_STEP = 0.2   # no single step may move a weight further: beyond it the class is diverging and fp32 activations say nothing about the step
TRAJ_KIND = {"sgd": 2, "adamax": 3, "adadelta": 4}
TRAJ_SEEDS = (23, 1, 2, 3, 5, 7, 11, 13)

C_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>
#include <algorithm>
#include GF_HEADER
#include "SGD.h"
#include "AdaMax.h"
#include "AdaDelta.h"

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
static std::vector<double> values(Net &net) {
    std::vector<double> v;
    for (size_t i = 0; i < net.sgd->params.size(); ++i)
        for (int j = 0; j < net.sgd->params[i]->size; ++j) v.push_back(net.sgd->params[i]->value[j]);
    return v;
}
static void print(const std::vector<double> &v) {
    for (size_t i = 0; i < v.size(); ++i) printf("%a ", v[i]);
    printf("\n");
}
int main() {
    int seed, n, F, kind, nSteps;
    double lr;
    if (scanf("%d %d %d %d %d %la", &seed, &n, &F, &kind, &nSteps, &lr) != 6) return 1;
    std::vector<DenseGraph *> x;
    std::vector<double> t(n);
    for (int i = 0; i < n; ++i) x.push_back(read_graph(F));
    for (int i = 0; i < n; ++i) scanf("%lf", &t[i]);
    srand((unsigned)seed);
    GF_CLASS &net = *new GF_CLASS(GF_ARGS);   // (leaked on purpose)
    SGD sgd;
    AdaMax adamax;
    AdaDelta adadelta;
    for (size_t i = 0; i < net.sgd->params.size(); ++i) {
        sgd.add(net.sgd->params[i]);
        adamax.add(net.sgd->params[i]);
        adadelta.add(net.sgd->params[i]);
    }
    print(values(net));
    double step_max = 0.0;
    for (int s = 0; s < nSteps; ++s) {
        const double before = net.getLoss(n, &x[0], &t[0]);
        GF_RESET;
        for (int i = 0; i < n; ++i) {
            net.complete_computation_graph(x[i]);
            net.target->value[0] = t[i];
            net.graph->forward();
            net.graph->backward();
            GF_CACHE;
        }
        GF_SUM;
        if (s == 0)
            for (size_t i = 0; i < net.sgd->params.size(); ++i) {
                bool any = false;
                for (int j = 0; j < net.sgd->params[i]->size; ++j) any = any || net.sgd->params[i]->gradient[j] != 0.0;
                if (!any) return 3;
            }
        const std::vector<double> old = values(net);
        if (kind == 2) sgd.Learn(lr, n);
        if (kind == 3) adamax.Learn(lr, n);
        if (kind == 4) adadelta.Learn(lr, n);
        const std::vector<double> now = values(net);
        for (size_t i = 0; i < now.size(); ++i) step_max = std::max(step_max, std::fabs(now[i] - old[i]));
        printf("%a %a\n", before, net.getLoss(n, &x[0], &t[0]));
    }
    print(values(net));
    printf("%a\n", step_max);
    return 0;
}
"""


def traj_batch(name):
    """(graphs, targets): the four toy molecules; the classifier's labels are the molecule's index modulo 3"""
    tm = toy_molecules()
    x = [(a, f) for _, a, f, _ in tm]
    t = [float(i % 3) for i in range(len(tm))] if name == "SMP_2D_ver6_classification" else [tg for *_, tg in tm]
    return x, t


def run_part_c(tmp, out):
    for name, (args, reset, cache, total) in TRAJ_CLASSES.items():
        exe = compile_driver(tmp, "traj_" + name, C_DRIVER, ['-DGF_HEADER="%s.h"' % name, "-DGF_CLASS=" + name, "-DGF_ARGS=" + args, "-DGF_RESET=" + reset,
                                                            "-DGF_CACHE=" + cache, "-DGF_SUM=" + total])
        x, t = traj_batch(name)
        for opt, kind in TRAJ_KIND.items():
            found = None
            for lr in TRAJ_LR[opt]:
                for seed in TRAJ_SEEDS:
                    text = "%d %d %d %d %d %s\n" % (seed, len(x), 4, kind, TRAJ_STEPS, float(lr).hex())
                    text += "".join(graph_text(a, f) for a, f in x) + " ".join("%.17g" % v for v in t) + "\n"
                    r = subprocess.run([exe], input=text, capture_output=True, text=True)
                    if r.returncode == 3 or "nan" in r.stdout or "inf" in r.stdout:   # a zero block at step 1, or an overflow: the next seed
                        continue
                    assert r.returncode == 0, (name, opt, r.returncode, r.stderr[-500:])
                    if float.fromhex(r.stdout.split()[-1]) <= MAX_STEP:   # (a rate at which the class itself runs away says nothing: the next one)
                        found = (r, seed, lr)
                        break
                if found:
                    break
            assert found, "%s / %s: no rate and seed keep the reference finite and its steps below %g" % (name, opt, MAX_STEP)
            r, seed, lr = found
            lines = r.stdout.strip().split("\n")
            assert len(lines) == TRAJ_STEPS + 3
            hx = lambda ln: np.array([float.fromhex(v) for v in ln.split()])   # noqa: E731
            p_ = "c_%s__%s__" % (name, opt)
            out[p_ + "params0"], out[p_ + "params"] = hx(lines[0]), hx(lines[-2])
            out[p_ + "losses"] = np.array([hx(ln) for ln in lines[1:-2]])
            out[p_ + "step_max"] = hx(lines[-1])
            out[p_ + "seed"] = np.array([seed], dtype=np.int32)
            out[p_ + "lr"] = np.array([lr])
            assert np.isfinite(out[p_ + "params"]).all() and np.isfinite(out[p_ + "losses"]).all()
            print("%-28s %-9s seed %-3d losses %s step_max %.3g" % (name, opt, seed, np.array2string(out[p_ + "losses"][:, 0], precision=5), out[p_ + "step_max"][0]))
    out["c_classes"] = np.array(list(TRAJ_CLASSES))


def main():
    if not os.path.exists(os.path.join(REF_ROOT, "GraphFlow", "AdaMax.h")):
        sys.exit("reference not found at %r: set GF_REFERENCE to the tree that holds GraphFlow/" % REF_ROOT)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        run_part_a(compile_driver(tmp, "operators", A_DRIVER), out)
        run_part_b(tmp, out)
        run_part_c(tmp, out)
    path = os.path.join(HERE, "optimisers.npz")
    np.savez_compressed(path, **out)
    print("wrote optimisers.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
