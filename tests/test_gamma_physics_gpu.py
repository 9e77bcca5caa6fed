"""GPU suite for SMP_gamma_physics / SMP_gamma_pairgraphs (GraphFlow/SMP_gamma_physics.h, SMP_gamma_pairgraphs.h): the `_physics`
(one tower) and `_pairgraphs` (two towers) models with RisiContraction_4 and K_l [4 C_{l-1}][C_l], through gf_smp_model_* with
nContractions = 4.  The towers compute at their own halving widths on the rectangular gamma level (smp_level_gamma.hip: packed
forward / backward gathers) and, under set_fused(False), op by op (promotion + the batched `_4` kernels + the K-projection).
Against the real classes' own numbers (tests/golden/smp_gamma_physics.npz, make_gamma_physics_golden.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from inputs import synthetic_molecule, toy_molecules
from util import golden_cases, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "smp_gamma_physics.npz")


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def channels(Cn, L):
    return [max(1, Cn >> l) for l in range(L + 1)]


def blocks(towers, L, Cn, feats):
    """(name, size) of every parameter block in registration order: H_t, (K_t_l, b_t_l)..., then the head's matrices and vector."""
    c = channels(Cn, L)
    out = [("H%d" % t, Cn * feats[t]) for t in range(towers)]
    for l in range(1, L + 1):
        for t in range(towers):
            out += [("K%d_%d" % (t, l), 4 * c[l - 1] * c[l]), ("b%d_%d" % (t, l), c[l])]
    w = towers * sum(c)
    widths = [w, w // 2] if towers == 1 else [w, max(w // 2, 10), max(max(w // 2, 10) // 2, 10)]
    out += [("W%d" % i, widths[i] * widths[i - 1]) for i in range(1, len(widths))] + [("w", widths[-1])]
    return out


def model(towers, L, Cn, cap, feats, fused=True):
    from graphflow_amd.smp import SMPModel
    net = SMPModel(L, Cn, cap, feats[:towers], nContractions=4)
    net.set_fused(fused)
    return net


def step(net, params, tg):
    p = dev(params)
    pred, loss = net.forward(p, dev(tg))
    g = torch.full((net.n_params,), float("nan"), device="cuda")
    net.backward(p, g)
    return pred.cpu().numpy().astype(np.float64), loss.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("fused", [True, False])
def test_goldens_of_the_real_classes(gf, fused):
    cs = golden_cases(golden(), "gphys_")
    assert len(cs) == 5
    for tag, c in cs.items():
        towers, L, Cn, cap, _, _ = (int(x) for x in c["cfg"])
        feats = [c["feature"].shape[1]] + ([c["feature2"].shape[1]] if towers == 2 else [])
        net = model(towers, L, Cn, cap, feats, fused)
        assert net.n_params == c["params"].size
        net.prepare([(c["adj"], c["feature"])], [(c["adj2"], c["feature2"])] if towers == 2 else None)
        pred, loss, grads = step(net, c["params"], c["target"])
        e = (rel_err(pred, c["predict"]), rel_err(loss, c["loss"]), rel_err(grads, c["grads"]))
        print("%-20s fused %d: predict %.2e loss %.2e grads %.2e" % (tag, fused, *e))
        assert e[0] <= TOL and e[1] <= 2 * TOL and e[2] <= TOL, (tag, e)
        net.close()


def test_initial_weights_are_the_reference_draw(gf):
    z = golden()
    for name in ("trainphys", "trainpair"):
        towers, L, Cn, cap, maxV, seed, _ = (int(x) for x in z[name + "__cfg"])
        net = model(towers, L, Cn, cap, [4, 4])
        C.CDLL(None).srand(seed)
        w = net.uniform_init_host()
        assert np.array_equal(w, z[name + "__params0"]), name
        net.close()


def qm9_batch(n, seed):
    rng = np.random.default_rng(seed)
    g1, g2, tg = [], [], []
    for i in range(n):
        a, x, t = synthetic_molecule(seed * 1000 + i, int(rng.integers(3, 30)))
        b, y, _ = synthetic_molecule(seed * 1000 + 500 + i, int(rng.integers(3, 30)))
        g1.append((a, x))
        g2.append((b, y))
        tg.append(t)
    return g1, g2, np.array(tg)


@pytest.mark.parametrize("towers,Cn", [(1, 16), (2, 16), (1, 64), (2, 64), (1, 10), (2, 10)])
def test_fused_equals_op_by_op_at_qm9_sizes(gf, towers, Cn):
    """About 200 QM9-size molecules, cap 29, L = 3: the packed gamma tower level against promotion + `_4` kernels + K-projection, on the
    same handle.  Every parameter block within 2e-5 (relative to max(|block|, 1))."""
    g1, g2, tg = qm9_batch(200, 31 + Cn + towers)
    L, cap = 3, 29
    net = model(towers, L, Cn, cap, [5, 5])
    params = np.random.default_rng(Cn).uniform(-0.1, 0.1, net.n_params)
    assert net.n_params == sum(n for _, n in blocks(towers, L, Cn, [5, 5]))
    net.prepare(g1, g2 if towers == 2 else None)
    got = {}
    for fused in (True, False):
        net.set_fused(fused)
        got[fused] = step(net, params, tg)
    net.close()
    (pa, la, ga), (pb, lb, gb) = got[True], got[False]
    assert np.isfinite(ga).all() and np.abs(ga).max() > 0
    assert rel_err(pa, pb) <= 2e-5 and rel_err(la, lb) <= 2e-5
    off = 0
    for name, n in blocks(towers, L, Cn, [5, 5]):
        e = rel_err(ga[off:off + n], gb[off:off + n])
        assert e <= 2e-5, (name, e)
        off += n
    assert off == ga.size


def test_fused_plan_runs_the_tower_gathers(gf):
    """The fused plan runs the packed forward and backward gathers once per level and tower, and no promotion / `_4` kernels;
    set_fused(False) runs none of the gathers."""
    g1, g2, tg = qm9_batch(24, 7)
    L, Cn = 3, 16
    net = model(2, L, Cn, 29, [5, 5])
    params = np.random.default_rng(3).uniform(-0.2, 0.2, net.n_params)
    net.prepare(g1, g2)
    counts = {}
    for fused in (True, False):
        net.set_fused(fused)
        net.ctx.set_timing(True)
        step(net, params, tg)
        counts[fused] = {k: n for k, (_, n) in net.ctx.timings().items()}
        net.ctx.set_timing(False)
    net.close()
    on, off = counts[True], counts[False]
    assert on.get("smpg_tower_fwd") == 2 * L and on.get("smpg_tower_bwd") == 2 * L, on
    assert "smp_promote_fwd" not in on and "smp_promote_bwd" not in on, on
    assert "smpg_level_fwd" not in on and "smpg_level_bwd" not in on, on
    assert "smpg_tower_fwd" not in off and "smpg_tower_bwd" not in off, off
    assert off.get("smp_promote_fwd") == 2 * L, off


def test_batch_gradient_is_the_sum_and_steps_are_bit_identical(gf):
    g1, g2, tg = qm9_batch(5, 11)
    L, Cn = 3, 10
    net = model(2, L, Cn, 29, [5, 5])
    params = np.random.default_rng(4).uniform(-0.3, 0.3, net.n_params)
    p = dev(params)
    net.prepare(g1, g2)
    a = step(net, params, tg)
    b = step(net, params, tg)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    total = torch.zeros(net.n_params, device="cuda")
    for i in range(len(tg)):
        net.prepare([g1[i]], [g2[i]])
        pi = net.forward(p, dev(tg[i:i + 1]))[0]
        assert abs(float(pi[0]) - a[0][i]) <= 1e-5 * max(1.0, abs(a[0][i]))
        net.backward(p, total, accumulate=True)
    assert rel_err(total.cpu().numpy(), a[2]) <= 2e-6
    net.close()


def test_refusals(gf):
    from graphflow_amd.ops import GraphFlowHipError
    from graphflow_amd.smp import SMPModel
    with pytest.raises(GraphFlowHipError, match="nKept"):
        SMPModel(3, 16, 6, [5, 5], nKept=7, nContractions=4)
    for nK in (5, 10, 50):
        with pytest.raises(GraphFlowHipError, match="nContractions"):
            SMPModel(3, 16, 6, [5], nContractions=nK)


def test_goldens_pass_under_poison(gf):
    """GF_POISON=1 (every buffer handed out without contents starts as NaN patterns): no tower kernel reads memory nobody wrote."""
    env = dict(os.environ, GF_POISON="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "goldens_of_the_real_classes",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert "2 passed" in tail and "failed" not in tail, tail


CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "SMP_physics_hip.h"

struct Molecule {  // public fields of GraphFlow/DenseGraph.h
    int nVertices, nFeatures;
    int **adj;
    double **feature;
};

static Molecule *read_molecule(FILE *in, int F) {
    Molecule *g = new Molecule;
    std::fscanf(in, "%d", &g->nVertices);
    g->nFeatures = F;
    g->adj = new int *[g->nVertices];
    g->feature = new double *[g->nVertices];
    for (int i = 0; i < g->nVertices; ++i) {
        g->adj[i] = new int[g->nVertices];
        for (int j = 0; j < g->nVertices; ++j) std::fscanf(in, "%d", &g->adj[i][j]);
    }
    for (int i = 0; i < g->nVertices; ++i) {
        g->feature[i] = new double[F];
        for (int f = 0; f < F; ++f) std::fscanf(in, "%lf", &g->feature[i][f]);
    }
    return g;
}

int main(int argc, char **argv) {
    FILE *in = std::fopen(argv[1], "r");
    int towers, L, C, cap, maxV, seed, nIter, nMol;
    double lr;
    if (std::fscanf(in, "%d %d %d %d %d %d %d %lf %d", &towers, &L, &C, &cap, &maxV, &seed, &nIter, &lr, &nMol) != 9) return 2;
    std::vector<Molecule *> m1(nMol), m2(nMol);
    std::vector<double> tgt(nMol);
    for (int m = 0; m < nMol; ++m) m1[m] = read_molecule(in, 4);
    if (towers == 2)
        for (int m = 0; m < nMol; ++m) m2[m] = read_molecule(in, 4);
    for (int m = 0; m < nMol; ++m) std::fscanf(in, "%lf", &tgt[m]);
    std::fclose(in);
    srand((unsigned)seed);
    if (towers == 1) {
        SMP_gamma_physics_hip net(maxV, cap, L, C, 4);   // SMP_gamma_physics.h:31
        for (int it = 0; it < nIter; ++it) {
            std::pair<double, double> r = net.BatchLearn(nMol, &m1[0], &tgt[0], lr);
            std::printf("%.17g %.17g\n", r.first, r.second);
        }
        SMP_gamma_physics_hip other(true, maxV, cap, L, C, 4);   // the use_coulomb constructor (SMP_gamma_physics.h:47) builds too
        std::vector<double> y(nMol);
        other.Threaded_Predict(nMol, &m1[0], &y[0]);
        std::fprintf(stderr, "predict %g\n", other.Predict(m1[0]));
    } else {
        SMP_gamma_pairgraphs_hip net(maxV, maxV, cap, L, C, 4, 4);
        for (int it = 0; it < nIter; ++it) {
            std::pair<double, double> r = net.BatchLearn(nMol, &m1[0], &m2[0], &tgt[0], lr);
            std::printf("%.17g %.17g\n", r.first, r.second);
        }
        std::vector<double> y(nMol);
        net.Threaded_Predict(nMol, &m1[0], &m2[0], &y[0]);
        std::fprintf(stderr, "predict %g %g\n", y[0], net.Predict(m1[0], m2[0]));
    }
    return 0;
}
"""


@pytest.mark.parametrize("name", ["trainphys", "trainpair"])
def test_cpp_dropins_reproduce_batchlearn(gf, tmp_path, name):
    """SMP_gamma_physics_hip / SMP_gamma_pairgraphs_hip (graphflow_amd/host/SMP_physics_hip.h) driven like the reference classes: srand,
    constructor, three BatchLearn calls; their (before, after) losses against the real classes'.  Compiled with the flags of
    tests/cpp/Makefile."""
    z = golden()
    towers, L, Cn, cap, maxV, seed, nIter = (int(x) for x in z[name + "__cfg"])
    mols = [(a, f) for _, a, f, _ in toy_molecules()]
    if towers == 1:
        m1, m2 = mols, []
    else:
        m1 = [mols[i] for i in range(4) for j in range(4)]
        m2 = [mols[j] for i in range(4) for j in range(4)]
    src, exe, inp = tmp_path / "gamma_physics_dropin.cpp", tmp_path / "gamma_physics_dropin", tmp_path / "input.txt"
    src.write_text(CPP)
    lines = ["%d %d %d %d %d %d %d %.17g %d" % (towers, L, Cn, cap, maxV, seed, nIter, float(z[name + "__lr"][0]), len(m1))]
    for adj, feat in m1 + m2:
        lines += [str(len(adj)), " ".join(str(int(v)) for v in adj.ravel()), " ".join("%.17g" % v for v in feat.ravel())]
    lines.append(" ".join("%.17g" % t for t in z[name + "__targets"]))
    inp.write_text("\n".join(lines) + "\n")
    csrc = os.path.join(ROOT, "graphflow_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "graphflow_amd", "host"),
                           "-o", str(exe), str(src), "-L" + csrc, "-lgf_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-lm"])
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array(r.stdout.split(), dtype=np.float64).reshape(nIter, 2)
    ref = z[name + "__losses"]
    print(name, got.ravel().tolist(), ref.ravel().tolist())
    assert np.all(np.abs(got[:, 0] - ref[:, 0]) <= TOL * np.maximum(1.0, ref[:, 0]))
    assert np.all(np.abs(got[:, 1] - ref[:, 1]) <= 5 * TOL * np.maximum(1.0, ref[:, 1]))
