"""GPU suite for SMP_gamma (GraphFlow/SMP_gamma.h): the batched driver with nContractions = 4 -- the SMP_omega DAG with RisiContraction_4,
no receptive-field cap, no reduced adjacency -- on its fused level (smp_level_gamma.hip: block products on the rows of the level below,
one gather with bias + LeakyReLU forward, one consumer gather backward; P, dP, T and dT are never written) and on the op-by-op level (gf_smp_set_fused(0), fields above 64 positions, more
than 64 channels: promotion + the batched `_4` contraction kernels).  Checked against the fp64 restatement smp_oracle.run(nK=4, cap=V),
which tests/test_smp_gamma_cpu.py pins to the real class, and against the real class's own numbers (tests/golden/smp_gamma.npz)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from field_suite import dev, run_under_poison
from inputs import er_graph, synthetic_molecule, toy_molecules
from make_gamma_golden import gamma_params
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5   # the suite's end-to-end tolerance (tests/test_smp_gpu.py)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def gamma_net(L, Cn, F, D, maxV, wl=True, fused=True):
    from graphflow_amd.smp import SMPGamma
    net = SMPGamma(L, Cn, F, D, maxV, wl)
    net.set_fused(fused)
    return net


def run_gamma(mols, targets, params, L, Cn, D, maxV, wl=True, fused=True, coulomb=None, accumulate_twice=False):
    net = gamma_net(L, Cn, mols[0][1].shape[1], D, maxV, wl, fused)
    net.prepare(mols, coulomb=coulomb)
    p = dev(params)
    pred, loss, feat = net.forward(p, dev(targets))
    out = [pred.cpu().numpy().astype(np.float64), loss.cpu().numpy().astype(np.float64), feat.cpu().numpy().astype(np.float64)]
    grads = torch.empty(net.n_params, device="cuda")
    net.backward(p, grads)
    out.append(grads.cpu().numpy().astype(np.float64))
    if accumulate_twice:
        net.forward(p, dev(targets))
        net.backward(p, grads, accumulate=True)
        out.append(grads.cpu().numpy().astype(np.float64))
    net.close()
    return out


def oracle_batch(mols, targets, params, L, Cn, D, maxV, wl=True):
    from oracle import smp_oracle
    pred, feat, g = [], [], 0.0
    for (adj, x), t in zip(mols, targets):
        r = smp_oracle.run(adj, x, float(t), np.asarray(params, dtype=np.float64), L, Cn, D, maxV, wl, nK=4)
        pred.append(r["predict"])
        feat.append(r["graph_feature"])
        g = g + r["grads"]
    return np.array(pred), np.array(feat), g


def small_batch(n, seed, vmax=14):
    rng = np.random.default_rng(seed)
    mols, tg = [], []
    for i in range(n):
        adj, x, t = synthetic_molecule(seed * 100 + i, int(rng.integers(3, vmax + 1)))
        mols.append((adj, x))
        tg.append(t)
    return mols, np.array(tg, dtype=np.float64)


@pytest.mark.parametrize("wl", [True, False])
@pytest.mark.parametrize("L", [2, 3, 4])
@pytest.mark.parametrize("Cn", [5, 32, 64])
@pytest.mark.parametrize("fused", [True, False])
def test_gamma_matches_the_oracle(gf, fused, Cn, L, wl):
    """Prediction, graph feature and the summed gradient of a small synthetic batch against smp_oracle.run(nK=4, cap=max_nVertices)."""
    mols, tg = small_batch(3, 10 * L + Cn + (1 if wl else 0), vmax=11)
    F, D = mols[0][1].shape[1], 2
    maxV = max(len(a) for a, _ in mols)
    params = gamma_params(Cn, F, D, L, 7000 + Cn + L)
    pred, _, feat, grads = run_gamma(mols, tg, params, L, Cn, D, maxV, wl, fused)
    rp, rf, rg = oracle_batch(mols, tg, params, L, Cn, D, maxV, wl)
    assert rel_err(pred, rp) <= TOL
    assert rel_err(feat, rf) <= TOL
    assert rel_err(grads, rg) <= TOL


def test_device_matches_the_real_smp_gamma(gf):
    """Every case of tests/golden/smp_gamma.npz (toy molecules, synthetic molecules at L = 2..4, an ER-20 graph at L = 4), one
    molecule per batch, fused and op by op, against the real class's numbers."""
    with np.load(os.path.join(HERE, "golden", "smp_gamma.npz")) as z:
        gz = {k: z[k] for k in z.files}
    for tag in gz["tags"]:
        p = "gamma_" + str(tag) + "__"
        L, Cn, D, wl, maxV = (int(x) for x in gz[p + "cfg"])
        for fused in (True, False):
            pred, loss, feat, grads = run_gamma([(gz[p + "adj"], gz[p + "feature"])], gz[p + "target"], gz[p + "params"], L, Cn, D, maxV,
                                                bool(wl), fused)
            assert rel_err(pred, gz[p + "predict"]) <= TOL, tag
            assert rel_err(feat[0], gz[p + "graph_feature"]) <= TOL, tag
            assert rel_err(loss, gz[p + "loss"]) <= 2 * TOL, tag
            assert rel_err(grads, gz[p + "grads"]) <= TOL, tag


def test_fused_equals_op_by_op_at_qm9_sizes(gf):
    """A few hundred QM9-size molecules at C = 64, L = 3: the fused level against the op-by-op level (promotion + `_4` kernels).
    Both are fp32 with different summation orders; the relative bound is the suite's."""
    rng = np.random.default_rng(5)
    mols, tg = [], []
    for i in range(300):
        adj, x, t = synthetic_molecule(90000 + i, int(rng.integers(3, 30)))
        mols.append((adj, x))
        tg.append(t)
    tg = np.array(tg)
    L, Cn, D = 3, 64, 2
    params = gamma_params(Cn, 5, D, L, 77)
    a = run_gamma(mols, tg, params, L, Cn, D, 29, True, True)
    b = run_gamma(mols, tg, params, L, Cn, D, 29, True, False)
    assert rel_err(a[0], b[0]) <= TOL
    assert rel_err(a[2], b[2]) <= TOL
    assert rel_err(a[3], b[3]) <= TOL


def test_fused_plan_runs_the_gamma_kernels(gf):
    """The fused plan really runs smp_level_gamma.hip at every level (one forward gather and one backward gather per level, no promotion,
    no `_4` contraction), and gf_smp_set_fused(0) runs none of it.  Read from the context's per-kernel launch counts."""
    mols, tg = small_batch(8, 12, vmax=20)
    L, Cn, D = 3, 32, 2
    params = dev(gamma_params(Cn, 5, D, L, 12))
    net = gamma_net(L, Cn, 5, D, 20)
    net.prepare(mols)
    grads = torch.empty(net.n_params, device="cuda")
    counts = {}
    for fused in (True, False):
        net.set_fused(fused)
        net.ctx.set_timing(True)
        net.forward(params, dev(tg))
        net.backward(params, grads)
        counts[fused] = {k: n for k, (_, n) in net.ctx.timings().items()}
        net.ctx.set_timing(False)
    net.close()
    on, off = counts[True], counts[False]
    assert on.get("smpg_level_fwd") == L and on.get("smpg_level_bwd") == L, on
    assert "smp_promote_fwd" not in on and "smp_promote_bwd" not in on, on
    assert "smpg_level_fwd" not in off and "smpg_level_bwd" not in off, off
    assert off.get("smp_promote_fwd") == L, off


@pytest.mark.parametrize("V,fused", [(50, True), (70, True), (70, False)])
def test_wide_fields_match_the_oracle(gf, V, fused):
    """ER graphs of 50 vertices (level-3 fields of 33 .. 50 positions: the fused level) and 70 (fields above 64: the op-by-op level
    whatever gf_smp_set_fused says) against the oracle."""
    adj, x = er_graph(V, 0.08, 4, 11 + V)
    L, Cn, D = 3, 8, 1
    from oracle import smp_oracle
    r = smp_oracle.run(adj, x, 3.0, gamma_params(Cn, 4, D, L, V), L, Cn, D, V, True, want_grads=False, nK=4)
    smax = max(len(f) for f in r["phi"][L])
    assert smax > (64 if V == 70 else 32), smax
    params = gamma_params(Cn, 4, D, L, V)
    pred, _, feat, grads = run_gamma([(adj, x)], np.array([3.0]), params, L, Cn, D, V, True, fused)
    rp, rf, rg = oracle_batch([(adj, x)], [3.0], params, L, Cn, D, V, True)
    assert rel_err(pred, rp) <= TOL
    assert rel_err(feat, rf) <= TOL
    assert rel_err(grads, rg) <= TOL


def test_feature_is_invariant_under_vertex_permutation(gf):
    mols, tg = small_batch(4, 3, vmax=16)
    rng = np.random.default_rng(0)
    perm_mols = []
    for adj, x in mols:
        p = rng.permutation(len(adj))
        perm_mols.append((adj[np.ix_(p, p)], x[p]))
    L, Cn, D = 3, 32, 2
    params = gamma_params(Cn, 5, D, L, 3)
    a = run_gamma(mols, tg, params, L, Cn, D, 16)
    b = run_gamma(perm_mols, tg, params, L, Cn, D, 16)
    assert rel_err(b[2], a[2]) <= TOL


def test_coulomb_prepare_equals_plain_prepare(gf):
    """SMP_gamma's use_coulomb constructors: RisiContraction_4 reads no adjacency, so the Coulomb entries change nothing."""
    mols, tg = small_batch(5, 4)
    rng = np.random.default_rng(4)
    cm = []
    for adj, _ in mols:
        M = rng.uniform(-1, 2, adj.shape)
        cm.append(0.5 * (M + M.T))
    L, Cn, D = 2, 32, 2
    params = gamma_params(Cn, 5, D, L, 4)
    a = run_gamma(mols, tg, params, L, Cn, D, 14)
    b = run_gamma(mols, tg, params, L, Cn, D, 14, coulomb=cm)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_bit_reproducible_and_accumulate_doubles(gf):
    mols, tg = small_batch(40, 6, vmax=29)
    L, Cn, D = 3, 64, 2
    params = gamma_params(Cn, 5, D, L, 6)
    a = run_gamma(mols, tg, params, L, Cn, D, 29, accumulate_twice=True)
    b = run_gamma(mols, tg, params, L, Cn, D, 29)
    for x, y in zip(a[:4], b):
        assert np.array_equal(x, y)
    assert np.array_equal(a[4], 2 * a[3])   # (x + x is exact in fp32)


def test_batchlearn_steps_match_the_real_smp_gamma(gf):
    """Three BatchLearn steps of the real SMP_gamma on the four toy molecules (tests/golden/smp_gamma.npz): initial weights from
    gf_smp_uniform_init_host after the same srand, gf_smp_adam_step.  Tolerances of test_batchlearn_steps_match_the_reference."""
    z = np.load(os.path.join(HERE, "golden", "smp_gamma.npz"))
    L, Cn, D, maxV, seed, nIter = (int(x) for x in z["train__cfg"])
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    tg = dev(z["train__targets"])
    lr = float(z["train__lr"][0])
    net = gamma_net(L, Cn, mols[0][1].shape[1], D, maxV)
    C.CDLL(None).srand(seed)
    p = dev(net.uniform_init())
    assert np.array_equal(p.cpu().numpy(), z["train__params0"].astype(np.float32))
    net.prepare(mols)
    grads = torch.empty(net.n_params, device="cuda")
    for it in range(nIter):
        _, loss, _ = net.forward(p, tg)
        before = float(loss.sum())
        net.backward(p, grads)
        net.adam_step(p, grads, lr, len(mols))
        _, loss, _ = net.forward(p, tg)
        after = float(loss.sum())
        assert abs(before - z["train__losses"][it, 0]) <= TOL * max(1.0, before), it
        assert abs(after - z["train__losses"][it, 1]) <= 5 * TOL * max(1.0, after), it
    err = np.abs(p.cpu().numpy().astype(np.float64) - z["train__params"])
    assert err.max() <= 0.005 * lr
    assert np.median(err) <= 1e-6
    net.close()


def test_checkpoint_round_trip(gf, tmp_path):
    L, Cn, F, D = 2, 6, 4, 3
    net = gamma_net(L, Cn, F, D, 10)
    n = Cn * F * (D + 1) + L * (4 * Cn * Cn + Cn) + Cn   # the reference's parameter count (SMP_gamma.h registration order)
    assert net.n_params == n
    params = dev(gamma_params(Cn, F, D, L, 9))
    path = str(tmp_path / "gamma.txt")
    net.save_model(params, path)
    with open(path) as f:
        vals = np.array(f.read().split(), dtype=np.float64)
    assert vals.size == n
    back = torch.empty(n, device="cuda")
    net.load_model(back, path)
    assert np.allclose(back.cpu().numpy(), params.cpu().numpy(), rtol=1e-5, atol=0)
    net.close()


def test_refusals(gf):
    from graphflow_amd.ops import GraphFlowHipError
    from graphflow_amd.smp import SMPOmega
    with pytest.raises(GraphFlowHipError, match="custom_matmul"):
        SMPOmega(2, 8, 4, 1, 10, True, nContractions=4, custom_matmul=True)
    with pytest.raises(GraphFlowHipError, match="physics"):
        SMPOmega(2, 8, 4, 0, 10, True, nContractions=4, physics=True)


def test_gamma_tests_pass_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no gamma kernel reads memory nobody
    wrote."""
    run_under_poison(__file__, "matches_the_oracle or real_smp_gamma or wide_fields or qm9_sizes", timeout=900)


CPP = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "SMP_omega_hip.h"

struct Molecule {  // public fields of GraphFlow/DenseGraph.h
    int nVertices, nFeatures;
    int **adj;
    double **feature;
};

int main(int argc, char **argv) {
    FILE *in = std::fopen(argv[1], "r");
    int maxV, L, C, F, D, seed, nIter, nMol;
    double lr;
    if (std::fscanf(in, "%d %d %d %d %d %d %d %lf %d", &maxV, &L, &C, &F, &D, &seed, &nIter, &lr, &nMol) != 9) return 2;
    std::vector<Molecule *> mol(nMol);
    std::vector<double> tgt(nMol);
    for (int m = 0; m < nMol; ++m) {
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
        mol[m] = g;
    }
    for (int m = 0; m < nMol; ++m) std::fscanf(in, "%lf", &tgt[m]);
    std::fclose(in);
    srand((unsigned)seed);
    SMP_gamma_hip net(maxV, L, C, F, D);   // SMP_gamma.h:31
    for (int it = 0; it < nIter; ++it) {
        std::pair<double, double> r = net.BatchLearn(nMol, &mol[0], &tgt[0], lr);
        std::printf("%.17g %.17g\n", r.first, r.second);
    }
    SMP_gamma_hip other(true, maxV, L, C, F, D, true);   // the use_coulomb constructor (SMP_gamma.h:82) builds too
    return 0;
}
"""


def test_cpp_dropin_batchlearn(gf, tmp_path):
    """SMP_gamma_hip (graphflow_amd/host/SMP_omega_hip.h) driven from C++ like the reference class: srand, constructor, three
    BatchLearn calls; its (before, after) losses against the real SMP_gamma's.  Compiled with the flags of tests/cpp/Makefile."""
    z = np.load(os.path.join(HERE, "golden", "smp_gamma.npz"))
    L, Cn, D, maxV, seed, nIter = (int(x) for x in z["train__cfg"])
    mols = toy_molecules()
    F = mols[0][2].shape[1]
    src, exe, inp = tmp_path / "gamma_dropin.cpp", tmp_path / "gamma_dropin", tmp_path / "input.txt"
    src.write_text(CPP)
    lines = ["%d %d %d %d %d %d %d %.17g %d" % (maxV, L, Cn, F, D, seed, nIter, float(z["train__lr"][0]), len(mols))]
    for _, adj, feat, _ in mols:
        lines += [str(len(adj)), " ".join(str(int(v)) for v in adj.ravel()), " ".join("%.17g" % v for v in feat.ravel())]
    lines.append(" ".join("%.17g" % t for t in z["train__targets"]))
    inp.write_text("\n".join(lines) + "\n")
    csrc = os.path.join(ROOT, "graphflow_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "graphflow_amd", "host"),
                           "-o", str(exe), str(src), "-L" + csrc, "-lgf_hip", "-Wl,-rpath," + csrc, "-Wl,-rpath,/opt/rocm/lib", "-lm"])
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array(r.stdout.split(), dtype=np.float64).reshape(nIter, 2)
    ref = z["train__losses"]
    assert np.all(np.abs(got[:, 0] - ref[:, 0]) <= TOL * np.maximum(1.0, ref[:, 0]))
    assert np.all(np.abs(got[:, 1] - ref[:, 1]) <= 5 * TOL * np.maximum(1.0, ref[:, 1]))
