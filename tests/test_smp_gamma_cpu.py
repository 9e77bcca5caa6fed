"""CPU suite for SMP_gamma (GraphFlow/SMP_gamma.h: RisiContraction_4, no receptive-field cap): the fp64 restatement the GPU tests check
against (oracle/smp_oracle.run with nK = 4 and the cap at the molecule's size) and the library's weight initialisation, both pinned to
the real reference class (tests/golden/smp_gamma.npz, generator tests/golden/make_gamma_golden.py)."""
import ctypes as C
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smp_gamma.npz")


@pytest.fixture(scope="module")
def gz():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def gamma_cases(gz):
    for tag in gz["tags"]:
        p = "gamma_" + str(tag)
        yield str(tag), {k[len(p) + 2:]: v for k, v in gz.items() if k.startswith(p + "__")}


def param_count(C_, F, D, L):
    return C_ * F * (D + 1) + L * (4 * C_ * C_ + C_) + C_


def test_fixture_has_the_reference_parameter_count(gz):
    n = 0
    for tag, c in gamma_cases(gz):
        L, C_, D, _, _ = (int(x) for x in c["cfg"])
        assert c["params"].size == c["grads"].size == param_count(C_, c["feature"].shape[1], D, L), tag
        n += 1
    assert n >= 9


def test_oracle_matches_the_real_smp_gamma(gz):
    """smp_oracle.run(nK=4, cap=V) == the real SMP_gamma's prediction, graph feature, loss and every parameter gradient, to 1e-12."""
    from oracle import smp_oracle
    for tag, c in gamma_cases(gz):
        L, C_, D, wl, maxV = (int(x) for x in c["cfg"])
        r = smp_oracle.run(c["adj"], c["feature"], float(c["target"][0]), c["params"].astype(np.float64), L, C_, D, maxV, bool(wl), nK=4)
        def rel(a, b):
            return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)
        assert rel(r["predict"], c["predict"]) <= 1e-12, tag
        assert rel(r["graph_feature"], c["graph_feature"]) <= 1e-12, tag
        assert rel(r["loss"], c["loss"]) <= 1e-12, tag
        assert rel(r["grads"], c["grads"]) <= 1e-12, tag


def test_uniform_init_draws_the_real_smp_gamma_weights(gf, gz):
    """gf_smp_uniform_init_host for a gamma configuration after srand(seed) == the weights SMP_gamma's constructor drew after the same
    srand (fp32 rounding of the reference's doubles)."""
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPConfig
    L, C_, D, maxV, seed, _ = (int(x) for x in gz["train__cfg"])
    from inputs import toy_molecules
    F = toy_molecules()[0][2].shape[1]
    lib = _lib.load()
    cfg = SMPConfig(L, C_, F, D, maxV, 1, 4, 0, 0)
    n = gz["train__params0"].size
    assert n == param_count(C_, F, D, L)
    out = np.zeros(n, dtype=np.float32)
    C.CDLL(None).srand(seed)
    assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert np.array_equal(out, gz["train__params0"].astype(np.float32))


def test_oracle_batchlearn_matches_the_real_smp_gamma(gz):
    """Three SMP_gamma::BatchLearn steps (summed gradients + Adam::Learn) restated with the oracle reproduce the reference's losses
    and parameters."""
    from inputs import toy_molecules
    from oracle import smp_oracle
    L, C_, D, maxV, seed, nIter = (int(x) for x in gz["train__cfg"])
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    tg = gz["train__targets"]
    p = gz["train__params0"].copy()
    m, v, n0 = np.zeros_like(p), np.zeros_like(p), 0

    def total_loss(p):
        return sum(smp_oracle.run(a, f, float(t), p, L, C_, D, maxV, True, want_grads=False, nK=4)["loss"] for (a, f), t in zip(mols, tg))

    for it in range(nIter):
        before = total_loss(p)
        g = sum(smp_oracle.run(a, f, float(t), p, L, C_, D, maxV, True, nK=4)["grads"] for (a, f), t in zip(mols, tg))
        p, m, v, n0 = smp_oracle.adam_learn(p, g, m, v, n0, float(gz["train__lr"][0]), len(mols))
        after = total_loss(p)
        assert abs(before - gz["train__losses"][it, 0]) <= 1e-9 * max(1, before)
        assert abs(after - gz["train__losses"][it, 1]) <= 1e-7 * max(1, after)
    assert np.abs(p - gz["train__params"]).max() <= 1e-9
