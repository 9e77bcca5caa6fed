"""CPU suite for NeuralFingerprint, GCN_1D and GCN_2D (gf_smp_config.neighbourhood = 1, 2, 3): tests/neighbourhood_ref.py, the fp64
restatement the GPU suite leans on, against the real classes' numbers (tests/golden/smp_neighbourhood.npz, written by
tests/golden/make_neighbourhood_golden.py), and what the library answers without a device: parameter counts, refusals, initial weights."""
import ctypes as C

import numpy as np
import pytest

import neighbourhood_ref as nref
from field_suite import blockwise, load_golden
from util import rel_err

FORMS = {1: "fingerprint", 2: "gcn_1d", 3: "gcn_2d"}


def golden():
    return load_golden("smp_neighbourhood.npz")


def case(gz, tag):
    form, L, H, D, R, V = (int(x) for x in gz[tag + "__cfg"])
    return form, L, H, D, R, gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"], gz[tag + "__params"].astype(np.float64)


def test_golden_holds_the_cases_of_every_form():
    gz = golden()
    tags = list(gz["tags"])
    for form in (1, 2, 3):
        mine = [t for t in tags if t.startswith("n%d_" % form)]
        assert len(mine) == (11 if form == 1 else 10)
        cfgs = np.array([gz[t + "__cfg"] for t in mine])
        assert {0, 1, 3} <= set(cfgs[:, 1]) and {5, 6, 20} <= set(cfgs[:, 2])
        assert set(cfgs[:, 3]) == ({0} if form == 1 else {0, 2})
        assert {1, 12} <= set(cfgs[:, 5])
    for k in gz:   # every input is float32-representable
        if k.endswith(("__feature", "__params")) and k.split("__")[0] in tags:
            assert np.array_equal(gz[k], gz[k].astype(np.float32).astype(gz[k].dtype)), k
    assert not np.array_equal(gz["n1_CH4_directed__adj"], gz["n1_CH4_directed__adj"].T)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_restatement_meets_the_real_classes(form):
    """every golden case at 1e-9: the neighbourhoods, final_feature, prediction, loss, every parameter block, CH4's h_l[v]"""
    gz = golden()
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        form, L, H, D, R, adj, feat, result, params = case(gz, tag)
        r = nref.run(form, adj, feat, result[2], params, L, H, D, R)
        assert np.array_equal(nref.lists_flat(r["N"], L), gz[tag + "__lists"]), tag
        e = blockwise(r["grads"], gz[tag + "__grads"], nref.blocks(H, feat.shape[1] * (D + 1), L))
        assert rel_err(r["final_feature"], gz[tag + "__final_feature"]) <= 1e-9, tag
        assert rel_err([r["predict"], r["loss"]], result[:2]) <= 1e-9, tag
        assert e[0] <= 1e-9, (tag, e)
        assert np.abs(gz[tag + "__grads"]).max() > 0
        if tag + "__activations" in gz:
            assert rel_err(nref.activations(r), gz[tag + "__activations"]) <= 1e-9, tag


def test_special_neighbourhoods_are_what_the_issue_says():
    gz = golden()
    r = {f: nref.neighbourhoods(f, gz["n%d_isolated__adj" % f], 1, 1) for f in (1, 3)}
    assert r[1][1][3] == [] and r[3][1][3] == [3]   # the isolated vertex: empty in form 1, itself in form 3
    adj = gz["n1_CH4_directed__adj"]
    N = nref.neighbourhoods(1, adj, 1, 1)
    assert 1 not in N[1][0] and 0 in N[1][1] and 0 not in N[1][0]   # one-sided, and no vertex is its own neighbour
    star = gz["n2_star8_far__adj"]
    assert nref.hop_distances(star).max() == 2 and int(gz["n2_star8_far__cfg"][4]) == 5   # a radius beyond the diameter


def test_pair_aggregate_loops_equal_closed_form():
    rng = np.random.default_rng(3)
    for m, H in ((1, 4), (2, 3), (5, 6), (9, 5)):
        a, g = rng.random((m, H)), rng.standard_normal(H)
        assert rel_err(nref.risi2d_closed(a), nref.risi2d_loops(a)) <= 1e-12
        assert rel_err(nref.risi2d_closed_backward(a, g), nref.risi2d_loops_backward(a, g)) <= 1e-12
    assert not nref.risi2d_loops(rng.random((1, 4))).any()   # a one-vertex neighbourhood gives n = 0
    gz = golden()
    form, L, H, D, R, adj, feat, result, params = case(gz, "n3_CH4")
    a = nref.run(form, adj, feat, result[2], params, L, H, D, R, aggregate="loops")
    b = nref.run(form, adj, feat, result[2], params, L, H, D, R, aggregate="closed")
    assert rel_err(a["grads"], b["grads"]) <= 1e-12 and rel_err(a["final_feature"], b["final_feature"]) <= 1e-12


@pytest.mark.parametrize("form", [1, 2, 3])
def test_full_jacobian_softmax_gradient_misses_the_classes(form):
    """Softmax::backward is diagonal-only: the true Jacobian is off by more than 1e-3 on CH4, the class's rule meets it at 1e-9"""
    gz = golden()
    form, L, H, D, R, adj, feat, result, params = case(gz, "n%d_CH4" % form)
    blocks = nref.blocks(H, feat.shape[1] * (D + 1), L)
    full = nref.run(form, adj, feat, result[2], params, L, H, D, R, softmax_grad="full")
    diag = nref.run(form, adj, feat, result[2], params, L, H, D, R)
    assert blockwise(full["grads"], gz["n%d_CH4__grads" % form], blocks)[0] > 1e-3
    assert blockwise(diag["grads"], gz["n%d_CH4__grads" % form], blocks)[0] <= 1e-9


def config(form, L, H, F, D, maxV, R=1, **over):
    from graphflow_amd.smp import SMPNeighbourhood
    cfg = SMPNeighbourhood.config(FORMS[form], L, H, F, D, maxV, R)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def refused_configs(form):
    """the configurations gf_smp_create answers GF_ERR_INVALID to"""
    D = 0 if form == 1 else 1
    bad = [config(form, 2, 8, 5, D, 9, **{k: 1}) for k in ("first_order", "steerable_2d", "unrestricted", "physics", "custom_matmul")]
    bad.append(config(form, 2, 8, 5, D, 9, nContractions=18))
    bad.append(config(form, 2, 8, 5, D, 9, max_receptive_field=6))
    bad.append(config(form, 2, 129, 5, D, 9))
    bad.append(config(form, 2, 128, 186, 0, 9))   # (W1_l and W2_l beyond the 160 KiB of LDS)
    if form == 1:
        bad.append(config(1, 2, 8, 5, 1, 9))
    if form == 2:
        bad.append(config(2, 2, 8, 5, 1, 9, R=-1))
    return bad


def test_parameter_counts(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    for form in (1, 2, 3):
        for L, H, F, D in ((0, 5, 4, 0), (1, 6, 4, 0), (3, 20, 5, 0), (3, 128, 5, 0)) + (() if form == 1 else ((3, 20, 5, 2), (0, 6, 4, 2))):
            cfg = config(form, L, H, F, D, 12, 2)
            assert lib.gf_smp_config_param_count(C.byref(cfg)) == nref.n_params(H, F * (D + 1), L), (form, L, H, F, D)
            assert lib.gf_smp_classifier_config_param_count(C.byref(cfg), 3) == 0
        assert lib.gf_smp_config_param_count(C.byref(config(form, 2, 128, 185, 0, 9))) == nref.n_params(128, 185, 2)
        for bad in refused_configs(form):
            assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
    assert lib.gf_smp_config_param_count(C.byref(config(3, 2, 8, 5, 1, 9, R=-1))) > 0   # (GCN_2D never reads max_Radius)


def test_uniform_init_draws_the_classes_weights(gf):
    """after srand(seed): W1_l, W2_l by uniform_init(Matrix*) (10 x nRows), W by uniform_init(Vector*) (10 x size), registration order"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    for form in (1, 2, 3):
        p_ = "train_n%d__" % form
        _, L, H, D, R, maxV, seed, _ = (int(x) for x in gz[p_ + "cfg"])
        cfg = config(form, L, H, 4, D, maxV, R)
        out = np.zeros(nref.n_params(H, 4 * (D + 1), L), dtype=np.float32)
        C.CDLL(None).srand(seed)
        assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
        assert np.array_equal(out, gz[p_ + "params0"].astype(np.float32))
        assert np.abs(out).max() > 0


@pytest.mark.parametrize("form", [1, 2, 3])
def test_momentum_trajectory_of_the_restatement(form):
    """three BatchLearn steps of the real class: the restatement follows them at 1e-9 (losses) and 1e-12 (weights)"""
    from inputs import toy_molecules
    gz = golden()
    p_ = "train_n%d__" % form
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in gz[p_ + "cfg"])
    mols = [(a, f) for _, a, f, _ in toy_molecules()]
    losses, p = nref.momentum_steps(form, mols, gz[p_ + "targets"], gz[p_ + "params0"], L, H, D, R, nIter, float(gz[p_ + "lr"][0]),
                                    float(gz[p_ + "momentum"][0]))
    assert rel_err(losses, gz[p_ + "losses"]) <= 1e-9
    assert np.abs(p - gz[p_ + "params"]).max() <= 1e-12


def test_checkpoint_is_the_parameters_in_registration_order():
    gz = golden()
    text = bytes(gz["checkpoint__text"]).decode().split()
    params = gz[str(gz["checkpoint__tag"]) + "__params"]
    assert text == ["%g" % x for x in params]
