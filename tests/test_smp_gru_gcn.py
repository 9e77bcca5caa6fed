"""CPU suite for GRU_GCN_1D and GRU_GCN_2D (gf_smp_config.neighbourhood = 4, 5): tests/gru_gcn_ref.py, the fp64 restatement the GPU suite
leans on, against the real classes' numbers (tests/golden/smp_gru_gcn.npz, written by tests/golden/make_gru_gcn_golden.py), and what the
library answers without a device: parameter counts, refusals, initial weights, and the agreement of the resolver (smp_config.cpp) with
the block enumeration (smp_prep.h) for the two forms."""
import ctypes as C

import numpy as np
import pytest

import gru_gcn_ref as gref
from field_suite import blockwise, load_golden
from util import rel_err

FORMS = {4: "gru_gcn_1d", 5: "gru_gcn_2d"}
WIDTHS = (1, 5, 8, 9, 16, 17, 32, 33, 64)
INVALID, UNSUPPORTED = 1, 4   # gf_status (include/gf_hip.h)


def golden():
    return load_golden("smp_gru_gcn.npz")


def case(gz, tag):
    form, L, H, D, R, V = (int(x) for x in gz[tag + "__cfg"])
    return form, L, H, D, R, gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"], gz[tag + "__params"].astype(np.float64)


def test_golden_holds_the_cases_the_issue_lists():
    gz = golden()
    tags = list(gz["tags"])
    cfgs = np.array([gz[t + "__cfg"] for t in tags])
    for form in (4, 5):
        mine = cfgs[cfgs[:, 0] == form]
        assert len(mine) == 16
        assert set(mine[:, 1]) == {0, 1, 3} and set(mine[:, 4]) == {0, 1, 2, 5} and set(mine[:, 3]) == {0, 2}
        assert {1, 9, 12, 29} <= set(mine[:, 5])
        for name in ("CH4", "NH3", "H2O", "C2H4", "single", "isolated", "disconnected", "cycle6", "star8_far", "syn9", "syn29"):
            assert "n%d_%s" % (form, name) in tags
    assert set(cfgs[:, 2]) == set(WIDTHS)
    for k in gz:   # every input is float32-representable
        if k.endswith(("__feature", "__params")) and k.split("__")[0] in tags:
            assert np.array_equal(gz[k], gz[k].astype(np.float32).astype(gz[k].dtype)), k
    assert sum(1 for t in tags if t + "__activations" in gz) >= 20


@pytest.mark.parametrize("form", [4, 5])
def test_restatement_meets_the_real_classes(form):
    """every golden case at 1e-9: the neighbourhoods, graph_feature, prediction, loss, each of the ten parameter blocks, the recorded h_l[v]"""
    gz = golden()
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        form, L, H, D, R, adj, feat, result, params = case(gz, tag)
        r = gref.run(form, adj, feat, result[2], params, L, H, D, R)
        assert np.array_equal(gref.lists_flat(r["N"], L), gz[tag + "__lists"]), tag
        blocks = gref.blocks(H, feat.shape[1] * (D + 1))
        assert len(blocks) == 10
        e = blockwise(r["grads"], gz[tag + "__grads"], blocks)
        assert rel_err(r["graph_feature"], gz[tag + "__graph_feature"]) <= 1e-9, tag
        assert rel_err([r["predict"], r["loss"]], result[:2]) <= 1e-9, tag
        assert e[0] <= 1e-9, (tag, e)
        assert np.abs(gz[tag + "__grads"]).max() > 0
        if tag + "__activations" in gz:
            assert rel_err(gref.activations(r), gz[tag + "__activations"]) <= 1e-9, tag


def test_neighbourhoods_read_max_radius_in_both_forms():
    gz = golden()
    for form in (4, 5):
        star = gz["n%d_star8_far__adj" % form]
        assert gref.hop_distances(star).max() == 2 and int(gz["n%d_star8_far__cfg" % form][4]) == 5   # a radius beyond the diameter
        N = gref.neighbourhoods(gz["n%d_star8_r0__adj" % form], 3, 0)
        assert all(N[l][v] == [v] for l in range(4) for v in range(9))   # radius 0: one member, at every level
        N = gref.neighbourhoods(gz["n%d_disconnected__adj" % form], 3, 5)
        assert N[3][0] == [0, 1, 2] and N[3][4] == [3, 4, 5]   # no radius joins the two components
        N = gref.neighbourhoods(gz["n%d_isolated__adj" % form], 3, 2)
        assert N[3][3] == [3]


def test_pair_aggregate_loops_equal_closed_form():
    gz = golden()
    form, L, H, D, R, adj, feat, result, params = case(gz, "n5_CH4")
    a = gref.run(form, adj, feat, result[2], params, L, H, D, R, aggregate="loops")
    b = gref.run(form, adj, feat, result[2], params, L, H, D, R, aggregate="closed")
    assert rel_err(a["grads"], b["grads"]) <= 1e-12 and rel_err(a["graph_feature"], b["graph_feature"]) <= 1e-12
    form, L, H, D, R, adj, feat, result, params = case(gz, "n5_star8_r0")
    r = gref.run(form, adj, feat, result[2], params, L, H, D, R, aggregate="loops")
    assert all(not n.any() for n in r["n"][1:])   # a one-member neighbourhood gives n = 0 exactly


def config(form, L, H, F, D, maxV, R=1, **over):
    from graphflow_amd.smp import SMPGatedNeighbourhood
    cfg = SMPGatedNeighbourhood.config(FORMS[form], L, H, F, D, maxV, R)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def refused_configs(form):
    """the configurations gf_smp_create answers GF_ERR_INVALID to, with a piece of the message"""
    needs = b"gf_smp_create: neighbourhood = %d (4: GRU_GCN_1D, 5: GRU_GCN_2D) needs" % form
    bad = [(config(form, 2, 8, 5, 1, 9, **{k: 1}), needs) for k in ("first_order", "steerable_2d", "unrestricted", "physics", "custom_matmul")]
    bad.append((config(form, 2, 8, 5, 1, 9, nContractions=18), needs))
    bad.append((config(form, 2, 8, 5, 1, 9, max_receptive_field=6), needs))
    bad.append((config(form, 2, 8, 5, 1, 9, R=-1), needs))   # (both forms read max_Radius)
    bad.append((config(form, 2, 65, 5, 1, 9), b"at most 64 channels"))
    bad.append((config(form, 2, 128, 5, 1, 9), b"resident in LDS"))
    return bad


def test_parameter_counts(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    for form in (4, 5):
        for L, H, F, D in ((0, 5, 4, 0), (1, 6, 4, 0), (3, 20, 5, 0), (3, 64, 5, 0), (3, 20, 5, 2), (0, 6, 4, 2), (7, 1, 1, 0)):
            cfg = config(form, L, H, F, D, 12, 2)
            assert lib.gf_smp_config_param_count(C.byref(cfg)) == gref.n_params(H, F * (D + 1), L) == H * F * (D + 1) + 8 * H * H + H, (form, L, H)
            assert lib.gf_smp_classifier_config_param_count(C.byref(cfg), 3) == 0
        assert lib.gf_smp_config_param_count(C.byref(config(form, 2, 8, 5, 1, 9, R=0))) > 0
        for bad, _ in refused_configs(form):
            assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
            assert lib.gf_smp_classifier_config_param_count(C.byref(bad), 3) == 0


def test_uniform_init_draws_the_classes_weights(gf):
    """after srand(seed): every block through sgd->params[i], a Vector* -- divisor 10 x the block's own size -- in registration order"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    for form in (4, 5):
        p_ = "train_n%d__" % form
        _, L, H, D, R, maxV, seed, _ = (int(x) for x in gz[p_ + "cfg"])
        cfg = config(form, L, H, 4, D, maxV, R)
        out = np.zeros(gref.n_params(H, 4 * (D + 1)), dtype=np.float32)
        C.CDLL(None).srand(seed)
        assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
        assert np.array_equal(out, gz[p_ + "params0"].astype(np.float32))
        assert np.abs(out).max() > 0
        assert np.abs(gz[p_ + "params0"][4 * (D + 1) * H:][:H * H]).max() <= 0.9 / (H * H) * (1 + 1e-12)   # (W_z: 10 H^2, not 10 H)


@pytest.mark.parametrize("form", [4, 5])
def test_momentum_trajectory_of_the_restatement(form):
    """three BatchLearn steps of the real class: the restatement follows them at 1e-9 (losses) and 1e-12 (weights)"""
    from inputs import toy_molecules
    gz = golden()
    p_ = "train_n%d__" % form
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in gz[p_ + "cfg"])
    mols = [(a, f) for _, a, f, _ in toy_molecules()]
    losses, p = gref.momentum_steps(form, mols, gz[p_ + "targets"], gz[p_ + "params0"], L, H, D, R, nIter, float(gz[p_ + "lr"][0]),
                                    float(gz[p_ + "momentum"][0]))
    assert rel_err(losses, gz[p_ + "losses"]) <= 1e-9
    assert np.abs(p - gz[p_ + "params"]).max() <= 1e-12
    assert (gz[p_ + "losses"][:, 1] <= gz[p_ + "losses"][:, 0]).all()


def test_checkpoint_is_the_parameters_in_registration_order():
    gz = golden()
    text = bytes(gz["checkpoint__text"]).decode().split()
    params = gz[str(gz["checkpoint__tag"]) + "__params"]
    assert text == ["%g" % x for x in params]


# ---- the resolver and the enumeration for the new forms, as tests/test_smp_config_agreement.py does it for the others ----
ACCEPTED = [("gru_gcn_1d", 4, dict(L=2, R=1)), ("gru_gcn_2d", 5, dict(L=2, R=1)), ("gru_gcn_1d_no_levels", 4, dict(L=0, R=1)),
            ("gru_gcn_2d_no_levels", 5, dict(L=0, R=2)), ("gru_gcn_2d_radius_0", 5, dict(L=3, R=0)), ("gru_gcn_1d_64", 4, dict(L=1, R=5, H=64))]


@pytest.mark.parametrize("name,form,kw", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_what_create_accepts_is_counted_as_the_restatement_lists_it(gf, name, form, kw):
    from graphflow_amd import _lib
    lib = _lib.load()
    H = kw.get("H", 4)
    c = config(form, kw["L"], H, 4, 1, 6, kw["R"])
    count = gref.n_params(H, 8)
    assert lib.gf_smp_config_param_count(C.byref(c)) == count
    out = np.full(count + 1, 7.0, dtype=np.float32)
    C.CDLL(None).srand(5)
    assert lib.gf_smp_uniform_init_host(C.byref(c), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
    assert out[count] == 7.0 and 0 < np.abs(out[:count]).max() < 1
    off = 0
    for bname, n in gref.blocks(H, 8):   # every draw is (rand() % 10) / (10 n), n the block's own size
        assert np.abs(out[off:off + n]).max() <= 0.9 / n * (1 + 1e-6), bname
        off += n
    assert lib.gf_smp_classifier_config_param_count(C.byref(c), 3) == 0
    assert lib.gf_smp_classifier_uniform_init_host(C.byref(c), 3, out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID


@pytest.mark.parametrize("form", [4, 5])
def test_what_create_refuses_has_no_host_only_answer(gf, form):
    from graphflow_amd import _lib
    lib = _lib.load()
    out = np.full(1 << 16, 7.0, dtype=np.float32)
    p = out.ctypes.data_as(C.POINTER(C.c_float))
    for bad, _ in refused_configs(form):
        assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
        assert lib.gf_smp_uniform_init_host(C.byref(bad), p) == _lib.GF_ERR_INVALID
        assert lib.gf_smp_classifier_config_param_count(C.byref(bad), 3) == 0
        assert lib.gf_smp_classifier_uniform_init_host(C.byref(bad), 3, p) == _lib.GF_ERR_INVALID
        assert (out == 7.0).all()
