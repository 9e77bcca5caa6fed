"""CPU suite for GCN_1D_Distance, GCN_2D_Distance and GCN_3D_Distance (gf_smp_config.distance_channel = 1 with neighbourhood = 2, 3, 6):
tests/distance_ref.py, the fp64 restatement the GPU suites lean on, against the real classes' numbers (tests/golden/smp_distance.npz,
written by tests/golden/make_distance_golden.py), and what the library answers without a device: parameter counts, refusals, initial
weights, and the agreement of gfsmp::resolve_config with the restatement's block list."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dref
from field_suite import blockwise, load_golden
from util import rel_err

FORMS = {2: "gcn_1d_distance", 3: "gcn_2d_distance", 6: "gcn_3d_distance"}
CASES = ("CH4", "single", "isolated", "cycle6", "syn12_L0", "syn12", "NH3_padded", "CH4_asymmetric", "H2O_tied_negative")
INVALID, UNSUPPORTED = 1, 4   # gf_status (include/gf_hip.h)


def golden():
    return load_golden("smp_distance.npz")


def case(gz, tag):
    """(form, L, H, D, R, M, (adj, feature, distance), result, params)"""
    form, L, H, D, R, V, M = (int(x) for x in gz[tag + "__cfg"])
    mol = (gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__distance"])
    assert len(mol[0]) == V
    return form, L, H, D, R, M, mol, gz[tag + "__result"], gz[tag + "__params"].astype(np.float64)


def test_golden_holds_the_cases_of_every_class():
    gz = golden()
    tags = list(gz["tags"])
    for form in FORMS:
        assert [t for t in tags if t.startswith("n%d_" % form)] == ["n%d_%s" % (form, c) for c in CASES]
        cfgs = np.array([gz["n%d_%s__cfg" % (form, c)] for c in CASES])
        assert {0, 3} <= set(cfgs[:, 1]) and {1, 12} <= set(cfgs[:, 5])
        assert (cfgs[:, 5] < cfgs[:, 6]).any() and (cfgs[:, 5] == cfgs[:, 6]).any()   # V < M and V == M
        d = gz["n%d_CH4_asymmetric__distance" % form]
        assert not np.array_equal(d, d.T)
        t = gz["n%d_H2O_tied_negative__distance" % form]
        assert (t < 0).any() and np.unique(t).size < t.size
        assert "n%d_CH4__activations" % form in gz
    for k in gz:   # every input is float32-representable, the distances are real-valued
        if k.endswith(("__feature", "__params", "__distance")) and k.split("__")[0] in tags:
            assert np.array_equal(gz[k], gz[k].astype(np.float32).astype(gz[k].dtype)), k
    assert any(np.abs(gz[t + "__distance"] * 16 % 16).max() > 0 for t in tags)


@pytest.mark.parametrize("form", list(FORMS))
def test_restatement_meets_the_real_classes(form):
    """every golden case at 1e-9: the neighbourhoods, the sorted rows (exactly), final feature, prediction, loss, every parameter block in
    registration order, CH4's h_l[v] of both channels"""
    gz = golden()
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        _, L, H, D, R, M, (adj, feat, dist), result, params = case(gz, tag)
        r = dref.run(form, adj, feat, dist, result[2], params, L, H, D, M, R)
        assert np.array_equal(dref.lists_flat(r["N"], L), gz[tag + "__lists"]), tag
        assert np.array_equal(r["x_d"], gz[tag + "__x_d"]), tag
        e = blockwise(r["grads"], gz[tag + "__grads"], dref.blocks(H, feat.shape[1] * (D + 1), M, L))
        assert rel_err(r["final_feature"], gz[tag + "__final_feature"]) <= 1e-9, tag
        assert rel_err([r["predict"], r["loss"]], result[:2]) <= 1e-9, tag
        assert e[0] <= 1e-9, (tag, e)
        assert np.abs(gz[tag + "__grads"]).max() > 0
        if tag + "__activations" in gz:
            assert rel_err(dref.activations(r), gz[tag + "__activations"]) <= 1e-9, tag


def test_row_builder_reads_columns():
    """x_d[v] is COLUMN v of the matrix (distance[u][v]), zeros up to M, sorted ascending -- written out in plain numpy.  The asymmetric
    case tells a column from a row; negative entries come before the zeros of the padding and of the diagonal."""
    gz = golden()
    for tag in gz["tags"]:
        d, M = gz[tag + "__distance"], int(gz[tag + "__cfg"][6])
        V = len(d)
        rows = np.array([sorted([d[u][v] for u in range(V)] + [0.0] * (M - V)) for v in range(V)])
        assert np.array_equal(rows, gz[tag + "__x_d"]), tag
        assert np.array_equal(dref.sorted_rows(d, M), rows), tag
    d = gz["n2_CH4_asymmetric__distance"]
    by_rows = np.sort(np.concatenate([d, np.zeros((len(d), 1))], axis=1), axis=1)
    assert not np.array_equal(by_rows, gz["n2_CH4_asymmetric__x_d"])
    t = gz["n2_H2O_tied_negative__x_d"]
    assert (t[:, 0] < 0).any() and (np.diff(t, axis=1) >= 0).all() and (t == 0).sum() >= 2 * len(t)


def config(form, L, H, F, D, maxV, R=1, **over):
    from graphflow_amd.smp import SMPDistance
    cfg = SMPDistance.config(FORMS[form], L, H, F, D, maxV, R)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def refused_configs(form):
    """the configurations gf_smp_create answers GF_ERR_INVALID to"""
    bad = [config(form, 2, 8, 5, 1, 9, **{k: 1}) for k in ("first_order", "steerable_2d", "unrestricted", "physics", "custom_matmul", "matrix_form")]
    bad.append(config(form, 2, 8, 5, 1, 9, nContractions=18))
    bad.append(config(form, 2, 8, 5, 1, 9, max_receptive_field=6))
    bad.append(config(form, 2, 8, 5, 1, 9, R=-1))          # max_Radius >= 0 in all three, the 2D class included
    bad.append(config(form, 2, 8, 5, 1, 9, distance_channel=2))
    bad.append(config(form, 2, 129, 5, 1, 9))
    bad.append(config(form, 2, 64, 600, 0, 9))             # F' beyond the 160 KiB of LDS at 64 channels
    bad.append(config(form, 2, 64, 5, 0, 600))             # ... and the other operand width, M
    bad += [config(form, 2, 8, 5, 1, 9, neighbourhood=n) for n in (0, 1, 4, 5, 7)]   # any other form
    if form == 6:
        bad.append(config(6, 2, 65, 5, 1, 9))
        bad.append(config(6, 2, 64, 5, 0, 475))            # form 6's max_nVertices bound (474 at 64 channels)
    return bad


def test_parameter_counts(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    for form in FORMS:
        for L, H, F, D, M in ((0, 5, 4, 0, 3), (1, 6, 4, 0, 29), (3, 20, 5, 2, 12), (3, 64, 5, 0, 64), (2, 33, 4, 1, 185)):
            cfg = config(form, L, H, F, D, M, 2)
            assert lib.gf_smp_config_param_count(C.byref(cfg)) == dref.n_params(H, F * (D + 1), M, L), (form, L, H, F, D, M)
            assert lib.gf_smp_classifier_config_param_count(C.byref(cfg), 3) == 0
        for bad in refused_configs(form):
            assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
    assert lib.gf_smp_config_param_count(C.byref(config(2, 2, 128, 5, 0, 185))) == dref.n_params(128, 5, 185, 2)   # the widest M at 128 channels
    assert lib.gf_smp_config_param_count(C.byref(config(2, 2, 128, 5, 0, 186))) == 0


def test_zero_tail_is_the_plain_form(gf):
    """distance_channel = 0 changes nothing: the plain forms count their own parameters"""
    import neighbourhood_ref as nref
    from graphflow_amd import _lib
    lib = _lib.load()
    for form in FORMS:
        cfg = config(form, 2, 8, 5, 1, 9, distance_channel=0)
        assert lib.gf_smp_config_param_count(C.byref(cfg)) == nref.n_params(8, 10, 2)


def test_uniform_init_draws_the_classes_weights(gf):
    """after srand(seed): every matrix by uniform_init(Matrix*) (10 x nRows = 10 H), W by uniform_init(Vector*) (10 x 2 H), in
    registration order -- bit for bit the weights the classes drew"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    for form in FORMS:
        p_ = "train_n%d__" % form
        _, L, H, D, R, maxV, seed, _ = (int(x) for x in gz[p_ + "cfg"])
        cfg = config(form, L, H, 4, D, maxV, R)
        out = np.zeros(dref.n_params(H, 4 * (D + 1), maxV, L), dtype=np.float32)
        C.CDLL(None).srand(seed)
        assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
        assert np.array_equal(out, gz[p_ + "params0"].astype(np.float32))
        assert np.abs(out).max() > 0


def train_molecules(gz):
    from inputs import toy_molecules
    return [(a, f, gz["train__distance_%d" % i]) for i, (_, a, f, _) in enumerate(toy_molecules())]


@pytest.mark.parametrize("form", list(FORMS))
def test_momentum_trajectory_of_the_restatement(form):
    """three BatchLearn steps of the real class: the restatement follows them at 1e-9 (losses) and 1e-12 (weights)"""
    gz = golden()
    p_ = "train_n%d__" % form
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in gz[p_ + "cfg"])
    losses, p, _ = dref.momentum_steps(form, train_molecules(gz), gz[p_ + "targets"], gz[p_ + "params0"], L, H, D, maxV, R, nIter,
                                       float(gz[p_ + "lr"][0]), float(gz[p_ + "momentum"][0]))
    assert rel_err(losses, gz[p_ + "losses"]) <= 1e-9
    assert np.abs(p - gz[p_ + "params"]).max() <= 1e-12


def test_checkpoint_is_written_channel_by_channel():
    """save_model writes the vertex channel's blocks by level, then the distance channel's, then W: NOT the registration order"""
    gz = golden()
    tag = str(gz["checkpoint__tag"])
    _, L, H, D, R, M, mol, _, params = case(gz, tag)
    FD = mol[1].shape[1] * (D + 1)
    text = bytes(gz["checkpoint__text"]).decode().split()
    assert text == ["%g" % x for x in dref.to_checkpoint(params, H, FD, M, L)]
    assert text != ["%g" % x for x in params]
    assert np.array_equal(dref.from_checkpoint(dref.to_checkpoint(params, H, FD, M, L), H, FD, M, L), params)


# ---- the resolver and the restatement's block list, in the manner of test_smp_config_agreement.py ----
GRID = [(form, L, H, F, D, M) for form in FORMS for (L, H, F, D, M) in ((2, 4, 4, 1, 6), (0, 4, 4, 1, 6), (3, 7, 3, 0, 5))]


@pytest.mark.parametrize("form,L,H,F,D,M", GRID)
def test_resolver_and_block_list_agree(gf, form, L, H, F, D, M):
    """gf_smp_config_param_count is the block list's total, and gf_smp_uniform_init_host draws block by block with the divisor the list
    implies: |w| < 1 / H inside a matrix, < 1 / (2 H) inside W, and nothing beyond the last block"""
    from graphflow_amd import _lib
    lib = _lib.load()
    cfg = config(form, L, H, F, D, M, 1)
    blocks = dref.blocks(H, F * (D + 1), M, L)
    count = sum(n for _, n in blocks)
    assert lib.gf_smp_config_param_count(C.byref(cfg)) == count
    out = np.full(count + 1, 7.0, dtype=np.float32)
    C.CDLL(None).srand(5)
    assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
    assert out[count] == 7.0
    off = 0
    for name, n in blocks:
        div = 10.0 * (2 * H if name == "W" else H)
        steps = np.abs(out[off:off + n].astype(np.float64)) * div
        assert np.abs(steps - np.round(steps)).max() < 1e-4 and steps.max() <= 9.0 + 1e-4, name   # (rand() % 10) / (10 x divisor)
        off += n
    assert np.abs(out[:count]).max() > 0


def test_refusals_have_no_host_only_answer(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    out = np.full(1 << 16, 7.0, dtype=np.float32)
    for form in FORMS:
        for bad in refused_configs(form):
            assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
            assert lib.gf_smp_uniform_init_host(C.byref(bad), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID
            assert (out == 7.0).all()
