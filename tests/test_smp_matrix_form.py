"""CPU suite for LCNN and GCN_MW (gf_smp_config.matrix_form = 1, 2): tests/matrix_form_ref.py, the fp64 restatement the GPU suite leans on,
against the real classes' numbers (tests/golden/smp_matrix_form.npz, written by tests/golden/make_matrix_form_golden.py), block by block;
and what the library answers without a device -- order, sequence and A-hat through gf_smp_matrix_form_molecule_host, parameter counts,
the classes' initial weights bit for bit, and every refusal that needs no handle with a piece of its message."""
import ctypes as C

import numpy as np
import pytest

import matrix_form_ref as mref
from field_suite import blockwise, load_golden
from util import rel_err

INVALID, UNSUPPORTED = 1, 4   # gf_status (include/gf_hip.h)
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)


def golden():
    return load_golden("smp_matrix_form.npz")


def tags(kind=None):
    return [str(t) for t in golden()["tags"] if kind is None or str(t).startswith(kind + "_")]


def kind_of(tag):
    return "lcnn" if tag.startswith("lcnn_") else "gcn_mw"


def case(tag):
    gz = golden()
    return (kind_of(tag), tuple(int(x) for x in gz[tag + "__cfg"]), gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"],
            gz[tag + "__params"].astype(np.float64))


def config(kind, cfg, F, maxV=None, **over):
    from graphflow_amd.smp import GCNMW, LCNN
    if kind == "lcnn":
        V, k, D, C1, C2, nD = cfg
        c = LCNN.config(V, F, k, D, C1, C2, nD)
    else:
        L, H, D = cfg
        c = GCNMW.config(L, maxV, F, H, D)
    assert c.matrix_form == (1 if kind == "lcnn" else 2)
    for k_, v in over.items():
        setattr(c, k_, v)
    return c


def structure(kind, r):
    if kind == "lcnn":
        return np.concatenate([r["order"], r["seq"].ravel()]).astype(np.float64)
    return r["norm_adj"].ravel()


def activations(kind, r):
    if kind == "lcnn":
        return np.concatenate([r["a1"].ravel(), r["c2"].ravel()])
    return np.concatenate([h.ravel() for h in r["activations"]])


# ---- the restatement against the real classes ----
@pytest.mark.parametrize("tag", tags())
def test_restatement_meets_the_real_class(tag):
    gz = golden()
    kind, cfg, adj, feat, result, params = case(tag)
    assert np.array_equal(feat, feat.astype(np.float32).astype(np.float64))
    r = mref.run(kind, cfg, adj, feat, result[2], params)
    assert rel_err(structure(kind, r), gz[tag + "__structure"]) <= (0 if kind == "lcnn" else 1e-15)
    assert rel_err(r["graph_feature"], gz[tag + "__graph_feature"]) <= 1e-9
    assert rel_err([r["predict"], r["loss"]], result[:2]) <= 1e-9
    e = blockwise(r["grads"], gz[tag + "__grads"], mref.blocks(kind, cfg, feat.shape[1]))
    assert e[0] <= 1e-9, e
    assert np.abs(gz[tag + "__grads"]).max() > 0
    if tag + "__activations" in gz:
        assert rel_err(activations(kind, r), gz[tag + "__activations"]) <= 1e-9
    assert r["margin"] >= 1e-3   # (no pre-activation near the kink of LeakyReLU)


def test_fixtures_cover_the_shapes_the_level_can_go_wrong_at():
    gz = golden()
    lc = [case(t) for t in tags("lcnn")]
    assert any(len(a) == 1 for _, _, a, *_ in lc) and any(c[1] > c[0] for _, c, *_ in lc)   # one vertex; k > V
    assert any((c[1] * f.shape[1] * (c[2] + 1)) % 32 and (c[1] * c[3]) % 32 for _, c, _, f, *_ in lc)   # k F', k C1 off the K tile
    assert {8, 10, 64, 80} <= {c[3] for _, c, *_ in lc} | {c[4] for _, c, *_ in lc}
    padded = [t for t in tags("lcnn") if (gz[t + "__structure"][int(gz[t + "__cfg"][0]):] == len(gz[t + "__adj"])).any()]
    assert "lcnn_disconnected" in padded and len(gz["lcnn_disconnected__adj"]) < int(gz["lcnn_disconnected__cfg"][0])
    assert len(gz["lcnn_C2H4__adj"]) == int(gz["lcnn_C2H4__cfg"][0]) and "lcnn_C2H4" not in padded   # full size, no pads
    gc = [case(t) for t in tags("gcn_mw")]
    assert {0, 1, 3} <= {c[0] for _, c, *_ in gc} and {8, 10, 64, 80} <= {c[1] for _, c, *_ in gc}
    assert any(len(a) == 1 for _, _, a, *_ in gc) and any(not np.array_equal(a, a.T) for _, _, a, *_ in gc)


@pytest.mark.parametrize("kind", ["lcnn", "gcn_mw"])
def test_restatement_follows_the_classes_batchlearn(kind):
    gz = golden()
    from inputs import f32exact, toy_molecules
    p_ = "train_%s__" % kind
    cfg = tuple(int(x) for x in gz[p_ + "cfg"])
    mols = [(a, f32exact(f)) for _, a, f, _ in toy_molecules()]
    losses, p, small = mref.momentum_steps(kind, cfg, mols, gz[p_ + "targets"], gz[p_ + "params0"], int(gz[p_ + "seed"][1]),
                                           float(gz[p_ + "lr"][0]), float(gz[p_ + "momentum"][0]))
    assert rel_err(losses, gz[p_ + "losses"]) <= 1e-9
    assert np.abs(p - gz[p_ + "params"]).max() <= 1e-12
    assert (gz[p_ + "losses"][:, 1] <= gz[p_ + "losses"][:, 0]).all() and small >= 1e-3


def test_checkpoint_is_the_parameters_in_registration_order():
    gz = golden()
    text = bytes(gz["checkpoint__text"]).decode().split()
    assert text == ["%g" % x for x in gz[str(gz["checkpoint__tag"]) + "__params"]]


# ---- the library without a device ----
@pytest.mark.parametrize("tag", tags())
def test_host_preparation_is_the_classes(gf, tag):
    """order and sequence (LCNN) or A-hat (GCN_MW) of every fixture, the padded and disconnected ones included"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    kind, cfg, adj, feat, *_ = case(tag)
    V = len(adj)
    c = config(kind, cfg, feat.shape[1], maxV=V + 2)
    a, f = np.ascontiguousarray(adj, dtype=np.int32), np.ascontiguousarray(feat, dtype=np.float64)
    if kind == "lcnn":
        order, seq = np.full(cfg[0], -7, dtype=np.int32), np.full(cfg[0] * cfg[1], -7, dtype=np.int32)
        assert lib.gf_smp_matrix_form_molecule_host(C.byref(c), V, a.ctypes.data_as(IP), f.ctypes.data_as(DP), order.ctypes.data_as(IP),
                                                    seq.ctypes.data_as(IP), None) == _lib.GF_OK
        assert np.array_equal(np.concatenate([order, seq]), gz[tag + "__structure"].astype(np.int32))
    else:
        ah = np.full(V * V, np.nan)
        assert lib.gf_smp_matrix_form_molecule_host(C.byref(c), V, a.ctypes.data_as(IP), f.ctypes.data_as(DP), None, None,
                                                    ah.ctypes.data_as(DP)) == _lib.GF_OK
        assert np.array_equal(ah, gz[tag + "__structure"])


def test_full_size_molecule_with_pad_entries_is_refused(gf):
    """molV == V and a vertex that reaches fewer than k vertices: the class reads row V of a V-row matrix"""
    from graphflow_amd import _lib
    from make_gru_gcn_golden import disconnected_molecule
    lib = _lib.load()
    adj, feat, _ = disconnected_molecule()
    a, f = np.ascontiguousarray(adj, dtype=np.int32), np.ascontiguousarray(feat, dtype=np.float64)
    order, seq = np.zeros(8, dtype=np.int32), np.zeros(8 * 5, dtype=np.int32)
    args = (6, a.ctypes.data_as(IP), f.ctypes.data_as(DP), order.ctypes.data_as(IP), seq.ctypes.data_as(IP), None)
    assert lib.gf_smp_matrix_form_molecule_host(C.byref(config("lcnn", (6, 5, 0, 4, 4, 3), 4)), *args) == INVALID
    assert b"past its matrix" in lib.gf_last_error(None)
    assert lib.gf_smp_matrix_form_molecule_host(C.byref(config("lcnn", (6, 3, 0, 4, 4, 3), 4)), *args) == _lib.GF_OK   # (k = 3: every fragment holds three)
    assert lib.gf_smp_matrix_form_molecule_host(C.byref(config("lcnn", (7, 5, 0, 4, 4, 3), 4)), *args) == _lib.GF_OK   # (below full size: a valid row)
    assert (seq[:35] == 6).any()
    assert lib.gf_smp_matrix_form_molecule_host(C.byref(config("lcnn", (5, 5, 0, 4, 4, 3), 4)), *args) == INVALID      # (more vertices than the model)
    assert b"max_nVertices = 5" in lib.gf_last_error(None)


def refused_configs():
    """the configurations gf_smp_create answers GF_ERR_INVALID to, with a piece of the message"""
    needs = b"(1: LCNN, 2: GCN_MW) needs"
    bad = []
    for kind, cfg in (("lcnn", (6, 5, 3, 16, 8, 128)), ("gcn_mw", (1, 20, 1))):
        for k in ("first_order", "steerable_2d", "unrestricted", "neighbourhood", "physics", "custom_matmul"):
            bad.append((config(kind, cfg, 4, 6, **{k: 1}), needs))
        bad.append((config(kind, cfg, 4, 6, nContractions=18), needs))
        bad.append((config(kind, cfg, 4, 6, max_receptive_field=5), needs))
        bad.append((config(kind, cfg, 4, 6, nLevels=3 if kind == "lcnn" else 65), needs))
        bad.append((config(kind, cfg, 4, 6, nChanels=0), needs))
        bad.append((config(kind, cfg, 4, 6, nChanels=65537), b"at most 65536"))
    bad.append((config("lcnn", (6, 0, 3, 16, 8, 128), 4), needs))
    bad.append((config("lcnn", (6, 5, 3, 16, 0, 128), 4), needs))
    bad.append((config("lcnn", (6, 5, 3, 16, 8, 0), 4), needs))
    bad.append((config("lcnn", (4096, 5, 3, 16, 17, 128), 4), b"indexes an operand row"))
    bad.append((config("lcnn", (4096, 5, 3, 16, 16, 65536), 4), b"must fit an int"))
    bad.append((config("gcn_mw", (1, 20, 1), 4, 6, matrix_form=3), needs))
    return bad


def test_parameter_counts_and_host_only_refusals(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    for L, H, F, D in ((0, 5, 4, 0), (1, 20, 4, 1), (3, 64, 5, 0), (3, 80, 5, 2), (64, 1, 1, 0)):
        c = config("gcn_mw", (L, H, D), F, 12)
        FD = F * (D + 1)
        assert lib.gf_smp_config_param_count(C.byref(c)) == mref.n_params_gcn(H, FD, L) == FD * H + L * H * H + H
        assert lib.gf_smp_classifier_config_param_count(C.byref(c), 3) == 0
    for V, k, D, C1, C2, nD, F in ((6, 5, 3, 16, 8, 128, 4), (4, 6, 2, 5, 10, 9, 4), (10, 3, 0, 7, 64, 6, 5)):
        c = config("lcnn", (V, k, D, C1, C2, nD), F)
        FD = F * (D + 1)
        expect = k * FD * C1 + C1 + k * C1 * C2 + C2 + nD * V * C2 + nD
        assert lib.gf_smp_config_param_count(C.byref(c)) == mref.n_params_lcnn(V, FD, k, C1, C2, nD) == expect
        assert lib.gf_smp_classifier_config_param_count(C.byref(c), 3) == 0
    out = np.full(1 << 16, 7.0, dtype=np.float32)
    p = out.ctypes.data_as(C.POINTER(C.c_float))
    one = np.zeros(1, dtype=np.int32)
    x = np.ones(4)
    for bad, text in refused_configs():
        assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
        assert lib.gf_smp_uniform_init_host(C.byref(bad), p) == _lib.GF_ERR_INVALID
        assert lib.gf_smp_matrix_form_molecule_host(C.byref(bad), 1, one.ctypes.data_as(IP), x.ctypes.data_as(DP), one.ctypes.data_as(IP),
                                                    one.ctypes.data_as(IP), x.ctypes.data_as(DP)) == INVALID
        assert text in lib.gf_last_error(None), (text, lib.gf_last_error(None))
    assert out.max() == out.min() == 7.0
    # the two host-only entry points that are not theirs
    c = config("gcn_mw", (1, 20, 1), 4, 6)
    phi = np.zeros(4096, dtype=np.int32)
    assert lib.gf_smp_prepare_molecule_host(C.byref(c), 1, one.ctypes.data_as(IP), x.ctypes.data_as(DP), phi.ctypes.data_as(IP), None) == INVALID
    assert b"has no receptive fields" in lib.gf_last_error(None)
    plain = config("gcn_mw", (1, 20, 1), 4, 6, matrix_form=0, nContractions=18)
    assert lib.gf_smp_matrix_form_molecule_host(C.byref(plain), 1, one.ctypes.data_as(IP), x.ctypes.data_as(DP), None, None,
                                                x.ctypes.data_as(DP)) == INVALID
    assert b"matrix_form = 0" in lib.gf_last_error(None)
    assert lib.gf_smp_matrix_form_molecule_host(C.byref(c), 1, one.ctypes.data_as(IP), x.ctypes.data_as(DP), None, None, None) == INVALID
    assert b"missing output" in lib.gf_last_error(None)


@pytest.mark.parametrize("kind", ["lcnn", "gcn_mw"])
def test_uniform_init_draws_the_classes_weights(gf, kind):
    """after srand(seed): GCN_MW draws every W_l as a Matrix (divisor 10 x rows) and W as a Vector, LCNN every block as a Vector (10 x its
    own size), in registration order -- the recorded weights of the real classes bit for bit"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    p_ = "train_%s__" % kind
    cfg = tuple(int(x) for x in gz[p_ + "cfg"])
    seed, _, maxV = (int(x) for x in gz[p_ + "seed"])
    c = config(kind, cfg, 4, maxV)
    out = np.zeros(gz[p_ + "params0"].size + 1, dtype=np.float32)
    assert lib.gf_smp_config_param_count(C.byref(c)) == out.size - 1
    C.CDLL(None).srand(seed)
    assert lib.gf_smp_uniform_init_host(C.byref(c), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
    assert np.array_equal(out[:-1], gz[p_ + "params0"].astype(np.float32)) and out[-1] == 0
    off = 0
    for name, n in mref.blocks(kind, cfg, 4):   # every draw is (rand() % 10) / (10 d)
        d = n if kind == "lcnn" or name == "W" else n // cfg[1]   # (a Matrix [rows][H]: its rows)
        assert 0 < np.abs(out[off:off + n]).max() <= 0.9 / d * (1 + 1e-6), name
        off += n


def test_python_classes_describe_themselves():
    from graphflow_amd import GCNMW, LCNN
    assert "GCN_MW" in GCNMW.__doc__ and "PATCHY-SAN" in LCNN.__doc__
    c = LCNN.config(6, 4, 5, 3, 16, 8, 128)
    assert (c.nLevels, c.nChanels, c.nNeighbors, c.nChanels2, c.nDense, c.max_nVertices, c.max_receptive_field) == (2, 16, 5, 8, 128, 6, 6)
    c = GCNMW.config(3, 29, 5, 64, 2)
    assert (c.nLevels, c.nChanels, c.nFeatures, c.nDepth, c.max_nVertices, c.matrix_form, c.nNeighbors) == (3, 64, 5, 2, 29, 2, 0)
