"""CPU suite for SMP_2D_ver5 (gf_smp_config.steerable_2d = 5): the parameter layout, the initial weights, the receptive fields of the host
preparation and the fp64 restatement tests/smp2d_ver5_ref.py, all against the real class's numbers in tests/golden/smp_2d_ver5.npz
(tests/golden/make_smp2d_ver5_golden.py).  Host code only: no device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import smp2d_ver5_ops_ref as ops
import smp2d_ver5_ref
from make_smp2d_ver5_golden import smp2d_ver5_blocks
from smp2d_ref import ALPHA
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_REF = 1e-9   # fp64 restatement against the fp64 reference: summation order only


@pytest.fixture(scope="module")
def lib():
    from graphflow_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gz():
    with np.load(os.path.join(HERE, "golden", "smp_2d_ver5.npz")) as z:
        return {k: z[k] for k in z.files}


def cfg_of(L, Cn, F, D, wl, maxV):
    from graphflow_amd.smp import SMP2D
    return SMP2D.config("ver5", maxV, L, Cn, F, D, bool(wl))


def blockwise(x, ref, blocks):
    off, worst = 0, (0.0, "")
    for name, n in blocks:
        worst = max(worst, (rel_err(x[off:off + n], ref[off:off + n]), name))
        off += n
    assert off == ref.size
    return worst


def ref_of(gz, tag):
    _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
    return smp2d_ver5_ref.run(gz[tag + "__adj"], gz[tag + "__feature"], float(gz[tag + "__target"][0]), gz[tag + "__params"], L, Cn, D, maxV,
                              smp2d_ver5_ref.fields_of(gz[tag + "__phi"]))


def test_parameter_count_is_the_sum_of_the_registration_order_blocks(lib, gz):
    """gf_smp_config_param_count against the length of the real class's gradient vector and the blocks H, (lambda1_s, lambda2_s, b_s) x
    max_nVertices, K_l [C][2C], scalar_l, W; steerable_2d = 3 and 4 stay refused, as do 129 channels and a capped configuration; there is
    no classifier of this form."""
    from graphflow_amd.smp import SMPConfig
    assert len(gz["tags"]) == 18
    for tag in gz["tags"]:
        form, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        assert form == 5
        F = gz[tag + "__feature"].shape[1]
        cfg = cfg_of(L, Cn, F, D, wl, maxV)
        assert cfg.steerable_2d == 5
        n = lib.gf_smp_config_param_count(C.byref(cfg))
        assert n == gz[tag + "__grads"].size, tag
        assert n == sum(sz for _, sz in smp2d_ver5_blocks(Cn, F * (D + 1), L, maxV)), tag
        assert n == smp2d_ver5_ref.param_count(Cn, F * (D + 1), L, maxV), tag
    assert lib.gf_smp_config_param_count(C.byref(SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 0, 12, 5))) == 4 * 8 + 2 * (12 * 12 + 32 + 4) + 4
    assert lib.gf_smp_config_param_count(C.byref(SMPConfig(2, 128, 4, 1, 12, 1, 0, 0, 0, 0, 12, 5))) > 0
    assert lib.gf_smp_config_param_count(C.byref(SMPConfig(2, 129, 4, 1, 12, 1, 0, 0, 0, 0, 12, 5))) == 0   # K1 would not fit in LDS
    for form in (3, 4, 6):
        assert lib.gf_smp_config_param_count(C.byref(SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 0, 12, form))) == 0   # no such forms
    for bad in (SMPConfig(2, 4, 4, 1, 6, 1, 0, 0, 0, 0, 12, 5), SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 0, 6, 5),   # capped
                SMPConfig(2, 4, 4, 1, 12, 1, 18, 0, 0, 0, 12, 5), SMPConfig(2, 4, 4, 1, 12, 1, 0, 1, 0, 0, 12, 5),
                SMPConfig(2, 4, 4, 0, 12, 1, 0, 0, 1, 0, 12, 5), SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 1, 12, 5),
                SMPConfig(2, 4, 4, 1, 5000, 1, 0, 0, 0, 0, 5000, 5)):
        assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
    ok = SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 0, 12, 5)
    assert lib.gf_smp_classifier_config_param_count(C.byref(ok), 5) == 0   # no SMP_2D_ver5_classification
    out = np.zeros(4096, dtype=np.float32)
    assert lib.gf_smp_classifier_uniform_init_host(C.byref(ok), 5, out.ctypes.data_as(C.POINTER(C.c_float))) != 0


def test_uniform_init_reproduces_weights_initialization(lib, gz):
    """gf_smp_uniform_init_host after srand(seed) against the weights the real constructor drew, block by block: every block has its own
    divisor (10 x its size) -- K_l is ONE block of 2 C^2 values (sgd->params holds Vector*), scalar_l one of C behind it."""
    form, L, Cn, D, wl, maxV, _, seed = (int(x) for x in gz["init__cfg"])
    cfg = cfg_of(L, Cn, 4, D, wl, maxV)
    ref = gz["init__params0"]
    out = np.zeros(ref.size, dtype=np.float32)
    C.CDLL(None).srand(seed)
    assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    off = 0
    for name, n in smp2d_ver5_blocks(Cn, 4 * (D + 1), L, maxV):
        assert np.array_equal(out[off:off + n], ref[off:off + n].astype(np.float32)), name
        if name.startswith("K_"):   # the block's own divisor: every value is a multiple of 1 / (10 * 2 C^2)
            assert np.abs(ref[off:off + n] * 10 * n - np.round(ref[off:off + n] * 10 * n)).max() < 1e-9 and np.abs(ref[off:off + n]).max() > 0
        off += n
    assert off == ref.size


def test_receptive_fields_match_the_reference(lib, gz):
    """phi_l(v) of every golden case from gf_smp_prepare_molecule_host; a capped configuration is refused."""
    for tag in gz["tags"]:
        _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        adj = np.ascontiguousarray(gz[tag + "__adj"], dtype=np.int32)
        feat = np.ascontiguousarray(gz[tag + "__feature"], dtype=np.float64)
        cfg = cfg_of(L, Cn, feat.shape[1], D, wl, maxV)
        phi = np.zeros((L + 1, len(adj), maxV + 1), dtype=np.int32)
        st = lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)),
                                              feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None)
        assert st == 0, tag
        assert np.array_equal(phi, gz[tag + "__phi"]), tag
    cfg.max_receptive_field = maxV - 1
    assert lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)),
                                            feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None) != 0


def test_smp2d_ver5_ref_matches_the_real_class(gz):
    """graph feature, prediction, loss and every parameter block of every case at 1e-9; the unused sizes' blocks are zero in both"""
    for tag in gz["tags"]:
        _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        r = ref_of(gz, tag)
        assert rel_err(r["graph_feature"], gz[tag + "__graph_feature"]) <= TOL_REF, tag
        assert rel_err([r["predict"]], gz[tag + "__predict"]) <= TOL_REF, tag
        assert rel_err([r["loss"]], gz[tag + "__loss"]) <= TOL_REF, tag
        blocks = smp2d_ver5_blocks(Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV)
        worst = blockwise(r["grads"], gz[tag + "__grads"], blocks)
        assert worst[0] <= TOL_REF, (tag, worst)
        used = {int(s) for s in gz[tag + "__phi"][1:, :, 0].ravel()}
        off = 0
        for name, n in blocks:
            if name[:3] in ("lam", "b_") and int(name.rsplit("_", 1)[1]) > max(used):
                assert not gz[tag + "__grads"][off:off + n].any() and not r["grads"][off:off + n].any(), (tag, name)
            off += n


def test_smp2d_ver5_ref_activations_and_adjacencies(gz):
    """the level activations ([s, s, C]) and the reduced adjacencies of CH4: unit diagonal, row sums of 1"""
    seen = 0
    for tag in gz["tags"]:
        if tag + "__activations" not in gz:
            continue
        seen += 1
        r = ref_of(gz, tag)
        act = np.concatenate([f.ravel() for fl in r["f"] for f in fl])
        assert rel_err(act, gz[tag + "__activations"]) <= TOL_REF, tag
        radj = np.concatenate([a.ravel() for al in r["radj"][1:] for a in al])
        assert rel_err(radj, gz[tag + "__adjacency"]) <= TOL_REF, tag
        for al in r["radj"][1:]:
            for a in al:
                assert np.allclose(a.sum(1), 1.0) and np.all(np.diag(a) > 0)
    assert seen == 2


def test_ch4_gradients_pin_the_multiplicities(gz):
    """On CH4 (four hydrogens of one field size at level 1, five atoms of one at level 2) the real class's dlambda of the shared size is
    NOT what multiplicity 1 or SMP_2D's j (j + 1) / 2 gives, and its dK_l is NOT what the j rule gives: lambda is counted j times, K once."""
    tag = "f5_CH4_c5"
    _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
    phi = gz[tag + "__phi"]
    assert list(phi[1, :, 0]) == [5, 2, 2, 2, 2] and list(phi[2, :, 0]) == [5] * 5
    blocks = smp2d_ver5_blocks(Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV)
    off = {name: o for (name, _), o in zip(blocks, np.cumsum([0] + [n for _, n in blocks])[:-1])}
    lam = lambda g: np.concatenate([g[off["lam1_2_5"]:off["lam1_2_5"] + Cn], g[off["lam2_1_2"]:off["lam2_1_2"] + Cn]])   # noqa: E731
    kk = lambda g: np.concatenate([g[off["K_%d" % l]:off["K_%d" % l] + 2 * Cn * Cn] for l in (1, 2)])   # noqa: E731
    real = gz[tag + "__grads"]
    assert rel_err(lam(ref_of(gz, tag)["grads"]), lam(real)) <= TOL_REF and rel_err(kk(ref_of(gz, tag)["grads"]), kk(real)) <= TOL_REF
    saved = smp2d_ver5_ref.multiplicity, smp2d_ver5_ref.k_multiplicity
    try:
        for rule in (lambda j: 1, lambda j: j * (j + 1) // 2):
            smp2d_ver5_ref.multiplicity = rule
            assert rel_err(lam(ref_of(gz, tag)["grads"]), lam(real)) > 1e-3
        smp2d_ver5_ref.multiplicity = saved[0]
        smp2d_ver5_ref.k_multiplicity = lambda j: j
        assert rel_err(kk(ref_of(gz, tag)["grads"]), kk(real)) > 1e-3
    finally:
        smp2d_ver5_ref.multiplicity, smp2d_ver5_ref.k_multiplicity = saved


def test_operator_references_compose_to_the_real_class(gz):
    """tests/smp2d_ver5_ops_ref.py (the reference of the stand-alone level operators) on the 12-vertex molecule at (C, nLevels) = (8, 3):
    with S, col = S.sum(0) and dz, cz = dz.sum(0) of smp2d_ver5_ref as operands, cols_forward -> rows_forward reproduce every level's
    f_l, and wgrad the K_l block of the real class's gradient, at 1e-9 -- so the operator suite cannot agree with itself and not with
    SMP_2D_ver5.  (row = r0 + i s + j, column = c0 + j: level_tables is the layout of v5_store_S.)"""
    tag = [t for t in gz["tags"] if gz[t + "__cfg"][2] == 8 and len(gz[t + "__adj"]) == 12][0]
    _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
    assert L == 3
    r = ref_of(gz, tag)
    phi = smp2d_ver5_ref.fields_of(gz[tag + "__phi"])
    FD = gz[tag + "__feature"].shape[1] * (D + 1)
    _, lv, _ = smp2d_ver5_ref.split(np.asarray(gz[tag + "__params"], dtype=np.float64), Cn, FD, L, maxV)
    blocks = smp2d_ver5_blocks(Cn, FD, L, maxV)
    off = {name: o for (name, _), o in zip(blocks, np.cumsum([0] + [n for _, n in blocks])[:-1])}
    for l in range(1, L + 1):
        lam1, lam2, b, K, _ = lv[l]
        sizes = np.concatenate([lam1, lam2, b], axis=1)
        node_sizes = [len(f) for f in phi[l]]
        assert len(set(node_sizes)) > 1   # (a tile of rows spans nodes of different sizes)
        row_cs, col_s = ops.level_tables(node_sizes)
        S = np.concatenate([x.reshape(-1, Cn) for x in r["S"][l]])
        dz = np.concatenate([x.reshape(-1, Cn) for x in r["dz"][l]])
        col = np.concatenate([x.sum(0) for x in r["S"][l]])
        cz = np.concatenate([x.sum(0) for x in r["dz"][l]])
        f, _ = ops.rows_forward(K, S, sizes, ops.cols_forward(K, col, sizes, col_s), row_cs, ALPHA)
        fl = np.concatenate([x.reshape(-1, Cn) for x in r["f"][l]])
        assert np.abs(f - fl).max() <= TOL_REF * np.abs(fl).max(), (tag, l)
        dK = ops.wgrad(dz, S, row_cs, cz, col, col_s, sizes)
        o = off["K_%d" % l]
        real = gz[tag + "__grads"][o:o + 2 * Cn * Cn].reshape(Cn, 2 * Cn)
        for h in (slice(0, Cn), slice(Cn, 2 * Cn)):   # (each half against its own size)
            assert np.abs(dK[:, h] - real[:, h]).max() <= TOL_REF * np.abs(real[:, h]).max(), (tag, l)
