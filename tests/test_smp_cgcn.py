"""CPU suite for CGCN_1D and CGCN_2D (gf_smp_config.covariant = 1, 2): tests/cgcn_ref.py, the numpy restatement the GPU suites lean on,
against the real classes' numbers (tests/golden/smp_cgcn.npz, written by tests/golden/make_cgcn_golden.py) at 1e-12, block by block; the
two forms of the 2D aggregate against each other; and what the library answers without a device -- parameter counts for accepted
configurations and for every refusal (with a piece of its message), the classes' initial weights bit for bit, and the host preparation
(lists, masks, x) entry by entry against what the classes filled."""
import ctypes as C

import numpy as np
import pytest

import cgcn_ref as cref
from field_suite import blockwise, load_golden
from util import rel_err

INVALID, UNSUPPORTED = 1, 4   # gf_status (include/gf_hip.h)
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)


def golden():
    return load_golden("smp_cgcn.npz")


def tags(form=None):
    return [str(t) for t in golden()["tags"] if form is None or str(t).startswith("c%d_" % form)]


def case(tag):
    """(form, L, M, D), adj, feature, (predict, loss, target), params"""
    gz = golden()
    return (tuple(int(x) for x in gz[tag + "__cfg"]), gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"],
            gz[tag + "__params"].astype(np.float64))


def config(form, L, M, F, D, **over):
    from graphflow_amd.smp import CGCN1D, CGCN2D
    c = (CGCN1D if form == 1 else CGCN2D).config(L, M, F, D)
    assert c.covariant == form and c.nChanels == 1
    for k, v in over.items():
        setattr(c, k, v)
    return c


def refused_configs():
    """(configuration, a piece of the message) for every GF_ERR_INVALID rule of the family"""
    out = [(config(1, 2, 6, 4, 1, covariant=3), b"covariant = 3"), (config(1, 2, 6, 4, 1, covariant=-1), b"covariant = -1")]
    for field in ("first_order", "steerable_2d", "unrestricted", "neighbourhood", "matrix_form", "distance_channel", "readout", "physics",
                  "nContractions", "custom_matmul"):
        out.append((config(2, 2, 6, 4, 1, **{field: 1}), b"every other form selector 0"))
    out += [(config(1, 2, 6, 4, 1, nChanels=2), b"nChanels = 1"), (config(1, 2, 6, 4, 1, nChanels=0), b"nChanels = 1"),
            (config(2, -1, 6, 4, 1), b"nLevels in 0 .. 64"), (config(2, 65, 6, 4, 1), b"nLevels in 0 .. 64"),
            (config(1, 2, 6, 0, 1), b"nFeatures >= 1"), (config(1, 2, 6, 4, -1), b"nDepth >= 0"),
            (config(1, 2, 6, 1 << 20, 1 << 20), b"at most 65536"),
            (config(1, 2, 0, 4, 1), b"max_nVertices in 1 .. 75"), (config(2, 2, 76, 4, 1), b"max_nVertices in 1 .. 75"),
            (config(2, 2, 0x7fffffff, 4, 1), b"max_nVertices in 1 .. 75")]
    return out


# ---- the restatement against the real classes ----
@pytest.mark.parametrize("tag", tags())
def test_restatement_meets_the_real_class(tag):
    gz = golden()
    (form, L, M, D), adj, feat, result, params = case(tag)
    assert np.array_equal(feat, feat.astype(np.float32).astype(np.float64))
    for pair_loops in (False, True):
        r = cref.run(form, adj, feat, result[2], params, L, M, D, pair_loops=pair_loops)
        assert rel_err(r["feature"], gz[tag + "__feature_out"]) <= 1e-12
        assert rel_err([r["predict"], r["loss"]], result[:2]) <= 1e-12
        e = blockwise(r["grads"], gz[tag + "__grads"], cref.blocks(feat.shape[1] * (D + 1), L, M))
        assert e[0] <= 1e-12, e
        if tag + "__activations" in gz:
            assert rel_err(r["h"], gz[tag + "__activations"]) <= 1e-12
    assert np.array_equal(r["masks"].astype(np.uint8), gz[tag + "__masks"])
    if L:
        assert np.array_equal(cref.lists_flat(r["lists"]), gz[tag + "__lists"])
    assert cref.min_preactivation_gap(form, adj, feat, params, L, M, D) >= 1e-3   # (no pre-activation near the kink of LeakyReLU)


def test_the_two_forms_of_the_2d_aggregate_agree():
    rng = np.random.default_rng(11)
    for members in (0, 1, 2, 3, 7):
        hs = [rng.uniform(-1, 1, 9) for _ in range(members)]
        a, b = cref.aggregate_pairs(hs, 9), cref.aggregate_closed(hs, 9)
        assert rel_err(b, a) <= 1e-14
        if members < 2:
            assert not a.any() and not b.any()
    for tag in tags(2):
        (form, L, M, D), adj, feat, result, params = case(tag)
        a = cref.run(2, adj, feat, result[2], params, L, M, D, pair_loops=True)
        b = cref.run(2, adj, feat, result[2], params, L, M, D)
        assert rel_err(b["n"], a["n"]) <= 1e-13 and rel_err(b["grads"], a["grads"]) <= 1e-12, tag


def test_fixtures_cover_the_cases_the_level_can_go_wrong_at():
    cs = {t: case(t) for t in tags()}
    for form in (1, 2):
        mine = [c for t, c in cs.items() if t.startswith("c%d_" % form)]
        assert {0, 1, 2, 3, 4} <= {c[0][1] for c in mine}
        assert {1, 2, 12} <= {len(c[1]) for c in mine} and any(len(c[1]) == c[0][2] for c in mine)
        assert any(np.diag(c[1]).any() for c in mine) and any(not np.array_equal(c[1], c[1].T) for c in mine)
        assert any((c[1].sum(axis=0) == 0).any() and len(c[1]) > 1 for c in mine)   # an isolated vertex
        assert all(c[0][:3] == (form, 1, 6) and c[0][3] == 5 for t, c in cs.items() if t.startswith("c%d_toy_" % form))
    assert np.abs(golden()["c2_syn12__grads"]).max() > 0 and np.abs(golden()["c2_diagonal__grads"]).max() > 0


@pytest.mark.parametrize("form", [1, 2])
def test_restatement_follows_the_classes_batchlearn(form):
    gz = golden()
    from inputs import f32exact, toy_molecules
    p_ = "train_c%d__" % form
    _, L, M, D, seed, n_iter = (int(x) for x in gz[p_ + "cfg"])
    mols = [(a, f32exact(f)) for _, a, f, _ in toy_molecules()]
    losses, p = cref.momentum_steps(form, mols, gz[p_ + "targets"], gz[p_ + "params0"], L, M, D, n_iter, float(gz[p_ + "lr"][0]),
                                    float(gz[p_ + "momentum"][0]))
    assert rel_err(losses, gz[p_ + "losses"]) <= 1e-12
    assert np.abs(p - gz[p_ + "params"]).max() <= 1e-12
    assert (gz[p_ + "losses"][:, 1] < gz[p_ + "losses"][:, 0]).all()


@pytest.mark.parametrize("form", [1, 2])
def test_checkpoint_is_the_parameters_in_registration_order(form):
    gz = golden()
    text = bytes(gz["checkpoint_c%d__text" % form]).decode().split()
    assert text == ["%g" % x for x in gz[str(gz["checkpoint_c%d__tag" % form]) + "__params"]]


# ---- the library without a device ----
def test_parameter_counts_and_refusals(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    for form, L, M, F, D in ((1, 0, 1, 1, 0), (1, 3, 29, 5, 2), (2, 1, 6, 4, 5), (2, 64, 64, 4, 1), (1, 2, 75, 3, 0)):
        c = config(form, L, M, F, D, max_receptive_field=0, has_WL_ordering=1, max_Radius=-7)   # (the three fields that are not read)
        assert lib.gf_smp_config_param_count(C.byref(c)) == cref.n_params(F * (D + 1), L, M) == F * (D + 1) + L * M * M
    for tag in tags():
        (form, L, M, D), adj, feat, _, params = case(tag)
        assert lib.gf_smp_config_param_count(C.byref(config(form, L, M, feat.shape[1], D))) == params.size
    buf = (C.c_float * 4096)()
    for bad, text in refused_configs():
        assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
        assert lib.gf_smp_uniform_init_host(C.byref(bad), buf) == INVALID
        lists, hop = (C.c_int * 64)(), (C.c_ubyte * 64)()
        adj, feat = (C.c_int * 1)(0), (C.c_double * 8)()
        assert lib.gf_smp_covariant_molecule_host(C.byref(bad), 1, adj, feat, lists, hop, None) == INVALID
        assert text in lib.gf_last_error(None), (text, lib.gf_last_error(None))
    ok = config(1, 2, 6, 4, 1)
    assert lib.gf_smp_classifier_config_param_count(C.byref(ok), 3) == 0
    phi = (C.c_int * 4096)()
    assert lib.gf_smp_prepare_molecule_host(C.byref(ok), 1, (C.c_int * 1)(0), (C.c_double * 4)(), phi, None) == INVALID
    assert b"gf_smp_covariant_molecule_host" in lib.gf_last_error(None)


def test_zero_tail_reproduces_every_existing_form(gf):
    """covariant = 0 is everything as before: a structure without the new field (the library is given a zero there) and one with it set to
    0 count the same parameters, for a configuration of every family the resolver takes; `covariant` is the full structure's last field"""
    from graphflow_amd import _lib
    from graphflow_amd.smp import (GCA1D, GCNMW, LCNN, SMP1D, SMP2D, SMPConfig, SMPConfigCovariant, SMPDistance, SMPGatedNeighbourhood,
                                   SMPKernelPairs, SMPNeighbourhood, SMPTheta, SMPUnrestricted)
    lib = _lib.load()
    cfgs = [SMPConfig(2, 8, 5, 1, 12, 1), SMPConfig(2, 8, 5, 1, 12, 1, 10, 1), SMPConfig(2, 8, 5, 1, 12, 1, 4), SMPTheta.config(12, 9, 2, 8, 5, 1),
            SMP1D.config(2, 9, 2, 6, 5, 1), SMP2D.config(list(SMP2D.FORMS)[0], 9, 2, 6, 5, 1),
            SMPUnrestricted.config(list(SMPUnrestricted.FORMS)[0], 9, 2, 6, 5, 1), SMPNeighbourhood.config("gcn_2d", 2, 8, 5, 1, 9, 1),
            SMPGatedNeighbourhood.config(list(SMPGatedNeighbourhood.FORMS)[0], 2, 8, 5, 1, 9, 1),
            SMPDistance.config(list(SMPDistance.FORMS)[0], 2, 8, 5, 1, 9, 1), GCNMW.config(2, 9, 5, 8, 1), LCNN.config(9, 5, 3, 1, 8, 6, 4),
            SMPKernelPairs.config(list(SMPKernelPairs.FORMS)[0], 2, 8, 5, 1, 9, 1), GCA1D.config("gca_1d", 2, 8, 5, 1, 9, 1)]
    assert [f[0] for f in SMPConfigCovariant._fields_] == ["covariant"] and issubclass(SMPConfigCovariant, SMPConfig)
    assert C.sizeof(SMPConfigCovariant) == C.sizeof(SMPConfig) + C.sizeof(C.c_int) == _lib.SMP_CONFIG_BYTES
    assert SMPConfigCovariant.covariant.offset == C.sizeof(SMPConfig)   # the structure's last field
    names = [f[0] for f in SMPConfig._fields_]
    for cfg in cfgs:
        n = lib.gf_smp_config_param_count(C.byref(cfg))   # (the earlier layout: the binding hands it on with a zero tail)
        assert n > 0, [getattr(cfg, f) for f in names]
        full = SMPConfigCovariant(*[getattr(cfg, f) for f in names], covariant=0)
        assert lib.gf_smp_config_param_count(C.byref(full)) == n
        assert lib.gf_smp_config_param_count(full) == n and lib.gf_smp_config_param_count(C.pointer(full)) == n
        full.covariant = 1   # (... and the tail is read: no other form goes with it)
        assert lib.gf_smp_config_param_count(C.byref(full)) == 0


def test_binding_pads_a_structure_of_an_earlier_layout(gf):
    """_lib.ConfigPointer: behind a structure that ends at `readout` the library sees zeros, whatever the caller's memory holds there; a
    structure of the full size, and an address without a size, go through as they are"""
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPConfig, SMPConfigCovariant, SMPNeighbourhood
    lib = _lib.load()
    cfg = SMPNeighbourhood.config("gcn_2d", 2, 8, 5, 1, 9, 1)
    n = lib.gf_smp_config_param_count(C.byref(cfg))
    assert n > 0
    ints = C.sizeof(SMPConfig) // C.sizeof(C.c_int)
    mem = (C.c_int * (ints + 1))()   # the earlier structure with something else behind it
    C.memmove(mem, C.addressof(cfg), C.sizeof(SMPConfig))
    mem[ints] = 0x7f12
    assert lib.gf_smp_config_param_count(C.cast(mem, C.POINTER(SMPConfig))) == n
    assert lib.gf_smp_config_param_count(C.cast(mem, C.POINTER(SMPConfigCovariant))) == 0     # (read as the full structure: covariant = 0x7f12)
    assert lib.gf_smp_config_param_count(C.cast(mem, C.c_void_p)) == 0                        # (an address: as it is)
    assert lib.gf_smp_config_param_count(None) == 0
    assert mem[ints] == 0x7f12 and bytes(mem)[:C.sizeof(SMPConfig)] == bytes(cfg)


@pytest.mark.parametrize("form", [1, 2])
def test_uniform_init_draws_the_classes_weights(gf, form):
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    p_ = "train_c%d__" % form
    _, L, M, D, seed, _ = (int(x) for x in gz[p_ + "cfg"])
    out = np.empty(gz[p_ + "params0"].size, dtype=np.float32)
    C.CDLL(None).srand(seed)
    assert lib.gf_smp_uniform_init_host(C.byref(config(form, L, M, 4, D)), out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert np.array_equal(out, gz[p_ + "params0"].astype(np.float32))
    FD = 4 * (D + 1)
    assert np.abs(out[:FD]).max() <= 9 / (10 * FD) + 1e-9 and np.abs(out[FD:]).max() <= 9 / (10 * M) + 1e-9   # a Vector, then Matrices


def host_molecule(lib, form, L, M, D, adj, feat):
    V, F = feat.shape
    lists = np.empty((V, M + 1), dtype=np.int32)
    hop = np.empty((V, M), dtype=np.uint8)
    x = np.empty((V, F * (D + 1)))
    a, f = np.ascontiguousarray(adj, dtype=np.int32), np.ascontiguousarray(feat, dtype=np.float64)
    st = lib.gf_smp_covariant_molecule_host(C.byref(config(form, L, M, F, D)), V, a.ctypes.data_as(IP), f.ctypes.data_as(DP),
                                            lists.ctypes.data_as(IP), hop.ctypes.data_as(C.c_void_p), x.ctypes.data_as(DP))
    assert st == 0, lib.gf_last_error(None)
    return lists, hop, x


@pytest.mark.parametrize("tag", tags())
def test_host_preparation_is_the_classes(gf, tag):
    """N(v), the masks of every level and x of every fixture, the asymmetric and the diagonal one included"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    (form, L, M, D), adj, feat, result, params = case(tag)
    V = len(adj)
    lists, hop, x = host_molecule(lib, form, L, M, D, adj, feat)
    N = [list(lists[v, 1:1 + lists[v, 0]]) for v in range(V)]
    assert all((lists[v, 1 + lists[v, 0]:] == -1).all() for v in range(V))
    assert N == cref.neighbours(adj)
    if L:
        assert np.array_equal(cref.lists_flat(N), gz[tag + "__lists"])
    for l in range(L + 1):
        assert np.array_equal((hop <= l).astype(np.uint8), gz[tag + "__masks"][l]), l
    assert (hop[:, V:] == 255).all()
    assert np.array_equal(x, cref.run(form, adj, feat, 0.0, params, L, M, D)["x"])


def test_host_preparation_refuses_a_molecule_above_max_nvertices(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    c = config(1, 1, 3, 4, 0)
    adj, feat = np.zeros((4, 4), dtype=np.int32), np.zeros((4, 4))
    lists, hop = np.empty((4, 4), dtype=np.int32), np.empty((4, 3), dtype=np.uint8)
    assert lib.gf_smp_covariant_molecule_host(C.byref(c), 4, adj.ctypes.data_as(IP), feat.ctypes.data_as(DP), lists.ctypes.data_as(IP),
                                              hop.ctypes.data_as(C.c_void_p), None) == INVALID
    assert b"max_nVertices = 3" in lib.gf_last_error(None)
