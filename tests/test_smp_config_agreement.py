"""One account of a handle's configuration (graphflow_amd/csrc/smp_config.cpp: gfsmp::resolve_config) and of its parameter blocks
(smp_prep.h: gfsmp::Config::level_blocks): the host-only gf_smp_config_param_count, gf_smp_classifier_config_param_count and the two
*_uniform_init_host calls answer 0 / GF_ERR_INVALID exactly where gf_smp_create / gf_smp_create_classifier refuse, and count what the
Python restatements and golden generators list where they accept.  One grid: an accepted configuration per family and form, and every
refusal the two create functions have.  The CPU half needs no device; the GPU half only creates and destroys handles."""
import ctypes as C

import numpy as np
import pytest

import neighbourhood_ref as nref
from make_smp1d_golden import smp1d_blocks
from make_smp2d_golden import smp2d_blocks
from make_smp2d_ver5_golden import smp2d_ver5_blocks
from make_theta_golden import theta_blocks
from make_unrestricted_golden import unrestricted_blocks

L, CH, F, D, FIELD = 2, 4, 4, 1, 6
FD = F * (D + 1)
INVALID, UNSUPPORTED = 1, 4   # gf_status (include/gf_hip.h)


def cfg(**over):
    from graphflow_amd.smp import SMPConfig
    d = dict(nLevels=L, nChanels=CH, nFeatures=F, nDepth=D, max_receptive_field=FIELD, has_WL_ordering=1)
    d.update(over)
    return SMPConfig(**d)


def total(blocks):
    return sum(n for _, n in blocks)


def slices(nK, nClass=0):
    """H [C][F (D + 1)]; (K_l [nK C][C], b_l [C]) per level; W [C] or [nClass][C] (include/gf_hip.h, gf_smp_config)"""
    return CH * FD + L * (nK * CH * CH + CH) + max(nClass, 1) * CH


def tower18():
    """physics = 1: H [C][F]; (K_l [18 C_{l-1}][C_l], b_l [C_l]) with C_l = max(1, C_{l-1} / 2); no W"""
    c = [max(1, CH >> l) for l in range(L + 1)]
    return CH * F + sum(18 * c[l - 1] * c[l] + c[l] for l in range(1, L + 1))


NO_CAP = dict(max_nVertices=FIELD)
# (name, configuration, nClass -- 0: gf_smp_create, else gf_smp_create_classifier --, parameter count)
ACCEPTED = [
    ("omega", cfg(), 0, slices(18)),
    ("ver8", cfg(nContractions=18, custom_matmul=1), 0, slices(18)),
    ("ver6", cfg(nContractions=10, custom_matmul=1), 0, slices(10)),
    ("ver7", cfg(nContractions=50, custom_matmul=1), 0, slices(50)),
    ("gamma", cfg(nContractions=4), 0, slices(4)),
    ("tower18", cfg(physics=1, nDepth=0), 0, tower18()),
    ("theta", cfg(first_order=1, **NO_CAP), 0, total(theta_blocks(CH, FD, L, FIELD))),
    ("theta_capped", cfg(first_order=1, max_nVertices=12), 0, total(theta_blocks(CH, FD, L, 12))),
] + [
    ("smp1d_%d" % v, cfg(first_order=1 + v, **NO_CAP), 0, total(smp1d_blocks(v, CH, FD, L, FIELD))) for v in (1, 2, 3)
] + [
    ("smp2d_%d" % f, cfg(steerable_2d=f, **NO_CAP), 0, total(smp2d_blocks(f, CH, FD, L, FIELD))) for f in (1, 2)
] + [
    ("smp2d_5", cfg(steerable_2d=5, **NO_CAP), 0, total(smp2d_ver5_blocks(CH, FD, L, FIELD))),
] + [
    ("unrestricted_%d" % f, cfg(unrestricted=f, **NO_CAP), 0, total(unrestricted_blocks(f, CH, FD, L, FIELD))) for f in (1, 2, 3)
] + [
    ("fingerprint", cfg(neighbourhood=1, nDepth=0, **NO_CAP), 0, nref.n_params(CH, F, L)),
    ("gcn_1d", cfg(neighbourhood=2, max_Radius=1, **NO_CAP), 0, nref.n_params(CH, FD, L)),
    ("gcn_2d", cfg(neighbourhood=3, **NO_CAP), 0, nref.n_params(CH, FD, L)),
    ("gcn_2d_no_levels", cfg(neighbourhood=3, nLevels=0, **NO_CAP), 0, nref.n_params(CH, FD, 0)),
] + [
    ("classes_%d" % nK, cfg(nContractions=nK, custom_matmul=int(nK != 4)), 3, slices(nK, 3)) for nK in (10, 50, 18, 4)
] + [
    ("smp1d_%d_classes" % v, cfg(first_order=1 + v, **NO_CAP), 3, total(smp1d_blocks(v, CH, FD, L, FIELD, 3))) for v in (1, 2, 3)
] + [
    ("smp2d_%d_classes" % f, cfg(steerable_2d=f, **NO_CAP), 3, total(smp2d_blocks(f, CH, FD, L, FIELD, 3))) for f in (1, 2)
]

# (name, configuration, nClass, status of the create function, text its message holds).  The first six are the configurations the host-only
# functions used to count although gf_smp_create refuses them.
REFUSED = [
    ("contractions_7", cfg(nContractions=7), 0, INVALID, b"gf_smp_create: nContractions = 7 (expected 4, 10, 18 or 50)"),
    ("gamma_custom_matmul", cfg(nContractions=4, custom_matmul=1), 0, INVALID, b"applies K_l [4 C][C] by Reshape2D + MatMul: set custom_matmul = 0"),
    ("tower_with_depth", cfg(physics=1), 0, INVALID, b"gf_smp_create: a physics tower has nDepth 0 (raw features), RisiContraction_18 or _4"),
    ("tower_contractions_10", cfg(physics=1, nDepth=0, nContractions=10), 0, INVALID, b"gf_smp_create: a physics tower has nDepth 0 (raw features)"),
    ("theta_tower", cfg(physics=1, nDepth=0, first_order=1, **NO_CAP), 0, INVALID, b"gf_smp_create: first_order = 1 has no single-handle physics tower"),
    ("gamma_tower", cfg(physics=1, nDepth=0, nContractions=4), 0, INVALID, b"gf_smp_create: nContractions = 4 (SMP_gamma) has no single-handle physics tower"),
    ("no_levels", cfg(nLevels=0), 0, INVALID, b"gf_smp_create: bad configuration"),
    ("no_channels", cfg(nChanels=0), 0, INVALID, b"gf_smp_create: bad configuration"),
    ("negative_depth", cfg(nDepth=-1), 0, INVALID, b"gf_smp_create: bad configuration"),
    ("fingerprint_with_depth", cfg(neighbourhood=1, **NO_CAP), 0, INVALID, b"gf_smp_create: neighbourhood = 1 (1: NeuralFingerprint, 2: GCN_1D, 3: GCN_2D) needs"),
    ("gcn_on_a_field_model", cfg(neighbourhood=2, first_order=2, **NO_CAP), 0, INVALID, b"gf_smp_create: neighbourhood = 2 (1: NeuralFingerprint"),
    ("unrestricted_capped", cfg(unrestricted=1, max_nVertices=8), 0, INVALID, b"gf_smp_create: unrestricted = 1 (1: Unrestricted_SMP_1D, 2: _1D_ver2, 3: _2D) needs"),
    ("unrestricted_4", cfg(unrestricted=4, **NO_CAP), 0, INVALID, b"gf_smp_create: unrestricted = 4 (1: Unrestricted_SMP_1D"),
    ("unrestricted_too_many_parameters", cfg(unrestricted=3, nChanels=65536, nLevels=4, max_receptive_field=4096, max_nVertices=4096), 0, INVALID,
     b"and a parameter count that fits an int"),
    ("steerable_3", cfg(steerable_2d=3, **NO_CAP), 0, INVALID, b"gf_smp_create: steerable_2d = 3 (1: SMP_2D, 2: SMP_2D_ver4, 5: SMP_2D_ver5) needs"),
    ("steerable_first_order", cfg(steerable_2d=1, first_order=2, **NO_CAP), 0, INVALID, b"gf_smp_create: steerable_2d = 1 (1: SMP_2D"),
    ("ver5_too_wide", cfg(steerable_2d=5, nChanels=129, **NO_CAP), 0, INVALID, b"for 5, nChanels (129) <= 128"),
    ("smp1d_capped", cfg(first_order=2, max_nVertices=8), 0, INVALID, b"gf_smp_create: first_order = 2 (2: SMP_1D, 3: SMP_1D_ver2, 4: SMP_1D_ver3) needs"),
    ("smp1d_ver2_too_deep", cfg(first_order=3, nLevels=17, **NO_CAP), 0, INVALID, b"gf_smp_create: first_order = 3 (2: SMP_1D"),
    ("first_order_5", cfg(first_order=5, **NO_CAP), 0, INVALID, b"gf_smp_create: first_order = 5 (2: SMP_1D"),
    ("theta_small_max_vertices", cfg(first_order=1, max_nVertices=5), 0, INVALID,
     b"gf_smp_create: first_order = 1 needs nContractions = custom_matmul = 0 and max_nVertices (5) >= max_receptive_field (6)"),
    ("theta_contractions", cfg(first_order=1, nContractions=18, **NO_CAP), 0, INVALID, b"gf_smp_create: first_order = 1 needs nContractions = custom_matmul = 0"),
    ("theta_classes", cfg(first_order=1, **NO_CAP), 3, UNSUPPORTED, b"gf_smp_create_classifier: a first-order model (first_order = 1) has no classifier read-out"),
    ("unrestricted_classes", cfg(unrestricted=1, **NO_CAP), 3, UNSUPPORTED, b"gf_smp_create_classifier: the Unrestricted_SMP_* models have no `_classification` class"),
    ("gcn_classes", cfg(neighbourhood=2, **NO_CAP), 3, UNSUPPORTED, b"gf_smp_create_classifier: NeuralFingerprint / GCN_1D / GCN_2D have no `_classification` class"),
    ("tower_classes", cfg(physics=1, nDepth=0), 3, INVALID, b"gf_smp_create_classifier: a physics tower has no read-out of its own (physics = 0)"),
    ("one_class", cfg(), 1, INVALID, b"gf_smp_create_classifier: nClass = 1 (at least 2)"),
    ("ver5_classes", cfg(steerable_2d=5, **NO_CAP), 3, UNSUPPORTED, b"gf_smp_create_classifier: SMP_2D_ver5 has no `_classification` class"),
    ("classes_contractions_7", cfg(nContractions=7), 3, INVALID, b"gf_smp_create: nContractions = 7 (expected 4, 10, 18 or 50)"),
    ("classes_smp1d_capped", cfg(first_order=2, max_nVertices=8), 3, INVALID, b"gf_smp_create: first_order = 2 (2: SMP_1D"),
]


def host_count(lib, c, nClass):
    return lib.gf_smp_classifier_config_param_count(C.byref(c), nClass) if nClass else lib.gf_smp_config_param_count(C.byref(c))


def host_init(lib, c, nClass, out):
    p = out.ctypes.data_as(C.POINTER(C.c_float))
    return lib.gf_smp_classifier_uniform_init_host(C.byref(c), nClass, p) if nClass else lib.gf_smp_uniform_init_host(C.byref(c), p)


def test_the_grid_holds_every_family_and_form():
    names = [n for n, _, _, _ in ACCEPTED]
    assert len(set(names)) == len(names) and len({n for n, _, _, _, _ in REFUSED}) == len(REFUSED)
    plain = [c for _, c, k, _ in ACCEPTED if not k]
    assert {c.nContractions for c in plain} >= {0, 4, 10, 18, 50} and any(c.physics for c in plain)
    assert {c.first_order for c in plain} >= {1, 2, 3, 4} and {c.steerable_2d for c in plain} >= {1, 2, 5}
    assert {c.unrestricted for c in plain} >= {1, 2, 3} and {c.neighbourhood for c in plain} >= {1, 2, 3}
    assert sum(1 for _, _, k, _ in ACCEPTED if k) == 9


@pytest.mark.parametrize("name,c,nClass,status,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_what_create_refuses_has_no_host_only_answer(gf, name, c, nClass, status, text):
    """count 0 and GF_ERR_INVALID from uniform_init_host, through the entry the refusal belongs to -- and, for a configuration refused
    whoever asks, through the other one too"""
    from graphflow_amd import _lib
    lib = _lib.load()
    out = np.full(1 << 16, 7.0, dtype=np.float32)   # (room for what the parent commit drew for the six it accepted)
    assert host_count(lib, c, nClass) == 0
    assert host_init(lib, c, nClass, out) == _lib.GF_ERR_INVALID
    assert (out == 7.0).all()
    if not nClass:   # (what gf_smp_create refuses, gf_smp_create_classifier refuses for some reason of its own or for the same one)
        assert host_count(lib, c, 3) == 0 and host_init(lib, c, 3, out) == _lib.GF_ERR_INVALID


@pytest.mark.parametrize("name,c,nClass,count", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_what_create_accepts_is_counted_as_the_oracles_list_it(gf, name, c, nClass, count):
    from graphflow_amd import _lib
    lib = _lib.load()
    assert host_count(lib, c, nClass) == count
    out = np.full(count + 1, 7.0, dtype=np.float32)
    C.CDLL(None).srand(5)
    assert host_init(lib, c, nClass, out) == _lib.GF_OK
    assert out[count] == 7.0 and 0 < np.abs(out[:count]).max() < 1   # (every draw is (rand() % 10) / (10 n), n the block's divisor)


def test_null_arguments():
    from graphflow_amd import _lib
    lib = _lib.load()
    out = np.zeros(8, dtype=np.float32)
    assert lib.gf_smp_config_param_count(None) == 0 and lib.gf_smp_classifier_config_param_count(None, 3) == 0
    assert lib.gf_smp_uniform_init_host(None, out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID
    assert lib.gf_smp_uniform_init_host(C.byref(cfg()), None) == _lib.GF_ERR_INVALID
    assert lib.gf_smp_classifier_uniform_init_host(C.byref(cfg()), 3, None) == _lib.GF_ERR_INVALID


def create(ctx, c, nClass):
    h = C.c_void_p()
    if nClass:
        return ctx.lib.gf_smp_create_classifier(ctx.handle, C.byref(c), nClass, C.byref(h)), h
    return ctx.lib.gf_smp_create(ctx.handle, C.byref(c), C.byref(h)), h


@pytest.mark.gpu
def test_create_agrees_with_the_host_only_answers(gf):
    """every grid entry through the create function itself: an accepted handle holds the host-only count, a refusal has the status and
    the message it always had.  No prepare, no kernel."""
    from graphflow_amd import _lib
    from graphflow_amd.ops import default_context
    ctx = default_context()
    for name, c, nClass, count in ACCEPTED:
        st, h = create(ctx, c, nClass)
        assert st == _lib.GF_OK, (name, ctx.lib.gf_last_error(ctx.handle))
        assert ctx.lib.gf_smp_param_count(h) == host_count(ctx.lib, c, nClass) == count, name
        assert ctx.lib.gf_smp_classes(h) == nClass, name
        assert ctx.lib.gf_smp_destroy(h) == _lib.GF_OK
    for name, c, nClass, status, text in REFUSED:
        st, h = create(ctx, c, nClass)
        assert st == status and not h.value, name
        assert text in ctx.lib.gf_last_error(ctx.handle), (name, ctx.lib.gf_last_error(ctx.handle))
