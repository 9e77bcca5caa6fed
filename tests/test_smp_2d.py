"""CPU suite for SMP_2D, SMP_2D_ver4 and their classifiers (gf_smp_config.steerable_2d = 1, 2): the parameter layout, the initial weights,
the receptive fields of the host preparation and the fp64 restatement tests/smp2d_ref.py, all against the real classes' numbers in
tests/golden/smp_2d.npz (tests/golden/make_smp2d_golden.py).  Host code only: no device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import smp2d_ref
from make_smp2d_golden import smp2d_blocks
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_REF = 1e-9   # fp64 restatement against the fp64 reference: summation order only
FORM = {1: "2d", 2: "ver4"}


@pytest.fixture(scope="module")
def lib():
    from graphflow_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gz():
    with np.load(os.path.join(HERE, "golden", "smp_2d.npz")) as z:
        return {k: z[k] for k in z.files}


def cfg_of(form, L, Cn, F, D, wl, maxV):
    from graphflow_amd.smp import SMP2D
    return SMP2D.config(FORM[form], maxV, L, Cn, F, D, bool(wl))


def blockwise(x, ref, blocks):
    off, worst = 0, (0.0, "")
    for name, n in blocks:
        worst = max(worst, (rel_err(x[off:off + n], ref[off:off + n]), name))
        off += n
    assert off == ref.size
    return worst


def ref_of(gz, tag, nClass=0):
    form, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
    return smp2d_ref.run(form, gz[tag + "__adj"], gz[tag + "__feature"], float(gz[tag + "__target"][0]), gz[tag + "__params"], L, Cn, D, maxV,
                         smp2d_ref.fields_of(gz[tag + "__phi"]), nClass)


def test_parameter_count_matches_the_reference(lib, gz):
    """gf_smp_config_param_count / gf_smp_classifier_config_param_count against the length of the real class's gradient vector and against
    the sum of the registration-order blocks, for every golden case of the two forms and the two classifiers."""
    for tag in list(gz["tags"]) + list(gz["class_tags"]):
        form, L, Cn, D, wl, maxV, nClass = (int(x) for x in gz[tag + "__cfg"])
        F = gz[tag + "__feature"].shape[1]
        cfg = cfg_of(form, L, Cn, F, D, wl, maxV)
        n = lib.gf_smp_classifier_config_param_count(C.byref(cfg), nClass) if nClass else lib.gf_smp_config_param_count(C.byref(cfg))
        assert n == gz[tag + "__grads"].size, tag
        assert n == sum(sz for _, sz in smp2d_blocks(form, Cn, F * (D + 1), L, maxV, nClass)), tag
        assert n == smp2d_ref.param_count(form, Cn, F * (D + 1), L, maxV, nClass), tag


def test_invalid_combinations_count_zero_and_others_count_what_they_counted(lib):
    """steerable_2d needs first_order = 0, max_receptive_field == max_nVertices <= 4096 and no contraction family, custom product or
    tower; there is no form 3; a zero tail leaves SMP_theta, SMP_1D and SMP_omega where they were."""
    from graphflow_amd.smp import SMP1D, SMPConfig, SMPTheta
    for form in (1, 2):
        ok = SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 0, 12, form)
        assert lib.gf_smp_config_param_count(C.byref(ok)) > 0
        assert lib.gf_smp_classifier_config_param_count(C.byref(ok), 5) > 0
        for bad in (SMPConfig(2, 4, 4, 1, 6, 1, 0, 0, 0, 0, 12, form), SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 0, 6, form),
                    SMPConfig(2, 4, 4, 1, 12, 1, 18, 0, 0, 0, 12, form), SMPConfig(2, 4, 4, 1, 12, 1, 0, 1, 0, 0, 12, form),
                    SMPConfig(2, 4, 4, 0, 12, 1, 0, 0, 1, 0, 12, form), SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 1, 12, form),
                    SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 2, 12, form), SMPConfig(2, 4, 4, 1, 5000, 1, 0, 0, 0, 0, 5000, form)):
            assert lib.gf_smp_config_param_count(C.byref(bad)) == 0, form
            assert lib.gf_smp_classifier_config_param_count(C.byref(bad), 5) == 0, form
    assert lib.gf_smp_config_param_count(C.byref(SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 0, 12, 3))) == 0   # no such form
    assert lib.gf_smp_config_param_count(C.byref(SMPConfig(20, 4, 4, 1, 12, 1, 0, 0, 0, 0, 12, 2))) == 0   # 4 << 20 channels
    theta = SMPTheta.config(10, 6, 2, 8, 4, 1, True)
    assert lib.gf_smp_config_param_count(C.byref(theta)) == 8 * 4 * 2 + 2 * (10 * (2 + 8) + 2 * 8 * 8) + 8
    one_d = SMP1D.config(1, 12, 2, 4, 4, 1, True)
    assert lib.gf_smp_config_param_count(C.byref(one_d)) == 4 * 4 * 2 + 2 * 12 * (2 + 4) + 4
    omega = SMPConfig(2, 8, 4, 1, 6, 1, 0, 0, 0, 0, 0, 0)
    assert lib.gf_smp_config_param_count(C.byref(omega)) == 8 * 4 * 2 + 2 * (18 * 64 + 8) + 8


def test_uniform_init_reproduces_weights_initialization(lib, gz):
    """gf_smp_uniform_init_host / gf_smp_classifier_uniform_init_host after srand(seed) against the weights the four real constructors
    drew, block by block: every block has its own divisor (10 x its size), so a block boundary in the wrong place shows -- lambda1_s,
    lambda2_s, b_s and scalar_l are blocks of their own, W [nClass][C_L] one."""
    for kind in (1, 2, 3, 4):
        form, L, Cn, D, wl, maxV, nClass, seed = (int(x) for x in gz["init_k%d__cfg" % kind])
        cfg = cfg_of(form, L, Cn, 4, D, wl, maxV)
        ref = gz["init_k%d__params0" % kind]
        out = np.zeros(ref.size, dtype=np.float32)
        C.CDLL(None).srand(seed)
        ptr = out.ctypes.data_as(C.POINTER(C.c_float))
        st = lib.gf_smp_classifier_uniform_init_host(C.byref(cfg), nClass, ptr) if nClass else lib.gf_smp_uniform_init_host(C.byref(cfg), ptr)
        assert st == 0, kind
        off = 0
        for name, n in smp2d_blocks(form, Cn, 4 * (D + 1), L, maxV, nClass):
            assert np.array_equal(out[off:off + n], ref[off:off + n].astype(np.float32)), (kind, name)
            off += n
        assert off == ref.size


def test_receptive_fields_match_the_reference(lib, gz):
    """phi_l(v) of every golden case from gf_smp_prepare_molecule_host: the uncapped union over the vertices within one hop, both WL
    settings; a capped configuration of these forms is refused."""
    for tag in gz["tags"]:
        form, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        adj = np.ascontiguousarray(gz[tag + "__adj"], dtype=np.int32)
        feat = np.ascontiguousarray(gz[tag + "__feature"], dtype=np.float64)
        cfg = cfg_of(form, L, Cn, feat.shape[1], D, wl, maxV)
        phi = np.zeros((L + 1, len(adj), maxV + 1), dtype=np.int32)
        st = lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)),
                                              feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None)
        assert st == 0, tag
        assert np.array_equal(phi, gz[tag + "__phi"]), tag
    cfg.max_receptive_field = maxV - 1
    assert lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)),
                                            feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None) != 0


def test_ch4_has_four_and_five_vertices_of_one_size(gz):
    """The fixture is what tells the multiplicities apart: the four hydrogens share a field size at level 1, all five atoms at level 2."""
    phi = gz["f1_CH4_c5__phi"]
    assert list(phi[1, :, 0]) == [5, 2, 2, 2, 2] and list(phi[2, :, 0]) == [5] * 5


def test_multiplicity_rules_follow_from_the_executor():
    """j for one shared op between vertex and lambda (SMP_2D_ver4), j (j + 1) / 2 for two (SMP_2D): the closed forms against a run of the
    accumulation itself."""
    for form in (1, 2):
        for k in (1, 2, 4, 7):
            assert smp2d_ref.executor_multiplicity(form, k) == [smp2d_ref.multiplicity(form, j) for j in range(1, k + 1)]
    assert [smp2d_ref.multiplicity(1, j) for j in (1, 2, 3, 4)] == [1, 3, 6, 10]


def test_smp2d_ref_matches_the_real_classes(gz):
    """graph feature, prediction, loss and every parameter block of every regression case at 1e-9 -- CH4's lambda blocks included, which
    neither multiplicity 1 nor the other form's rule would pass; the unused sizes' blocks are zero in both."""
    for tag in gz["tags"]:
        form, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        r = ref_of(gz, tag)
        assert rel_err(r["graph_feature"], gz[tag + "__graph_feature"]) <= TOL_REF, tag
        assert rel_err([r["predict"]], gz[tag + "__predict"]) <= TOL_REF, tag
        assert rel_err([r["loss"]], gz[tag + "__loss"]) <= TOL_REF, tag
        blocks = smp2d_blocks(form, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV)
        worst = blockwise(r["grads"], gz[tag + "__grads"], blocks)
        assert worst[0] <= TOL_REF, (tag, worst)
        used = {int(s) for s in gz[tag + "__phi"][1:, :, 0].ravel()}
        off = 0
        for name, n in blocks:
            if name[:3] in ("lam", "b_") and int(name.rsplit("_", 1)[1]) > max(used):
                assert not gz[tag + "__grads"][off:off + n].any() and not r["grads"][off:off + n].any(), (tag, name)
            off += n


def test_smp2d_ref_activations_and_adjacencies(gz):
    """the level activations ([s, s, C_l]) and the reduced adjacencies of CH4 -- SMP_2D_ver4's with its unit diagonal and row sums of 1"""
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
    assert seen == 4


def test_ch4_lambda_gradients_tell_the_rules_apart(gz):
    """On CH4 the real class's dlambda of the shared size is NOT what multiplicity 1 or the other form's rule gives."""
    for form in (1, 2):
        tag = "f%d_CH4_c5" % form
        _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        blocks = smp2d_blocks(form, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV)
        off = {name: o for (name, _), o in zip(blocks, np.cumsum([0] + [n for _, n in blocks])[:-1])}
        pick = lambda g: np.concatenate([g[off["lam1_2_5"]:off["lam1_2_5"] + Cn], g[off["lam2_1_2"]:off["lam2_1_2"] + Cn]])   # noqa: E731
        real = pick(gz[tag + "__grads"])
        saved = smp2d_ref.multiplicity
        try:
            for rule in (lambda f, j: 1, lambda f, j: saved(3 - f, j)):
                smp2d_ref.multiplicity = rule
                assert rel_err(pick(ref_of(gz, tag)["grads"]), real) > 1e-3, form
        finally:
            smp2d_ref.multiplicity = saved


def test_smp2d_ref_matches_the_real_classifiers(gz):
    for tag in gz["class_tags"]:
        form, L, Cn, D, wl, maxV, nClass = (int(x) for x in gz[tag + "__cfg"])
        r = ref_of(gz, tag, nClass)
        for k in ("graph_feature", "scores", "probability"):
            assert rel_err(r[k], gz[tag + "__" + k]) <= TOL_REF, (tag, k)
        assert rel_err([r["loss"]], gz[tag + "__loss"]) <= TOL_REF, tag
        assert r["label"] == int(gz[tag + "__label"][0]), tag
        blocks = smp2d_blocks(form, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV, nClass)
        worst = blockwise(r["grads"], gz[tag + "__grads"], blocks)
        assert worst[0] <= TOL_REF, (tag, worst)
