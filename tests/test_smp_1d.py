"""CPU suite for SMP_1D, SMP_1D_ver2, SMP_1D_ver3 and their classifiers (gf_smp_config.first_order = 2, 3, 4): the parameter layout, the
initial weights, the receptive fields of the host preparation and the fp64 restatement tests/smp1d_ref.py, all against the real classes'
numbers in tests/golden/smp_1d.npz (tests/golden/make_smp1d_golden.py).  Host code only: no device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import smp1d_ref
from make_smp1d_golden import smp1d_blocks
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_REF = 1e-9   # fp64 restatement against the fp64 reference: summation order only


@pytest.fixture(scope="module")
def lib():
    from graphflow_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gz():
    with np.load(os.path.join(HERE, "golden", "smp_1d.npz")) as z:
        return {k: z[k] for k in z.files}


def cfg_of(version, L, Cn, F, D, wl, maxV):
    from graphflow_amd.smp import SMP1D
    return SMP1D.config(version, maxV, L, Cn, F, D, bool(wl))


def blockwise(x, ref, blocks):
    off, worst = 0, (0.0, "")
    for name, n in blocks:
        worst = max(worst, (rel_err(x[off:off + n], ref[off:off + n]), name))
        off += n
    assert off == ref.size
    return worst


def test_parameter_count_matches_the_reference(lib, gz):
    """gf_smp_config_param_count / gf_smp_classifier_config_param_count against the length of the real class's gradient vector and against
    the sum of the registration-order blocks, for every golden case of the three forms and the two classifiers."""
    for tag in list(gz["tags"]) + list(gz["class_tags"]):
        version, L, Cn, D, wl, maxV, nClass = (int(x) for x in gz[tag + "__cfg"])
        F = gz[tag + "__feature"].shape[1]
        cfg = cfg_of(version, L, Cn, F, D, wl, maxV)
        n = lib.gf_smp_classifier_config_param_count(C.byref(cfg), nClass) if nClass else lib.gf_smp_config_param_count(C.byref(cfg))
        assert n == gz[tag + "__grads"].size, tag
        assert n == sum(sz for _, sz in smp1d_blocks(version, Cn, F * (D + 1), L, maxV, nClass)), tag
    # no SMP_1D_ver2_classification exists in the reference: the count follows the block list
    cfg = cfg_of(2, 2, 3, 4, 1, 1, 6)
    assert lib.gf_smp_classifier_config_param_count(C.byref(cfg), 5) == sum(sz for _, sz in smp1d_blocks(2, 3, 8, 2, 6, 5))


def test_other_configurations_count_what_they_counted(lib):
    """first_order = 1 (SMP_theta) and a zero-initialised tail are untouched; forms 2 to 4 need max_receptive_field == max_nVertices and no
    contraction family, custom product or tower; a first_order = 1 classifier still counts 0."""
    from graphflow_amd.smp import SMPConfig, SMPTheta
    theta = SMPTheta.config(10, 6, 2, 8, 4, 1, True)
    per = 10 * (2 + 8) + 2 * 8 * 8
    assert lib.gf_smp_config_param_count(C.byref(theta)) == 8 * 4 * 2 + 2 * per + 8
    assert lib.gf_smp_classifier_config_param_count(C.byref(theta), 5) == 0
    omega = SMPConfig(2, 8, 4, 1, 6, 1, 0, 0, 0, 0, 0)
    assert lib.gf_smp_config_param_count(C.byref(omega)) == 8 * 4 * 2 + 2 * (18 * 64 + 8) + 8
    for form in (2, 3, 4):
        ok = SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, form, 12)
        assert lib.gf_smp_config_param_count(C.byref(ok)) > 0
        for bad in (SMPConfig(2, 4, 4, 1, 6, 1, 0, 0, 0, form, 12), SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, form, 6),
                    SMPConfig(2, 4, 4, 1, 12, 1, 18, 0, 0, form, 12), SMPConfig(2, 4, 4, 1, 12, 1, 0, 1, 0, form, 12),
                    SMPConfig(2, 4, 4, 0, 12, 1, 0, 0, 1, form, 12)):
            assert lib.gf_smp_config_param_count(C.byref(bad)) == 0, form
            assert lib.gf_smp_classifier_config_param_count(C.byref(bad), 5) == 0, form
    assert lib.gf_smp_config_param_count(C.byref(SMPConfig(2, 4, 4, 1, 12, 1, 0, 0, 0, 5, 12))) == 0   # no such form


def test_uniform_init_reproduces_weights_initialization(lib, gz):
    """gf_smp_uniform_init_host / gf_smp_classifier_uniform_init_host after srand(seed) against the weights the five real constructors
    drew, block by block: every block has its own divisor (10 x its size), so a block boundary in the wrong place shows -- K_eye and K_one
    are two blocks, W [nClass][C_L] one."""
    for kind in (1, 2, 3, 4, 5):
        version, L, Cn, D, wl, maxV, nClass, seed = (int(x) for x in gz["init_k%d__cfg" % kind])
        cfg = cfg_of(version, L, Cn, 4, D, wl, maxV)
        ref = gz["init_k%d__params0" % kind]
        out = np.zeros(ref.size, dtype=np.float32)
        C.CDLL(None).srand(seed)
        ptr = out.ctypes.data_as(C.POINTER(C.c_float))
        st = lib.gf_smp_classifier_uniform_init_host(C.byref(cfg), nClass, ptr) if nClass else lib.gf_smp_uniform_init_host(C.byref(cfg), ptr)
        assert st == 0, kind
        off = 0
        for name, n in smp1d_blocks(version, Cn, 4 * (D + 1), L, maxV, nClass):
            assert np.array_equal(out[off:off + n], ref[off:off + n].astype(np.float32)), (kind, name)
            off += n
        assert off == ref.size


def test_receptive_fields_match_the_reference(lib, gz):
    """phi_l(v) of every golden case from gf_smp_prepare_molecule_host: the uncapped union over the vertices within one hop, both WL
    settings; a capped configuration of these forms is refused."""
    for tag in gz["tags"]:
        version, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        adj = np.ascontiguousarray(gz[tag + "__adj"], dtype=np.int32)
        feat = np.ascontiguousarray(gz[tag + "__feature"], dtype=np.float64)
        cfg = cfg_of(version, L, Cn, feat.shape[1], D, wl, maxV)
        phi = np.zeros((L + 1, len(adj), maxV + 1), dtype=np.int32)
        st = lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)),
                                              feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None)
        assert st == 0, tag
        assert np.array_equal(phi, gz[tag + "__phi"]), tag
    cfg.max_receptive_field = maxV - 1
    assert lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)),
                                            feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None) != 0


def test_cycle_case_has_four_vertices_of_one_size(gz):
    """The fixture is what tells the multiplicities apart: at every level >= 1 the four vertices of the ring share one field size."""
    phi = gz["v1_cycle4_c4__phi"]
    assert list(phi[1, :, 0]) == [3] * 4 and list(phi[2, :, 0]) == [4] * 4


def test_multiplicity_rules_follow_from_the_executor():
    """j for one shared op between vertex and lambda (ver2, ver3), j (j + 1) (j + 2) / 6 for three (SMP_1D): the closed forms against a run
    of the accumulation itself."""
    for version in (1, 2, 3):
        for k in (1, 2, 4, 7):
            assert smp1d_ref.executor_multiplicity(version, k) == [smp1d_ref.multiplicity(version, j) for j in range(1, k + 1)]
    assert [smp1d_ref.multiplicity(1, j) for j in (1, 2, 3, 4)] == [1, 4, 10, 20]


def test_smp1d_ref_matches_the_real_classes(gz):
    """graph feature, prediction, loss and every parameter block of every regression case at 1e-9 -- the lambda blocks of the 4-cycle
    included, which neither multiplicity 1 nor the other form's rule would pass."""
    for tag in gz["tags"]:
        version, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        r = smp1d_ref.run(version, gz[tag + "__adj"], gz[tag + "__feature"], float(gz[tag + "__target"][0]), gz[tag + "__params"], L, Cn, D, maxV,
                          smp1d_ref.fields_of(gz[tag + "__phi"]))
        assert rel_err(r["graph_feature"], gz[tag + "__graph_feature"]) <= TOL_REF, tag
        assert rel_err([r["predict"]], gz[tag + "__predict"]) <= TOL_REF, tag
        assert rel_err([r["loss"]], gz[tag + "__loss"]) <= TOL_REF, tag
        blocks = smp1d_blocks(version, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV)
        worst = blockwise(r["grads"], gz[tag + "__grads"], blocks)
        assert worst[0] <= TOL_REF, (tag, worst)


def test_cycle_lambda_gradients_tell_the_rules_apart(gz):
    """On the 4-cycle the real class's dlambda of the shared size is NOT what multiplicity 1 or the other form's rule gives."""
    for version in (1, 2, 3):
        tag = "v%d_cycle4_c4" % version
        _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        blocks = smp1d_blocks(version, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV)
        off = {name: o for (name, _), o in zip(blocks, np.cumsum([0] + [n for _, n in blocks])[:-1])}
        real = np.array([gz[tag + "__grads"][off["lam1_2_4"]], gz[tag + "__grads"][off["lam2_2_4"]]])
        saved = smp1d_ref.multiplicity
        try:
            for rule in (lambda v, j: 1, lambda v, j: saved(1 if v != 1 else 2, j)):
                smp1d_ref.multiplicity = rule
                r = smp1d_ref.run(version, gz[tag + "__adj"], gz[tag + "__feature"], float(gz[tag + "__target"][0]), gz[tag + "__params"], L, Cn, D,
                                  maxV, smp1d_ref.fields_of(gz[tag + "__phi"]))
                other = np.array([r["grads"][off["lam1_2_4"]], r["grads"][off["lam2_2_4"]]])
                assert rel_err(other, real) > 1e-3, version
        finally:
            smp1d_ref.multiplicity = saved


def test_smp1d_ref_matches_the_real_classifiers(gz):
    for tag in gz["class_tags"]:
        version, L, Cn, D, wl, maxV, nClass = (int(x) for x in gz[tag + "__cfg"])
        r = smp1d_ref.run(version, gz[tag + "__adj"], gz[tag + "__feature"], float(gz[tag + "__target"][0]), gz[tag + "__params"], L, Cn, D, maxV,
                          smp1d_ref.fields_of(gz[tag + "__phi"]), nClass)
        for k in ("graph_feature", "scores", "probability"):
            assert rel_err(r[k], gz[tag + "__" + k]) <= TOL_REF, (tag, k)
        assert rel_err([r["loss"]], gz[tag + "__loss"]) <= TOL_REF, tag
        assert r["label"] == int(gz[tag + "__label"][0]), tag
        blocks = smp1d_blocks(version, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV, nClass)
        worst = blockwise(r["grads"], gz[tag + "__grads"], blocks)
        assert worst[0] <= TOL_REF, (tag, worst)
