"""CPU suite for CCN_1D (GraphFlow/CCN_1D.h): the fp64 restatement tests/ccn1d_ref.py, the width and head rules, the parameter layout
of gf_smp_model_config_param_count, the receptive fields of the host preparation and the refusals, all against the real class's numbers
in tests/golden/ccn_1d.npz / ccn_1d_demo.npz (tests/golden/make_ccn1d_golden.py).  Host code only: no device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import ccn1d_ref
from make_ccn1d_golden import channels, head_widths, model_blocks
from theta_ref import fields_of
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_REF = 1e-12   # fp64 restatement against the fp64 class: summation order only


@pytest.fixture(scope="module")
def lib():
    from graphflow_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    """{tag: {field: array}} of both golden files"""
    out = {}
    for name in ("ccn_1d.npz", "ccn_1d_demo.npz"):
        with np.load(os.path.join(HERE, "golden", name)) as z:
            for tag in z["tags"]:
                p = "ccn_%s__" % tag
                out[str(tag)] = {k[len(p):]: z[k] for k in z.files if k.startswith(p)}
    return out


def settings(c):
    maxV1, maxV2, cap, L, Cn = (int(x) for x in c["cfg"])
    return maxV1, maxV2, cap, L, Cn, float(c["decay"][0]), [c["feature"].shape[1], c["feature2"].shape[1]]


def restated(c, **kw):
    maxV1, maxV2, cap, L, Cn, decay, _ = settings(c)
    return ccn1d_ref.run([(c["adj"], c["feature"]), (c["adj2"], c["feature2"])], float(c["target"][0]), c["params"], L, Cn, [maxV1, maxV2],
                         decay, [fields_of(c["phi"]), fields_of(c["phi2"])], **kw)


def blockwise(x, ref, blocks):
    """the largest rel_err over the parameter blocks, and the block it is in"""
    off, worst = 0, (0.0, "")
    for name, n in blocks:
        worst = max(worst, (rel_err(x[off:off + n], ref[off:off + n]), name))
        off += n
    assert off == ref.size
    return worst


def test_the_goldens_hold_the_cases_the_model_needs(cases):
    """The asymmetric pair has the widths 27, 22, 18, 16 (lane vectors of 1, 2 and 4 floats), its cap bites on both graphs, and its rows
    are not unit rows; decay 1.0 keeps the width; the star's centre has children outside its field; one input has negative entries."""
    assert set(cases) == {"toy_L7", "toy_L3", "asym_c27", "decay1", "star5_cap4", "negative"}
    a = cases["asym_c27"]
    assert channels(27, 3, 0.8) == [27, 22, 18, 16] and tuple(a["cfg"]) == (12, 8, 5, 3, 27)
    assert a["feature"].shape == (12, 5) and a["feature2"].shape == (8, 3)
    assert a["phi"][3, :, 0].max() == 5 and a["phi2"][3, :, 0].max() == 5 and a["phi"][1, :, 0].min() < 5
    assert (np.abs(np.abs(a["feature"]).sum(1) - 1) > 0.1).sum() >= 8 and (np.abs(np.abs(a["feature2"]).sum(1) - 1) > 0.1).sum() >= 4
    assert channels(16, 7, 0.5) == [16] * 8 and head_widths(16, 7, 0.5) == (256, 128, 64)
    assert float(cases["decay1"]["decay"][0]) == 1.0 and head_widths(16, 1, 1.0) == (64, 64, 64)
    phi = cases["star5_cap4"]["phi"]
    assert phi[1, 0, 0] == 1 and list(phi[1, 0, 1:2]) == [0] and all(phi[1, v, 0] == 2 for v in range(1, 6))
    assert cases["negative"]["feature"].min() < 0
    for c in cases.values():
        assert float(c["margin"][0]) >= 1e-3


def test_restatement_matches_the_real_class(cases):
    for tag, c in cases.items():
        maxV1, maxV2, cap, L, Cn, decay, F = settings(c)
        r = restated(c)
        e = blockwise(r["grads"], c["grads"], model_blocks(Cn, L, F, [maxV1, maxV2], decay))
        print(tag, rel_err([r["predict"]], c["predict"]), rel_err(r["graph_feature"], c["graph_feature"]), rel_err([r["loss"]], c["loss"]), e)
        assert rel_err([r["predict"]], c["predict"]) <= TOL_REF, tag
        assert rel_err(r["graph_feature"], c["graph_feature"]) <= TOL_REF, tag
        assert rel_err([r["loss"]], c["loss"]) <= TOL_REF, tag
        assert e[0] <= TOL_REF, (tag, e)


def test_a_wrong_multiplicity_fails_the_toy_case(cases):
    """dlambda with the plain derivative (1 instead of j): CH4's four hydrogens share a field size, so the class counts them 1, 2, 3, 4
    times.  Every block but lambda's stays right."""
    c = cases["toy_L3"]
    maxV1, maxV2, cap, L, Cn, decay, F = settings(c)
    r = restated(c, multiplicity="one")
    assert rel_err([r["predict"]], c["predict"]) <= TOL_REF
    err, name = blockwise(r["grads"], c["grads"], model_blocks(Cn, L, F, [maxV1, maxV2], decay))
    assert err > 1e-3 and "lam" in name, (err, name)


def test_halving_instead_of_the_decay_fails_the_asymmetric_case(cases):
    """27 -> 13 -> 6 -> 3 is not the class's 27 -> 22 -> 18 -> 16: not even the parameter count survives; nor does it at the demo's
    settings, where halving would leave 16 -> 8 -> 4 -> 2."""
    for tag in ("asym_c27", "toy_L3"):
        c = cases[tag]
        maxV1, maxV2, cap, L, Cn, decay, F = settings(c)
        assert ccn1d_ref.param_count(Cn, L, F, [maxV1, maxV2], decay) == c["grads"].size
        assert ccn1d_ref.param_count(Cn, L, F, [maxV1, maxV2], decay, halving=True) != c["grads"].size
        with pytest.raises((AssertionError, ValueError)):
            restated(c, halving=True)


def test_parameter_counts_match_the_real_class(lib, cases):
    """the width and head rules, as the restatement, the generator's block list and gf_smp_model_config_param_count have them, against
    the length of the real class's gradient vector"""
    from graphflow_amd.smp import CCN1D
    for tag, c in cases.items():
        maxV1, maxV2, cap, L, Cn, decay, F = settings(c)
        n = c["grads"].size
        assert sum(sz for _, sz in model_blocks(Cn, L, F, [maxV1, maxV2], decay)) == n, tag
        assert ccn1d_ref.param_count(Cn, L, F, [maxV1, maxV2], decay) == n, tag
        cfg = CCN1D.config(maxV1, maxV2, cap, L, Cn, F[0], F[1], decay)
        assert lib.gf_smp_model_config_param_count(C.byref(cfg)) == n, tag


def test_refused_configurations_count_zero(lib):
    from graphflow_amd.smp import CCN1D, SMPModel
    count = lambda cfg: lib.gf_smp_model_config_param_count(C.byref(cfg))  # noqa: E731
    assert count(CCN1D.config(10, 10, 6, 3, 16, 4, 4, 0.5)) > 0
    assert count(CCN1D.config(10, 10, 6, 3, 15, 4, 4, 0.5)) == 0       # nChanels < 16
    assert count(CCN1D.config(10, 10, 6, 3, 16, 4, 4, 0.0)) == 0       # decay 0
    assert count(CCN1D.config(10, 10, 6, 3, 16, 4, 4, 1.5)) == 0       # decay > 1
    assert count(CCN1D.config(10, 10, 6, 3, 16, 4, 4, -0.5)) == 0
    assert count(CCN1D.config(10, 10, 6, 3, 16, 4, 4, float("nan"))) == 0
    assert count(CCN1D.config(10, 5, 6, 3, 16, 4, 4, 0.5)) == 0        # the cap above a vertex limit
    assert count(SMPModel.config(3, 16, 6, [4], first_order=True, max_nVertices=10, ccn_1d=True, nChanels_decay=0.5)) == 0       # one tower
    assert count(SMPModel.config(3, 16, 6, [4, 4], max_nVertices=[10, 10], ccn_1d=True, nChanels_decay=0.5)) == 0                # not first order
    assert count(SMPModel.config(3, 16, 6, [4, 4], nContractions=4, ccn_1d=True, nChanels_decay=0.5)) == 0
    kept = CCN1D.config(10, 10, 6, 3, 16, 4, 4, 0.5)
    kept.nKept = 3
    assert count(kept) == 0
    assert count(CCN1D.config(10, 10, 6, 3, 16, 4, 0, 0.5)) == 0        # a tower without features
    assert lib.gf_smp_model_config_param_count(None) == 0


def test_a_zero_tail_counts_what_the_theta_towers_always_did(lib):
    """ccn_1d = 0: halving widths and the nTotal / 2 heads, whatever nChanels_decay holds; against the real SMP_theta_physics /
    SMP_theta_pairgraphs gradient vectors of tests/golden/smp_theta_physics.npz"""
    from graphflow_amd.smp import SMPModel
    with np.load(os.path.join(HERE, "golden", "smp_theta_physics.npz")) as pz:
        for tag in pz["tags"]:
            p = "tphys_%s__" % tag
            towers, L, Cn, cap, maxV1, maxV2 = (int(x) for x in pz[p + "cfg"])
            F = [pz[p + "feature"].shape[1]] + ([pz[p + "feature2"].shape[1]] if towers == 2 else [])
            cfg = SMPModel.config(L, Cn, cap, F, first_order=True, max_nVertices=[maxV1, maxV2][:towers])
            assert cfg.ccn_1d == 0 and cfg.nChanels_decay == 0.0
            assert lib.gf_smp_model_config_param_count(C.byref(cfg)) == pz[p + "grads"].size, tag
            cfg.nChanels_decay = 0.8   # (not read without the flag)
            assert lib.gf_smp_model_config_param_count(C.byref(cfg)) == pz[p + "grads"].size, tag
    # SMP_omega_pairgraphs at 8 channels, two levels: H x 2, (K [18 C', C], b) per level and tower, 28 -> 14 -> 10 -> 1
    omega = SMPModel.config(2, 8, 6, [4, 5])
    towers = 8 * 4 + 8 * 5 + 2 * (18 * 8 * 4 + 4) + 2 * (18 * 4 * 2 + 2)
    assert lib.gf_smp_model_config_param_count(C.byref(omega)) == towers + 14 * 28 + 10 * 14 + 10


def test_receptive_fields_match_the_real_class(lib, cases):
    """phi_l(v) of both towers of every case from gf_smp_prepare_molecule_host (a first-order physics tower): the GPU suite builds the
    fields of its batches this way"""
    from graphflow_amd.smp import SMPTheta
    for tag, c in cases.items():
        maxV1, maxV2, cap, L, Cn, decay, F = settings(c)
        for sfx, maxV in (("", maxV1), ("2", maxV2)):
            adj = np.ascontiguousarray(c["adj" + sfx], dtype=np.int32)
            feat = np.ascontiguousarray(c["feature" + sfx], dtype=np.float64)
            cfg = SMPTheta.config(maxV, cap, L, Cn, feat.shape[1], 0, False)
            cfg.physics = 1
            phi = np.zeros((L + 1, len(adj), cap + 1), dtype=np.int32)
            st = lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)),
                                                  feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None)
            assert st == 0
            assert np.array_equal(phi, c["phi" + sfx]), (tag, sfx)
