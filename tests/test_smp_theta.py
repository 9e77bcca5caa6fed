"""CPU suite for the first-order models (SMP_theta, SMP_theta_physics, SMP_theta_pairgraphs): the parameter layout, the initial weights,
the receptive fields of the host preparation and the fp64 restatement tests/theta_ref.py, all against the real classes' numbers in
tests/golden/smp_theta.npz / smp_theta_physics.npz (tests/golden/make_theta_golden.py).  Host code only: no device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import theta_ref
from make_theta_golden import model_blocks, theta_blocks
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_REF = 1e-9   # fp64 restatement against the fp64 reference: summation order only


@pytest.fixture(scope="module")
def lib():
    from graphflow_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def gz():
    with np.load(os.path.join(HERE, "golden", "smp_theta.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def pz():
    with np.load(os.path.join(HERE, "golden", "smp_theta_physics.npz")) as z:
        return {k: z[k] for k in z.files}


def theta_cfg(L, Cn, F, D, wl, cap, maxV):
    from graphflow_amd.smp import SMPTheta
    return SMPTheta.config(maxV, cap, L, Cn, F, D, bool(wl))


def host_fields(lib, cfg, adj, feat):
    V = len(adj)
    cap = cfg.max_receptive_field
    phi = np.zeros((cfg.nLevels + 1, V, cap + 1), dtype=np.int32)
    adj = np.ascontiguousarray(adj, dtype=np.int32)
    feat = np.ascontiguousarray(feat, dtype=np.float64)
    st = lib.gf_smp_prepare_molecule_host(C.byref(cfg), V, adj.ctypes.data_as(C.POINTER(C.c_int)), feat.ctypes.data_as(C.POINTER(C.c_double)),
                                          phi.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert st == 0
    return phi


def test_parameter_count_matches_the_reference(lib, gz):
    """gf_smp_config_param_count against the length of the real class's gradient vector, and against the sum of the registration-order
    blocks; a configuration gf_smp_create would refuse counts 0."""
    for tag in gz["tags"]:
        p = "theta_%s__" % tag
        L, Cn, D, wl, cap, maxV = (int(x) for x in gz[p + "cfg"])
        F = gz[p + "feature"].shape[1]
        cfg = theta_cfg(L, Cn, F, D, wl, cap, maxV)
        n = lib.gf_smp_config_param_count(C.byref(cfg))
        assert n == gz[p + "grads"].size, tag
        assert n == sum(sz for _, sz in theta_blocks(Cn, F * (D + 1), L, maxV)), tag
    bad = theta_cfg(2, 8, 4, 1, 1, 6, 4)   # max_nVertices < max_receptive_field
    assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
    # a second-order configuration still counts what it always did: H, (K_l [18 C, C], b_l) x L, W
    from graphflow_amd.smp import SMPConfig
    omega = SMPConfig(2, 8, 4, 1, 6, 1, 0, 0, 0, 0, 0)
    assert lib.gf_smp_config_param_count(C.byref(omega)) == 8 * 4 * 2 + 2 * (18 * 64 + 8) + 8


def test_uniform_init_reproduces_weights_initialization(lib, gz):
    """gf_smp_uniform_init_host after srand(seed) against the weights the real constructor drew, block by block: every block has its own
    divisor (10 x its size), so a block boundary in the wrong place shows."""
    L, Cn, D, cap, maxV, seed, _ = (int(x) for x in gz["train__cfg"])
    cfg = theta_cfg(L, Cn, 4, D, 1, cap, maxV)
    ref = gz["train__params0"]
    assert lib.gf_smp_config_param_count(C.byref(cfg)) == ref.size
    out = np.zeros(ref.size, dtype=np.float32)
    C.CDLL(None).srand(seed)
    assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == 0
    off = 0
    for name, n in theta_blocks(Cn, 4 * (D + 1), L, maxV):
        assert np.array_equal(out[off:off + n], ref[off:off + n].astype(np.float32)), name
        off += n
    assert off == ref.size


def test_receptive_fields_match_the_reference(lib, gz, pz):
    """phi_l(v) of every golden case from gf_smp_prepare_molecule_host (capped star, capped 12-vertex molecule, both WL settings, towers)."""
    for tag in gz["tags"]:
        p = "theta_%s__" % tag
        L, Cn, D, wl, cap, maxV = (int(x) for x in gz[p + "cfg"])
        cfg = theta_cfg(L, Cn, gz[p + "feature"].shape[1], D, wl, cap, maxV)
        assert np.array_equal(host_fields(lib, cfg, gz[p + "adj"], gz[p + "feature"]), gz[p + "phi"]), tag
    for tag in pz["tags"]:
        p = "tphys_%s__" % tag
        towers, L, Cn, cap, maxV1, maxV2 = (int(x) for x in pz[p + "cfg"])
        for sfx, maxV in (("", maxV1), ("2", maxV2))[:towers]:
            cfg = theta_cfg(L, Cn, pz[p + "feature" + sfx].shape[1], 0, 0, cap, maxV)
            cfg.physics = 1
            assert np.array_equal(host_fields(lib, cfg, pz[p + "adj" + sfx], pz[p + "feature" + sfx]), pz[p + "phi" + sfx]), tag


def test_star_case_has_children_outside_the_field(gz):
    """The fixture is what the issue asks for: at level 1 the cap drops the centre's whole hop-1 shell, so its children lie outside
    its field, and the centre and the leaves have different field sizes."""
    phi = gz["theta_star5_cap4__phi"]
    assert phi[1, 0, 0] == 1 and list(phi[1, 0, 1:2]) == [0]
    assert all(phi[1, v, 0] == 2 for v in range(1, 6))


def blockwise(x, ref, blocks):
    off, worst = 0, 0.0
    for _, n in blocks:
        worst = max(worst, rel_err(x[off:off + n], ref[off:off + n]))
        off += n
    assert off == ref.size
    return worst


def test_theta_ref_matches_the_real_smp_theta(gz):
    for tag in gz["tags"]:
        p = "theta_%s__" % tag
        L, Cn, D, wl, cap, maxV = (int(x) for x in gz[p + "cfg"])
        r = theta_ref.run(gz[p + "adj"], gz[p + "feature"], float(gz[p + "target"][0]), gz[p + "params"], L, Cn, D, maxV,
                          theta_ref.fields_of(gz[p + "phi"]))
        assert rel_err(r["graph_feature"], gz[p + "graph_feature"]) <= TOL_REF, tag
        assert rel_err([r["predict"]], gz[p + "predict"]) <= TOL_REF, tag
        assert rel_err([r["loss"]], gz[p + "loss"]) <= TOL_REF, tag
        blocks = theta_blocks(Cn, gz[p + "feature"].shape[1] * (D + 1), L, maxV)
        assert blockwise(r["grads"], gz[p + "grads"], blocks) <= TOL_REF, tag


def test_theta_ref_matches_the_real_towers(pz):
    for tag in pz["tags"]:
        p = "tphys_%s__" % tag
        towers, L, Cn, cap, maxV1, maxV2 = (int(x) for x in pz[p + "cfg"])
        graphs = [(pz[p + "adj"], pz[p + "feature"])] + ([(pz[p + "adj2"], pz[p + "feature2"])] if towers == 2 else [])
        phis = [theta_ref.fields_of(pz[p + "phi"])] + ([theta_ref.fields_of(pz[p + "phi2"])] if towers == 2 else [])
        r = theta_ref.run_model(graphs, float(pz[p + "target"][0]), pz[p + "params"], L, Cn, [maxV1, maxV2][:towers], phis)
        assert rel_err(r["graph_feature"], pz[p + "graph_feature"]) <= TOL_REF, tag
        assert rel_err([r["predict"]], pz[p + "predict"]) <= TOL_REF, tag
        blocks = model_blocks(towers, Cn, L, [g[1].shape[1] for g in graphs], [maxV1, maxV2])
        assert blockwise(r["grads"], pz[p + "grads"], blocks) <= TOL_REF, tag
