"""CPU checks for SMP_gamma_physics / SMP_gamma_pairgraphs: the goldens of the real classes (tests/golden/smp_gamma_physics.npz)
follow the [4 C_{l-1}][C_l] parameter layout, and the host preparation of a physics = 1, nContractions = 4 configuration gives the
reference's receptive fields list for list."""
import ctypes as C
import os

import numpy as np

from util import golden_cases

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "smp_gamma_physics.npz")


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def channels(Cn, L):
    return [max(1, Cn >> l) for l in range(L + 1)]


def model_params(towers, Cn, L, feats, nK=4):
    c = channels(Cn, L)
    n = sum(Cn * f + sum(nK * c[l - 1] * c[l] + c[l] for l in range(1, L + 1)) for f in feats[:towers])
    w = towers * sum(c)
    if towers == 1:
        return n + (w // 2) * w + w // 2
    h1 = max(w // 2, 10)
    h2 = max(h1 // 2, 10)
    return n + h1 * w + h2 * h1 + h2


def fields_of(phi):
    L1, V, _ = phi.shape
    return [[list(phi[l, v, 1:1 + phi[l, v, 0]]) for v in range(V)] for l in range(L1)]


def test_golden_parameter_counts_follow_the_gamma_layout():
    z = golden()
    cs = golden_cases(z, "gphys_")
    assert len(cs) == 5
    for tag, c in cs.items():
        towers, L, Cn, cap, _, _ = (int(x) for x in c["cfg"])
        feats = [c["feature"].shape[1]] + ([c["feature2"].shape[1]] if towers == 2 else [])
        assert c["params"].size == c["grads"].size == model_params(towers, Cn, L, feats), tag
        assert c["params"].size != model_params(towers, Cn, L, feats, nK=18), tag
        assert c["graph_feature"].size == towers * sum(channels(Cn, L)), tag
    for name in ("trainphys", "trainpair"):
        towers, L, Cn, cap, maxV, seed, nIter = (int(x) for x in z[name + "__cfg"])
        assert z[name + "__params0"].size == model_params(towers, Cn, L, [4, 4]), name
        assert z[name + "__losses"].shape == (nIter, 2)
    widths = {tuple(channels(int(c["cfg"][2]), int(c["cfg"][1]))) for c in cs.values()}
    assert (10, 5, 2, 1) in widths and (16, 8, 4, 2) in widths
    assert max(int(c["phi"][..., 0].max()) for c in cs.values()) > 32   # (a tower whose fields reach 33 - 64 positions)


def test_host_preparation_matches_the_real_classes_fields(gf):
    """Distance-only cap order, no WL ordering: gf_smp_prepare_molecule_host with physics = 1, nContractions = 4."""
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPConfig
    lib = _lib.load()
    checked = 0
    for tag, c in golden_cases(golden(), "gphys_").items():
        towers, L, Cn, cap, _, _ = (int(x) for x in c["cfg"])
        for adj_k, feat_k, phi_k in (("adj", "feature", "phi"), ("adj2", "feature2", "phi2"))[:towers]:
            adj = np.ascontiguousarray(c[adj_k], dtype=np.int32)
            feat = np.ascontiguousarray(c[feat_k], dtype=np.float64)
            V, F = feat.shape
            cfg = SMPConfig(L, Cn, F, 0, cap, 0, 4, 0, 1)
            phi = np.zeros((L + 1, V, cap + 1), dtype=np.int32)
            st = lib.gf_smp_prepare_molecule_host(C.byref(cfg), V, adj.ctypes.data_as(C.POINTER(C.c_int)),
                                                  feat.ctypes.data_as(C.POINTER(C.c_double)), phi.ctypes.data_as(C.POINTER(C.c_int)), None)
            assert st == 0
            assert fields_of(phi) == fields_of(c[phi_k]), (tag, adj_k)
            checked += 1
    assert checked == 7
