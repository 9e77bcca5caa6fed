"""CPU suite of the classification models: the fp64 checker (tests/classification_ref.py) against the goldens recorded from the real
reference (tests/golden/smp_classification.npz), the classifier's weight initialisation, and the new entry points of the C ABI."""
import ctypes as C
import os
import re

import numpy as np

import classification_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gf_smp_create_classifier", "gf_smp_classes", "gf_smp_class_scores", "gf_smp_classifier_uniform_init_host")


def rel(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1.0))


def test_fixture_covers_what_it_should():
    cs = cref.golden_cases()
    for ver, nK in ((6, 10), (7, 50)):
        mine = {t: c for t, c in cs.items() if t.startswith("v%d_" % ver)}
        assert len(mine) == 10, sorted(mine)
        sat = [t for t, c in mine.items() if c["cfg"][7]]
        assert len(sat) == 1
        for t, c in mine.items():
            assert c["cfg"][6] == nK
            z = c["scores"]
            if c["cfg"][7]:   # saturated: an fp32 probability is 0, the fp64 loss finite
                gap = z.max() - z[int(c["target"][0])]
                assert 150.0 < gap < 600.0 and np.isfinite(c["loss"][0]) and c["loss"][0] != cref.LOG_ZERO
                assert np.float32(c["probability"][int(c["target"][0])]) == 0
            else:
                assert np.abs(z).max() <= 2.0, t
        assert {int(c["cfg"][1]) for c in mine.values()} == {1, 2, 3} and {int(c["cfg"][4]) for c in mine.values()} == {0, 1}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "smp_classification.npz")) < 300 * 1024


def test_fp64_checker_reproduces_every_golden_case(oracle):
    """Scores, probabilities, loss, label and all parameter gradients to 1e-12: pins the fixtures, the restated head and the
    W := dg construction of the level gradients."""
    n = 0
    for tag, c in cref.golden_cases().items():
        o = cref.run_case(c)
        errs = {k: rel(o[k], c[k]) for k in ("graph_feature", "scores", "probability", "grads")}
        errs["loss"] = abs(o["loss"] - c["loss"][0]) / max(1.0, abs(c["loss"][0]))
        assert max(errs.values()) <= 1e-12, (tag, errs)
        assert o["predict"] == int(c["label"][0]), tag
        n += 1
    assert n == 20


def test_head_edge_cases():
    g = np.array([1.0, -2.0, 0.5])
    W = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    o = cref.head(g, W, 2)
    assert o["predict"] == 0                       # a tie: the lowest index
    assert abs(o["probability"].sum() - 1.0) < 1e-15 and abs(o["dz"].sum()) < 1e-15
    assert cref.head(g, 400.0 * W, 2)["loss"] == cref.LOG_ZERO   # gap 1200: exp underflows in fp64 too
    assert np.isfinite(cref.head(g, 100.0 * W, 2)["loss"]) and cref.head(g, 100.0 * W, 2)["loss"] < -256.0   # gap 300


def test_classifier_uniform_init_equals_the_reference_constructor(gf):
    """Fails without the feature: gf_smp_classifier_uniform_init_host draws rand() in the reference's order, W with the divisor
    10 * nClass * C (uniform_init(Vector*), GraphFlow.h:1297-1306)."""
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPConfig
    lib = _lib.load()
    g = cref.load_golden()
    libc = C.CDLL(None)
    for ver in (6, 7):
        nClass, L, Cn, D, maxV, seed, nIter, nEpochs, nK = (int(x) for x in g["v%d_train__cfg" % ver])
        cfg = SMPConfig(L, Cn, 4, D, maxV, 1, nK, 1, 0)
        ref = g["v%d_train__params0" % ver]
        out = np.zeros(ref.size, dtype=np.float32)
        libc.srand(seed)
        assert lib.gf_smp_classifier_uniform_init_host(C.byref(cfg), nClass, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
        assert ref.dtype == np.float32 and np.array_equal(out, ref), np.abs(out - ref).max()
        w = np.abs(out[-nClass * Cn:])
        assert 0 < w.max() <= 9.0 / (10.0 * nClass * Cn) * (1 + 1e-6)
    cfg = SMPConfig(1, 4, 4, 1, 10, 1, 10, 1, 0)
    buf = np.zeros(4096, dtype=np.float32)
    assert lib.gf_smp_classifier_uniform_init_host(C.byref(cfg), 1, buf.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID
    assert lib.gf_smp_classifier_uniform_init_host(None, 3, buf.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID
    cfg.physics = 1
    assert lib.gf_smp_classifier_uniform_init_host(C.byref(cfg), 3, buf.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID


def test_new_entry_points_are_declared_exported_and_prototyped(gf):
    """Fails without the feature.  A NULL context / handle is refused with GF_ERR_INVALID, not a crash."""
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPConfig
    txt = open(os.path.join(ROOT, "include", "gf_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gf_[a-z0-9_]+)\s*\(", txt))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(raw, name), name
    lib = _lib.load()
    cfg = SMPConfig(1, 10, 4, 5, 10, 1, 10, 1, 0)
    h = C.c_void_p()
    assert lib.gf_smp_create_classifier(None, C.byref(cfg), 11, C.byref(h)) == _lib.GF_ERR_INVALID and not h.value
    assert lib.gf_smp_classes(None) == 0
    assert lib.gf_smp_class_scores(None, None, None) == _lib.GF_ERR_INVALID


def test_python_class_exists():
    from graphflow_amd.smp import SMPClassifier, SMPOmega
    assert issubclass(SMPClassifier, SMPOmega)
