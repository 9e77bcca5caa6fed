"""GPU parity suite of the classification models (gf_smp_create_classifier: SMP_2D_ver6_classification / SMP_2D_ver7_classification)
against goldens recorded from the real reference (tests/golden/smp_classification.npz) and the fp64 checker (classification_ref.py).

Bounds.  TOL_FWD = 1e-5 on graph_feature and scores is the suite's end-to-end bound (tests/test_smp_gpu.py).  The loss is a score minus
a log-sum-exp of the scores, so it moves by at most twice the largest score error: |loss - ref| <= 2 TOL_FWD max(1, max |z_ref|).
TOL_GRAD = 1e-5: the softmax multiplies the forward error by at most 2 max |score| <= 4 in the ordinary cases (the generator asserts
max |score| <= 2) and the suite's measured forward maxima are about 1e-6 (profiles/r02_parity_margins.txt).  The measured maxima of this
head are printed by test_zz_print_margins and kept in profiles/classification_parity_margins.txt.

The head in isolation (saturated cases): every score against the fp64 head on the device's own graph_feature and W within the fp32
dot-product bound 2 C 2^-24 sum_f |W_cf g_f|; dz and dW against that fp64 head within 4 x the error measured on this fixture
(HEAD_DZ_MEASURED / HEAD_DW_MEASURED, profiles/classification_parity_margins.txt).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import classification_ref as cref
from field_suite import dev
from inputs import f32exact, synthetic_molecule, toy_molecules
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL_FWD, TOL_GRAD = 1e-5, 1e-5
# measured on the saturated fixtures against the fp64 head on the device's own graph_feature and W (margins head_saturated.dz / .dW):
# dz is the absolute error of p - onehot, dW = dz g^T relative to its largest entry.  (The device's saturated probabilities are exactly 0 and
# 1 there, so what is left is the fp64 head's own rounding.)
HEAD_DZ_MEASURED, HEAD_DW_MEASURED = 4.441e-16, 4.112e-16
MARGINS = {}
NK = {6: 10, 7: 50}


def note(name, **errs):
    for k, v in errs.items():
        MARGINS[name + "." + k] = max(MARGINS.get(name + "." + k, 0.0), float(v))


def make(nClass, L, C, F, D, cap, wl=True, nK=10, custom=True, fused=True, ctx=None):
    from graphflow_amd.smp import SMPClassifier
    net = SMPClassifier(nClass, L, C, F, D, cap, wl, ctx=ctx, nContractions=nK, custom_matmul=custom)
    net.set_fused(fused)
    return net


def step(net, mols, labels, params, accumulate_into=None):
    """prepare + forward + backward; everything back as float64 numpy."""
    net.prepare(mols)
    p = dev(params)
    pred, loss, feat = net.forward(p, dev(labels))
    z, pr = net.scores()
    grads = accumulate_into if accumulate_into is not None else torch.full((net.n_params,), float("nan"), device="cuda")
    net.backward(p, grads, accumulate=accumulate_into is not None)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)  # noqa: E731
    return {"predict": f64(pred), "loss": f64(loss), "feature": f64(feat), "scores": f64(z), "probability": f64(pr), "grads": f64(grads),
            "raw": (pred.clone(), loss.clone(), feat.clone(), z, pr, grads)}


def case_net(c, fused=True):
    nClass, L, C, D, wl, maxV, nK, _ = (int(x) for x in c["cfg"])
    return make(nClass, L, C, c["feature"].shape[1], D, maxV, bool(wl), nK=nK, fused=fused)


def loss_bound(z_ref):
    return 2 * TOL_FWD * max(1.0, float(np.abs(z_ref).max()))


def synthetic_batch(n, nClass, seed0, lo=4, hi=10):
    rng = np.random.default_rng(seed0)
    mols, labels = [], []
    for i in range(n):
        adj, feat, _ = synthetic_molecule(seed0 + i, nV=int(rng.integers(lo, hi + 1)))
        mols.append((adj, feat))
        labels.append(int(rng.integers(0, nClass)))
    return mols, np.array(labels, dtype=np.float64)


def class_params(n_params, nClass, C, seed, w_scale=1.0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, n_params) / np.sqrt(10 * C)
    p[-nClass * C:] = rng.uniform(-1, 1, nClass * C) * w_scale
    return f32exact(p)


def checker_sum(mols, labels, params, nClass, L, C, D, cap, wl=True, nK=10, custom=True):
    outs = [cref.run(adj, feat, None if lb is None else int(lb), params, nClass, L, C, D, cap, wl, nK=nK, custom=custom)
            for (adj, feat), lb in zip(mols, labels)]
    g = sum(o["grads"] for o in outs if "grads" in o)
    return outs, g


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ver", [6, 7])
def test_reference_goldens_ordinary_cases(gf, ver, fused):
    n = 0
    for tag, c in cref.golden_cases().items():
        if not tag.startswith("v%d_" % ver) or c["cfg"][7]:
            continue
        net = case_net(c, fused)
        assert net.lib.gf_smp_classes(net.handle) == int(c["cfg"][0])
        o = step(net, [(c["adj"], c["feature"])], c["target"].astype(np.float64), c["params"])
        errs = dict(feat=rel_err(o["feature"][0], c["graph_feature"]), scores=rel_err(o["scores"][0], c["scores"]),
                    prob=rel_err(o["probability"][0], c["probability"]), loss=abs(o["loss"][0] - c["loss"][0]),
                    grads=rel_err(o["grads"], c["grads"]))
        name = "goldens_v%d_%s" % (ver, "fused" if fused else "opbyop")
        note(name, **errs)
        print(name, tag, errs)
        assert errs["feat"] <= TOL_FWD and errs["scores"] <= TOL_FWD and errs["prob"] <= TOL_FWD, (tag, errs)
        assert errs["loss"] <= loss_bound(c["scores"]), (tag, errs)
        assert o["predict"][0] == float(c["label"][0]), tag
        assert errs["grads"] <= TOL_GRAD, (tag, errs)
        net.close()
        n += 1
    assert n == 9


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("ver", [6, 7])
def test_saturated_cases_and_the_head_in_isolation(gf, ver, fused):
    """A gap max(z) - z[label] between 150 and 600: the fp32 probability of the label is 0, the loss must still be the reference's
    finite value (it is computed from the scores, not from the probability)."""
    cs = [c for t, c in cref.golden_cases().items() if t.startswith("v%d_" % ver) and c["cfg"][7]]
    assert len(cs) == 1
    c = cs[0]
    nClass, C = int(c["cfg"][0]), int(c["cfg"][2])
    label = int(c["target"][0])
    net = case_net(c, fused)
    o = step(net, [(c["adj"], c["feature"])], c["target"].astype(np.float64), c["params"])
    net.close()
    assert o["probability"][0][label] == 0.0 and c["probability"][label] > 0.0
    err = abs(o["loss"][0] - c["loss"][0])
    note("saturated_v%d" % ver, loss=err, scores=rel_err(o["scores"][0], c["scores"]), grads=rel_err(o["grads"], c["grads"]))
    print("saturated v%d: loss %.9g reference %.9g |diff| %.3e bound %.3e" % (ver, o["loss"][0], c["loss"][0], err, loss_bound(c["scores"])))
    assert np.isfinite(o["loss"][0]) and err <= loss_bound(c["scores"])
    assert o["predict"][0] == float(c["label"][0])
    # the head alone: fp64 on the device's own graph_feature and the (fp32) W
    W = c["params"][-nClass * C:].astype(np.float64).reshape(nClass, C)
    g = o["feature"][0]
    h = cref.head(g, W, label)
    dot_bound = 2 * C * 2.0 ** -24 * (np.abs(W) * np.abs(g)[None, :]).sum(axis=1)
    assert (np.abs(o["scores"][0] - h["scores"]) <= dot_bound).all(), (np.abs(o["scores"][0] - h["scores"]), dot_bound)
    onehot = np.zeros(nClass)
    onehot[label] = 1.0
    dz_dev = (o["probability"][0].astype(np.float32) - onehot.astype(np.float32)).astype(np.float64)
    e_dz = float(np.abs(dz_dev - h["dz"]).max())
    e_dW = rel_err(o["grads"][-nClass * C:], h["dW"].ravel())
    note("head_saturated", dz=e_dz, dW=e_dW)
    print("head in isolation v%d: dz %.3e dW %.3e" % (ver, e_dz, e_dW))
    assert e_dz <= 4 * HEAD_DZ_MEASURED and e_dW <= 4 * HEAD_DW_MEASURED, (e_dz, e_dW)


@pytest.mark.parametrize("C", [10, 32])
def test_batch_of_64_equals_the_per_molecule_checker_and_the_unpadded_model(gf, monkeypatch, C):
    nClass, L, D, F, cap = 6, 2, 2, 5, 10
    mols, labels = synthetic_batch(64, nClass, 5200 + C)
    net = make(nClass, L, C, F, D, cap)
    params = class_params(net.n_params, nClass, C, 77 + C, w_scale=0.05)
    # (the scores are linear in W: scaled, as the golden generator does, so that max |score| is about 1.5 -- asserted on the checker below)
    zmax = np.abs(step(net, mols, labels, params)["scores"]).max()
    params[-nClass * C:] = f32exact(params[-nClass * C:] * (1.5 / zmax))
    o = step(net, mols, labels, params)
    net.close()
    outs, g_ref = checker_sum(mols, labels, params, nClass, L, C, D, cap)
    z_ref = np.stack([r["scores"] for r in outs])
    assert np.abs(z_ref).max() <= 2.0   # (the gradient bound's premise)
    errs = dict(feat=rel_err(o["feature"], np.stack([r["graph_feature"] for r in outs])), scores=rel_err(o["scores"], z_ref),
                loss=float(np.abs(o["loss"] - np.array([r["loss"] for r in outs])).max()), grads=rel_err(o["grads"], g_ref))
    note("batch64_C%d" % C, **errs)
    print("batch64 C=%d" % C, errs)
    assert errs["feat"] <= TOL_FWD and errs["scores"] <= TOL_FWD and errs["loss"] <= loss_bound(z_ref) and errs["grads"] <= TOL_GRAD, errs
    assert np.array_equal(o["predict"], np.array([float(r["predict"]) for r in outs]))
    assert len(set(labels.tolist())) > 1 and len(set(o["predict"].tolist())) >= 1
    # the same model computed at its own channel count
    monkeypatch.setenv("GF_SMP_PAD_CHANNELS", "0")
    plain = make(nClass, L, C, F, D, cap)
    q = step(plain, mols, labels, params)
    plain.close()
    e = dict(scores=rel_err(o["scores"], q["scores"]), loss=rel_err(o["loss"], q["loss"]), grads=rel_err(o["grads"], q["grads"]))
    note("padded_vs_unpadded_C%d" % C, **e)
    assert max(e.values()) <= 2e-6, e


def test_an_asymmetric_adjacency_takes_the_op_by_op_plan(gf):
    nClass, L, C, D, F, cap = 5, 2, 6, 2, 5, 8
    mols, labels = synthetic_batch(6, nClass, 6100, lo=5, hi=8)
    bad = np.array(mols[2][0]).copy()
    i, j = np.argwhere(bad > 0)[0]
    bad[j, i] = 0
    assert not np.array_equal(bad, bad.T)
    for nK in (10, 50):
        net = make(nClass, L, C, F, D, cap, nK=nK)
        params = class_params(net.n_params, nClass, C, 91, w_scale=0.05)
        sym = step(net, mols, labels, params)                       # the embedded plan
        mixed = mols[:2] + [(bad, mols[2][1])] + mols[3:]
        o = step(net, mixed, labels, params)                        # op-by-op `_10` / `_50` levels, chosen by gf_smp_prepare
        again = step(net, mols, labels, params)                     # and back
        net.close()
        assert all(torch.equal(a, b) for a, b in zip(sym["raw"], again["raw"]))
        outs, g_ref = checker_sum(mixed, labels, params, nClass, L, C, D, cap, nK=nK)
        z_ref = np.stack([r["scores"] for r in outs])
        errs = dict(scores=rel_err(o["scores"], z_ref), loss=float(np.abs(o["loss"] - np.array([r["loss"] for r in outs])).max()),
                    grads=rel_err(o["grads"], g_ref))
        note("asymmetric_nK%d" % nK, **errs)
        assert errs["scores"] <= TOL_FWD and errs["loss"] <= loss_bound(z_ref) and errs["grads"] <= TOL_GRAD, errs


def test_runs_are_bit_identical_and_accumulate_doubles(gf):
    nClass, L, C, D, F, cap = 11, 2, 10, 2, 5, 10
    mols, labels = synthetic_batch(48, nClass, 6300)
    for nK, fused in ((10, True), (50, True), (10, False)):
        net = make(nClass, L, C, F, D, cap, nK=nK, fused=fused)
        params = class_params(net.n_params, nClass, C, 3, w_scale=0.1)
        a = step(net, mols, labels, params)
        b = step(net, mols, labels, params)
        assert all(torch.equal(x, y) for x, y in zip(a["raw"], b["raw"])), (nK, fused)
        acc = a["raw"][5].clone()
        c = step(net, mols, labels, params, accumulate_into=acc)
        assert rel_err(c["grads"], 2 * a["grads"]) <= 1e-5
        net.close()


def test_invalid_labels_and_missing_targets_are_safe(gf):
    nClass, L, C, D, F, cap = 4, 1, 10, 1, 5, 10
    mols, labels = synthetic_batch(8, nClass, 6400)
    net = make(nClass, L, C, F, D, cap)
    params = class_params(net.n_params, nClass, C, 5, w_scale=0.1)
    bad = labels.copy()
    bad[1], bad[4], bad[6] = -1.0, float(nClass), float("nan")
    o = step(net, mols, bad, params)
    ok = np.array([m not in (1, 4, 6) for m in range(8)])
    assert np.isnan(o["loss"][~ok]).all() and np.isfinite(o["loss"][ok]).all() and np.isfinite(o["grads"]).all()
    outs, g_ref = checker_sum(mols, [lb if k else None for lb, k in zip(labels, ok)], params, nClass, L, C, D, cap)
    assert rel_err(o["grads"], g_ref) <= TOL_GRAD
    assert np.array_equal(o["predict"], np.array([float(r["predict"]) for r in outs]))
    # no targets: scores, probabilities and predict; a reverse sweep is refused
    p = dev(params)
    pred, _, _ = net.forward(p, None)
    z, pr = net.scores()
    assert torch.equal(pred, o["raw"][0]) and torch.equal(z, o["raw"][3]) and torch.equal(pr, o["raw"][4])
    with pytest.raises(gf.GraphFlowHipError):
        net.backward(p, torch.empty(net.n_params, device="cuda"))
    with pytest.raises(gf.GraphFlowHipError):   # never a physics tower
        net.backward_features(p, torch.empty(net.n_params, device="cuda"), torch.zeros_like(net.feature))
    net.close()


@pytest.mark.parametrize("ver", [6, 7])
def test_batchlearn_matches_the_reference(gf, ver):
    """Three BatchLearn steps of the real classifier (Momentum 0.9): same srand -> same initial weights, then forward / backward /
    gf_smp_momentum_step; the tolerances of the regression model's trajectory test (test_smp_2d_ver6_batchlearn_matches_the_reference)."""
    z = cref.load_golden()
    k = "v%d_train__" % ver
    nClass, L, Cn, D, maxV, seed, nIter, nEpochs, nK = (int(x) for x in z[k + "cfg"])
    lr, gamma = (float(x) for x in z[k + "lr"])
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    tg = dev(z[k + "targets"].astype(np.float64))
    net = make(nClass, L, Cn, 4, D, maxV, nK=nK)
    ctypes.CDLL(None).srand(seed)
    p = dev(net.uniform_init())
    assert np.array_equal(p.cpu().numpy(), z[k + "params0"])
    net.prepare(mols)
    grads = torch.empty(net.n_params, device="cuda")
    for it in range(nIter):
        _, loss, _ = net.forward(p, tg)
        before = float(loss.double().sum())
        net.backward(p, grads)
        net.momentum_step(p, grads, lr, len(mols), gamma)
        _, loss, _ = net.forward(p, tg)
        after = float(loss.double().sum())
        print("BatchLearn v%d step %d: %.9g %.9g reference %s" % (ver, it, before, after, z[k + "losses"][it]))
        assert before <= 0 and after <= 0   # the reference's sign: sums of log-probabilities
        assert abs(before - z[k + "losses"][it, 0]) <= 5 * TOL_FWD * max(1.0, abs(before)), it
        assert abs(after - z[k + "losses"][it, 1]) <= 5 * TOL_FWD * max(1.0, abs(after)), it
    err = np.abs(p.cpu().numpy().astype(np.float64) - z[k + "params"])
    scale = np.abs(z[k + "params"].astype(np.float64) - z[k + "params0"]).max()
    print("max |param - reference| %.3e, largest parameter change %.3e" % (err.max(), scale))
    assert err.max() <= 1e-3 * scale
    net.close()


def test_checkpoint_round_trip(gf, tmp_path):
    nClass, L, C, D, F, cap = 11, 1, 10, 5, 4, 10
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    a, b = make(nClass, L, C, F, D, cap), make(nClass, L, C, F, D, cap)
    assert a.n_params == C * F * (D + 1) + L * (10 * C * C + C) + nClass * C
    p = dev(class_params(a.n_params, nClass, C, 9, w_scale=0.3))
    path = tmp_path / "classifier.dat"
    a.save_model(p, path)
    vals = [float(x) for x in open(path).read().split()]
    assert len(vals) == a.n_params
    q = torch.zeros(b.n_params, device="cuda")
    b.load_model(q, path)
    a.prepare(mols)
    b.prepare(mols)
    pa, _, _ = a.forward(q, None)      # (the checkpoint holds 6 significant digits: both handles run the loaded weights)
    pb, _, _ = b.forward(q, None)
    assert torch.equal(pa, pb) and all(torch.equal(x, y) for x, y in zip(a.scores(), b.scores()))
    assert rel_err(q.cpu().numpy(), p.cpu().numpy()) <= 1e-5
    a.close()
    b.close()


def test_one_rank_communicator_gives_the_same_bits(gf):
    nClass, L, C, D, F, cap = 7, 2, 10, 2, 5, 10
    mols, labels = synthetic_batch(32, nClass, 6500)
    for nK in (10, 50):
        plain = make(nClass, L, C, F, D, cap, nK=nK)
        params = class_params(plain.n_params, nClass, C, 13, w_scale=0.1)
        a = step(plain, mols, labels, params)
        plain.close()
        ctx = gf.Context(0)
        ctx.dist_init(ctx.dist_unique_id(), 0, 1)
        net = make(nClass, L, C, F, D, cap, nK=nK, ctx=ctx)
        net.set_grad_allreduce(True)
        b = step(net, mols, labels, params)
        ctx.dist_quiesce()
        g = b["raw"][5].cpu().numpy()
        net.close()
        ctx.close()
        assert np.array_equal(g, a["raw"][5].cpu().numpy()), nK


def test_refusals(gf):
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPClassifier, SMPConfig
    with pytest.raises(gf.GraphFlowHipError):
        SMPClassifier(1, 1, 10, 4, 5, 10)
    with pytest.raises(gf.GraphFlowHipError):
        SMPClassifier(0, 1, 10, 4, 5, 10)
    ctx = gf.default_context()
    cfg = SMPConfig(1, 8, 4, 0, 10, 1, 18, 0, 1)   # physics = 1
    h = ctypes.c_void_p()
    assert ctx.lib.gf_smp_create_classifier(ctx.handle, ctypes.byref(cfg), 5, ctypes.byref(h)) == _lib.GF_ERR_INVALID and not h.value


@pytest.mark.parametrize("nK,custom", [(18, False), (18, True), (4, False)])
def test_the_other_wirings_come_for_free(gf, nK, custom):
    nClass, L, C, D, F, cap = 5, 2, 8, 2, 5, 10
    mols, labels = synthetic_batch(5, nClass, 6600, lo=5, hi=9)
    net = make(nClass, L, C, F, D, cap, nK=nK, custom=custom)
    params = class_params(net.n_params, nClass, C, 21, w_scale=0.1)
    o = step(net, mols, labels, params)
    net.close()
    W = params[-nClass * C:].reshape(nClass, C)
    for m in range(len(mols)):   # the head against the device's own graph_feature
        h = cref.head(o["feature"][m], W, int(labels[m]))
        assert rel_err(o["scores"][m], h["scores"]) <= TOL_FWD and abs(o["loss"][m] - h["loss"]) <= loss_bound(h["scores"])
        assert o["predict"][m] == float(h["predict"])
    dW = sum(cref.head(o["feature"][m], W, int(labels[m]))["dW"] for m in range(len(mols)))
    assert rel_err(o["grads"][-nClass * C:], dW.ravel()) <= TOL_GRAD
    if nK == 18:   # RisiContraction_18 levels: the whole model against the checker
        outs, g_ref = checker_sum(mols, labels, params, nClass, L, C, D, cap, nK=18, custom=custom)
        assert rel_err(o["grads"], g_ref) <= TOL_GRAD


def test_a_regression_handle_is_untouched(gf):
    """gf_smp_classes == 0, the regression kernels only (no *_classes name in the kernel-timing table), results against the oracle."""
    from graphflow_amd.smp import SMPOmega
    from oracle import smp_oracle
    L, C, D, F, cap = 1, 10, 5, 4, 10
    mols = toy_molecules()
    ctx = gf.Context(0)
    reg = SMPOmega(L, C, F, D, cap, True, ctx=ctx, nContractions=10, custom_matmul=True)
    assert ctx.lib.gf_smp_classes(reg.handle) == 0
    with pytest.raises(gf.GraphFlowHipError):
        ctx.check(ctx.lib.gf_smp_class_scores(reg.handle, None, None))
    rng = np.random.default_rng(4)
    params = f32exact(rng.uniform(-1, 1, reg.n_params) / np.sqrt(10 * C))
    reg.prepare([(adj, feat) for _, adj, feat, _ in mols])
    p, tg = dev(params), dev(np.array([t for *_, t in mols]))
    ctx.set_timing(True)
    pred, loss, _ = reg.forward(p, tg)
    g = torch.empty(reg.n_params, device="cuda")
    reg.backward(p, g)
    names = set(ctx.timings())
    ctx.set_timing(False)
    assert names and not [n for n in names if "classes" in n], names
    assert {"smp_readout_mol", "smp_readout_dW", "smp_readout_bwd"} <= names
    ref = [smp_oracle.run(adj, feat, t, params, L, C, D, cap, nK=10, custom=True) for _, adj, feat, t in mols]
    assert rel_err(pred.cpu().numpy(), np.array([r["predict"] for r in ref])) <= TOL_FWD
    assert rel_err(g.cpu().numpy(), sum(r["grads"] for r in ref)) <= TOL_GRAD
    reg.close()
    # ... and a classifier launches the kernels of its own, under their own names
    net = make(11, L, C, F, D, cap, ctx=ctx)
    pc = class_params(net.n_params, 11, C, 2, w_scale=0.1)
    ctx.set_timing(True)
    step(net, [(adj, feat) for _, adj, feat, _ in mols], np.array([t for *_, t in mols]), pc)
    names = set(ctx.timings())
    ctx.set_timing(False)
    assert {"smp_readout_mol_classes", "smp_readout_dW_classes", "smp_readout_bwd_classes"} <= names, names
    net.close()
    ctx.close()


def test_no_kernel_reads_what_nobody_wrote():
    """The golden, batch and asymmetric tests above once more in a process with GF_POISON=1 (every buffer the library hands out without
    contents is filled with NaN patterns first)."""
    env = dict(os.environ, GF_POISON="1")
    env.pop("GF_MARGINS_OUT", None)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "reference_goldens or saturated or asymmetric or invalid_labels", "-p", "no:cacheprovider"], env=env, capture_output=True,
                       text=True, timeout=900)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail


def test_zz_print_margins(gf):
    """Not a check: prints the measured maxima collected above (run with -s; copied to profiles/classification_parity_margins.txt)."""
    lines = ["margin %-56s %.3e" % (k, MARGINS[k]) for k in sorted(MARGINS)]
    for ln in lines:
        print(ln)
    if os.environ.get("GF_MARGINS_OUT"):
        with open(os.environ["GF_MARGINS_OUT"], "w") as fh:
            fh.write("\n".join(lines) + "\n")
