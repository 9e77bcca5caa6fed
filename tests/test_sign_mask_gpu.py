"""The reverse sweep of the fused level at C = 64 with LeakyReLU' taken from the sign words combine-forward leaves (default) against the
sweep that reads f_l and stores / reads dz (GF_SMP_SIGN_MASK=0): the same bits.  f > 0 holds exactly where z > 0 (the slope is positive;
+-0 and NaN fail both tests), and every product and sum keeps its operands and its order, so nothing may differ -- array_equal, no tolerance.
The batch: molecules of 3 .. 29 atoms -- panels of several row groups (s <= 16) and of one (17 <= s <= 32), last panels of a node with
fewer groups than the others, rows past the end of a panel."""
import numpy as np
import pytest

from field_suite import dev
from inputs import smp_params, synthetic_molecule

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F, D, C, CAP = 5, 5, 64, 29
SIZES = (3, 5, 9, 12, 16, 17, 23, 29)


def batch(sizes=SIZES, seed0=9100):
    mols, tg = [], []
    for i, nV in enumerate(sizes):
        adj, feat, t = synthetic_molecule(seed0 + i, nV=nV)
        mols.append((adj, feat))
        tg.append(t)
    return mols, np.array(tg)


def blocks(L, C, F, D):
    """(name, lo, hi) of every parameter block: H, (K_l, b_l), W."""
    o = C * F * (D + 1)
    out = [("H", 0, o)]
    for l in range(1, L + 1):
        out.append(("K_%d" % l, o, o + 18 * C * C))
        out.append(("b_%d" % l, o + 18 * C * C, o + 18 * C * C + C))
        o += 18 * C * C + C
    out.append(("W", o, o + C))
    return out


def step(mols, tg, params, L, D=D, cap=CAP):
    from graphflow_amd.smp import SMPOmega
    net = SMPOmega(L, C, F, D, cap, True)
    net.prepare(mols)
    p = dev(params)
    pred, loss, feat = net.forward(p, dev(tg))
    grads = torch.full((net.n_params,), float("nan"), device="cuda")
    net.backward(p, grads)
    return {"predict": pred.cpu().numpy(), "loss": loss.cpu().numpy(), "feature": feat.cpu().numpy(), "grads": grads.cpu().numpy(), "net": net}


def both_paths(monkeypatch, mols, tg, params, L, D=D, cap=CAP):
    monkeypatch.delenv("GF_SMP_SIGN_MASK", raising=False)
    a = step(mols, tg, params, L, D, cap)
    monkeypatch.setenv("GF_SMP_SIGN_MASK", "0")
    b = step(mols, tg, params, L, D, cap)
    monkeypatch.delenv("GF_SMP_SIGN_MASK", raising=False)
    return a, b


def assert_same_bits(a, b, L, D=D):
    for k in ("predict", "loss", "feature"):
        assert np.array_equal(a[k], b[k]), k
    assert np.isfinite(a["grads"]).all()
    for name, lo, hi in blocks(L, C, F, D):
        assert np.array_equal(a["grads"][lo:hi], b["grads"][lo:hi]), "gradient block %s" % name


@pytest.mark.parametrize("L", [3, 2])
def test_sign_mask_sweep_equals_the_sweep_that_reads_f(gf, monkeypatch, L):
    mols, tg = batch()
    params = smp_params(C, F, D, L, 21)
    a, b = both_paths(monkeypatch, mols, tg, params, L)
    assert np.abs(a["grads"]).max() > 0
    assert_same_bits(a, b, L)
    a["net"].close()
    b["net"].close()


def test_exact_zeros_take_the_small_slope_on_both_paths(gf, monkeypatch):
    """K_L = 0 and b_L = 0: every z of the top level is an exact zero, so every slope there is alpha on both paths."""
    L = 3
    mols, tg = batch()
    params = smp_params(C, F, D, L, 22).copy()
    name, lo, hi = [b for b in blocks(L, C, F, D) if b[0] == "K_%d" % L][0]
    params[lo:hi + C] = 0.0   # (b_L follows K_L)
    a, b = both_paths(monkeypatch, mols, tg, params, L)
    assert not a["feature"].any()                       # f_L = LeakyReLU(0) = 0 everywhere
    assert np.abs(a["grads"][lo:hi]).max() > 0          # ... and dK_L is a gradient all the same: alpha times the read-out's vector
    assert_same_bits(a, b, L)
    a["net"].close()
    b["net"].close()


def test_a_level_with_nodes_above_32_positions(gf, monkeypatch):
    """A 40-atom molecule beside small ones under a cap of 48: level 3 has nodes above 32 positions, which the workgroup kernels serve
    (they read f_l on both paths) beside the panels of the other nodes; the top level's products read the stored dz."""
    L, Db, cap = 3, 2, 48
    adj, feat, t = synthetic_molecule(8003, nV=40)
    mols, tg = batch((5, 12, 17, 29), seed0=9200)
    mols, tg = [(adj, feat)] + mols, np.concatenate([[t], tg])
    params = smp_params(C, F, Db, L, 23)
    a, b = both_paths(monkeypatch, mols, tg, params, L, Db, cap)
    net = a["net"]
    assert max(len(net.receptive_field(0, L, v)) for v in range(40)) > 32
    assert_same_bits(a, b, L, Db)
    # the sign words are pool buffers of the batch: 8 bytes per row of every level, beside f_l and df_l (2 x 4 C bytes per row)
    rows = sum(net.level_sizes(l)[1] for l in range(1, L + 1))
    assert net.device_bytes()[0] >= rows * (8 + 8 * C)
    a["net"].close()
    b["net"].close()


def test_outputs_written_by_the_readout_are_the_handles_own(gf):
    """predict and graph_feature are written by the read-out kernel itself, not copied: the reverse sweep reads the handle's own copies, and
    dW = sum_m (predict - target)[m] feature[m] -- within the rounding of an fp32 sum of nMol terms -- shows they are the same numbers;
    predict = <feature, W> likewise.  A second forward into the same buffers gives the same bits."""
    L = 2
    mols, tg = batch()
    params = smp_params(C, F, D, L, 24)
    a = step(mols, tg, params, L)
    net = a["net"]
    name, lo, hi = blocks(L, C, F, D)[-1]
    assert name == "W"
    dy = a["predict"].astype(np.float64) - tg
    terms = dy[:, None] * a["feature"].astype(np.float64)
    bound = len(mols) * 2.0 ** -23 * np.abs(terms).sum(axis=0) + 1e-30
    assert (np.abs(a["grads"][lo:hi] - terms.sum(axis=0)) <= bound).all()
    w = params[lo:hi].astype(np.float64)
    yb = C * 2.0 ** -23 * (np.abs(a["feature"].astype(np.float64)) * np.abs(w)).sum(axis=1) + 1e-30
    assert (np.abs(a["predict"] - a["feature"].astype(np.float64) @ w) <= yb).all()
    pred, loss, feat = net.forward(dev(params), dev(tg))
    assert np.array_equal(pred.cpu().numpy(), a["predict"]) and np.array_equal(feat.cpu().numpy(), a["feature"])
    assert np.array_equal(loss.cpu().numpy(), a["loss"])
    net.close()
