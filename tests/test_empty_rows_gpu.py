"""The EMPTY rows of a fused 64-channel level -- rows (a, b) with no data in any block of T: none of bits 31 / 30 / 29 of the packed table,
no source covers the pair -- are neither stored nor read in the projected matrix O / dO (FusedRoute::skip_empty): the forward products
and combine-backward leave them unwritten, combine-forward and the weight gradients do not request them, the row-class lists of the
backward products leave them out.  Every comparison is bit for bit against the same library with GF_SMP_EMPTY_ROWS=0; the handle's
count of level passes that skipped them (gf_smp_empty_row_calls) says which ran, and under GF_POISON=1 the unwritten rows must still
hold the poison pattern (gf_smp_level_projected_f32)."""
import os

import numpy as np
import pytest

import level_ref as lr
from field_suite import dev, run_under_poison
from inputs import smp_params
from test_level1_tail_gpu import ATOM, CAP, D, F, batches, blocks, graph, run
from test_level_ops_ex_gpu import context, ptr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CH = 64
# a path: a pair of positions farther apart than 2 (l - 1) has no common source, so every level has empty rows; a ring closes it
PATH8 = graph(8, [(k, k + 1) for k in range(7)], 21)
RING10 = graph(10, [(k, (k + 1) % 10) for k in range(10)], 22)
SPARSE = ("path of 8", "10-ring", "mixed batch of 7 and the path")   # batches with empty rows at every level
REF_ENV = "GF_TEST_EMPTY_ROWS_REFERENCE"


def all_batches(golden):
    out = dict(batches(golden))
    out["path of 8"] = [PATH8]
    out["10-ring"] = [RING10]
    out["mixed batch of 7 and the path"] = out["mixed batch of 7"] + [PATH8]
    out["isolated vertex"] = [ATOM]
    return out


def step(mols, L, C=CH, seed=3, projected=False):
    """one forward and backward as test_level1_tail_gpu.run: (its outputs, the handle's empty-row passes, per level (rows, covered rows),
    and with `projected` the levels' O after the forward and dO after the backward)"""
    from graphflow_amd.smp import SMPOmega
    net = SMPOmega(L, C, F, D, CAP, True)
    net.prepare(mols)
    p = dev(smp_params(C, F, D, L, seed))
    tg = np.array([float(len(a)) for a, _ in mols])
    pred, loss, feat = net.forward(p, dev(tg))
    acts = [net.activation(m, l, v) for m, (a, _) in enumerate(mols) for l in range(L + 1) for v in range(len(a))]
    O = [net.level_projected(l).cpu().numpy() for l in range(1, L + 1)] if projected else None
    grads = torch.empty(net.n_params, device="cuda")
    net.backward(p, grads)
    dO = [net.level_projected(l).cpu().numpy() for l in range(1, L + 1)] if projected else None
    out = [pred.cpu().numpy(), loss.cpu().numpy(), feat.cpu().numpy(), grads.cpu().numpy()] + acts
    sizes = [(net.level_sizes(l)[1], net.level_covered_rows(l)) for l in range(1, L + 1)]
    n = net.empty_row_calls()
    net.close()
    return out, n, sizes, O, dO


def same(on, off, C, L, what):
    """predict, loss, feature, every gradient block and every f_l: np.array_equal (a -0.0 equals a +0.0)"""
    assert np.isfinite(on[3]).all() and np.abs(on[3]).max() > 0, what
    for k, name in enumerate(("predict", "loss", "feature")):
        assert np.array_equal(on[k], off[k]), (what, name)
    for blk, sl in blocks(C, L).items():
        assert np.array_equal(on[3][sl], off[3][sl]), (what, blk, np.abs(on[3][sl].astype(np.float64) - off[3][sl]).max())
    assert len(on) == len(off) and all(np.array_equal(x, y) for x, y in zip(on[4:], off[4:])), what


def on_off(monkeypatch, mols, L, C=CH):
    monkeypatch.delenv("GF_SMP_EMPTY_ROWS", raising=False)
    on = step(mols, L, C)
    monkeypatch.setenv("GF_SMP_EMPTY_ROWS", "0")
    off = step(mols, L, C)
    monkeypatch.delenv("GF_SMP_EMPTY_ROWS")
    return on, off


@pytest.mark.parametrize("L", [1, 2, 3])
def test_switch_on_and_off_give_the_same_bits(gf, golden, monkeypatch, L):
    for name, mols in all_batches(golden).items():
        on, off = on_off(monkeypatch, mols, L)
        # what the test relies on: the sparse batches have empty rows at every level, the isolated vertex has none
        if name in SPARSE[:2]:
            assert all(cov < rows for rows, cov in on[2]), (name, on[2])
        if name == "isolated vertex":
            assert all(cov == rows for rows, cov in on[2]), (name, on[2])
        assert on[1] == 2 * L and off[1] == 0, (name, on[1], off[1])
        same(on[0], off[0], CH, L, name)
        again = run(mols, L, CH)
        assert all(np.array_equal(x, y) for x, y in zip(on[0], again)), name   # two runs with the switch on: identical bits


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("switch", ["GF_SMP_ROW_CLASSES", "GF_SMP_SIGN_MASK"])
def test_with_the_other_readers_selected(gf, golden, monkeypatch, switch, L):
    """the unclassed backward products (they read dO where a source covers the row) and the combine-backward that reads f_l: both mask
    the empty rows, so the route stays and stays bit-equal -- the counter says that it ran"""
    monkeypatch.setenv(switch, "0")
    b = all_batches(golden)
    for name in SPARSE:
        on, off = on_off(monkeypatch, b[name], L)
        assert on[1] == 2 * L and off[1] == 0, (name, on[1], off[1])
        same(on[0], off[0], CH, L, name)


def test_a_32_channel_handle_reports_no_skipped_pass(gf, golden, monkeypatch):
    on, off = on_off(monkeypatch, all_batches(golden)["path of 8"], 2, C=32)
    assert on[1] == 0 and off[1] == 0
    same(on[0], off[0], 32, 2, "C = 32")


def test_projected_matrix_rows(gf, monkeypatch):
    """O after the forward and dO after the backward of the path at L = 3: every row with data equals the switch-off run's, and under
    GF_POISON=1 (the child process of the test below) every empty row still holds the poison pattern -- nobody wrote it -- while the
    results stay finite and equal to the unpoisoned run's (the file the parent process names)"""
    L = 3
    monkeypatch.delenv("GF_SMP_EMPTY_ROWS", raising=False)
    on = step([PATH8], L, projected=True)
    monkeypatch.setenv("GF_SMP_EMPTY_ROWS", "0")
    off = step([PATH8], L, projected=True)
    monkeypatch.delenv("GF_SMP_EMPTY_ROWS")
    assert on[1] == 2 * L and off[1] == 0
    same(on[0], off[0], CH, L, "path of 8")
    poisoned = os.environ.get("GF_POISON") == "1"
    ref = os.environ.get(REF_ENV)
    if poisoned:
        assert ref, "the poisoned run compares with the unpoisoned run's results"
    if ref and os.path.exists(ref):
        z = np.load(ref)
        assert all(np.isfinite(x).all() for x in on[0])
        assert all(np.array_equal(x, z["a%d" % k]) for k, x in enumerate(on[0]))
    for l in range(L):
        rows, covered = on[2][l]
        # with the switch off an empty row of O is stored as exact zeros; a row with data is not all zeros, or the count would not match
        empty = ~off[3][l].any(axis=1)
        assert rows - covered == int(empty.sum()) > 0, (l + 1, rows, covered, int(empty.sum()))
        for which, a, b in (("O", on[3][l], off[3][l]), ("dO", on[4][l], off[4][l])):
            assert a.shape == b.shape == (rows, 2 * CH)
            assert np.array_equal(a[~empty], b[~empty]), (l + 1, which)
            assert np.isfinite(b).all() and np.isfinite(a[~empty]).all(), (l + 1, which)
            if poisoned:
                assert (a[empty].view(np.uint32) == 0xFFFFFFFF).all(), (l + 1, which, "an empty row was written")


def test_projected_matrix_rows_under_poison(gf, monkeypatch, tmp_path):
    monkeypatch.delenv("GF_SMP_EMPTY_ROWS", raising=False)
    out = step([PATH8], 3)[0]
    path = str(tmp_path / "unpoisoned.npz")
    np.savez(path, **{"a%d" % k: x for k, x in enumerate(out)})
    monkeypatch.setenv(REF_ENV, path)
    run_under_poison(os.path.abspath(__file__), "test_projected_matrix_rows and not under_poison")


# ---- the row-class lists without the empty rows (gf_smp_level_row_classes_ex, live_only = 1) ----
SIZES = [1, 2, 5, 31, 32, 33, 3]   # 3,113 rows: not a multiple of 32, several 1,024-row blocks of the builder


def packed_level(n_empty, seed):
    """a level of SIZES: bit 31 drawn, bit 30 = bit 31 of the transposed row, bit 29 wherever either is set and on every other row but
    n_empty drawn ones (None: on none of them -- the level-1 shape, where every absent row is empty)"""
    rng = np.random.default_rng(seed)
    trow, _ = lr.level_rows(SIZES)
    rows = trow.size
    own = rng.random(rows) < 0.4
    own[trow == np.arange(rows)] = True   # (the diagonal rows always hold data)
    if n_empty is None:
        own = trow == np.arange(rows)
    trp = own[trow]
    free = np.flatnonzero(~own & ~trp)
    bc = np.ones(rows, bool)
    gone = free if n_empty is None else rng.permutation(free)[:n_empty]
    assert n_empty is None or gone.size == n_empty
    bc[gone] = False
    return lr.pack(trow, (own, trp, bc)), own, ~bc


@pytest.mark.parametrize("n_empty", [0, 31, 32, 33, None])
def test_the_lists_leave_the_empty_rows_out(gf, n_empty):
    trowf, own, empty = packed_level(n_empty, 7 + (n_empty or 0))
    rows = trowf.size
    ctx = context()
    buf = torch.full((4 + 2 * (rows + 64) + 2 * (rows // 1024 + 2),), -7, dtype=torch.int32, device="cuda")
    t = dev(trowf, np.int32)
    ctx.check(ctx.lib.gf_smp_level_row_classes_ex(ctx.handle, rows, ptr(t), ptr(buf), 1))
    torch.cuda.synchronize()
    buf = buf.cpu().numpy()
    absent = ~own & ~empty
    n_own, n_abs = int(buf[0]), int(buf[1])
    assert (n_own, n_abs) == (int(own.sum()), int(absent.sum()))
    assert int(empty.sum()) == (n_empty if n_empty is not None else rows - n_own) and n_own + n_abs + int(empty.sum()) == rows
    own_pad, abs_pad = -(-n_own // 32) * 32, -(-n_abs // 32) * 32
    ent = buf[4:4 + 2 * (own_pad + abs_pad)].view(np.uint32).reshape(-1, 2)
    row, pad, word = (ent[:, 0] & 0x1FFFFFFF).astype(np.int64), (ent[:, 0] >> 31) != 0, ent[:, 1]
    # both lists ascending, every row with data exactly once, no empty row in either
    assert np.array_equal(row[:n_own], np.flatnonzero(own)) and np.array_equal(row[own_pad:own_pad + n_abs], np.flatnonzero(absent))
    assert not pad[:n_own].any() and not pad[own_pad:own_pad + n_abs].any()
    assert pad[n_own:own_pad].all() and pad[own_pad + n_abs:].all()
    assert (row < rows).all() and not empty[row].any()                     # padding stays inside the matrix, and inside the rows with data
    assert np.array_equal(word, trowf.view(np.uint32)[row])
    assert own[row[:own_pad]].all() and not own[row[own_pad:]].any()       # ... and inside its class
