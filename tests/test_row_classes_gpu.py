"""Panels of one row class in the backward block products at C = 64 (smp_rowpanel_split with CLS, smp_level_c64_split.hip): under
skip_zero_grads, rows whose S_ab / T6 blocks are structural zeros are dealt into panels of their own and run the three products that
are stored.  (The forward products and the backward ones without skip_zero_grads stay on mixed panels -- NOTES.md -- and are held to
the same checks.)  Through gf_smp_level_products_ex_f32 on the packed table, with presence bits that put the two classes on the
panel's edges (0, 31, 32, 33 rows of a class, all rows, alternating rows, a ragged row count):
  * every stored block equals the unclassed kernel's (GF_SMP_ROW_CLASSES=0) -- a row's arithmetic does not depend on its panel mates, so
    there is no tolerance (-0.0 == +0.0 counts as equal);
  * every stored block is within TOL = 1e-5 of the fp64 product per (row, block), tests/level_ref.py;
  * gradients of structural zeros are left unwritten under skip_zero_grads, and garbage in absent blocks changes nothing;
and the list builder itself (gf_smp_level_row_classes): both lists ascending, every row exactly once, padding inside the matrix."""
import ctypes as C
import functools

import numpy as np
import pytest

import level_ref as lr
from test_level_ops_ex_gpu import SENTINEL, TOL, context, dev, ptr, run_products

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CH = 64
SIZES = [1, 2, 5, 31, 32, 33]          # 3,104 rows = 97 panels
RAGGED_SIZES = [1, 2, 5, 31, 32, 33, 3]  # 3,113 rows: not a multiple of 32


def own_patterns(rows):
    """name -> bit 31 of every row"""
    idx = np.arange(rows)
    pat = {"all_own": np.ones(rows, bool), "none_own": np.zeros(rows, bool), "alternating": idx % 2 == 0}
    rng = np.random.default_rng(rows)
    for n in (31, 32, 33):
        pick = np.zeros(rows, bool)
        pick[rng.permutation(rows)[:n]] = True
        pat["own_%d" % n] = pick
        pat["absent_%d" % n] = ~pick
    return pat


class Case:
    """a level of SIZES with the given bit 31; bit 30 = bit 31 of the transposed row, bit 29 drawn (set wherever bit 31 is, symmetric)"""

    def __init__(self, sizes, own, seed):
        rng = np.random.default_rng(seed)
        self.trow, _ = lr.level_rows(sizes)
        self.rows = rows = self.trow.size
        bc = rng.random(rows) < 0.8
        bc = bc | bc[self.trow] | own | own[self.trow]
        self.bits = (own, own[self.trow], bc)
        self.trowf = lr.pack(self.trow, self.bits)
        self.rf = lr.row_factors(sizes, rng, 2)
        T = (rng.standard_normal((rows, 4 * CH)) * np.exp(rng.uniform(-2.3, 2.3, (rows, 1)))).astype(np.float32)
        self.T = lr.fill_absent(T, CH, self.bits, rng)
        self.T2 = lr.fill_absent(T, CH, self.bits, rng)   # other garbage in the absent blocks
        self.dO = (rng.standard_normal((rows, 2 * CH)) * np.exp(rng.uniform(-2.3, 2.3, (rows, 1)))).astype(np.float32)
        self.dO_skip = np.array(self.dO)
        gone = np.flatnonzero(~bc)
        self.dO_skip[gone] = (5.0 * rng.standard_normal((gone.size, 2 * CH))).astype(np.float32)
        self.W = rng.uniform(-1, 1, (8, CH, CH)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name, ragged):
    sizes = RAGGED_SIZES if ragged else SIZES
    rows = sum(s * s for s in sizes)
    return Case(sizes, own_patterns(rows)[name], seed=rows + len(name))


def both(monkeypatch, *args, **kw):
    """(classed, unclassed) results of one call"""
    monkeypatch.delenv("GF_SMP_ROW_CLASSES", raising=False)
    on = run_products(*args, **kw)
    monkeypatch.setenv("GF_SMP_ROW_CLASSES", "0")
    off = run_products(*args, **kw)
    monkeypatch.delenv("GF_SMP_ROW_CLASSES")
    return on, off


PATTERNS = sorted(own_patterns(64))
CASES = [(n, False) for n in PATTERNS] + [("alternating", True), ("own_33", True), ("none_own", True), ("all_own", True)]


@pytest.mark.parametrize("name,ragged", CASES)
def test_classed_products_equal_the_unclassed_ones(gf, monkeypatch, name, ragged):
    c = case(name, ragged)
    assert (c.rows % 32 != 0) == ragged
    err = {}
    # forward
    on, off = both(monkeypatch, False, CH, 2, 0, c.T, c.rf, c.W, None, c.trow, c.trowf)
    assert np.array_equal(on, off), "forward: %d values differ" % int((on != off).sum())
    err["fwd"] = lr.row_block_err(on, lr.forward_ref(c.T, c.rf, c.W, c.trow, CH, None, c.bits), CH)
    monkeypatch.delenv("GF_SMP_ROW_CLASSES", raising=False)
    again = run_products(False, CH, 2, 0, c.T2, c.rf, c.W, None, c.trow, c.trowf)
    assert np.array_equal(on, again), "forward: garbage in the absent blocks of T changed the result"
    # backward, every block written
    on, off = both(monkeypatch, True, CH, 2, 0, c.dO, c.rf, c.W, None, c.trow, c.trowf)
    assert np.array_equal(on, off)
    err["bwd"] = lr.row_block_err(on, lr.backward_ref(c.dO, c.rf, c.W, c.trow, CH, None, c.bits), CH)
    # backward without the gradients of structural zeros
    on, off = both(monkeypatch, True, CH, 2, 0, c.dO_skip, c.rf, c.W, None, c.trow, c.trowf, skip=True)
    assert np.array_equal(on, off), "backward, skip_zero_grads: %d values differ" % int((on != off).sum())
    st = lr.stored_blocks(c.rows, c.bits, True)
    err["bwd_skip"] = lr.row_block_err(on, lr.backward_ref(c.dO_skip, c.rf, c.W, c.trow, CH, None, c.bits, True), CH, st)
    left = on.reshape(c.rows, 4, CH)[~st]
    assert np.all(left == SENTINEL), "skip_zero_grads wrote %d values of absent blocks" % int((left != SENTINEL).sum())
    print("%s%s: %s" % (name, " ragged" if ragged else "", ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, bad


def row_classes(trowf):
    ctx = context()
    rows = trowf.size
    n = 4 + 2 * (rows + 64) + rows // 1024 + 2
    buf = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    t = dev(trowf, np.int32)
    ctx.check(ctx.lib.gf_smp_level_row_classes(ctx.handle, rows, ptr(t), ptr(buf)))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.parametrize("name,ragged", CASES)
def test_the_lists_hold_every_row_once_in_ascending_order(gf, name, ragged):
    c = case(name, ragged)
    own = c.bits[0]
    buf = row_classes(c.trowf)
    n_own, n_abs = int(buf[0]), int(buf[1])
    assert (n_own, n_abs) == (int(own.sum()), int((~own).sum()))
    own_pad, abs_pad = -(-n_own // 32) * 32, -(-n_abs // 32) * 32
    ent = buf[4:4 + 2 * (own_pad + abs_pad)].view(np.uint32).reshape(-1, 2)
    row, pad, word = (ent[:, 0] & 0x1FFFFFFF).astype(np.int64), (ent[:, 0] >> 31) != 0, ent[:, 1]
    assert np.array_equal(row[:n_own], np.flatnonzero(own)) and np.array_equal(row[own_pad:own_pad + n_abs], np.flatnonzero(~own))
    assert not pad[:n_own].any() and not pad[own_pad:own_pad + n_abs].any()
    assert pad[n_own:own_pad].all() and pad[own_pad + n_abs:].all()
    assert (row < c.rows).all()
    assert np.array_equal(word, c.trowf.view(np.uint32)[row])          # every entry carries its row's packed word
    assert own[row[:own_pad]].all() and not own[row[own_pad:]].any()   # ... and padding stays inside its class
