"""The masked operand paths of the fused level's block products and weight gradients (smp_rowpanel_split with the packed table, its
row-class backward build, smp_wgrad_split / smp_wgrad_all behind gf_smp_level_products_ex_f32 / gf_smp_level_wgrad_ex_f32, and the
C = 64 weight gradients behind gf_smp_level_wgrad_f32): where a block's address is a select between the matrix and the page of zeros,
where a store's address is a select between the output and the scratch rows, and where the weight gradients stage their slices.

Shapes are the smallest at which that addressing can go wrong: row counts 1, 15, 16, 17, 31, 33, 47 and 8 x 16 x 3 + 5 = 389 (partial
last panels of 32 rows, partial last slices of 16 rows; a workgroup of the staged weight gradients gets 1, 2 or 3 slices of the small
counts and 6 or 7 of the 25 slices of the last one -- one and two turns of the three-interval loop and every exit of it, `left % 3` in
{0, 1, 2}), and presence patterns that put an absent block first, last, alone and beside a present transposed row.  Absent blocks of
the inputs hold NaN: a masked reader that fetches one poisons its output row (products) or every sum of the column (weight gradients).

One bound, TOL = 1e-5 per (row, block of C columns) and per (weight-gradient block, row) against the fp64 product of the same operands
with zeros in the absent blocks (tests/level_ref.py) -- the bound of tests/test_level_ops_ex_gpu.py, which measures <= 6e-7 there.  Masked
against dense and run against run the outputs are compared bit for bit.

The stand-alone weight-gradient operator at C = 64 takes the plain table only (gf_smp_level_wgrad_f32), so the packed weight gradients are
exercised at C = 128 (the same kernel, W = 2) and C = 32 / 16 here, and at C = 64 by the model tests of tests/test_smp_gpu.py."""
import functools

import numpy as np
import pytest

import level_ref as lr
import test_level_ops_ex_gpu as ex

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
ROWS = [1, 15, 16, 17, 31, 33, 47, 8 * 16 * 3 + 5]
PATTERNS = ["all_present", "all_sab_absent", "alternating", "last_absent", "last_present", "transposed_differs", "sbc_absent_on_present"]


def pattern_bits(name, trow):
    """(own, trp, bc) of every row: own = the row's S_ab / T6 blocks hold data, trp = own of the transposed row, bc = its S_bc / T10 do"""
    rows = trow.size
    r = np.arange(rows)
    own, bc = np.ones(rows, dtype=bool), np.ones(rows, dtype=bool)
    if name == "all_sab_absent":
        own[:] = False
    elif name == "alternating":
        own = r % 2 == 0
    elif name == "last_absent":
        own[-1] = False
    elif name == "last_present":
        own[:] = False
        own[-1] = True
    elif name == "transposed_differs":
        # every off-diagonal row with the smaller index keeps its data, its transposed row has none: both directions occur
        own = ~(trow < r)
    elif name == "sbc_absent_on_present":
        bc = r % 3 != 1
    else:
        assert name == "all_present"
    return own, own[trow], bc


class Level:
    """operands of one level of `rows` rows (nodes of 3, 2, 1, 3, .. positions) under one presence pattern: the masked inputs carry NaN
    in every absent block (T) and in dO of the rows no source covers (for skip_zero_grads), the dense ones explicit zeros"""

    def __init__(self, rows, Cc, pattern, seed):
        rng = np.random.default_rng(seed)
        sizes = ex.small_sizes(rows, False)
        self.C, self.rows, self.pattern = Cc, rows, pattern
        self.trow, _ = lr.level_rows(sizes)
        assert self.trow.size == rows
        self.bits = own, trp, bc = pattern_bits(pattern, self.trow)
        self.trowf = lr.pack(self.trow, self.bits)
        self.rf = lr.row_factors(sizes, rng, 2)
        self.W = rng.uniform(-1, 1, (8, Cc, Cc)).astype(np.float32)
        T = (rng.standard_normal((rows, 4, Cc)) * np.exp(rng.uniform(-2.3, 2.3, (rows, 1, 1)))).astype(np.float32)
        dO = (rng.standard_normal((rows, 2 * Cc)) * np.exp(rng.uniform(-2.3, 2.3, (rows, 1)))).astype(np.float32)
        have = np.stack([own, bc, own, bc], axis=1)[:, :, None]
        self.T_dense = np.where(have, T, np.float32(0)).reshape(rows, 4 * Cc)
        self.T_nan = np.where(have, T, np.float32(np.nan)).reshape(rows, 4 * Cc)
        self.dO = dO
        self.dO_skip_dense = np.where(bc[:, None], dO, np.float32(0))
        self.dO_skip_nan = np.where(bc[:, None], dO, np.float32(np.nan))
        self.stored = lr.stored_blocks(rows, self.bits, True)


@functools.lru_cache(maxsize=None)
def level(rows, Cc, pattern):
    return Level(rows, Cc, pattern, seed=7919 * rows + 31 * Cc + PATTERNS.index(pattern))


@functools.lru_cache(maxsize=None)
def references(rows, Cc, pattern):
    """the fp64 references of one level, computed once and shared: forward, backward, backward with skip_zero_grads, weight gradients"""
    c = level(rows, Cc, pattern)
    return (lr.forward_ref(c.T_dense, c.rf, c.W, c.trow, Cc, None, c.bits),
            lr.backward_ref(c.dO, c.rf, c.W, c.trow, Cc, None, c.bits),
            lr.backward_ref(c.dO_skip_dense, c.rf, c.W, c.trow, Cc, None, c.bits, True),
            lr.wgrad_ref(c.T_dense, c.dO, c.rf, c.trow, Cc, 0, c.bits)[0])


def same_bits(a, b, keep=None):
    a, b = a.view(np.uint32), b.view(np.uint32)
    return np.array_equal(a, b) if keep is None else np.array_equal(a[keep], b[keep])


def products_and_gradients(c, wgrad):
    """every direction of one level on the masked path against the reference and against the dense path: {name: worst error}"""
    Cc = c.C
    f_ref, b_ref, bs_ref, w_ref = references(c.rows, Cc, c.pattern)
    err = {}
    fwd = ex.run_products(False, Cc, 2, 0, c.T_nan, c.rf, c.W, None, c.trow, c.trowf)
    assert np.isfinite(fwd).all(), "forward read an absent block"
    err["fwd"] = lr.row_block_err(fwd, f_ref, Cc)
    assert same_bits(fwd, ex.run_products(False, Cc, 2, 0, c.T_dense, c.rf, c.W, None, c.trow)), "forward: masked and dense differ"
    bwd = ex.run_products(True, Cc, 2, 0, c.dO, c.rf, c.W, None, c.trow, c.trowf)
    err["bwd"] = lr.row_block_err(bwd, b_ref, Cc)
    assert same_bits(bwd, ex.run_products(True, Cc, 2, 0, c.dO, c.rf, c.W, None, c.trow)), "backward: masked and dense differ"
    if c.pattern != "sbc_absent_on_present":
        # (skip_zero_grads takes dO of a row without bit 29 as zero, and the table's contract -- level_ref.presence_bits -- is that bit 31
        #  implies bit 29 and bit 29 is symmetric: a present row whose S_bc / T10 blocks are absent is outside it, the kernel reads dU of
        #  its transposed row.  That pattern runs forward, backward without the option and the weight gradients.)
        bsk = ex.run_products(True, Cc, 2, 0, c.dO_skip_nan, c.rf, c.W, None, c.trow, c.trowf, skip=True)
        blocks = bsk.reshape(c.rows, 4, Cc)
        assert np.isfinite(blocks[c.stored]).all(), "backward read dO of a row no source covers"
        assert np.all(blocks[~c.stored] == ex.SENTINEL), "skip_zero_grads wrote a block of structural zeros"
        err["bwd_skip"] = lr.row_block_err(bsk, bs_ref, Cc, c.stored)
        dense = ex.run_products(True, Cc, 2, 0, c.dO_skip_dense, c.rf, c.W, None, c.trow).reshape(c.rows, 4, Cc)
        assert same_bits(blocks, dense, c.stored), "backward with skip_zero_grads: masked and dense differ in a stored block"
    if wgrad:
        dW, _ = ex.run_wgrad(Cc, 2, 0, c.T_nan, c.dO, c.rf, c.trow, c.trowf)
        assert np.isfinite(dW).all(), "the weight gradients read an absent block"
        err["wgrad"] = lr.wgrad_row_err(dW, w_ref)
        assert same_bits(dW, ex.run_wgrad(Cc, 2, 0, c.T_dense, c.dO, c.rf, c.trow)[0]), "weight gradients: masked and dense differ"
    return err


def sweep(Cc, pattern, wgrad):
    worst = {}
    for rows in ROWS:
        c = level(rows, Cc, pattern)
        for k, v in products_and_gradients(c, wgrad).items():
            print("C=%d %s rows=%d %s %.2e" % (Cc, pattern, rows, k, v))
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= TOL, (rows, k, v)
    ex.report("masked paths C=%d %s" % (Cc, pattern), worst)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_products_at_64_channels(gf, pattern):
    """forward, backward and backward with skip_zero_grads (the row-class build) on the packed table, NaN in what must not be read"""
    sweep(64, pattern, wgrad=False)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("Cc", [32, 16])
def test_products_and_weight_gradients_at_32_and_16_channels(gf, Cc, pattern):
    sweep(Cc, pattern, wgrad=True)


def run_wgrad64(T, dO, rf, trow):
    ctx = ex.context()
    out = torch.full((8, 64, 64), ex.SENTINEL, device="cuda")
    a, b, r, t = ex.dev(T), ex.dev(dO), ex.dev(rf), ex.dev(trow, np.int32)
    ctx.check(ctx.lib.gf_smp_level_wgrad_f32(ctx.handle, T.shape[0], ex.ptr(a), ex.ptr(b), ex.ptr(r), ex.ptr(t), ex.ptr(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("pattern", ["all_present", "alternating", "last_present"])
def test_weight_gradients_at_64_channels(gf, pattern):
    """the staged kernel's slices at every row count (the plain table: explicit zeros in the absent blocks), twice for the same bits"""
    worst = 0.0
    for rows in ROWS:
        c = level(rows, 64, pattern)
        dW = run_wgrad64(c.T_dense, c.dO, c.rf, c.trow)
        e = lr.wgrad_row_err(dW, references(rows, 64, pattern)[3])
        print("C=64 %s rows=%d wgrad %.2e" % (pattern, rows, e))
        assert e <= TOL, (rows, e)
        worst = max(worst, e)
        assert same_bits(dW, run_wgrad64(c.T_dense, c.dO, c.rf, c.trow)), "weight gradients differ from run to run"
    ex.report("staged weight gradients C=64 %s" % pattern, {"wgrad": worst})


@pytest.mark.parametrize("i,j", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_one_sub_block_pair_at_128_channels(gf, i, j):
    """the masked passes of sub-block (i, j) alone: weights that are nonzero in rows [64 i, +64) x columns [64 j, +64) of every product for
    forward and backward, operands that are nonzero in those halves for the weight gradients (the other three jobs add exact zeros)"""
    rows, Cc = ROWS[-1], 128
    c = level(rows, Cc, "alternating")
    ki, kj = slice(64 * i, 64 * i + 64), slice(64 * j, 64 * j + 64)
    W = np.zeros_like(c.W)
    W[:, ki, kj] = c.W[:, ki, kj]
    err = {}
    fwd = ex.run_products(False, Cc, 2, 0, c.T_nan, c.rf, W, None, c.trow, c.trowf)
    assert np.isfinite(fwd).all()
    err["fwd"] = lr.row_block_err(fwd, lr.forward_ref(c.T_dense, c.rf, W, c.trow, Cc, None, c.bits), Cc)
    assert same_bits(fwd, ex.run_products(False, Cc, 2, 0, c.T_dense, c.rf, W, None, c.trow))
    bsk = ex.run_products(True, Cc, 2, 0, c.dO_skip_nan, c.rf, W, None, c.trow, c.trowf, skip=True)
    blocks = bsk.reshape(rows, 4, Cc)
    assert np.isfinite(blocks[c.stored]).all() and np.all(blocks[~c.stored] == ex.SENTINEL)
    err["bwd_skip"] = lr.row_block_err(bsk, lr.backward_ref(c.dO_skip_dense, c.rf, W, c.trow, Cc, None, c.bits, True), Cc, c.stored)
    dense = ex.run_products(True, Cc, 2, 0, c.dO_skip_dense, c.rf, W, None, c.trow).reshape(rows, 4, Cc)
    assert same_bits(blocks, dense, c.stored)
    # the weight gradients: T in columns [64 i, +64) of every block (NaN where the block is absent), dO in [64 j, +64)
    colsT = np.zeros((1, 4, Cc), dtype=bool)
    colsT[:, :, ki] = True
    T_nan = np.where(colsT | np.isnan(c.T_nan.reshape(rows, 4, Cc)), c.T_nan.reshape(rows, 4, Cc), np.float32(0)).reshape(rows, 4 * Cc)
    T_dense = np.where(colsT, c.T_dense.reshape(rows, 4, Cc), np.float32(0)).reshape(rows, 4 * Cc)
    dO = np.zeros((rows, 2, Cc), dtype=np.float32)
    dO[:, :, kj] = c.dO.reshape(rows, 2, Cc)[:, :, kj]
    dO = dO.reshape(rows, 2 * Cc)
    dW, _ = ex.run_wgrad(Cc, 2, 0, T_nan, dO, c.rf, c.trow, c.trowf)
    assert np.isfinite(dW).all(), "the weight gradients read an absent block"
    rW, _ = lr.wgrad_ref(T_dense, dO, c.rf, c.trow, Cc, 0, c.bits)
    err["wgrad"] = lr.wgrad_row_err(dW[:, ki, kj], rW[:, ki, kj])
    keep = np.zeros((Cc, Cc), dtype=bool)
    keep[ki, kj] = True
    assert np.all(dW[:, ~keep] == 0.0)
    assert same_bits(dW, ex.run_wgrad(Cc, 2, 0, T_dense, dO, c.rf, c.trow)[0]), "weight gradients: masked and dense differ"
    ex.report("masked C=128 sub-block (%d, %d)" % (i, j), err)


@pytest.mark.parametrize("Cc", [64, 32, 16, 128])
def test_same_bits_twice(gf, Cc):
    c = level(ROWS[-1], Cc, "transposed_differs")
    runs = []
    for _ in range(2):
        a = [ex.run_products(False, Cc, 2, 0, c.T_nan, c.rf, c.W, None, c.trow, c.trowf),
             ex.run_products(True, Cc, 2, 0, c.dO_skip_nan, c.rf, c.W, None, c.trow, c.trowf, skip=True).reshape(c.rows, 4, Cc)[c.stored]]
        if Cc != 64:
            a.append(ex.run_wgrad(Cc, 2, 0, c.T_nan, c.dO, c.rf, c.trow, c.trowf)[0])
        runs.append(a)
    for x, y in zip(*runs):
        assert same_bits(np.ascontiguousarray(x), np.ascontiguousarray(y))
