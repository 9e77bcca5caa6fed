"""Every variant of the fused level's block products (gf_smp_level_products_ex_f32 / gf_smp_level_wgrad_ex_f32: smp_rowpanel_split of
smp_level_c64_split.hip and smp_wgrad_all of smp_level_wgrad_split.hip at C = 64 / 32 / 16, two or eight row factors, with and without the three extra products, on the
plain and on the packed table) against the fp64 product of the same operands (tests/level_ref.py), normalised per (row, block of C
columns) and per (weight-gradient block, row) -- on level-shaped rows that sit on the kernels' edges: nodes of 1 .. 64 positions (the
gathered row 3,969 rows before and after its slice, at both ends of the buffer), row counts around the 32-row panel and the 16 / 32-row
slice, absent blocks filled with garbage.  One bound, TOL = 1e-5; the measured figures are in the table of
tests/test_level_ops_gpu.py's docstring."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import level_ref as lr
from field_suite import dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
SENTINEL = 12345.0
SIZES = [1, 2, 5, 31, 32, 33, 36, 64]                 # 8,496 rows
SIZES_ENDS = [64] + SIZES                             # the 64-position node first and again last
RAGGED = [1, 15, 16, 17, 31, 32, 33, 48, 63, 65, 80]  # around the 32-row panel and the 16-row slice (32 rows at C = 16, in two halves:
                                                      # 17, 33, 48, 65, 80 leave a half-slice short or empty, 33 .. 80 make 2 or 3 slices)
# (C, row factors, extra products) the kernels have
VARIANTS = [(64, 2, 0), (32, 2, 0), (32, 8, 0), (32, 2, 3), (16, 2, 0), (16, 8, 0), (16, 2, 3)]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def context():
    from graphflow_amd.ops import default_context
    return default_context(0)


def products_status(backward, Cc, nf, nx, A, rf, W, X, trow, trowf=None, skip=False):
    """(status, Out prefilled with SENTINEL)"""
    ctx = context()
    rows = A.shape[0]
    out = torch.full((rows, (4 if backward else 2) * Cc), SENTINEL, device="cuda")
    a, r, w, t = dev(A), dev(rf), dev(W), dev(trow, np.int32)
    x = dev(X) if X is not None else None
    tf = dev(trowf, np.int32) if trowf is not None else None
    st = ctx.lib.gf_smp_level_products_ex_f32(ctx.handle, 1 if backward else 0, Cc, nf, nx, rows, ptr(a), ptr(r), ptr(w), ptr(x), ptr(t), ptr(tf),
                                              1 if skip else 0, ptr(out))
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


def run_products(*args, **kw):
    st, out = products_status(*args, **kw)
    context().check(st)
    return out


def wgrad_status(Cc, nf, nx, T, dO, rf, trow, trowf=None):
    ctx = context()
    dW = torch.full((8, Cc, Cc), SENTINEL, device="cuda")
    dX = torch.full((3, Cc, Cc), SENTINEL, device="cuda") if nx else None
    a, b, r, t = dev(T), dev(dO), dev(rf), dev(trow, np.int32)
    tf = dev(trowf, np.int32) if trowf is not None else None
    st = ctx.lib.gf_smp_level_wgrad_ex_f32(ctx.handle, Cc, nf, nx, T.shape[0], ptr(a), ptr(b), ptr(r), ptr(t), ptr(tf), ptr(dW), ptr(dX))
    torch.cuda.synchronize()
    return st, dW.cpu().numpy(), (dX.cpu().numpy() if nx else None)


def run_wgrad(*args, **kw):
    st, dW, dX = wgrad_status(*args, **kw)
    context().check(st)
    return dW, dX


class Case:
    """operands of one level: T with garbage in the absent blocks when `packed`, dO, factors, weights, tables"""

    def __init__(self, sizes, Cc, nf, nx, packed, seed):
        rng = np.random.default_rng(seed)
        self.C, self.nf, self.nx = Cc, nf, nx
        self.trow, _ = lr.level_rows(sizes)
        self.rows = rows = self.trow.size
        self.rf = lr.row_factors(sizes, rng, nf)
        # Rows of O(1) entries whose scale wanders over two decades (2^6.6) from row to row: the products' per-row exponents must follow
        # it.  Not more, because the weight gradients carry ONE exponent per operand column for all rows (smp_wgrad_split's comment: an
        # element keeps its 22 bits down to 2^-17 of the column's BOUND), the bounds of a level are up to max |tot| < 2^5 above the
        # column's maximum, and dropout or an absent block can remove the largest rows from a sum: 2^-(6.6 + 5) stays inside that window
        # with five bits to spare.  (Over four decades the nf = 8 gradients of 32 rows measured 1.1e-5: NOTES.md.)
        self.T = (rng.standard_normal((rows, 4 * Cc)) * np.exp(rng.uniform(-2.3, 2.3, (rows, 1)))).astype(np.float32)
        self.dO = (rng.standard_normal((rows, 2 * Cc)) * np.exp(rng.uniform(-2.3, 2.3, (rows, 1)))).astype(np.float32)
        self.W = rng.uniform(-1, 1, (8, Cc, Cc)).astype(np.float32)
        self.X = rng.uniform(-1, 1, (3, Cc, Cc)).astype(np.float32) if nx else None
        self.bits = lr.presence_bits(sizes, rng) if packed else None
        self.trowf = lr.pack(self.trow, self.bits) if packed else None
        if packed:
            self.T = lr.fill_absent(self.T, Cc, self.bits, rng)
            # dO of a row no source covers is never read under skip_zero_grads: garbage there as well (kept apart: without
            # skip_zero_grads, and in the weight gradients, every row of dO is an operand)
            self.dO_skip = np.array(self.dO)
            gone = np.flatnonzero(~self.bits[2])
            self.dO_skip[gone] = (5.0 * rng.standard_normal((gone.size, 2 * Cc))).astype(np.float32)


def check_case(c, what=("fwd", "bwd", "wgrad")):
    """every direction of one case against the fp64 reference: {name: worst error}"""
    Cc, nf, nx = c.C, c.nf, c.nx
    err = {}
    if "fwd" in what:
        got = run_products(False, Cc, nf, nx, c.T, c.rf, c.W, c.X, c.trow, c.trowf)
        err["fwd"] = lr.row_block_err(got, lr.forward_ref(c.T, c.rf, c.W, c.trow, Cc, c.X, c.bits), Cc)
    if "bwd" in what:
        got = run_products(True, Cc, nf, nx, c.dO, c.rf, c.W, c.X, c.trow, c.trowf)
        err["bwd"] = lr.row_block_err(got, lr.backward_ref(c.dO, c.rf, c.W, c.trow, Cc, c.X, c.bits), Cc)
        if c.bits is not None:
            got = run_products(True, Cc, nf, nx, c.dO_skip, c.rf, c.W, c.X, c.trow, c.trowf, skip=True)
            st = lr.stored_blocks(c.rows, c.bits, True)
            err["bwd_skip"] = lr.row_block_err(got, lr.backward_ref(c.dO_skip, c.rf, c.W, c.trow, Cc, c.X, c.bits, True), Cc, st)
            # the blocks that are gradients of structural zeros still hold what was there
            left = got.reshape(c.rows, 4, Cc)[~st]
            assert np.all(left == SENTINEL), "skip_zero_grads wrote %d values of absent blocks" % int((left != SENTINEL).sum())
    if "wgrad" in what and Cc != 64:
        dW, dX = run_wgrad(Cc, nf, nx, c.T, c.dO, c.rf, c.trow, c.trowf)
        rW, rX = lr.wgrad_ref(c.T, c.dO, c.rf, c.trow, Cc, nx, c.bits)
        err["wgrad"] = lr.wgrad_row_err(dW, rW)
        if nx:
            err["wgrad_x"] = lr.wgrad_row_err(dX, rX)
    return err


def report(title, err):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def level_case(ends, Cc, nf, nx, packed):
    return Case(SIZES_ENDS if ends else SIZES, Cc, nf, nx, packed, seed=1000 * Cc + 100 * nf + 10 * nx + 2 * packed + ends)


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("Cc,nf,nx", VARIANTS)
@pytest.mark.parametrize("ends", [False, True], ids=["nodes_1_to_64", "node_64_at_both_ends"])
def test_level_of_nodes_up_to_64_positions(gf, ends, Cc, nf, nx, packed):
    """8,496 rows of nodes with 1 .. 64 positions (266 panels, 531 slices, 66 workgroups of weight gradients); with the 64-position node
    at both ends of the buffer its transposed rows lie 3,969 rows from their slice where the gather window and the rebased descriptor
    clamp to the matrix."""
    c = level_case(ends, Cc, nf, nx, packed)
    if packed:   # (rows without S_ab / T6, rows without anything, and rows whose transposed row alone has data all occur)
        own, trp, bc = c.bits
        assert (~own & bc).any() and (~bc).any() and (~own & trp).any() and (own & ~trp).any()
    err = check_case(c)
    report("level %s C=%d nf=%d nx=%d %s" % ("64|1..64" if ends else "1..64", Cc, nf, nx, "packed" if packed else "plain"), err)


def test_c64_on_the_fp32_pipe_through_the_same_entry_point(gf, monkeypatch):
    monkeypatch.setenv("GF_SMP_SPLIT", "0")
    report("level 1..64 C=64 fp32 pipe", check_case(level_case(False, 64, 2, 0, False)))


def small_sizes(rows, ones):
    """nodes of one position each, or nodes of 3, 2, 1, 3, 2, 1, .. positions as long as they fit"""
    if ones:
        return [1] * rows
    sizes = []
    for s in itertools.cycle((3, 2, 1)):
        if rows == 0:
            return sizes
        if s * s <= rows:
            sizes.append(s)
            rows -= s * s


@pytest.mark.parametrize("Cc,nf,nx", VARIANTS)
def test_ragged_row_counts(gf, Cc, nf, nx):
    """row counts around the panel of 32 rows and the slices of 16 rows (32 at C = 16, two half-slices of 16 to a tile: an odd number
    of half-slices leaves one empty), single-position nodes (trow = the row itself; every bit of the packed table set) and small nodes,
    plain and packed tables"""
    worst = {}
    for rows in RAGGED:
        for ones in (True, False):
            for packed in (False, True):
                sizes = small_sizes(rows, ones)
                assert sum(s * s for s in sizes) == rows
                c = Case(sizes, Cc, nf, nx, packed, seed=rows + 1000 * ones)
                for k, v in check_case(c).items():
                    worst[k] = max(worst.get(k, 0.0), v)
                    assert v <= TOL, (rows, ones, packed, k, v)
    report("ragged rows C=%d nf=%d nx=%d" % (Cc, nf, nx), worst)


def loud_case(rng, rows, width, Cc, big):
    """tests/test_level_ops_gpu.py's make_case at C channels: in every block of C columns one channel is `big` times the rest of its row"""
    A = rng.standard_normal((rows, width)) * np.exp(rng.uniform(-9, 9, (rows, 1)))
    hot = [Cc * b + int(rng.integers(Cc)) for b in range(width // Cc)]
    A[:, hot] *= big
    return A.astype(np.float32), hot


@pytest.mark.parametrize("Cc", [32, 16])
def test_products_per_row_with_a_loud_channel_inside_a_block(gf, Cc):
    """1e6 : 1 inside a block, weights that IGNORE the loud channel in the first half of the output columns: those outputs are made of
    the small entries alone and are held to the fp64 product relative to their own size (per row and HALF block, as the C = 64 test)."""
    big, h = 1e6, Cc // 2
    sizes = [7] * 21   # 1,029 rows
    rng = np.random.default_rng(Cc)
    trow, _ = lr.level_rows(sizes)
    rows = trow.size
    rf = lr.row_factors(sizes, rng, 2)
    T, hot = loud_case(rng, rows, 4 * Cc, Cc, big)
    W = rng.uniform(-1, 1, (8, Cc, Cc)).astype(np.float32)
    for ch in hot:
        W[:, ch % Cc, :h] = 0.0
    e_f = lr.row_block_err(run_products(False, Cc, 2, 0, T, rf, W, None, trow), lr.forward_ref(T, rf, W, trow, Cc), h)
    dO, hot = loud_case(rng, rows, 2 * Cc, Cc, big)
    W = rng.uniform(-1, 1, (8, Cc, Cc)).astype(np.float32)
    for ch in hot:
        W[:, :h, ch % Cc] = 0.0
    e_b = lr.row_block_err(run_products(True, Cc, 2, 0, dO, rf, W, None, trow), lr.backward_ref(dO, rf, W, trow, Cc), h)
    report("loud channel 1e6 : 1, C=%d, per (row, half block)" % Cc, {"fwd": e_f, "bwd": e_b})


@pytest.mark.parametrize("Cc", [32, 16])
def test_wgrad_per_row_when_one_molecule_dominates_the_level(gf, Cc):
    """tests/test_level_ops_gpu.py's case at C channels: 200 rows are 1e6 times larger than the other 5,000 in half of the channels;
    the rows of dW of the other channels are sums of small terms only (per block, row, column class)."""
    big = 1e6
    sizes = [10] * 52   # 5,200 rows
    rng = np.random.default_rng(7 + Cc)
    trow, _ = lr.level_rows(sizes)
    rows = trow.size
    rf = lr.row_factors(sizes, rng, 2)
    T, dO = rng.standard_normal((rows, 4 * Cc)), rng.standard_normal((rows, 2 * Cc))
    loud = rng.permutation(Cc)[:Cc // 2]
    for b in range(4):
        T[:200, Cc * b + loud] *= big
    for b in range(2):
        dO[:200, Cc * b + loud] *= big
    T, dO = T.astype(np.float32), dO.astype(np.float32)
    got, _ = run_wgrad(Cc, 2, 0, T, dO, rf, trow)
    ref, _ = lr.wgrad_ref(T, dO, rf, trow, Cc)
    quiet = np.setdiff1d(np.arange(Cc), loud)
    worst = max(lr.wgrad_row_err(got[:, :, cols], ref[:, :, cols]) for cols in (loud, quiet))
    report("one molecule 1e6 : 1, C=%d, per (block, row, column class)" % Cc, {"wgrad": worst})


def test_refusals_leave_the_context_usable(gf):
    from graphflow_amd import _lib
    good = Case([3, 2, 1], 32, 2, 0, False, seed=5)

    def still_works():
        report("after a refusal", check_case(good))

    def prod(Cc, nf, nx, trow=None):
        c = Case([3, 2, 1], Cc, nf if nf in (2, 8) else 2, nx, False, seed=6)
        return products_status(False, Cc, nf, nx, c.T, c.rf, c.W, c.X, c.trow if trow is None else trow)

    def wg(Cc, nf, nx, trow=None, sizes=(3, 2, 1)):
        c = Case(list(sizes), Cc, nf if nf in (2, 8) else 2, nx, False, seed=6)
        return wgrad_status(Cc, nf, nx, c.T, c.dO, c.rf, c.trow if trow is None else trow)

    for Cc, nf, nx in [(32, 8, 3), (16, 8, 3), (64, 2, 3), (64, 8, 0), (48, 2, 0), (32, 4, 0), (32, 2, 1), (128, 8, 0), (128, 2, 3)]:
        st, out = prod(Cc, nf, nx)
        assert st == _lib.GF_ERR_UNSUPPORTED and np.all(out == SENTINEL), (Cc, nf, nx, st)
        st, dW, _ = wg(Cc, nf, nx)
        assert st == _lib.GF_ERR_UNSUPPORTED and np.all(dW == SENTINEL), (Cc, nf, nx, st)
        still_works()
    st, dW, _ = wg(64, 2, 0)   # (the weight gradients at C = 64 are gf_smp_level_wgrad_f32's kernel)
    assert st == _lib.GF_ERR_UNSUPPORTED and np.all(dW == SENTINEL)
    # a transposed row outside the matrix, and one beyond the gather window of the weight gradients
    bad = np.arange(14, dtype=np.int32)
    bad[3] = 14
    assert prod(32, 2, 0, bad)[0] == _lib.GF_ERR_INVALID and wg(32, 2, 0, bad)[0] == _lib.GF_ERR_INVALID
    bad[3] = -1
    assert prod(32, 2, 0, bad)[0] == _lib.GF_ERR_INVALID and wg(32, 2, 0, bad)[0] == _lib.GF_ERR_INVALID
    far_sizes = [1] * 4200
    far = np.arange(4200, dtype=np.int32)
    far[0], far[4097] = 4097, 0      # 4,097 rows apart: one more than the window of 64 x 64
    st, dW, _ = wg(16, 2, 0, far, far_sizes)
    assert st == _lib.GF_ERR_INVALID and np.all(dW == SENTINEL)
    assert b"window" in context().lib.gf_last_error(context().handle)
    far = np.arange(4200, dtype=np.int32)
    far[0], far[4096] = 4096, 0      # exactly the window: served
    assert wg(16, 2, 0, far, far_sizes)[0] == _lib.GF_OK
    # a packed table that names other rows than the plain one
    c = Case([3, 2, 1], 32, 2, 0, True, seed=8)
    tf = np.array(c.trowf)
    tf[1] ^= 1
    assert products_status(False, 32, 2, 0, c.T, c.rf, c.W, None, c.trow, tf)[0] == _lib.GF_ERR_INVALID
    assert wgrad_status(32, 2, 0, c.T, c.dO, c.rf, c.trow, tf)[0] == _lib.GF_ERR_INVALID
    still_works()


def test_c32_is_refused_on_the_fp32_pipe(gf, monkeypatch):
    from graphflow_amd import _lib
    c = Case([3, 2, 1], 32, 2, 0, False, seed=9)
    monkeypatch.setenv("GF_SMP_SPLIT", "0")
    st, out = products_status(False, 32, 2, 0, c.T, c.rf, c.W, None, c.trow)
    assert st == _lib.GF_ERR_UNSUPPORTED and np.all(out == SENTINEL)
    st, dW, _ = wgrad_status(32, 2, 0, c.T, c.dO, c.rf, c.trow)
    assert st == _lib.GF_ERR_UNSUPPORTED and np.all(dW == SENTINEL)
    monkeypatch.delenv("GF_SMP_SPLIT")
    report("after a refusal", check_case(c))


def test_the_window_edge_is_served_exactly(gf):
    """rows 0 and 4,096 name each other (the farthest pair the gather window holds) in a level of single positions: dW7 sees both"""
    Cc, rows = 16, 4200
    c = Case([1] * rows, Cc, 2, 0, False, seed=11)
    c.trow = np.arange(rows, dtype=np.int32)
    c.trow[0], c.trow[4096] = 4096, 0
    report("transposed row 4,096 rows away", check_case(c))


@pytest.mark.parametrize("Cc,nf,nx,packed", [(32, 2, 3, True), (16, 8, 0, True), (64, 2, 0, True), (16, 2, 3, False)])
def test_same_bits_twice(gf, Cc, nf, nx, packed):
    c = level_case(False, Cc, nf, nx, packed)
    for _ in range(2):
        a = [run_products(False, Cc, nf, nx, c.T, c.rf, c.W, c.X, c.trow, c.trowf), run_products(True, Cc, nf, nx, c.dO, c.rf, c.W, c.X, c.trow, c.trowf)]
        if Cc != 64:
            a += [x for x in run_wgrad(Cc, nf, nx, c.T, c.dO, c.rf, c.trow, c.trowf) if x is not None]
        if _ == 0:
            first = a
    for x, y in zip(first, a):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
