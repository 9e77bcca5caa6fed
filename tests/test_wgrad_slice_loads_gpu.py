"""The slice-based operand loads of the staged weight gradients (smp_wgrad_split of smp_level_wgrad_split.hip, W = 1 at 64 channels and
W = 2 at 128): every request goes through a buffer descriptor rebased per 16-row slice -- the slice's own rows of T and dO, the gathered
rows dU[trow] through a window of 64 x 64 rows on either side of the slice, trow and the row factors through descriptors over their
tables -- and whatever must not be fetched (rows past the end of the level, absent blocks of the packed table) takes an out-of-range
offset and arrives as zeros.

Reach of the stand-alone operators at 64 channels, as of this kernel: gf_smp_level_wgrad_f32 takes the plain table (any permutation of
the rows), gf_smp_level_wgrad_ex_f32 takes C = 64 WITH a packed table (nf = 2, nx = 0) -- the packed weight gradients at 64 channels on
caller-supplied operands, which tests/test_masked_operand_paths_gpu.py's docstring still describes as reachable inside models only.
With the plain table alone the ex operator keeps refusing C = 64 (tests/test_level_ops_ex_gpu.py and tests/test_c128_gpu.py hold it to
that answer).

One bound: every output row of every weight-gradient block against the fp64 product of the same operands (tests/level_ref.py,
wgrad_row_err) at TOL = 1e-5, the bound of tests/test_level_ops_ex_gpu.py and tests/test_masked_operand_paths_gpu.py, which measure
<= 6e-7 there (here: <= 6.1e-7 over every case).  Every call runs twice and must give the same bits.

Absent blocks: at C = 128 they hold NaN (a masked reader that fetches one poisons every sum of the column) and the masked run equals the
dense run bit for bit.  At C = 64 the stand-alone call takes exact column bounds over ALL of T, which NaN would poison: there the absent
blocks hold values drawn like the present ones -- a reader that fetches one is off by O(1) -- and the comparison is against the
reference and run against run.

A table beyond the gather window: gf_smp_level_wgrad_ex_f32 refuses it (GF_ERR_INVALID before any launch) at 64 and 128 channels.
gf_smp_level_wgrad_f32 does NOT: its contract is any permutation of the rows, and tests/test_level_ops_gpu.py runs it on a random
pairing of 5,200 rows, so a refusal there would fail that suite.  It serves such a table through one descriptor over all of dO instead,
and the case of a row 4,097 rows from its transposed row is held here to the reference like every other."""
import functools

import numpy as np
import pytest

import level_ref as lr
import test_level_ops_ex_gpu as ex
from test_masked_operand_paths_gpu import pattern_bits, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
SLICE = 16
# partial last slices; a workgroup gets 1, 2 or 3 slices of the small counts and 6 or 7 of the 25 slices of the last: one and two turns
# of the three-interval loop and each of its exits
ROWS = [1, 15, 16, 17, 31, 33, 47, 8 * 16 * 3 + 5]
PATTERNS = ["all_present", "all_sab_absent", "alternating", "last_absent", "last_present", "transposed_differs"]
# (channels, packed): 64 plain = gf_smp_level_wgrad_f32, the others gf_smp_level_wgrad_ex_f32
PATHS = [(64, False), (64, True), (128, True)]


def draw(rng, rows, blocks, Cc):
    return (rng.standard_normal((rows, blocks, Cc)) * np.exp(rng.uniform(-2.3, 2.3, (rows, 1, 1)))).astype(np.float32)


class Level:
    """operands of one level under presence bits: T_full holds drawn values everywhere, T_dense zeros and T_nan NaN in the absent blocks"""

    def __init__(self, sizes, Cc, bits, seed):
        rng = np.random.default_rng(seed)
        self.C = Cc
        self.trow, _ = lr.level_rows(sizes)
        self.rows = rows = self.trow.size
        self.bits = own, _, bc = bits(self.trow, rng)
        self.trowf = lr.pack(self.trow, self.bits)
        self.rf = lr.row_factors(sizes, rng, 2)
        T = draw(rng, rows, 4, Cc)
        have = np.stack([own, bc, own, bc], axis=1)[:, :, None]
        self.T_full = T.reshape(rows, 4 * Cc)
        self.T_dense = np.where(have, T, np.float32(0)).reshape(rows, 4 * Cc)
        self.T_nan = np.where(have, T, np.float32(np.nan)).reshape(rows, 4 * Cc)
        self.dO = draw(rng, rows, 1, 2 * Cc).reshape(rows, 2 * Cc)

    @functools.cached_property
    def ref(self):
        return lr.wgrad_ref(self.T_dense, self.dO, self.rf, self.trow, self.C, 0, None)[0]

    def operands(self, packed):
        """(T, trowf) of the call: the plain table reads every block, so it gets the explicit zeros"""
        if not packed:
            return self.T_dense, None
        return (self.T_nan if self.C == 128 else self.T_full), self.trowf


@functools.lru_cache(maxsize=None)
def level(rows, Cc, pattern):
    return Level(ex.small_sizes(rows, False), Cc, lambda trow, rng: pattern_bits(pattern, trow), seed=104729 * rows + 31 * Cc + PATTERNS.index(pattern))


def embedded(x, dtype, pad_value):
    """x inside a larger device buffer with one slice's worth of `pad_value` rows before and after: (view, buffer)"""
    x = np.ascontiguousarray(x, dtype=dtype)
    pad = np.full((SLICE,) + x.shape[1:], pad_value, dtype=dtype)
    buf = ex.dev(np.concatenate([pad, x, pad]), dtype)
    return buf[SLICE:SLICE + x.shape[0]], buf


def call(Cc, T, dO, rf, trow, trowf, embed=False):
    """(status, dW prefilled with SENTINEL) of one call of the path's operator"""
    ctx = ex.context()
    keep = []
    if embed:
        huge = np.int32(0x1FFFFFFF)
        a, b, r, t = (embedded(x, d, p) for x, d, p in ((T, np.float32, np.nan), (dO, np.float32, np.nan), (rf, np.float32, np.nan), (trow, np.int32, huge)))
        tf = embedded(trowf, np.int32, np.int32(-1)) if trowf is not None else (None, None)
        keep = [a[1], b[1], r[1], t[1], tf[1]]
        a, b, r, t, tf = a[0], b[0], r[0], t[0], tf[0]
    else:
        a, b, r, t = ex.dev(T), ex.dev(dO), ex.dev(rf), ex.dev(trow, np.int32)
        tf = ex.dev(trowf, np.int32) if trowf is not None else None
    dW = torch.full((8, Cc, Cc), ex.SENTINEL, device="cuda")
    if Cc == 64 and trowf is None:
        st = ctx.lib.gf_smp_level_wgrad_f32(ctx.handle, T.shape[0], ex.ptr(a), ex.ptr(b), ex.ptr(r), ex.ptr(t), ex.ptr(dW))
    else:
        st = ctx.lib.gf_smp_level_wgrad_ex_f32(ctx.handle, Cc, 2, 0, T.shape[0], ex.ptr(a), ex.ptr(b), ex.ptr(r), ex.ptr(t), ex.ptr(tf), ex.ptr(dW), None)
    torch.cuda.synchronize()
    del keep
    return st, dW.cpu().numpy()


def run(*args, **kw):
    st, dW = call(*args, **kw)
    ex.context().check(st)
    return dW


def check_level(c, packed, title):
    """one level on one path: against the reference, twice for the same bits, and (NaN in the absent blocks) masked against dense"""
    T, trowf = c.operands(packed)
    dW = run(c.C, T, c.dO, c.rf, c.trow, trowf)
    assert np.isfinite(dW).all(), "%s: the weight gradients read an absent block" % title
    e = lr.wgrad_row_err(dW, c.ref)
    print("%s wgrad %.2e" % (title, e))
    assert e <= TOL, (title, e)
    assert same_bits(dW, run(c.C, T, c.dO, c.rf, c.trow, trowf)), "%s: weight gradients differ from run to run" % title
    if packed and c.C == 128:
        assert same_bits(dW, run(c.C, c.T_dense, c.dO, c.rf, c.trow, None)), "%s: masked and dense differ" % title
    return e


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("Cc,packed", PATHS, ids=["c64_plain", "c64_packed", "c128_packed"])
def test_slices_and_loop_exits(gf, Cc, packed, pattern):
    worst = 0.0
    for rows in ROWS:
        worst = max(worst, check_level(level(rows, Cc, pattern), packed, "C=%d %s %s rows=%d" % (Cc, "packed" if packed else "plain", pattern, rows)))
    ex.report("slice loads C=%d %s %s" % (Cc, "packed" if packed else "plain", pattern), {"wgrad": worst})


@functools.lru_cache(maxsize=None)
def three_nodes(Cc):
    """nodes of 64, 1 and 64 positions, 8,193 rows: transposed rows up to 63 x 63 = 3,969 rows away, the window cut at row 0 and at the last row"""
    return Level([64, 1, 64], Cc, lambda trow, rng: lr.presence_bits([64, 1, 64], rng), seed=8193 + Cc)


@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("Cc", [64, 128])
def test_both_clamps_of_the_gather_window(gf, Cc, packed):
    c = three_nodes(Cc)
    assert c.rows == 8193 and int(np.abs(c.trow - np.arange(c.rows)).max()) == 63 * 63
    own, trp, _ = c.bits
    assert (own & trp).any() and (own & ~trp).any() and (~own & trp).any()
    ex.report("64 | 1 | 64 positions C=%d %s" % (Cc, "packed" if packed else "plain"),
              {"wgrad": check_level(c, packed, "64|1|64 C=%d %s" % (Cc, "packed" if packed else "plain"))})


@pytest.mark.parametrize("rows", [1, 17, 389])
@pytest.mark.parametrize("Cc,packed", PATHS, ids=["c64_plain", "c64_packed", "c128_packed"])
def test_nothing_outside_the_matrices_is_read(gf, Cc, packed, rows):
    """T, dO, the row factors and the tables inside larger buffers that hold NaN (the tables: a huge index) for a slice's worth of rows
    before and after: finite, and the bits of the run on exact-size buffers"""
    c = level(rows, Cc, "alternating")
    T, trowf = c.operands(packed)
    if Cc == 128:   # (NaN inside the matrix would hide NaN from outside it)
        T = c.T_dense
    exact = run(Cc, T, c.dO, c.rf, c.trow, trowf)
    inside = run(Cc, T, c.dO, c.rf, c.trow, trowf, embed=True)
    assert np.isfinite(inside).all(), "a request left the matrices"
    assert same_bits(inside, exact)
    assert same_bits(inside, run(Cc, T, c.dO, c.rf, c.trow, trowf, embed=True))
    e = lr.wgrad_row_err(inside, c.ref)
    assert e <= TOL, e


def far_table(rows, apart):
    t = np.arange(rows, dtype=np.int32)
    t[0], t[apart] = apart, 0
    return t


def test_a_table_beyond_the_window(gf):
    """4,097 rows apart, one more than the window: refused by the ex operator at 64 and 128 channels before any launch, served by
    gf_smp_level_wgrad_f32 (any permutation of the rows, see the module docstring) -- where dW7 must see both far rows"""
    from graphflow_amd import _lib
    rows = 4200
    sizes = [1] * rows
    far, edge = far_table(rows, 4097), far_table(rows, 4096)
    for Cc in (64, 128):
        c = Level(sizes, Cc, lambda trow, rng: lr.all_present(rows), seed=Cc)
        st, dW = call(Cc, c.T_full, c.dO, c.rf, far, lr.pack(far, c.bits))
        assert st == _lib.GF_ERR_INVALID and np.all(dW == ex.SENTINEL), (Cc, st)
        assert b"window" in ex.context().lib.gf_last_error(ex.context().handle)
        for t in (edge, far) if Cc == 64 else (edge,):   # exactly the window: served by both; beyond it: by the plain C = 64 operator
            for packed in ((False, True) if t is edge else (False,)):
                dW = run(Cc, c.T_full, c.dO, c.rf, t, lr.pack(t, c.bits) if packed else None)
                e = lr.wgrad_row_err(dW, lr.wgrad_ref(c.T_full, c.dO, c.rf, t, Cc)[0])
                print("C=%d %s transposed row %d rows away: %.2e" % (Cc, "packed" if packed else "plain", int(t[0]), e))
                assert e <= TOL, (Cc, packed, int(t[0]), e)
                assert same_bits(dW, run(Cc, c.T_full, c.dO, c.rf, t, lr.pack(t, c.bits) if packed else None))
    # a row outside the matrix is refused by both
    bad = np.arange(rows, dtype=np.int32)
    bad[3] = rows
    c = Level(sizes, 64, lambda trow, rng: lr.all_present(rows), seed=64)
    assert call(64, c.T_full, c.dO, c.rf, bad, None)[0] == _lib.GF_ERR_INVALID


def test_variants_the_kernel_does_not_have_stay_refused(gf):
    """C = 64 with eight row factors or the three extra products: GF_ERR_UNSUPPORTED with and without the packed table, nothing written"""
    from graphflow_amd import _lib
    c = level(17, 64, "alternating")
    for nf, nx in ((8, 0), (2, 3)):
        rf = np.repeat(c.rf[:, :1], nf, axis=1) if nf == 8 else c.rf
        for trowf in (c.trowf, None):
            st, dW, dX = ex.wgrad_status(64, nf, nx, c.T_full, c.dO, rf, c.trow, trowf)
            assert st == _lib.GF_ERR_UNSUPPORTED and np.all(dW == ex.SENTINEL), (nf, nx, st)
            assert dX is None or np.all(dX == ex.SENTINEL)
    check_level(c, True, "after a refusal")
