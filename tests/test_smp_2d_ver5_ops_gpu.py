"""The kernels of SMP_2D_ver5's level one by one (gf_smp_2d_ver5_rows_ex_f32 / _cols_ex_f32 / _wgrad_ex_f32: v5_row_proj, v5_col_proj,
v5_wgrad and v5_wgrad_fold of smp_level_2d_ver5.hip, launched as the level launches them) against the fp64 evaluation of the same
operands (tests/smp2d_ver5_ops_ref.py), per output row and per row of each half of dK, relative to the row's magnitude sum.  One bound,
TOL = 1e-5 (tests/util.py).  A correct fp32 evaluation measures 1e-7 .. 5e-7 by these measures (asserted per case,
on the reference alone, with the other conditions on the inputs: Level.check_conditions); a misplaced element is wrong by the order
of the magnitude itself.  The shapes: every instantiation of the row projection and the weight gradients (C = 5 .. 128: one to four
32-channel tiles, 16-byte and scalar operand loads, full and ragged last tiles), row counts around the 32-row tile, the 4-tile
workgroup, the 16-row group and the 512-row chunk, a grid that strides over the tiles, the fold with several images per run, with short
and empty runs, and one node 1e4 times louder than the rest.  The measured figures are in NOTES.md."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import smp2d_ver5_ops_ref as ops
from field_suite import dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5
SENTINEL = 12345.0
TAIL = 8                          # sentinel floats behind the last row of every output
CHUNK, FOLD_RUNS = 512, 16        # kV5Chunk, kV5FoldGroups of smp_level_2d_ver5.hip
WIDTHS = [5, 6, 8, 31, 32, 33, 40, 64, 65, 66, 72, 96, 97, 100, 127, 128]
NODES = [1, 2, 3, 5, 7, 9, 12] * 6   # 1,878 rows (58 full tiles and one of 22 rows, four chunks of dK1), 234 columns
RAGGED = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1023, 1025]


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def context():
    from graphflow_amd.ops import default_context
    return default_context(0)


def guarded(n, fill=None):
    """n floats of SENTINEL (or `fill`) with TAIL sentinels behind them"""
    t = torch.full((n + TAIL,), SENTINEL, device="cuda")
    if fill is not None:
        t[:n] = dev(fill).reshape(-1)
    return t


def taken(t, shape, written=True):
    """the result inside a guarded buffer: the tail intact, and no sentinel left inside"""
    a = t.cpu().numpy()
    n = int(np.prod(shape))
    assert np.all(a[n:] == SENTINEL), "wrote behind the last row"
    if written:
        assert not np.any(a[:n] == SENTINEL), "%d elements were not written" % int((a[:n] == SENTINEL).sum())
    return a[:n].reshape(shape)


def rows_status(lv, backward, cap=0, C_=None, rows=None, cols=None, nsizes=None, row_cs=None):
    ctx = context()
    Cn = lv.C if C_ is None else C_
    out = guarded(lv.rows * lv.C)
    k, x, sz, u, rc = dev(lv.K), dev(lv.dz if backward else lv.S), dev(lv.sizes), dev(lv.u), dev(lv.row_cs if row_cs is None else row_cs, np.int32)
    st = ctx.lib.gf_smp_2d_ver5_rows_ex_f32(ctx.handle, 1 if backward else 0, Cn, lv.rows if rows is None else rows, lv.cols if cols is None else cols,
                                            lv.nsizes if nsizes is None else nsizes, ptr(k), ptr(x), ptr(sz), ptr(u), ptr(rc), ops.ALPHA, cap, ptr(out))
    torch.cuda.synchronize()
    return st, out


def run_rows(lv, backward, cap=0):
    st, out = rows_status(lv, backward, cap)
    context().check(st)
    return taken(out, (lv.rows, lv.C))


def cols_status(lv, backward, C_=None, cols=None, nsizes=None, ldin=None, col_s=None):
    ctx = context()
    out = guarded(lv.cols * lv.C)
    ld = (lv.ldcz if backward else lv.C) if ldin is None else ldin
    k, x, sz, cs = dev(lv.K), dev(lv.cz_wide if backward else lv.col), dev(lv.sizes), dev(lv.col_s if col_s is None else col_s, np.int32)
    st = ctx.lib.gf_smp_2d_ver5_cols_ex_f32(ctx.handle, 1 if backward else 0, lv.C if C_ is None else C_, lv.cols if cols is None else cols,
                                            lv.nsizes if nsizes is None else nsizes, ptr(k), ptr(x), ld, ptr(sz), ptr(cs), ptr(out))
    torch.cuda.synchronize()
    return st, out


def run_cols(lv, backward):
    st, out = cols_status(lv, backward)
    context().check(st)
    return taken(out, (lv.cols, lv.C))


def wgrad_status(lv, zero=None, C_=None, rows=None, cols=None, nsizes=None, ldcz=None, row_cs=None, col_s=None):
    """dK prefilled with lv.dK0; zero = "dz" / "cz": that operand all zeros (its half of dK gets nothing added)"""
    ctx = context()
    dK = guarded(2 * lv.C * lv.C, lv.dK0)
    dz = dev(np.zeros_like(lv.dz) if zero == "dz" else lv.dz)
    czw = np.array(lv.cz_wide)
    if zero == "cz":
        czw[:, :lv.C] = 0
    S, cz, col, sz = dev(lv.S), dev(czw), dev(lv.col), dev(lv.sizes)
    rc, cs = dev(lv.row_cs if row_cs is None else row_cs, np.int32), dev(lv.col_s if col_s is None else col_s, np.int32)
    st = ctx.lib.gf_smp_2d_ver5_wgrad_ex_f32(ctx.handle, lv.C if C_ is None else C_, lv.rows if rows is None else rows, lv.cols if cols is None else cols,
                                             lv.nsizes if nsizes is None else nsizes, ptr(dz), ptr(S), ptr(rc), ptr(cz), lv.ldcz if ldcz is None else ldcz,
                                             ptr(col), ptr(cs), ptr(sz), ptr(dK))
    torch.cuda.synchronize()
    return st, dK


def run_wgrad(lv, zero=None):
    st, dK = wgrad_status(lv, zero)
    context().check(st)
    return taken(dK, (lv.C, 2 * lv.C), written=False)


RUN = {"rows_fwd": lambda lv: run_rows(lv, False), "rows_bwd": lambda lv: run_rows(lv, True), "cols_fwd": lambda lv: run_cols(lv, False),
       "cols_bwd": lambda lv: run_cols(lv, True), "wgrad": run_wgrad}


def check_level(lv, what=ops.Level.OPS):
    """the conditions on the inputs, then every operation of `what` against the reference: {name: worst error} (dK per half)"""
    lv.check_conditions(TOL, what)
    err = {}
    for op in what:
        got = RUN[op](lv)
        if op == "wgrad":
            err["dK1"], err["dK2"] = ops.half_err(got, *lv.ref(op))
        else:
            err[op] = lv.err(op, got)
    return err


def report(title, err):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, (title, bad)


@functools.lru_cache(maxsize=None)
def level_case(Cn, loud=False):
    """the level of NODES, shuffled: tiles and 16-row groups span nodes of different sizes; ldcz = 4 C as in the level's backward"""
    sizes = [int(s) for s in np.random.default_rng(100 + Cn).permutation(NODES)]
    lv = ops.Level(sizes, Cn, seed=Cn + (1000 if loud else 0), ldcz=4 * Cn, loud=sizes.index(12) if loud else None)
    assert lv.rows == 1878 and lv.rows % 32 != 0 and lv.rows > CHUNK and lv.cols == 234
    return lv


@pytest.mark.parametrize("Cn", WIDTHS)
def test_every_instantiation(gf, Cn):
    """NT = 1 .. 4 tiles of 32 channels, 16-byte (4 | C) and scalar operand loads, full and ragged last tiles in the output and in the
    reduction dimension, both sides of every 32-channel boundary; at C = 128 the LDS images of both projections need the opt-in.  Both row
    projections, both column projections (the backward with rows 4 C floats apart) and the weight gradients over four chunks."""
    report("level of 1,878 rows, C=%d" % Cn, check_level(level_case(Cn)))


def sizes_adding_up_to(rows, cycle=(3, 2, 1)):
    """nodes of the cycle's sizes (1 among them) as long as they fit: a trailing run of single positions fills up"""
    sizes = []
    for s in itertools.cycle(cycle):
        if rows == 0:
            return sizes
        if s * s <= rows:
            sizes.append(s)
            rows -= s * s


@pytest.mark.parametrize("Cn", [32, 40, 96, 128])
def test_ragged_row_counts(gf, Cn):
    """row counts around the 32-row tile, the 4-tile workgroup (128), the 16-row group of the weight gradients and the 512-row chunk"""
    worst = {}
    for rows in RAGGED:
        sizes = sizes_adding_up_to(rows)
        lv = ops.Level(sizes, Cn, seed=rows, ldcz=4 * Cn)
        assert lv.rows == rows
        for k, v in check_level(lv).items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= TOL, (rows, k, v)
    report("ragged rows C=%d" % Cn, worst)


STRIDE_ROWS = 32 * 37 + 5   # 38 tiles, the last one of five rows


@functools.lru_cache(maxsize=None)
def stride_case(Cn):
    lv = ops.Level(sizes_adding_up_to(STRIDE_ROWS, (5, 3, 7, 2, 1)), Cn, seed=7 * Cn)
    assert lv.rows == STRIDE_ROWS
    lv.check_conditions(TOL, ("rows_fwd", "rows_bwd"))
    return lv


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("Cn", [8, 64, 72, 128])
def test_grid_stride(gf, Cn, backward):
    """38 tiles on 1, 2, 3 and 7 workgroups of four waves: one workgroup runs ten rounds; with 3 and 7 some waves have no tile in the
    last round, and the last tile is ragged.  Within the bound, and the bits of the level's own grid (here: every tile in round one)."""
    lv = stride_case(Cn)
    op = "rows_bwd" if backward else "rows_fwd"
    whole = run_rows(lv, backward, 0)
    err = {"cap 0": lv.err(op, whole)}
    for cap in (1, 2, 3, 7):
        got = run_rows(lv, backward, cap)
        err["cap %d" % cap] = lv.err(op, got)
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), cap
    report("38 tiles, C=%d %s" % (Cn, op), err)


def test_the_levels_own_grid_strides(gf):
    """300,001 rows at C = 64 with max_workgroups = 0: no occupancy puts more than 2,048 workgroups of 256 threads on 256 CUs, and those
    hold 262,144 rows in one round, so the level's own grid strides here whatever the device reports -- with a ragged last tile"""
    lv = ops.Level([12] * 2083 + [7], 64, seed=64)
    assert lv.rows == 300001
    what = ("rows_fwd", "rows_bwd")
    report("300,001 rows, C=64", check_level(lv, what))


def fold_sizes(n1, n2, seed):
    """nodes of 20, 3 and 1 positions, shuffled, whose rows make n1 chunks of dK1 and whose columns make n2 of dK2"""
    for big in range(0, 200):
        for mid in (5, 0):
            r0, c0 = 400 * big + 9 * mid, 20 * big + 3 * mid
            lo = max((n1 - 1) * CHUNK + 1 - r0, (n2 - 1) * CHUNK + 1 - c0, 0)
            hi = min(n1 * CHUNK - r0, n2 * CHUNK - c0)
            if lo <= hi:
                ones = (lo + hi) // 2
                sizes = [20] * big + [3] * mid + [1] * ones
                return [int(s) for s in np.random.default_rng(seed).permutation(sizes)]
    raise AssertionError((n1, n2))


# (n1, n2): per = ceil(n / 16) images per run.  (16, 1): one image per run, every run used; (17, 2): per1 = 2, a short ninth run and
# seven empty ones, per2 = 1; (31, 2): a short last run; (33, 17): per1 = 3 with five empty runs, per2 = 2 with a short ninth run and
# seven empty ones; (48, 17): per1 = 3, every run full; (17, 17): per1 = per2 = 2 on a level of single positions mostly
FOLDS = [(16, 1), (17, 2), (31, 2), (33, 17), (48, 17), (17, 17)]


@functools.lru_cache(maxsize=None)
def fold_case(Cn, n1, n2):
    lv = ops.Level(fold_sizes(n1, n2, n1 + n2), Cn, seed=Cn + n1 + n2, ldcz=Cn + 4)
    assert ((lv.rows + CHUNK - 1) // CHUNK, (lv.cols + CHUNK - 1) // CHUNK) == (n1, n2)
    return lv


def test_fold_cases_cover_the_runs():
    """what the list above says of itself"""
    per = lambda n: -(-n // FOLD_RUNS)   # noqa: E731
    empty = lambda n: sum(1 for g in range(FOLD_RUNS) if g * per(n) >= n)   # noqa: E731
    short = lambda n: n % per(n) != 0   # noqa: E731
    assert {n for n, _ in FOLDS} == {16, 17, 31, 33, 48} and {n for _, n in FOLDS} == {1, 2, 17}
    assert any(per(a) != per(b) and per(a) >= 2 and per(b) >= 2 for a, b in FOLDS)
    assert empty(17) == 7 and short(17) and empty(33) == 5 and short(31) and empty(48) == 0 and empty(16) == 0 and empty(2) == 14


@pytest.mark.parametrize("n1,n2", FOLDS)
@pytest.mark.parametrize("Cn", [8, 40, 100])
def test_fold_with_several_images_per_run(gf, Cn, n1, n2):
    """dK prefilled with random values (the +=); both halves against the reference; then each half with the OTHER half's operands zeroed,
    where the untouched half must equal its prefill bit for bit"""
    lv = fold_case(Cn, n1, n2)
    lv.check_conditions(TOL, ("wgrad",))
    ref, mag = lv.ref("wgrad")
    err = {}
    err["dK1"], err["dK2"] = ops.half_err(run_wgrad(lv), ref, mag)
    pre = lv.dK0.view(np.uint32)
    only2 = run_wgrad(lv, zero="dz")
    assert np.array_equal(only2[:, :Cn].view(np.uint32), pre[:, :Cn])
    err["dK2 alone"] = ops.half_err(only2, ref, mag)[1]
    only1 = run_wgrad(lv, zero="cz")
    assert np.array_equal(only1[:, Cn:].view(np.uint32), pre[:, Cn:])
    err["dK1 alone"] = ops.half_err(only1, ref, mag)[0]
    report("fold n1=%d n2=%d (%d rows, %d columns), C=%d" % (n1, n2, lv.rows, lv.cols, Cn), err)


@pytest.mark.parametrize("Cn", [40, 128])
def test_one_loud_node(gf, Cn):
    """One 12-position node's rows and columns are 1e4 times the rest.  The projections are per row, so every quiet row -- also one that
    shares its tile with loud rows -- is held to its own magnitude sum.  dK is one sum over all rows: its measure is relative to the
    magnitude sum of the image's row, which the loud node dominates, and a float32 evaluation of that sum holds TOL / 2 (asserted by
    check_conditions), so the same bound applies.  The measured figures are in NOTES.md."""
    lv = level_case(Cn, loud=True)
    assert 0 < lv.loud_rows.sum() == 144
    err = check_level(lv)
    quiet = ~lv.loud_rows
    for op, backward in (("rows_fwd", False), ("rows_bwd", True)):
        ref, den = lv.ref(op)
        err[op + " quiet"] = ops.row_err(run_rows(lv, backward)[quiet], ref[quiet], den[quiet])
    report("one node 1e4 : 1, C=%d" % Cn, err)


def all_outputs(lv, cap=0):
    return [run_rows(lv, False, cap), run_rows(lv, True, cap), run_cols(lv, False), run_cols(lv, True), run_wgrad(lv)]


@pytest.mark.parametrize("case", ["level C=5", "level C=128", "fold C=100 (33, 17)", "stride C=72 cap 3"])
def test_same_bits_twice(gf, case):
    lv, cap = {"level C=5": (level_case(5), 0), "level C=128": (level_case(128), 0), "fold C=100 (33, 17)": (fold_case(100, 33, 17), 0),
               "stride C=72 cap 3": (stride_case(72), 3)}[case]
    first, again = all_outputs(lv, cap), all_outputs(lv, cap)
    for x, y in zip(first, again):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_refusals_leave_the_context_usable(gf):
    """every refusal answers GF_ERR_INVALID and writes nothing; then the same context serves a call"""
    from graphflow_amd import _lib
    lv = ops.Level([3, 2, 1, 4], 8, seed=3, ldcz=12)

    def refused(st_out, prefill=None):
        st, out = st_out
        a = out.cpu().numpy()
        assert st == _lib.GF_ERR_INVALID, st
        assert np.all(a == SENTINEL) if prefill is None else np.array_equal(a[:prefill.size], prefill.ravel()) and np.all(a[prefill.size:] == SENTINEL)
        assert context().lib.gf_last_error(context().handle)

    def still_works():
        err = {}
        for op in ops.Level.OPS:
            got = RUN[op](lv)
            err[op] = max(ops.half_err(got, *lv.ref(op))) if op == "wgrad" else lv.err(op, got)
        report("after a refusal", err)

    bad_s, bad_0, bad_col, neg_col = (np.array(lv.row_cs) for _ in range(4))
    bad_s[5, 1], bad_0[29, 1], bad_col[7, 0], neg_col[0, 0] = lv.nsizes + 1, 0, lv.cols, -1
    cs_hi, cs_lo = np.array(lv.col_s), np.array(lv.col_s)
    cs_hi[-1], cs_lo[0] = lv.nsizes + 1, 0
    for backward in (0, 1):
        for kw in (dict(C_=0), dict(C_=129), dict(C_=-1), dict(rows=0), dict(rows=-5)):
            refused(rows_status(lv, backward, **kw))
        for kw in (dict(C_=0), dict(C_=129), dict(cols=0), dict(ldin=lv.C - 1)):
            refused(cols_status(lv, backward, **kw))
        still_works()
    for kw in (dict(cols=0), dict(row_cs=bad_s), dict(row_cs=bad_0), dict(row_cs=bad_col), dict(row_cs=neg_col), dict(nsizes=lv.nsizes - 1)):
        refused(rows_status(lv, 0, **kw))
    for kw in (dict(col_s=cs_hi), dict(col_s=cs_lo), dict(nsizes=lv.nsizes - 1)):
        refused(cols_status(lv, 0, **kw))
    still_works()
    for kw in (dict(C_=0), dict(C_=129), dict(rows=0), dict(cols=0), dict(ldcz=lv.C - 1), dict(row_cs=bad_s), dict(row_cs=bad_0),
               dict(row_cs=bad_col), dict(row_cs=neg_col), dict(col_s=cs_hi), dict(col_s=cs_lo), dict(nsizes=lv.nsizes - 1)):
        refused(wgrad_status(lv, **kw), prefill=lv.dK0)
    still_works()
