"""The cases tests/test_smp_gru_ops_gpu.py runs through gf_smp_gru_*_ex_f32, built from fixed seeds on the host so that
tests/test_smp_gru_ops.py can check the very operands the GPU suite will use (a numpy float32 evaluation of every case stays within
TOL / 2 of the fp64 one by every measure, and outside the gate-range cases at least half of z, r and c is unsaturated), and the checks
both suites share: a backend (the device, or Numpy32 here) runs an operator on a case's operands, check_* holds every output row to
tests/gru_ops_ref.py in fp64.

Operands are dyadic: gradients, targets and U in eighths; hprev in multiples of 2^-12 within [-1, 1], both signs (h_l is no softmax
vector); Tprev exactly its row sums; the eight matrices integers in -8 .. 8 over 2 * 2^max(1, ceil(log2 H)) (eighths over a power of two of
at least H / 4; at one channel quarters, or more than half of z would sit at an end), W_z, W_r, W_h halved further until the aggregate's part of a pre-activation stays at a few units."""
import functools

import numpy as np

import gru_ops_ref as ops
from neighbourhood_ops_cases import eighths, long_lists, mixed_lists, molecules_of, slots, sparse_lists

TOL = 1e-5
TINY = 2.0 ** -126
SUM, PAIRS, GIVEN = ops.SUM, ops.PAIRS, ops.GIVEN
FORM_NAMES = {SUM: "sum", PAIRS: "pairs", GIVEN: "given"}
WIDTHS = (1, 5, 8, 9, 16, 17, 32, 33, 63, 64)
ROUND_WIDTHS = (8, 20, 64)
RANGE_WIDTHS = (1, 5, 33, 64)
LONG_WIDTHS = (20, 64)
READOUT_MOLS = (1, 15, 16, 17, 33)
READOUT_WIDTHS = (5, 33, 64)
CELL_OWN_WIDTHS = (64, 20)
READOUT_OWN_WIDTHS = (64,)


def round_sizes(H):
    s = slots(H)
    return (1, s - 1, s, s + 1, 2 * s - 1, 2 * s + 1, 6 * s + 1)


def lds_bytes(kernel, H):
    """the dynamic LDS of a kernel of the level (smp_level_gru.hip's launchers)"""
    s = slots(H)
    return 4 * {"cell_fwd": 6 * H * (H | 1) + 3 * s * H, "cell_bwd": 6 * H * H + 3 * s * H, "readout_fwd": 2 * H * (H | 1) + s * H,
                "readout_bwd": 2 * H * H + 2 * s * H}[kernel]


def own_round(kernels, H):
    """the vertices of one round of the level's own grid (vertices_per_group): 256 CUs times the workgroups whose LDS fits one CU side
    by side, at most four, times the slots -- the same for every kernel named, or the case would not reach the second round of each"""
    per = {slots(H) * 256 * max(1, min(4, 160 * 1024 // lds_bytes(k, H))) for k in kernels}
    assert len(per) == 1, (kernels, H, per)
    return per.pop()


def weights(rng, count, H):
    return (rng.integers(-8, 9, (count, H, H)) / (2.0 * 2 ** max(1, int(np.ceil(np.log2(H)))))).astype(np.float32)


class Case:
    """One level's operands (float32) over nV vertices: lists (ptr, idx) with their transpose, M6, hprev, Tprev, the aggregate
    n_given that is the operand of the given form, dh, and a read-out over molecules mol_ptr: M2, U, target, dU0, vmol"""

    def __init__(self, H, agg, lists, seed, mol_sizes=(1, 3, 40, 2)):
        rng = np.random.default_rng(seed)
        self.H, self.agg, self.pairs = H, agg, agg == PAIRS
        self.ptr, self.idx = ops.csr(lists) if isinstance(lists, list) else lists
        self.nV = nV = len(self.ptr) - 1
        self.tptr, self.tidx = ops.transpose(self.ptr, self.idx, nV)
        self.hprev = (rng.integers(-4096, 4097, (nV, H)) / 4096).astype(np.float32)
        self.set_T()
        self.M6, self.M2 = weights(rng, 6, H), weights(rng, 2, H)
        nmag = float(np.median(ops.row_den(ops.aggregate(self.hprev, self.Tprev, self.ptr, self.idx, self.pairs, magnitude=True))))
        self.M6[0::2] *= np.float32(2.0 ** -int(np.ceil(np.log2(max(1.0, nmag / 4)))))
        self.dh = eighths(rng, -8, 8, (nV, H))
        self.mol_ptr = molecules_of(nV, mol_sizes)
        self.nMol = len(self.mol_ptr) - 1
        self.vmol = np.repeat(np.arange(self.nMol), np.diff(self.mol_ptr)).astype(np.int32)
        self.U, self.target, self.dU0 = eighths(rng, -4, 4, H), eighths(rng, -8, 8, self.nMol), eighths(rng, -8, 8, H)
        self.A_any, self.Tt_any = eighths(rng, -8, 8, (nV, H)), eighths(rng, -8, 8, nV)   # (a backward on gates that are operands)
        self.single = np.diff(self.ptr) == 1   # pairs: n is exactly 0 there
        self.saturating = False

    def set_T(self):
        T = self.hprev.astype(np.float64).sum(axis=1)
        self.Tprev = T.astype(np.float32)
        assert np.array_equal(self.Tprev.astype(np.float64), T)
        # (the sums over the TRANSPOSED lists: an n of the same kind that is not what a gather over ptr / idx would give)
        self.n_given = ops.aggregate(self.hprev, None, self.tptr, self.tidx, False, dt=np.float32)["n"]


class Numpy32:
    """the operators evaluated by tests/gru_ops_ref.py in float32: the backend of the CPU suite"""

    def cell_fwd(self, c, rounds=0, agg=None, given=None):
        agg = c.agg if agg is None else agg
        out = ops.cell_forward(c.M6, c.hprev, c.Tprev, c.ptr, c.idx, agg, c.n_given if given is None else given, dt=np.float32)
        if agg != PAIRS:
            out["T"] = None
        return out

    def cell_bwd(self, c, z, r, cc, A, Tt, rounds=0, pairs=None):
        return ops.cell_backward(c.M6, c.hprev, c.dh, z, r, cc, A, Tt, c.pairs if pairs is None else pairs, dt=np.float32)

    def gather(self, c, dn, gTt, sA):
        return ops.gather_backward(c.tptr, c.tidx, dn, c.hprev, c.Tprev, c.pairs, dt=np.float32)

    def readout_fwd(self, c, hL, rounds=0, target=True, loss=True):
        r = ops.readout_forward(c.M2, c.U, hL, c.mol_ptr, c.target if target else None, dt=np.float32)
        if not loss:
            r["loss"] = None
        return r

    def readout_bwd(self, c, s, t, g, dy, rounds=0):
        return ops.readout_backward(c.M2, c.U, s, t, g, dy, c.vmol, c.dU0, dt=np.float32)


def gate_err(x, ref, den):
    """row_err of a sigmoid output; a row whose reference lies wholly below 2^-126 (no normal fp32 number) must be finite, non-negative
    and at most 2^-126"""
    x = np.asarray(x, dtype=np.float64)
    tiny = ref.max(axis=1) < TINY
    assert np.all(np.isfinite(x[tiny])) and np.all(x[tiny] >= 0) and np.all(x[tiny] <= TINY), "a gate below 2^-126 is not a small number"
    return ops.row_err(x[~tiny], ref[~tiny], den[~tiny]) if (~tiny).any() else 0.0


def check_cell_forward(c, out, agg=None, n=None):
    """{output: worst row error}; every stored value finite; with pairs a list of one member must give n = +0 bit for bit; where the
    stored z is exactly 0 h is hp bit for bit, where it is exactly 1 h is c"""
    agg = c.agg if agg is None else agg
    n = c.n_given if n is None else n
    args = (c.M6, c.hprev, c.Tprev, c.ptr, c.idx, agg, n)
    ref = ops.cell_forward(*args)
    den = ops.cell_forward_dens(*args, ref)
    for k in den:
        assert np.all(np.isfinite(out[k])), "%s is not finite" % k
    err = {k: gate_err(out[k], ref[k], den[k]) if k in "zr" else ops.row_err(out[k], ref[k], den[k]) for k in den}
    if agg == PAIRS and c.single.any():   # (a member's entry that is 0 itself gives 0 with the sign of Tt: a Tt = -0, and -0 - +0 = -0)
        n1, a1 = np.asarray(out["n"], dtype=np.float32)[c.single], c.hprev[c.idx[c.ptr[:-1][c.single]]]
        assert not n1.any() and not n1.view(np.uint32)[a1 != 0].any(), "one member: n is not exactly +0"
    z, h = np.asarray(out["z"]), np.asarray(out["h"], dtype=np.float32)
    assert np.array_equal(h[z == 0].view(np.uint32), c.hprev[z == 0].view(np.uint32)), "z = 0: h is not hp"
    assert np.array_equal(h[z == 1].view(np.uint32), np.asarray(out["c"], dtype=np.float32)[z == 1].view(np.uint32)), "z = 1: h is not c"
    return err


def check_cell_backward(c, z, r, cc, A, Tt, out, pairs=None):
    """z, r, c, A, Tt are those the backend was given.  dz' is exactly 0 where z is 0 or 1, dc' where z = 0 or |c| = 1, dr' where r is
    0 or 1"""
    pairs = c.pairs if pairs is None else pairs
    args = (c.M6, c.hprev, c.dh, z, r, cc, A, Tt, pairs)
    ref, mag = ops.cell_backward(*args), ops.cell_backward(*args, magnitude=True)
    z, r, cc = (np.asarray(a) for a in (z, r, cc))
    assert not np.asarray(out["dzp"])[(z == 0) | (z == 1)].any(), "dz' at a saturated z"
    assert not np.asarray(out["dcp"])[(z == 0) | (np.abs(cc) == 1)].any(), "dc' at z = 0 or |c| = 1"
    assert not np.asarray(out["drp"])[(r == 0) | (r == 1)].any(), "dr' at a saturated r"
    return {k: ops.row_err(out[k], ref[k], ops.row_den(mag[k])) for k in ref}


def check_prev(c, dn, direct, gathered):
    """dh_{l-1} = the gather of the backend's dn + its direct part, added on the host in fp32 in that order"""
    args = (c.tptr, c.tidx, dn, c.hprev, c.Tprev, c.pairs)
    ref = ops.gather_backward(*args)   # (hprev has both signs here: the magnitude sum is that of |hprev|, |Tprev|)
    mag = ops.gather_backward(c.tptr, c.tidx, dn, np.abs(c.hprev), np.abs(c.Tprev), c.pairs, magnitude=True)
    if c.pairs:   # a source nobody consumes: exactly 0
        assert not np.asarray(gathered)[np.diff(c.tptr) == 0].any(), "a source without consumers has a gradient"
    total = np.asarray(gathered, dtype=np.float32) + np.asarray(direct, dtype=np.float32)
    d = np.asarray(direct, dtype=np.float64)
    return {"gather": ops.row_err(gathered, ref, ops.row_den(mag)), "dhprev": ops.row_err(total, ref + d, ops.row_den(mag + np.abs(d)))}, total


def check_readout_forward(c, hL, out, target=True, loss=True):
    """an empty molecule gives g = 0 exactly"""
    args = (c.M2, c.U, hL, c.mol_ptr, c.target if target else None)
    ref = ops.readout_forward(*args)
    den = ops.readout_forward_dens(*args, ref)
    keys = ["s", "t", "g", "yhat", "dy"] + (["loss"] if loss else [])
    for k in keys:
        assert np.all(np.isfinite(out[k])), "%s is not finite" % k
    assert not np.asarray(out["g"])[np.diff(c.mol_ptr) == 0].any(), "an empty molecule has a graph feature"
    return {k: gate_err(out[k], ref[k], den[k]) if k == "s" else ops.row_err(out[k], ref[k], den[k]) for k in keys}


def check_readout_backward(c, s, t, g, dy, out):
    """ds is exactly 0 where s is 0 or 1 or |g| = 1, dt where s = 0, |t| = 1 or |g| = 1"""
    args = (c.M2, c.U, s, t, g, dy, c.vmol, c.dU0)
    ref, mag = ops.readout_backward(*args), ops.readout_backward(*args, magnitude=True)
    s, t, gv = np.asarray(s), np.asarray(t), np.abs(np.asarray(g))[c.vmol]
    assert not np.asarray(out["ds"])[(s == 0) | (s == 1) | (gv == 1)].any(), "ds at a saturated end"
    assert not np.asarray(out["dt"])[(s == 0) | (np.abs(t) == 1) | (gv == 1)].any(), "dt at a saturated end"
    return {k: ops.row_err(np.atleast_2d(out[k]), np.atleast_2d(ref[k]), ops.row_den(np.atleast_2d(mag[k]))) for k in ref}


def check_chain(c, backend, rounds=0, what=("fwd", "bwd", "gather", "readout")):
    """cell forward -> cell backward on the forward's z, r, c, A, Tt -> gather of the backward's dn plus its direct part -> read-out of
    the forward's h -> its reverse on the read-out's s, t, g, dy: each operator against the fp64 evaluation of the operands it was given.
    Returns ({name: error}, every output array in order)."""
    err, arrays = {}, []
    if "fwd" in what:
        f = backend.cell_fwd(c, rounds)
        err.update(check_cell_forward(c, f))
        arrays += [f[k] for k in ("h", "n", "z", "r", "c", "A", "T", "Tt") if f.get(k) is not None]
        hL = f["h"]
    else:
        hL = c.hprev
    if "bwd" in what:
        b = backend.cell_bwd(c, f["z"], f["r"], f["c"], f["A"], f["Tt"], rounds)
        err.update(check_cell_backward(c, f["z"], f["r"], f["c"], f["A"], f["Tt"], b))
        arrays += [b[k] for k in ("dzp", "drp", "dcp", "q", "dn", "gTt", "sA", "direct") if b.get(k) is not None]
        if "gather" in what and c.agg != GIVEN:
            g = backend.gather(c, b["dn"], b.get("gTt"), b.get("sA"))
            e, total = check_prev(c, b["dn"], b["direct"], g)
            err.update(e)
            arrays.append(total)
    if "readout" in what:
        rf = backend.readout_fwd(c, hL, rounds)
        err.update(check_readout_forward(c, hL, rf))
        rb = backend.readout_bwd(c, rf["s"], rf["t"], rf["g"], rf["dy"], rounds)
        err.update(check_readout_backward(c, rf["s"], rf["t"], rf["g"], rf["dy"], rb))
        arrays += [rf[k] for k in ("s", "t", "g", "yhat", "dy", "loss")] + [rb[k] for k in ("ds", "dt", "dh", "dU")]
    return err, arrays


# ---- the cases, by test of the GPU file ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def instantiation_case(H, agg):
    nV = 3 * slots(H) + 1
    return Case(H, agg, mixed_lists(nV, np.random.default_rng(1000 + H)), seed=10 * H + agg)


@functools.lru_cache(maxsize=None)
def rounds_case(H, nV, agg):
    return Case(H, agg, mixed_lists(nV, np.random.default_rng(2000 + H + nV)), seed=3 * H + nV + agg)


@functools.lru_cache(maxsize=None)
def own_rounds_case(H, nV, agg):
    return Case(H, agg, sparse_lists(nV, np.random.default_rng(3000 + H)), seed=H + agg, mol_sizes=(5, 1, 40))


@functools.lru_cache(maxsize=None)
def long_case(H, agg):
    return Case(H, agg, long_lists(np.random.default_rng(4000 + H)), seed=7 * H + agg, mol_sizes=(1, 300, 40))


@functools.lru_cache(maxsize=None)
def readout_case(H, nMol):
    """nMol molecules, among them (nMol allowing) one of 300 vertices, several of one and an empty one; hL = the case's hprev"""
    sizes = [1, 300, 0, 2, 1, 7][:max(1, nMol)] if nMol > 1 else [300]
    sizes = (sizes * nMol)[:nMol]
    c = Case(H, SUM, [[]] * sum(sizes), seed=13 * H + nMol)
    c.mol_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    c.nMol = nMol
    c.vmol = np.repeat(np.arange(nMol), sizes).astype(np.int32)
    rng = np.random.default_rng(17 * H + nMol)
    c.target = eighths(rng, -8, 8, nMol)
    return c


def range_rows(H):
    """[(name, a [H])] of integer arguments of z: one channel (0, H - 1) at +-30, +-90, +-120, +-80 among moderate ones (-3 .. 3), all
    +120, all -120, all 0.  r's argument is the row rotated by one channel, c's the row rotated by two, over 4: +-7.5, +-22.5, +-30,
    +-20 and 0"""
    rng = np.random.default_rng(77 + H)
    rows = []
    for p in sorted({0, H - 1}):
        for v in (30, -30, 90, -90, 120, -120, 80, -80):
            a = rng.integers(-3, 4, H).astype(np.float64)
            a[p] = v
            rows.append(("%+d at %d" % (v, p), a))
    return rows + [("all +120", np.full(H, 120.0)), ("all -120", np.full(H, -120.0)), ("all 0", np.zeros(H))]


RANGE_TAIL = 20   # vertices behind the rows and their sources: all +120, one molecule of the read-out (sum of s t = 20: g = 1 exactly)


@functools.lru_cache(maxsize=None)
def range_case(H, agg=SUM):
    """R row vertices, their R sources and RANGE_TAIL more.  Row v has the list [R + v] and hprev[R + v] = range_rows[v] / 128; W_z =
    128 I, W_r = 128 x a rotation by one channel, W_h = 32 x a rotation by two, U_z = U_r = U_h = 0: the arguments of row v are the
    intended numbers exactly, in fp32 as in fp64 (a source has an empty list: its three arguments are exactly 0).  The read-out on
    hL = hprev with W_g = 128 I, U_g = 32 x the rotation by two sees the same arguments at the sources; its molecules are the rows, the
    sources four by four (a row of s below 2^-126 beside rows that are not: no graph feature underflows) and the tail.  dh, U and the backward's own matrices M6_bwd are a main case's."""
    rows = range_rows(H)
    R = len(rows)
    nV = 2 * R + RANGE_TAIL
    c = Case(H, agg, [[R + v] for v in range(R)] + [[]] * (nV - R), seed=31 * H + agg)
    c.hprev[R:2 * R] = np.stack([a for _, a in rows]) / 128
    c.hprev[2 * R:] = 120.0 / 128
    c.set_T()
    eye = np.eye(H, dtype=np.float32)
    c.M6_bwd = c.M6
    c.M6 = np.stack([128 * eye, 0 * eye, 128 * np.roll(eye, 1, axis=0), 0 * eye, 32 * np.roll(eye, 2, axis=0), 0 * eye]).astype(np.float32)
    c.M2 = np.stack([128 * eye, 32 * np.roll(eye, 2, axis=0)]).astype(np.float32)
    c.mol_ptr = np.array([0] + list(range(R, 2 * R, 4)) + [2 * R, nV], dtype=np.int32)
    c.nMol = len(c.mol_ptr) - 1
    c.vmol = np.repeat(np.arange(c.nMol), np.diff(c.mol_ptr)).astype(np.int32)
    rng = np.random.default_rng(5 * H)
    c.target = eighths(rng, -8, 8, c.nMol)
    c.saturating = True
    return c


def with_matrices(c, M6):
    """a shallow copy of a case with other cell matrices"""
    d = Case.__new__(Case)
    d.__dict__.update(c.__dict__)
    d.M6 = M6
    return d


def range_checks(c, backend):
    """the gate-range run of a backend: the cell forward (sum form, and the given form on the same n), the backward on the stored
    saturated gates with a main case's matrices in both forms (A, Tt: any eighths), the read-out and its reverse"""
    err = {}
    f = backend.cell_fwd(c)
    err.update(check_cell_forward(c, f))
    gv = backend.cell_fwd(c, agg=GIVEN, given=f["n"])
    err.update({"given " + k: v for k, v in check_cell_forward(c, gv, agg=GIVEN, n=f["n"]).items()})
    cb = with_matrices(c, c.M6_bwd)
    for pairs in (False, True):
        A, Tt = (c.A_any, c.Tt_any) if pairs else (None, None)
        b = backend.cell_bwd(cb, f["z"], f["r"], f["c"], A, Tt, pairs=pairs)
        err.update({("pairs " if pairs else "") + k: v for k, v in check_cell_backward(cb, f["z"], f["r"], f["c"], A, Tt, b, pairs=pairs).items()})
    rf = backend.readout_fwd(c, c.hprev)
    err.update(check_readout_forward(c, c.hprev, rf))
    rb = backend.readout_bwd(c, rf["s"], rf["t"], rf["g"], rf["dy"])
    err.update(check_readout_backward(c, rf["s"], rf["t"], rf["g"], rf["dy"], rb))
    return err, f, rf


def own_rounds(H, kernels):
    """the first vertex count at which vertices_per_group itself picks two rounds, and three vertices more"""
    return own_round(kernels, H) + 3


def every_case():
    """(test group, label, case, what to run with it): what the CPU suite walks; the GPU file builds the same cases through the same
    functions"""
    for H in WIDTHS:
        for agg in (SUM, PAIRS, GIVEN):
            yield "every_instantiation", (H, agg), instantiation_case(H, agg), ("fwd", "bwd", "gather", "readout")
    for H in ROUND_WIDTHS:
        for nV in round_sizes(H):
            for agg in (SUM, PAIRS):
                yield "rounds_and_ragged_tails", (H, nV, agg), rounds_case(H, nV, agg), ("fwd", "bwd", "readout")
    for H in CELL_OWN_WIDTHS:
        for agg in (SUM, PAIRS):
            yield "the_levels_own_two_rounds", (H, agg), own_rounds_case(H, own_rounds(H, ("cell_fwd", "cell_bwd")), agg), ("fwd", "bwd")
    for H in READOUT_OWN_WIDTHS:
        yield "the_levels_own_two_rounds", (H, "readout"), own_rounds_case(H, own_rounds(H, ("readout_fwd", "readout_bwd")), SUM), ("readout",)
    for H in LONG_WIDTHS:
        for agg in (SUM, PAIRS):
            yield "long_lists", (H, agg), long_case(H, agg), ("fwd", "bwd", "gather")
    for H in READOUT_WIDTHS:
        for nMol in READOUT_MOLS:
            yield "readout", (H, nMol), readout_case(H, nMol), ("readout",)
