"""The cases tests/test_smp_neighbourhood_ops_gpu.py runs through gf_smp_neighbourhood_*_ex_f32, built from fixed seeds on the host so
that tests/test_smp_neighbourhood_ops.py can check the very operands the GPU suite will use (a numpy float32 evaluation of every case
stays within TOL / 2 of the fp64 one by every measure), and the checks both suites share: a backend (the device, or Numpy32 here) runs
an operator on a case's operands, check_* holds every output row to tests/neighbourhood_ops_ref.py in fp64.

Operands are small dyadic multiples, as in the goldens: weights and gradients in eighths, features in eighths, hprev positive multiples
of 2^-12 whose row sums spread over 0.5 .. 2, Tprev exactly those sums (so sums of hundreds of members are exact in fp32 and T differs
from 1 by tens of percent).  W2 is scaled by a power of two so that the aggregate's part of a pre-activation stays at a few units."""
import functools

import numpy as np

import neighbourhood_ops_ref as ops

TOL = 1e-5
WIDTHS = (5, 6, 8, 9, 16, 17, 31, 32, 33, 64, 65, 66, 127, 128)
FDS = (1, 4, 15)
ROUND_WIDTHS = (8, 20, 64, 128)
OWN_ROUNDS = ((64, 2051), (20, 4101), (12, 8195), (8, 16387))   # 2 x 256 x slots, where vertices_per_group first picks two rounds, and a few vertices more
RANGE_WIDTHS = (5, 33, 65, 128)
LONG_WIDTHS = (20, 64, 128)
READOUT_MOLS = (1, 15, 16, 17, 33)
READOUT_WIDTHS = (5, 64, 65, 128)


def group_width(H):
    return 64 if H > 32 else 32 if H > 16 else 16 if H > 8 else 8


def slots(H):
    return 256 // group_width(H)


def round_sizes(H):
    s = slots(H)
    return (1, s - 1, s, s + 1, 2 * s - 1, 2 * s + 1, 6 * s + 1)


def eighths(rng, lo, hi, shape):
    return (rng.integers(lo, hi + 1, shape) / 8).astype(np.float32)


def mixed_lists(nV, rng):
    """0, 1, 2, 12 members and more, three vertices in eight members of their own lists (of the 1-member lists every other one is the vertex itself)"""
    sizes = [0, 1, 2, 12, 3, 1, 5, 7]
    out = []
    for v in range(nV):
        m = min(sizes[v % len(sizes)], nV)
        mem = set(int(u) for u in rng.choice(nV, m, replace=False))
        if v % 8 in (1, 3, 6) and mem and v not in mem:
            mem.pop()
            mem.add(v)
        out.append(sorted(mem))
    return out


def sparse_lists(nV, rng, most=4):
    """(ptr, idx) of 0 .. `most` random members per vertex, ascending (a member may repeat), without a Python loop"""
    counts = rng.integers(0, most + 1, nV)
    ptr = np.zeros(nV + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(counts)
    idx = rng.integers(0, nV, int(ptr[-1]))
    own = ops.owners(ptr)
    return ptr, idx[np.lexsort((idx, own))].astype(np.int32)


def long_lists(rng):
    """400 vertices: vertex 0 has 300 members, 1 / 2 / 3 have 63 / 64 / 65; vertex 399 is a member of 300 lists; 380 .. 389 of none"""
    nV = 400
    usable = np.arange(0, 380)
    out = []
    for v in range(nV):
        m = {0: 300, 1: 63, 2: 64, 3: 65}.get(v, 1 + v % 3)
        mem = set(int(u) for u in rng.choice(usable, m, replace=False))
        if 50 <= v < 350 or v == 0:
            mem.add(399)
        out.append(sorted(mem))
    return out


def molecules_of(nV, sizes):
    """mol_ptr int32 of molecules of `sizes` vertices, repeated until nV is used up (the last one takes the rest)"""
    ptr = [0]
    while ptr[-1] < nV:
        ptr.append(min(nV, ptr[-1] + sizes[(len(ptr) - 1) % len(sizes)]))
    return np.array(ptr, dtype=np.int32)


class Case:
    """One level's operands (float32) over nV vertices: lists (ptr, idx) with their transpose, W1, x, W2 (None: level 0), hprev, Tprev,
    dh, and a read-out over molecules mol_ptr: W, target, dW0, dy_top (the top level's dy per molecule), vmol"""

    def __init__(self, H, FD, pairs, lists, seed, level0=False, mol_sizes=(1, 3, 40, 2), nV=None):
        rng = np.random.default_rng(seed)
        self.H, self.FD, self.pairs = H, FD, bool(pairs)
        self.ptr, self.idx = ops.csr(lists) if isinstance(lists, list) else lists
        self.nV = nV = len(self.ptr) - 1 if nV is None else nV
        assert len(self.ptr) == nV + 1
        self.tptr, self.tidx = ops.transpose(self.ptr, self.idx, nV)
        self.W1, self.x = eighths(rng, -4, 4, (H, FD)), eighths(rng, 0, 8, (nV, FD))
        want = rng.uniform(0.5, 2.0, (nV, 1))
        self.hprev = (np.round((0.5 + rng.random((nV, H))) * want * (4096.0 / H)) / 4096).astype(np.float32)
        self.hprev[:, 0] += np.float32(2.0 ** -12)   # (no row of zeros)
        T = self.hprev.astype(np.float64).sum(axis=1)
        self.Tprev = T.astype(np.float32)
        assert np.array_equal(self.Tprev.astype(np.float64), T) and T.min() > 0.2 and T.max() < 3.1
        self.W2 = None
        if not level0:
            nmag = float(np.median(ops.aggregate(self.hprev, self.Tprev, self.ptr, self.idx, pairs, magnitude=True).max(axis=1)))
            k = int(np.ceil(np.log2(max(1.0, H * 0.25 * nmag / 8))))
            self.W2 = (eighths(rng, -4, 4, (H, H)) * np.float32(2.0 ** -k)).astype(np.float32)
        self.dh = eighths(rng, -8, 8, (nV, H))
        self.mol_ptr = molecules_of(nV, mol_sizes)
        self.nMol = len(self.mol_ptr) - 1
        self.vmol = np.repeat(np.arange(self.nMol), np.diff(self.mol_ptr)).astype(np.int32)
        self.W, self.target = eighths(rng, -4, 4, H), eighths(rng, -8, 8, self.nMol)
        self.dW0, self.dy_top = eighths(rng, -8, 8, H), eighths(rng, -8, 8, self.nMol)
        self.single = np.diff(self.ptr) == 1   # pairs: n is exactly 0 there


class Numpy32:
    """the operators evaluated by tests/neighbourhood_ops_ref.py in float32: the backend of the CPU suite"""

    def forward(self, c, rounds=0):
        return ops.forward(c.W1, c.x, c.W2, c.hprev, c.Tprev, c.ptr, c.idx, c.pairs, dt=np.float32)

    def node(self, c, h, A, Tt, top=False, rounds=0):
        return ops.node_backward(c.W2, h, c.dh, c.dy_top if top else None, c.W, c.vmol, A, Tt, c.pairs, dt=np.float32)

    def gather(self, c, dn, gTt, sA):
        return ops.gather_backward(c.tptr, c.tidx, dn, c.hprev, c.Tprev, c.pairs, dt=np.float32)

    def readout(self, c, hL, target=True, loss=True):
        r = ops.readout(hL, c.mol_ptr, c.W, c.target if target else None, c.dW0, dt=np.float32)
        if not loss:
            r["loss"] = None
        return r


def check_forward(c, out):
    """{output: worst row error}; with pairs a list of one member must give n = 0 bit for bit"""
    ref = ops.forward(c.W1, c.x, c.W2, c.hprev, c.Tprev, c.ptr, c.idx, c.pairs)
    den = ops.forward_dens(c.W1, c.x, c.W2, c.hprev, c.Tprev, c.ptr, c.idx, c.pairs, ref)
    assert np.all(np.isfinite(out["h"])), "h is not finite"
    err = {k: ops.row_err(out[k], ref[k], den[k]) for k in den if k != "T" or c.pairs}
    if c.pairs and c.W2 is not None and c.single.any():
        assert not np.asarray(out["n"])[c.single].view(np.uint32).any(), "one member: n is not exactly +0"
    return err


def check_node(c, h, A, Tt, top, out):
    """the operands h, A, Tt are those the backend was given; dz is what it left in dh"""
    args = (c.W2, h, c.dh, c.dy_top if top else None, c.W, c.vmol, A, Tt, c.pairs)
    ref, mag = ops.node_backward(*args), ops.node_backward(*args, magnitude=True)
    return {k: ops.row_err(out[k], ref[k], ops.row_den(mag[k])) for k in ref}


def check_gather(c, dn, out):
    args = (c.tptr, c.tidx, dn, c.hprev, c.Tprev, c.pairs)
    ref, mag = ops.gather_backward(*args), ops.gather_backward(*args, magnitude=True)
    if c.pairs:   # a source nobody consumes: exactly 0
        assert not np.asarray(out)[np.diff(c.tptr) == 0].any(), "a source without consumers has a gradient"
    return {"dhprev": ops.row_err(out, ref, ops.row_den(mag))}


def check_readout(c, hL, out, target=True, loss=True):
    args = (hL, c.mol_ptr, c.W, c.target if target else None, c.dW0)
    ref, mag = ops.readout(*args), ops.readout(*args, magnitude=True)
    keys = ["g", "yhat", "dy", "dW"] + (["loss"] if loss else [])
    return {k: ops.row_err(out[k], ref[k], ops.row_den(mag[k])) for k in keys}


def check_chain(c, backend, rounds=0, what=("fwd", "node", "gather", "readout"), top=False):
    """forward -> node backward on the forward's h, A, Tt -> gather on the node kernel's outputs -> read-out of the forward's h: each
    operator against the fp64 evaluation of the operands it was given.  Returns ({name: error}, every output array in order)."""
    err, arrays = {}, []
    f = backend.forward(c, rounds)
    err.update(check_forward(c, f))
    arrays += [f[k] for k in ("h", "n", "A", "T", "Tt") if f.get(k) is not None]
    if "node" in what:
        nb = backend.node(c, f["h"], f["A"], f["Tt"], top, rounds)
        err.update(check_node(c, f["h"], f["A"], f["Tt"], top, nb))
        arrays += [nb[k] for k in ("dz", "dn", "gTt", "sA") if nb.get(k) is not None]
        if "gather" in what and c.W2 is not None:
            g = backend.gather(c, nb["dn"], nb.get("gTt"), nb.get("sA"))
            err.update(check_gather(c, nb["dn"], g))
            arrays.append(g)
    if "readout" in what:
        r = backend.readout(c, f["h"])
        err.update(check_readout(c, f["h"], r))
        arrays += [r[k] for k in ("g", "yhat", "dy", "loss", "dW")]
    return err, arrays


# ---- the cases, by test of the GPU file ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def instantiation_case(H, FD, pairs):
    nV = 3 * slots(H) + 1
    return Case(H, FD, pairs, mixed_lists(nV, np.random.default_rng(1000 + H)), seed=10 * H + FD + pairs)


@functools.lru_cache(maxsize=None)
def rounds_case(H, nV, pairs):
    return Case(H, 4, pairs, mixed_lists(nV, np.random.default_rng(2000 + H + nV)), seed=3 * H + nV + pairs)


@functools.lru_cache(maxsize=None)
def own_rounds_case(H, nV, pairs):
    return Case(H, 4, pairs, sparse_lists(nV, np.random.default_rng(3000 + H)), seed=H + pairs, mol_sizes=(5, 1, 40))


@functools.lru_cache(maxsize=None)
def long_case(H, pairs):
    return Case(H, 4, pairs, long_lists(np.random.default_rng(4000 + H)), seed=7 * H + pairs, mol_sizes=(1, 300, 40))


def range_rows(H):
    """[(name, z [H])] of integer pre-activations: one channel 100 above the rest (at channel 0, H - 1 and, above 64 channels, at the
    second channel of a lane), all +120, all -120, a spread over [-100, 100] with its maximum at each of those places, all equal"""
    peaks = [0, H - 1] + ([64, 64 + (H - 65) // 2] if H > 64 else [])
    spread = np.round(np.linspace(-100, 100, H))
    rows = []
    for p in peaks:
        z = np.full(H, -3.0)
        z[p] = 97.0
        rows.append(("peak at %d" % p, z))
        rows.append(("spread, maximum at %d" % p, np.roll(spread, p + 1)))   # (spread[-1] = +100 lands on channel p)
    rows += [("all +120", np.full(H, 120.0)), ("all -120", np.full(H, -120.0)), ("all equal", np.full(H, 7.0))]
    for name, z in rows:
        assert np.array_equal(z, np.round(z)) and (not name.startswith("spread") or z.argmax() == int(name.split()[-1]))
    return rows


@functools.lru_cache(maxsize=None)
def range_case(H, level0):
    """vertex r has the pre-activations range_rows(H)[r], exactly: x[r] = e_r and column r of W1 holds the row; at a level with W2 every
    list is [0], hprev[0] = e_0, and column 0 of W2 (a ramp of -1, 0, 1) is taken off W1's column.  Level 0 runs the pair form (it stores
    T, the device's own row sum), the level with W2 the sum form."""
    rows = range_rows(H)
    R = len(rows)
    c = Case(H, R, pairs=level0, lists=[[0]] * R, seed=H, level0=level0, mol_sizes=(R,))
    Z = np.stack([z for _, z in rows], axis=1)   # [H][R]
    c.x = np.eye(R, dtype=np.float32)
    if not level0:
        c.hprev = np.zeros((R, H), dtype=np.float32)
        c.hprev[:, 0] = 1
        c.Tprev = np.ones(R, dtype=np.float32)
        c.W2[:, 0] = np.arange(H) % 3 - 1
        Z = Z - c.W2[:, :1].astype(np.float64)
    c.W1 = Z.astype(np.float32)
    z = ops.pre_activation(c.W1, c.x, c.W2, None if level0 else ops.aggregate(c.hprev, c.Tprev, c.ptr, c.idx, False)["n"])
    assert np.array_equal(z.T, np.stack([r for _, r in rows], axis=1)), "the pre-activations are not the intended integers"
    return c


@functools.lru_cache(maxsize=None)
def node_case(H, kind, pairs):
    """kind "top" (dy, Wout, vmol: molecules of 1 and 40 vertices), "inner", "level0" (W2 None).  Returns (case, h, A, Tt): h is an
    operand here -- rows of a softmax of dyadic pre-activations, every fifth row one-hot (exact 0 and exact 1: dz = 0 exactly), every
    seventh with one exact 0 -- and A, Tt the fp32 aggregate of the case's own lists"""
    nV = max(2 * slots(H) + 3, 45)   # (two rounds of slots and a ragged third; room for the 40-vertex molecule)
    c = Case(H, 4, pairs, mixed_lists(nV, np.random.default_rng(5000 + H)), seed=11 * H + pairs, level0=kind == "level0", mol_sizes=(1, 40))
    rng = np.random.default_rng(6000 + H)
    h = ops.softmax(rng.integers(-8, 9, (nV, H)) / 4).astype(np.float32)
    h[::5] = 0
    h[np.arange(0, nV, 5), rng.integers(0, H, len(h[::5]))] = 1
    h[2::7, H // 2] = 0
    agg = ops.aggregate(c.hprev, c.Tprev, c.ptr, c.idx, pairs, dt=np.float32)
    return c, h, agg["A"] if pairs else None, agg["Tt"] if pairs else None


@functools.lru_cache(maxsize=None)
def readout_case(H, nMol):
    """nMol molecules, among them (nMol allowing) one of 300 vertices and several of one; hL = the case's positive hprev"""
    sizes = [1, 300, 2, 1, 7][:max(1, nMol)] if nMol > 1 else [300]
    sizes = (sizes * nMol)[:nMol]
    c = Case(H, 1, False, [[]] * sum(sizes), seed=13 * H + nMol, level0=True, mol_sizes=tuple(sizes))
    assert c.nMol == nMol
    return c


def every_case():
    """(test group, label, what to run with it): what the CPU suite walks; the GPU file builds the same cases through the same functions"""
    for H in WIDTHS:
        for FD in FDS:
            for pairs in (False, True):
                yield "every_instantiation", (H, FD, pairs), instantiation_case(H, FD, pairs)
    for H in ROUND_WIDTHS:
        for nV in round_sizes(H):
            for pairs in (False, True):
                yield "rounds_and_ragged_tails", (H, nV, pairs), rounds_case(H, nV, pairs)
    for H, nV in OWN_ROUNDS:
        for pairs in (False, True):
            yield "the_levels_own_two_rounds", (H, nV, pairs), own_rounds_case(H, nV, pairs)
    for H in RANGE_WIDTHS:
        for level0 in (True, False):
            yield "softmax_range", (H, level0), range_case(H, level0)
    for H in LONG_WIDTHS:
        for pairs in (False, True):
            yield "long_lists", (H, pairs), long_case(H, pairs)
    for H in READOUT_WIDTHS:
        for nMol in READOUT_MOLS:
            yield "readout", (H, nMol), readout_case(H, nMol)
