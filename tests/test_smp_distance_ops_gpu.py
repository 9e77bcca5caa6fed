"""The kernels a distance handle adds (gf_smp_config.distance_channel), one by one on caller-supplied operands:
  gf_smp_distance_rows_ex_f32            dist_rows_sort_wave / _lds of smp_level_distance.hip against np.sort, exactly
  gf_smp_neighbourhood_fwd2_ex_f32, _node_bwd2_ex_f32, _gather_bwd2_ex_f32
                                         nbh_level_fwd, nbh_node_bwd, nbh_gather_bwd on two operand sets in one launch (blockIdx.y picks
                                         the set) against tests/neighbourhood_ops_ref.py run once per channel, per output row at
                                         field_suite.TOL; the channel-0 half bit for bit the single-channel operator's on the same operands
Operands are those of tests/neighbourhood_ops_cases.py (one Case per channel over the same lists); every output lies in a buffer with
sentinel rows behind its last row."""
import ctypes as C

import numpy as np
import pytest

import neighbourhood_ops_cases as cases
from field_suite import TOL, dev
from test_smp_neighbourhood_ops_gpu import (DEVICE, SENTINEL, FwdSet, GatherSet, NodeSet, addr, context, flat, guarded, merge, padded, ptr, report,
                                            same_bits, taken)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROW_WIDTHS = (1, 2, 3, 29, 63, 64, 65, 185)
CHAIN_WIDTHS = (5, 16, 33, 64, 65, 128)
OPERAND_WIDTHS = ((4, 29), (30, 3))   # (F', M): the narrower operand in either channel
INVALID = 1


# ---- the row builder -----------------------------------------------------------------------------------------------------------------
def row_batch(M, seed):
    """molecules of V = 1, V = M and V < M vertices (where M allows), repeated so that there are more vertices than one workgroup takes:
    sixteenths in [-4, 4] with ties, negatives, a -0.0, zeros off the diagonal, and one molecule whose matrix is asymmetric"""
    rng = np.random.default_rng(seed)
    sizes = sorted({1, M, max(1, M // 2), max(1, M - 1)})
    reps = max(1, -(-300 // sum(sizes))) if M <= 64 else 1
    mats = []
    for V in sizes * reps:
        d = rng.integers(-64, 65, (V, V)) / 16.0
        d = np.triu(d, 1) + np.triu(d, 1).T          # symmetric, zero diagonal
        if V > 2:
            d[0, 1] = d[1, 0] = d[0, 2] = d[2, 0]    # a tie inside a column
            d[1, 2] = d[2, 1] = -0.0
        mats.append(d)
    k = [len(d) for d in mats].index(M)
    mats[k] = mats[k] + np.triu(rng.integers(1, 9, mats[k].shape) / 16.0, 1)   # the asymmetric one (M = 1: nothing to move)
    return mats


def expected_rows(mats, M):
    out = []
    for d in mats:
        V = len(d)
        rows = np.zeros((V, M), dtype=np.float32)
        rows[:, :V] = d.T.astype(np.float32)          # row v = COLUMN v
        out.append(np.sort(rows, axis=1))
    return np.concatenate(out)


def rows_call(mats, M, **over):
    nv = np.array([len(d) for d in mats], dtype=np.int32)
    mp = np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)
    flat = np.concatenate([np.asarray(d, dtype=np.float64).ravel() for d in mats])
    nV = int(mp[-1])
    out = guarded(nV, M)
    args = {"nMol": len(mats), "M": M, "mol_ptr": dev(mp, np.int32), "nVertices": dev(nv, np.int32), "distance": dev(flat, np.float64), "x_d": out}
    for k, v in over.items():
        args[k] = torch.as_tensor(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v
    ctx = context()
    st = ctx.lib.gf_smp_distance_rows_ex_f32(ctx.handle, args["nMol"], args["M"], ptr(args["mol_ptr"]), ptr(args["nVertices"]), ptr(args["distance"]),
                                             ptr(args["x_d"]))
    torch.cuda.synchronize()
    return st, out, nV


@pytest.mark.parametrize("M", ROW_WIDTHS)
def test_rows_are_the_sorted_columns(gf, M):
    """exactly np.sort of the fp32 columns with their zeros: across the lanes of a group up to 64 entries (M = 1, 2, 3, 29, 63, 64: groups
    of 1, 2, 4, 32 and 64 lanes), through LDS above (65, 185: networks of 128 and 256 entries); a width that is no power of two pads with
    +inf, which must never reach a row"""
    mats = row_batch(M, 100 + M)
    assert {len(d) for d in mats} >= {1, M} and (M < 3 or any(len(d) < M and len(d) > 1 for d in mats))
    assert any(not np.array_equal(d, d.T) for d in mats) or M == 1
    st, out, nV = rows_call(mats, M)
    context().check(st)
    got = taken(out, nV, M)
    want = expected_rows(mats, M)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got.reshape(nV, M), want)
    if M >= 3:
        assert (want < 0).any() and (np.diff(want, axis=1) == 0).any()


def test_rows_refusals(gf):
    """a non-finite entry, a molecule above M, inconsistent tables: GF_ERR_INVALID, nothing written, and the context goes on working"""
    M = 5
    mats = row_batch(M, 7)
    good = expected_rows(mats, M)

    def untouched(out):
        assert np.all(out.cpu().numpy() == SENTINEL)

    def works():
        st, out, nV = rows_call(mats, M)
        context().check(st)
        assert np.array_equal(taken(out, nV, M).reshape(nV, M), good)

    for bad in (np.nan, np.inf, -np.inf):
        broken = [d.copy() for d in mats]
        broken[-1][0, 0] = bad
        st, out, _ = rows_call(broken, M)
        assert st == INVALID and b"not finite" in context().lib.gf_last_error(context().handle)
        untouched(out)
        works()
    st, out, _ = rows_call(mats, M - 1)   # a molecule of M vertices in rows of M - 1 entries
    assert st == INVALID
    untouched(out)
    works()
    nv = np.array([len(d) for d in mats], dtype=np.int32)
    wrong = nv.copy()
    wrong[0] += 1
    st, out, _ = rows_call(mats, M, nVertices=wrong)
    assert st == INVALID
    untouched(out)
    works()
    for kw in ({"M": 0}, {"M": 4097}, {"nMol": 0}, {"x_d": None}, {"distance": None}):
        st, out, _ = rows_call(mats, kw.pop("M", M), **kw)
        assert st == INVALID
        works()


# ---- the level's kernels on two operand sets ----------------------------------------------------------------------------------------
def channel_cases(H, pairs, widths):
    """one Case per channel over the same lists and molecules; the top level's dy is shared"""
    nV = 3 * cases.slots(H) + 1   # more vertices than one workgroup's slots, a ragged last round
    lists = cases.mixed_lists(nV, np.random.default_rng(7000 + H))
    c = [cases.Case(H, FD, pairs, lists, seed=17 * H + FD + pairs + 100 * k) for k, FD in enumerate(widths)]
    c[1].dy_top = c[0].dy_top
    assert np.array_equal(c[0].ptr, c[1].ptr) and np.array_equal(c[0].mol_ptr, c[1].mol_ptr) and c[0].FD != c[1].FD
    return c


def forward2(cs, rounds=0):
    c0 = cs[0]
    H, nV = c0.H, c0.nV
    lvl = c0.W2 is not None
    keep, outs, sets = [], [], (FwdSet * 2)()
    for k, c in enumerate(cs):
        out = {q: guarded(nV, H) for q in ("h", "n", "A")}
        out.update({q: guarded(nV, 1) for q in ("T", "Tt")})
        ins = {"W1": dev(c.W1), "x": dev(c.x), "W2": dev(c.W2) if lvl else None, "hprev": dev(c.hprev), "Tprev": dev(c.Tprev)}
        keep.append(ins)
        sets[k].FD = c.FD
        for q, t in list(ins.items()) + list(out.items()):
            setattr(sets[k], q, addr(t))
        outs.append(out)
    ctx = context()
    p, i = dev(c0.ptr, np.int64), padded(c0.idx)
    ctx.check(ctx.lib.gf_smp_neighbourhood_fwd2_ex_f32(ctx.handle, int(c0.pairs), H, nV, rounds, C.byref(sets), ptr(p), ptr(i)))
    torch.cuda.synchronize()
    wr = {"h": True, "n": lvl, "A": lvl and c0.pairs, "T": c0.pairs, "Tt": lvl and c0.pairs}
    return [{q: taken(out[q], nV, H if q in ("h", "n", "A") else 1, wr[q]) for q in out} for out in outs]


def node2(cs, fwd, top, rounds=0):
    c0 = cs[0]
    H, nV = c0.H, c0.nV
    lvl = c0.W2 is not None
    keep, outs, sets = [], [], (NodeSet * 2)()
    for k, (c, f) in enumerate(zip(cs, fwd)):
        out = {"dz": guarded(nV, H, c.dh), "dn": guarded(nV, H), "gTt": guarded(nV, H), "sA": guarded(nV, 1)}
        ins = {"W2": dev(c.W2) if lvl else None, "h": dev(f["h"]), "Wout": dev(c.W), "A": dev(f["A"]) if f["A"] is not None else None,
               "Tt": dev(f["Tt"]) if f["Tt"] is not None else None}
        keep.append(ins)
        for q, t in ins.items():
            setattr(sets[k], q, addr(t))
        sets[k].dh = addr(out["dz"])
        for q in ("dn", "gTt", "sA"):
            setattr(sets[k], q, addr(out[q]))
        outs.append(out)
    ctx = context()
    dy, vmol = (dev(c0.dy_top) if top else None), dev(c0.vmol, np.int32)
    ctx.check(ctx.lib.gf_smp_neighbourhood_node_bwd2_ex_f32(ctx.handle, int(c0.pairs), H, nV, rounds, C.byref(sets), ptr(dy), ptr(vmol), c0.nMol))
    torch.cuda.synchronize()
    wr = {"dz": True, "dn": lvl, "gTt": lvl and c0.pairs, "sA": lvl and c0.pairs}
    return [{q: taken(out[q], nV, 1 if q == "sA" else H, wr[q], prefilled=q == "dz") for q in out} for out in outs]


def gather2(cs, nodes):
    c0 = cs[0]
    keep, outs, sets = [], [], (GatherSet * 2)()
    for k, (c, nb) in enumerate(zip(cs, nodes)):
        out = guarded(c.nV, c.H)
        ins = {"dn": dev(nb["dn"]), "gTt": dev(nb["gTt"]) if nb["gTt"] is not None else None, "sA": dev(nb["sA"]) if nb["sA"] is not None else None,
               "hprev": dev(c.hprev), "Tprev": dev(c.Tprev)}
        keep.append(ins)
        for q, t in ins.items():
            setattr(sets[k], q, addr(t))
        sets[k].dhprev = addr(out)
        outs.append(out)
    ctx = context()
    tp, ti = dev(c0.tptr, np.int64), padded(c0.tidx)
    ctx.check(ctx.lib.gf_smp_neighbourhood_gather_bwd2_ex_f32(ctx.handle, int(c0.pairs), c0.H, c0.nV, ptr(tp), ptr(ti), C.byref(sets)))
    torch.cuda.synchronize()
    return [taken(out, c.nV, c.H) for c, out in zip(cs, outs)]


@pytest.mark.parametrize("top", [False, True], ids=["inner", "top"])
@pytest.mark.parametrize("widths", OPERAND_WIDTHS, ids=["F4_M29", "F30_M3"])
@pytest.mark.parametrize("H", CHAIN_WIDTHS)
def test_two_channel_chain(gf, H, widths, top):
    """forward -> node backward -> gather, both channels in one launch each, sum and pair form: every row of every output of either channel
    against the fp64 evaluation of that channel's operands, and channel 0 bit for bit what the single-channel operators give"""
    for pairs in (False, True):
        cs = channel_cases(H, pairs, widths)
        assert cs[0].nV > cases.slots(H)
        worst = {}
        f = forward2(cs)
        nb = node2(cs, f, top)
        g = gather2(cs, nb)
        for k, c in enumerate(cs):
            merge(worst, {"%s/%d" % (q, k): e for q, e in cases.check_forward(c, f[k]).items()})
            merge(worst, {"%s/%d" % (q, k): e for q, e in cases.check_node(c, f[k]["h"], f[k]["A"], f[k]["Tt"], top, nb[k]).items()})
            merge(worst, {"%s/%d" % (q, k): e for q, e in cases.check_gather(c, nb[k]["dn"], g[k]).items()})
        report("H=%d F'=%d M=%d %s %s" % (H, widths[0], widths[1], "pairs" if pairs else "sum", "top" if top else "inner"), worst)
        # the single-channel launches (grid.y = 1) on channel 0's operands, then on channel 1's: the same bits either way
        for k, c in enumerate(cs):
            f1 = DEVICE.forward(c)
            n1 = DEVICE.node(c, f1["h"], f1["A"], f1["Tt"], top)
            g1 = DEVICE.gather(c, n1["dn"], n1.get("gTt"), n1.get("sA"))
            same_bits(flat(f[k], ("h", "n", "A", "T", "Tt")), flat(f1, ("h", "n", "A", "T", "Tt")))
            same_bits(flat(nb[k], ("dz", "dn", "gTt", "sA")), flat(n1, ("dz", "dn", "gTt", "sA")))
            same_bits([g[k]], [g1])


@pytest.mark.parametrize("H", (5, 65))
def test_two_channel_level0(gf, H):
    """level 0 (no W2 in either set: no aggregate, n / A / Tt untouched) and its node kernel (dz alone)"""
    for pairs in (False, True):
        nV = 3 * cases.slots(H) + 1
        lists = cases.mixed_lists(nV, np.random.default_rng(7100 + H))
        cs = [cases.Case(H, FD, pairs, lists, seed=19 * H + FD + pairs, level0=True) for FD in (4, 29)]
        f = forward2(cs)
        nb = node2(cs, f, False)
        worst = {}
        for k, c in enumerate(cs):
            merge(worst, {"%s/%d" % (q, k): e for q, e in cases.check_forward(c, f[k]).items()})
            merge(worst, {"%s/%d" % (q, k): e for q, e in cases.check_node(c, f[k]["h"], None, None, False, nb[k]).items()})
            f1 = DEVICE.forward(c)
            same_bits(flat(f[k], ("h", "T")), flat(f1, ("h", "T")))
        report("level 0 H=%d %s" % (H, "pairs" if pairs else "sum"), worst)


def test_two_channel_refusals(gf):
    """W2 in one set only, a missing operand, an operand too wide for the LDS: GF_ERR_INVALID before anything is launched"""
    cs = channel_cases(16, False, (4, 29))
    ctx = context()
    c0 = cs[0]
    p, i = dev(c0.ptr, np.int64), padded(c0.idx)
    bufs = [{q: dev(getattr(c, q)) for q in ("W1", "x", "W2", "hprev", "Tprev")} for c in cs]
    outs = [{q: guarded(c0.nV, c0.H) for q in ("h", "n")} for _ in cs]

    def sets_of(over=()):
        sets = (FwdSet * 2)()
        for k, c in enumerate(cs):
            sets[k].FD = c.FD
            for q, t in list(bufs[k].items()) + list(outs[k].items()):
                setattr(sets[k], q, addr(t))
        for (k, q), v in dict(over).items():
            setattr(sets[k], q, v)
        return sets

    def status(sets):
        st = ctx.lib.gf_smp_neighbourhood_fwd2_ex_f32(ctx.handle, 0, c0.H, c0.nV, 0, C.byref(sets), ptr(p), ptr(i))
        torch.cuda.synchronize()
        return st

    for over in ({(1, "W2"): None}, {(0, "x"): None}, {(1, "h"): None}, {(1, "FD"): 0}, {(1, "FD"): 70000}):
        assert status(sets_of(over)) == INVALID
        for o in outs:
            for t in o.values():
                assert np.all(t.cpu().numpy() == SENTINEL)
        assert status(sets_of()) == 0
        for o in outs:
            for t in o.values():
                t.fill_(SENTINEL)
    assert ctx.lib.gf_smp_neighbourhood_fwd2_ex_f32(ctx.handle, 0, c0.H, c0.nV, 0, None, ptr(p), ptr(i)) == INVALID
    assert TOL == 1e-5
