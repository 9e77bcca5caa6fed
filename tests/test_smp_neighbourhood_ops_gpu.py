"""The kernels of the softmax neighbourhood level one by one (gf_smp_neighbourhood_fwd_ex_f32 / _node_bwd_ex_f32 / _gather_bwd_ex_f32 /
_readout_ex_f32: nbh_level_fwd, nbh_node_bwd, nbh_gather_bwd, nbh_readout and nbh_readout_dW of smp_level_neighbourhood.hip, through the
level's own launchers) against the fp64 evaluation of the same operands (tests/neighbourhood_ops_ref.py), per output row, relative to
the row's magnitude sum.  One bound, field_suite.TOL = 1e-5; a numpy float32 evaluation of every case here measures at most 7.5e-7
(tests/test_smp_neighbourhood_ops.py asserts TOL / 2 on these very operands, built by tests/neighbourhood_ops_cases.py).  Every output
lies in a buffer with sentinels behind its last row (the kernels take no row stride: rows are dense, so there is no tail behind channel
H - 1 to guard), and an output the chosen form does not store must stay untouched.  The measured figures are in NOTES.md."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import neighbourhood_ops_cases as cases
import neighbourhood_ops_ref as ops
from field_suite import TOL, dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 12345.0
TAIL_ROWS = 3   # sentinel rows behind row nV - 1 of every output


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def context():
    from graphflow_amd.ops import default_context
    return default_context(0)


def guarded(rows, width, fill=None):
    t = torch.full(((rows + TAIL_ROWS) * width,), SENTINEL, device="cuda")
    if fill is not None:
        t[:rows * width] = dev(fill).reshape(-1)
    return t


def taken(t, rows, width, written=True, prefilled=False):
    """the result inside a guarded buffer: the sentinel rows intact, and no sentinel left inside -- or, for an output the form does not
    store, nothing but sentinels"""
    a = t.cpu().numpy()
    n = rows * width
    assert np.all(a[n:] == SENTINEL), "wrote behind the last row"
    if not written:
        assert np.all(a[:n] == SENTINEL), "wrote an output this form does not have"
        return None
    assert prefilled or not np.any(a[:n] == SENTINEL), "%d elements were not written" % int((a[:n] == SENTINEL).sum())
    return a[:n].reshape((rows, width) if width > 1 else (rows,))


_V = C.c_void_p


class FwdSet(C.Structure):   # gf_nbh_fwd_set
    _fields_ = [("FD", C.c_int)] + [(k, _V) for k in ("W1", "x", "W2", "hprev", "Tprev", "h", "n", "A", "T", "Tt")]


class NodeSet(C.Structure):   # gf_nbh_node_set
    _fields_ = [(k, _V) for k in ("W2", "h", "dh", "Wout", "A", "Tt", "dn", "gTt", "sA")]


class GatherSet(C.Structure):   # gf_nbh_gather_set
    _fields_ = [(k, _V) for k in ("dn", "gTt", "sA", "hprev", "Tprev", "dhprev")]


def addr(t):
    return t.data_ptr() if t is not None else None


def padded(idx):
    """an index list on the device, one spare entry behind it (an empty list still has an address)"""
    return dev(np.append(np.asarray(idx, dtype=np.int64), 0), np.int32)


def call(name, args, over):
    """one operator: args = [(name, int | tensor | None)]; over replaces by name (arrays go to the device as they are typed)"""
    ctx = context()
    unknown = set(over) - {k for k, _ in args}
    assert not unknown, unknown
    vals = []
    for k, v in args:
        if k in over:
            v = over[k]
            v = torch.as_tensor(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v
        vals.append(v if isinstance(v, int) else ptr(v))
    st = getattr(ctx.lib, name)(ctx.handle, *vals)
    torch.cuda.synchronize()
    return st


def call2(name, cls, at, args, over, second):
    """the two-set entry of an operator on the arguments of its one-set entry: those that are fields of cls are set 0; set 1 is the same
    set with the buffers `second` (by argument name) in place of set 0's and with `over`'s fields -- an offence sits in position 1.  The
    other arguments, with `over`'s, are the call's own; the sets go in at position `at` of them."""
    ctx = context()
    fields = [f for f, _ in cls._fields_]
    unknown = set(over) - {k for k, _ in args}
    assert not unknown, unknown
    keep, sets, shared = [], (cls * 2)(), []

    def value(v):
        if isinstance(v, np.ndarray):
            v = torch.as_tensor(np.ascontiguousarray(v)).cuda()
            keep.append(v)
        return v if isinstance(v, int) else addr(v)

    for k, v in args:
        if k in fields:
            setattr(sets[0], k, value(v))
            setattr(sets[1], k, value(over[k] if k in over else second.get(k, v)))
        else:
            shared.append(value(over[k] if k in over else v))
    shared.insert(at, C.byref(sets))
    st = getattr(ctx.lib, name)(ctx.handle, *shared)
    torch.cuda.synchronize()
    return st


class Device:
    """the backend of neighbourhood_ops_cases.check_*: with status=True a method returns (status, the output buffers, [(in/out
    buffer, its prefill)]), else it checks the status and returns the outputs as arrays (None for one the form does not store).
    twice=True: the two-set entry with the call's one set given twice, each with output buffers of its own -- the buffers of both sets
    with status=True, else [the outputs of set 0, of set 1]"""

    def forward(self, c, rounds=0, status=False, twice=False, **over):
        H, nV = c.H, c.nV
        outs = [{k: guarded(nV, 1 if k in ("T", "Tt") else H) for k in ("h", "n", "A", "T", "Tt")} for _ in range(2 if twice else 1)]
        out = outs[0]
        lvl = c.W2 is not None
        args = [("pairs", int(c.pairs)), ("H", H), ("FD", c.FD), ("nV", nV), ("rounds", rounds), ("W1", dev(c.W1)), ("x", dev(c.x)),
                ("W2", dev(c.W2) if lvl else None), ("hprev", dev(c.hprev)), ("Tprev", dev(c.Tprev)), ("ptr", dev(c.ptr, np.int64)),
                ("idx", padded(c.idx))] + [(k, out[k]) for k in ("h", "n", "A", "T", "Tt")]
        st = call2("gf_smp_neighbourhood_fwd2_ex_f32", FwdSet, 4, args, over, outs[1]) if twice else call("gf_smp_neighbourhood_fwd_ex_f32", args, over)
        if status:
            return st, [t for o in outs for t in o.values()], []
        context().check(st)
        wr = {"h": True, "n": lvl, "A": lvl and c.pairs, "T": c.pairs, "Tt": lvl and c.pairs}
        res = [{k: taken(o[k], nV, H if k in ("h", "n", "A") else 1, wr[k]) for k in o} for o in outs]
        return res if twice else res[0]

    def node(self, c, h_, A_, Tt_, top=False, rounds=0, status=False, twice=False, **over):
        H, nV = c.H, c.nV
        lvl = c.W2 is not None
        outs = [{"dz": guarded(nV, H, c.dh), "dn": guarded(nV, H), "gTt": guarded(nV, H), "sA": guarded(nV, 1)} for _ in range(2 if twice else 1)]
        out = outs[0]
        args = [("pairs", int(c.pairs)), ("H", H), ("nV", nV), ("rounds", rounds), ("W2", dev(c.W2) if lvl else None), ("h", dev(h_)),
                ("dh", out["dz"]), ("dy", dev(c.dy_top) if top else None), ("Wout", dev(c.W)), ("vmol", dev(c.vmol, np.int32)),
                ("nMol", c.nMol), ("A", dev(A_) if A_ is not None else None), ("Tt", dev(Tt_) if Tt_ is not None else None),
                ("dn", out["dn"]), ("gTt", out["gTt"]), ("sA", out["sA"])]
        if twice:
            second = {"dh" if k == "dz" else k: t for k, t in outs[1].items()}
            st = call2("gf_smp_neighbourhood_node_bwd2_ex_f32", NodeSet, 4, args, over, second)
        else:
            st = call("gf_smp_neighbourhood_node_bwd_ex_f32", args, over)
        if status:
            return st, [o[k] for o in outs for k in ("dn", "gTt", "sA")], [(o["dz"], c.dh) for o in outs]
        context().check(st)
        wr = {"dz": True, "dn": lvl, "gTt": lvl and c.pairs, "sA": lvl and c.pairs}
        res = [{k: taken(o[k], nV, 1 if k == "sA" else H, wr[k], prefilled=k == "dz") for k in o} for o in outs]
        return res if twice else res[0]

    def gather(self, c, dn_, gTt_, sA_, status=False, twice=False, **over):
        outs = [guarded(c.nV, c.H) for _ in range(2 if twice else 1)]
        out = outs[0]
        args = [("pairs", int(c.pairs)), ("H", c.H), ("nV", c.nV), ("tptr", dev(c.tptr, np.int64)), ("tidx", padded(c.tidx)), ("dn", dev(dn_)),
                ("gTt", dev(gTt_) if gTt_ is not None else None), ("sA", dev(sA_) if sA_ is not None else None), ("hprev", dev(c.hprev)),
                ("Tprev", dev(c.Tprev)), ("dhprev", out)]
        if twice:
            st = call2("gf_smp_neighbourhood_gather_bwd2_ex_f32", GatherSet, 5, args, over, {"dhprev": outs[1]})
        else:
            st = call("gf_smp_neighbourhood_gather_bwd_ex_f32", args, over)
        if status:
            return st, outs, []
        context().check(st)
        res = [taken(o, c.nV, c.H) for o in outs]
        return res if twice else res[0]

    def readout(self, c, hL_, target=True, loss=True, status=False, **over):
        H, nMol = c.H, c.nMol
        out = {"g": guarded(nMol, H), "yhat": guarded(nMol, 1), "loss": guarded(nMol, 1), "dy": guarded(nMol, 1), "dW": guarded(1, H, c.dW0)}
        args = [("H", H), ("nV", c.nV), ("nMol", nMol), ("hL", dev(hL_)), ("mol_ptr", dev(c.mol_ptr, np.int32)), ("W", dev(c.W)),
                ("target", dev(c.target) if target else None), ("g", out["g"]), ("yhat", out["yhat"]), ("loss", out["loss"] if loss else None),
                ("dy", out["dy"]), ("dW", out["dW"])]
        st = call("gf_smp_neighbourhood_readout_ex_f32", args, over)
        if status:
            return st, [out[k] for k in ("g", "yhat", "loss", "dy")], [(out["dW"], c.dW0)]
        context().check(st)
        r = {k: taken(out[k], nMol, H if k == "g" else 1, written=loss or k != "loss") for k in ("g", "yhat", "loss", "dy")}
        r["dW"] = taken(out["dW"], 1, H, prefilled=True)[0]
        return r


DEVICE = Device()


def merge(worst, err):
    for k, v in err.items():
        worst[k] = max(worst.get(k, 0.0), v)


def report(title, err):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in sorted(err.items()))))
    bad = {k: v for k, v in err.items() if not v <= TOL}
    assert not bad, (title, bad)


def flat(d, keys):
    return [d[k] for k in keys if d.get(k) is not None]


def same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x, dtype=np.float32).view(np.uint32), np.asarray(y, dtype=np.float32).view(np.uint32))


@pytest.mark.parametrize("H", cases.WIDTHS)
def test_every_instantiation(gf, H):
    """sum and pairs at every lane-group width and both channel counts per lane, F' = 1, 4, 15, three rounds of slots and one vertex:
    lists of 0, 1 (pairs: n exactly 0), 2 and 12 members, some with the vertex itself; all four kernels and the read-out, every row of
    h, n, A, T, Tt, dz, dn, dn Tt, <dn, A>, dh_{l-1}, g, the prediction, dy, the loss and dW"""
    for pairs in (False, True):
        worst = {}
        for FD in cases.FDS:
            c = cases.instantiation_case(H, FD, pairs)
            assert c.nV == 3 * cases.slots(H) + 1
            merge(worst, cases.check_chain(c, DEVICE)[0])
        report("H=%d %s" % (H, "pairs" if pairs else "sum"), worst)


@pytest.mark.parametrize("H", cases.ROUND_WIDTHS)
def test_rounds_and_ragged_tails(gf, H):
    """one, two and three rounds of a workgroup's slots over 1 .. 6 slots + 1 vertices (ragged first rounds, dead later rounds, the
    clamp to vertex nV - 1): each run per row against fp64, and rounds = 2, 3 give the bits of rounds = 1 -- a vertex's arithmetic does
    not depend on its slot or round"""
    for pairs in (False, True):
        worst = {}
        for nV in cases.round_sizes(H):
            c = cases.rounds_case(H, nV, pairs)
            err, first = cases.check_chain(c, DEVICE, rounds=1, what=("fwd", "node"))
            merge(worst, err)
            for rounds in (2, 3):
                err, again = cases.check_chain(c, DEVICE, rounds=rounds, what=("fwd", "node"))
                merge(worst, err)
                same_bits(first, again)
        report("rounds H=%d %s" % (H, "pairs" if pairs else "sum"), worst)


@pytest.mark.parametrize("H,nV", cases.OWN_ROUNDS)
def test_the_levels_own_two_rounds(gf, H, nV):
    """rounds = 0 at the smallest vertex count where vertices_per_group itself picks two rounds, with a last workgroup whose first round
    is ragged and whose second round is dead"""
    for pairs in (False, True):
        err, _ = cases.check_chain(cases.own_rounds_case(H, nV, pairs), DEVICE, rounds=0)
        report("the level's own grid H=%d nV=%d %s" % (H, nV, "pairs" if pairs else "sum"), err)


@pytest.mark.parametrize("level0", [True, False], ids=["level0", "with_W2"])
@pytest.mark.parametrize("H", cases.RANGE_WIDTHS)
def test_softmax_range(gf, H, level0):
    """integer pre-activations far outside what expf takes without the row maximum: one channel 100 above the rest, all +120, all -120,
    a spread over [-100, 100], the maximum at channel 0, at H - 1 and at a lane's second channel, and a row of equal z.  Every h finite,
    every row within the measure of the fp64 softmax and of sum 1."""
    c = cases.range_case(H, level0)
    out = DEVICE.forward(c)
    err = cases.check_forward(c, out)
    ref = ops.forward(c.W1, c.x, c.W2, c.hprev, c.Tprev, c.ptr, c.idx, c.pairs)
    den = ops.forward_dens(c.W1, c.x, c.W2, c.hprev, c.Tprev, c.ptr, c.idx, c.pairs, ref)
    err["row sum"] = ops.row_err(out["h"].astype(np.float64).sum(axis=1), np.ones(c.nV), den["T"])
    equal = [n for n, _ in cases.range_rows(H)].index("all equal")
    assert np.abs(out["h"][equal] * H - 1).max() <= 4 * np.finfo(np.float32).eps
    report("softmax range H=%d %s" % (H, "level 0" if level0 else "with W2"), err)


@pytest.mark.parametrize("H", cases.LONG_WIDTHS)
def test_long_lists(gf, H):
    """a hub of 300 members (301 with the shared source), lists of 63, 64 and 65, a source with 301 consumers, ten sources with none
    (pairs: their gradient is exactly 0): forward and gather, both forms"""
    for pairs in (False, True):
        err, _ = cases.check_chain(cases.long_case(H, pairs), DEVICE, what=("fwd", "node", "gather"))
        report("long lists H=%d %s" % (H, "pairs" if pairs else "sum"), err)


@pytest.mark.parametrize("kind", ["top", "inner", "level0"])
@pytest.mark.parametrize("H", cases.ROUND_WIDTHS)
def test_node_backward(gf, H, kind):
    """the top level (dy[mol] W: molecules of 1 and 40 vertices), an inner level and level 0 (no W2: dz alone, nothing else stored); h
    rows with exact 0 and exact 1, where dz -- and for a one-hot row dn, dn Tt and <dn, A> -- must be exactly 0; dz replaces dh"""
    for pairs in (False, True):
        c, h, A, Tt = cases.node_case(H, kind, pairs)
        out = DEVICE.node(c, h, A, Tt, kind == "top")
        assert not out["dz"][(h == 0) | (h == 1)].any()
        report("node backward H=%d %s %s" % (H, kind, "pairs" if pairs else "sum"), cases.check_node(c, h, A, Tt, kind == "top", out))


@pytest.mark.parametrize("nMol", cases.READOUT_MOLS)
@pytest.mark.parametrize("H", cases.READOUT_WIDTHS)
def test_readout(gf, H, nMol):
    """fewer molecules than the 16 rows of the dW fold, exactly 16, 17 and 33; molecules of 1 and of 300 vertices; one and two 64-channel
    workgroups; dW from a non-zero prefill; without targets and without a loss buffer"""
    c = cases.readout_case(H, nMol)
    worst = {}
    for target, loss in ((True, True), (False, True), (True, False)):
        merge(worst, cases.check_readout(c, c.hprev, DEVICE.readout(c, c.hprev, target, loss), target, loss))
    report("read-out H=%d nMol=%d (%d vertices)" % (H, nMol, c.nV), worst)


@pytest.mark.parametrize("case", ["H=5 sum", "H=128 pairs", "two rounds H=20 pairs", "long H=64 pairs"])
def test_same_bits_twice(gf, case):
    c, rounds = {"H=5 sum": (cases.instantiation_case(5, 4, False), 0), "H=128 pairs": (cases.instantiation_case(128, 15, True), 0),
                 "two rounds H=20 pairs": (cases.own_rounds_case(20, 4101, True), 0), "long H=64 pairs": (cases.long_case(64, True), 0)}[case]
    same_bits(cases.check_chain(c, DEVICE, rounds)[1], cases.check_chain(c, DEVICE, rounds)[1])


@pytest.mark.parametrize("pairs", [False, True], ids=["sum", "pairs"])
@pytest.mark.parametrize("H", [5, 65])
def test_one_set_and_two_set_entries_share_one_path(gf, H, pairs):
    """each of the three kernels through its one-set entry, and through its two-set entry with that set given twice and outputs of its
    own per set: the three results are the same bits.  One and two channels per lane; 37 vertices are more than a workgroup's slots at
    either width (32 and 4), the last round ragged; the node kernel as an inner and as the top level"""
    c = cases.Case(H, 4, pairs, cases.mixed_lists(37, np.random.default_rng(8000 + H)), seed=23 * H + pairs)
    assert c.nV == 37 > cases.slots(H)
    f, f2 = DEVICE.forward(c), DEVICE.forward(c, twice=True)
    for two in f2:
        same_bits(flat(f, ("h", "n", "A", "T", "Tt")), flat(two, ("h", "n", "A", "T", "Tt")))
    for top in (False, True):
        nb, nb2 = DEVICE.node(c, f["h"], f["A"], f["Tt"], top), DEVICE.node(c, f["h"], f["A"], f["Tt"], top, twice=True)
        for two in nb2:
            same_bits(flat(nb, ("dz", "dn", "gTt", "sA")), flat(two, ("dz", "dn", "gTt", "sA")))
    g, g2 = DEVICE.gather(c, nb["dn"], nb["gTt"], nb["sA"]), DEVICE.gather(c, nb["dn"], nb["gTt"], nb["sA"], twice=True)
    same_bits([g, g], g2)


def test_parity_under_poison(gf):
    """GF_POISON=1: no kernel of the level reads memory nobody wrote -- the instantiation and rounds tests in a fresh child process"""
    kit.run_under_poison(__file__, "every_instantiation or rounds_and_ragged")


def test_refusals_leave_the_context_usable(gf):
    """every refusal answers GF_ERR_INVALID, names its reason and writes nothing; then the same context serves a call.  Every case of
    a level kernel is asked of its one-set entry and of its two-set entry with the offending set in position 1"""
    from graphflow_amd import _lib
    c = cases.instantiation_case(9, 4, True)
    f = cases.Numpy32().forward(c)
    nb = cases.Numpy32().node(c, f["h"], f["A"], f["Tt"])
    i64, i32 = (lambda a: np.asarray(a, dtype=np.int64)), (lambda a: np.asarray(a, dtype=np.int32))

    def refused(answer):
        st, untouched, prefilled = answer
        assert st == _lib.GF_ERR_INVALID, st
        assert all(bool((t == SENTINEL).all()) for t in untouched)
        for t, was in prefilled:
            a = t.cpu().numpy()
            assert np.array_equal(a[:was.size], was.ravel()) and np.all(a[was.size:] == SENTINEL)
        assert context().lib.gf_last_error(context().handle)

    def still_works():
        report("after a refusal", cases.check_chain(c, DEVICE)[0])

    def bad(a, at, value):
        a = np.array(a)
        a[at] = value
        return a

    shapes = [dict(H=0), dict(H=129), dict(H=-1), dict(nV=0), dict(nV=-3)]
    for kw in shapes + [dict(FD=0), dict(rounds=-1), dict(W1=None), dict(x=None), dict(h=None), dict(hprev=None),
                        dict(ptr=None), dict(idx=None), dict(n=None), dict(Tprev=None), dict(A=None), dict(T=None), dict(Tt=None),
                        dict(H=128, FD=186), dict(ptr=i64(bad(c.ptr, 0, 1))), dict(ptr=i64(bad(c.ptr, 5, c.ptr[4] - 1))),
                        dict(idx=i32(bad(np.append(c.idx, 0), 3, c.nV))), dict(idx=i32(bad(np.append(c.idx, 0), 0, -1)))]:
        refused(DEVICE.forward(c, status=True, **kw))
        refused(DEVICE.forward(c, status=True, twice=True, **kw))
    still_works()
    for kw in shapes + [dict(rounds=-1), dict(h=None), dict(dh=None), dict(dn=None), dict(A=None), dict(Tt=None), dict(gTt=None), dict(sA=None)]:
        refused(DEVICE.node(c, f["h"], f["A"], f["Tt"], status=True, **kw))
        refused(DEVICE.node(c, f["h"], f["A"], f["Tt"], status=True, twice=True, **kw))
    for kw in (dict(Wout=None), dict(vmol=None), dict(nMol=0), dict(vmol=i32(bad(c.vmol, 2, c.nMol))), dict(vmol=i32(bad(c.vmol, c.nV - 1, -1)))):
        refused(DEVICE.node(c, f["h"], f["A"], f["Tt"], top=True, status=True, **kw))
        refused(DEVICE.node(c, f["h"], f["A"], f["Tt"], top=True, status=True, twice=True, **kw))
    still_works()
    for kw in shapes + [dict(tptr=None), dict(tidx=None), dict(dn=None), dict(dhprev=None), dict(gTt=None), dict(sA=None), dict(hprev=None),
                        dict(Tprev=None), dict(tptr=i64(bad(c.tptr, 0, 2))), dict(tptr=i64(bad(c.tptr, 7, c.tptr[6] - 1))),
                        dict(tidx=i32(bad(np.append(c.tidx, 0), 1, c.nV))), dict(tidx=i32(bad(np.append(c.tidx, 0), 1, -2)))]:
        refused(DEVICE.gather(c, nb["dn"], nb["gTt"], nb["sA"], status=True, **kw))
        refused(DEVICE.gather(c, nb["dn"], nb["gTt"], nb["sA"], status=True, twice=True, **kw))
    still_works()
    for kw in shapes + [dict(nMol=0), dict(hL=None), dict(mol_ptr=None), dict(W=None), dict(g=None), dict(yhat=None), dict(dy=None), dict(dW=None),
                        dict(mol_ptr=i32(bad(c.mol_ptr, 0, 1))), dict(mol_ptr=i32(bad(c.mol_ptr, 2, c.mol_ptr[1] - 1))),
                        dict(mol_ptr=i32(bad(c.mol_ptr, c.nMol, c.nV + 1)))]:
        refused(DEVICE.readout(c, f["h"], status=True, **kw))
    still_works()
