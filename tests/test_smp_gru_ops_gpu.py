"""The kernels of the gated neighbourhood level one by one (gf_smp_gru_cell_fwd_ex_f32 / _cell_bwd_ex_f32 / _readout_fwd_ex_f32 /
_readout_bwd_ex_f32: gru_cell_fwd in its three instantiations, gru_cell_bwd, gru_readout_fwd and gru_readout_mol, gru_readout_dU and
gru_readout_bwd of smp_level_gru.hip, through the level's own launchers; the gather is gf_smp_neighbourhood_gather_bwd_ex_f32) against
the fp64 evaluation of the same operands (tests/gru_ops_ref.py), per output row, relative to the row's magnitude sum.  One bound,
field_suite.TOL = 1e-5; a numpy float32 evaluation of every case here measures at most 6.4e-7 (tests/test_smp_gru_ops.py asserts
TOL / 2 on these very operands, built by tests/gru_ops_cases.py).  The helpers are tests/test_smp_neighbourhood_ops_gpu.py's: every
output lies in a buffer with sentinels behind its last row, and an output the chosen form does not store must stay untouched.  The
measured figures are in NOTES.md."""
import numpy as np
import pytest

import field_suite as kit
import gru_ops_cases as cases
from field_suite import dev
from gru_ops_cases import GIVEN, PAIRS, SUM
from test_smp_neighbourhood_ops_gpu import DEVICE as NBH, SENTINEL, call, context, guarded, merge, padded, report, same_bits, taken

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FWD = ("h", "n", "z", "r", "c", "A", "T", "Tt")
BWD = ("dzp", "drp", "dcp", "q", "dn", "gTt", "sA", "direct")


def opt(a):
    return dev(a) if a is not None else None


def rows_of(t, rows, H, **kw):
    """taken() of an [rows][H] output: two dimensions at H = 1 too"""
    a = taken(t, rows, H, **kw)
    return a if a is None else a.reshape(rows, H)


class Device:
    """the backend of gru_ops_cases.check_*: `over` replaces arguments by name; with status=True a method returns (status, the output
    buffers, [(in/out buffer, its prefill)]), else it checks the status and returns the outputs as arrays (None for one the form does
    not store)"""

    def cell_fwd(self, c, rounds=0, agg=None, given=None, status=False, over=None):
        H, nV = c.H, c.nV
        agg = c.agg if agg is None else agg
        n_in = np.asarray(c.n_given if given is None else given, dtype=np.float32)
        out = {k: guarded(nV, 1 if k in ("T", "Tt") else H, n_in if k == "n" and agg == GIVEN else None) for k in FWD}
        args = [("aggregate", agg), ("H", H), ("nV", nV), ("rounds", rounds), ("M6", dev(c.M6)), ("hprev", dev(c.hprev)), ("Tprev", dev(c.Tprev)),
                ("ptr", dev(c.ptr, np.int64)), ("idx", padded(c.idx))] + [(k, out[k]) for k in FWD]
        st = call("gf_smp_gru_cell_fwd_ex_f32", args, over or {})
        if status:
            pre = [(out["n"], n_in)] if agg == GIVEN else []
            return st, [out[k] for k in FWD if not (k == "n" and agg == GIVEN)], pre
        context().check(st)
        r = {k: (taken(out[k], nV, 1, written=agg == PAIRS) if k in ("T", "Tt") else
                 rows_of(out[k], nV, H, written=agg == PAIRS or k != "A", prefilled=k == "n" and agg == GIVEN)) for k in FWD}
        if agg == GIVEN:
            same_bits([r["n"]], [n_in])   # an operand: untouched
        return r

    def cell_bwd(self, c, z, r, cc, A, Tt, rounds=0, pairs=None, status=False, over=None):
        H, nV = c.H, c.nV
        pairs = c.pairs if pairs is None else pairs
        out = {k: guarded(nV, 1 if k == "sA" else H) for k in BWD}
        args = [("pairs", int(pairs)), ("H", H), ("nV", nV), ("rounds", rounds), ("M6", dev(c.M6)), ("hprev", dev(c.hprev)), ("dh", dev(c.dh)),
                ("z", dev(z)), ("r", dev(r)), ("c", dev(cc)), ("A", opt(A)), ("Tt", opt(Tt))] + [(k, out[k]) for k in BWD]
        st = call("gf_smp_gru_cell_bwd_ex_f32", args, over or {})
        if status:
            return st, list(out.values()), []
        context().check(st)
        return {k: taken(out[k], nV, 1, written=pairs) if k == "sA" else rows_of(out[k], nV, H, written=pairs or k != "gTt") for k in BWD}

    def gather(self, c, dn, gTt, sA):
        return NBH.gather(c, dn, gTt, sA).reshape(c.nV, c.H)

    def readout_fwd(self, c, hL, rounds=0, target=True, loss=True, status=False, over=None):
        H, nV, nMol = c.H, c.nV, c.nMol
        out = {k: guarded(nV, H) for k in ("s", "t")}
        out.update({k: guarded(nMol, H if k == "g" else 1) for k in ("g", "yhat", "loss", "dy")})
        args = [("H", H), ("nV", nV), ("nMol", nMol), ("rounds", rounds), ("M2", dev(c.M2)), ("U", dev(c.U)), ("hL", dev(hL)),
                ("mol_ptr", dev(c.mol_ptr, np.int32)), ("target", dev(c.target) if target else None), ("s", out["s"]), ("t", out["t"]),
                ("g", out["g"]), ("yhat", out["yhat"]), ("loss", out["loss"] if loss else None), ("dy", out["dy"])]
        st = call("gf_smp_gru_readout_fwd_ex_f32", args, over or {})
        if status:
            return st, list(out.values()), []
        context().check(st)
        r = {k: rows_of(out[k], nV, H) for k in ("s", "t")}
        r["g"] = rows_of(out["g"], nMol, H)
        r.update({k: taken(out[k], nMol, 1, written=loss or k != "loss") for k in ("yhat", "loss", "dy")})
        return r

    def readout_bwd(self, c, s, t, g, dy, rounds=0, status=False, over=None):
        H, nV = c.H, c.nV
        out = {"ds": guarded(nV, H), "dt": guarded(nV, H), "dh": guarded(nV, H), "dU": guarded(1, H, c.dU0)}
        args = [("H", H), ("nV", nV), ("nMol", c.nMol), ("rounds", rounds), ("M2", dev(c.M2)), ("U", dev(c.U)), ("s", dev(s)), ("t", dev(t)),
                ("g", dev(g)), ("dy", dev(dy)), ("vmol", dev(c.vmol, np.int32))] + [(k, out[k]) for k in ("ds", "dt", "dh", "dU")]
        st = call("gf_smp_gru_readout_bwd_ex_f32", args, over or {})
        if status:
            return st, [out[k] for k in ("ds", "dt", "dh")], [(out["dU"], c.dU0)]
        context().check(st)
        r = {k: rows_of(out[k], nV, H) for k in ("ds", "dt", "dh")}
        r["dU"] = rows_of(out["dU"], 1, H, prefilled=True)[0]
        return r


DEVICE = Device()


@pytest.mark.parametrize("H", cases.WIDTHS)
def test_every_instantiation(gf, H):
    """sum, pairs and given at both edges of every lane-group width and at one channel, three rounds of slots and one vertex: lists of
    0, 1 (pairs: n exactly +0), 2 and 12 members, some with the vertex itself; the cell, its reverse, the gather plus the direct part, the
    read-out and its reverse, every row of every output.  Given: n untouched, A, T, Tt all sentinels, h, z, r, c the bits of the sum form
    on the same n"""
    first = None
    for agg in (SUM, PAIRS, GIVEN):
        c = cases.instantiation_case(H, agg)
        assert c.nV == 3 * cases.slots(H) + 1
        err, arrays = cases.check_chain(c, DEVICE)
        report("H=%d %s" % (H, cases.FORM_NAMES[agg]), err)
        if agg == SUM:
            first = (c, arrays)
    c, arrays = first
    given = DEVICE.cell_fwd(c, agg=GIVEN, given=arrays[1])
    same_bits([given[k] for k in ("h", "z", "r", "c")], [arrays[i] for i in (0, 2, 3, 4)])


@pytest.mark.parametrize("H", cases.ROUND_WIDTHS)
def test_rounds_and_ragged_tails(gf, H):
    """one, two and three rounds of a workgroup's slots over 1 .. 6 slots + 1 vertices (ragged first rounds, dead later rounds, the
    clamp to vertex nV - 1) in the four kernels that take the vertices per workgroup: each run per row against fp64, and rounds = 2, 3
    give the bits of rounds = 1 -- a vertex's arithmetic does not depend on its slot or round"""
    for agg in (SUM, PAIRS):
        worst = {}
        for nV in cases.round_sizes(H):
            c = cases.rounds_case(H, nV, agg)
            err, first = cases.check_chain(c, DEVICE, rounds=1, what=("fwd", "bwd", "readout"))
            merge(worst, err)
            for rounds in (2, 3):
                err, again = cases.check_chain(c, DEVICE, rounds=rounds, what=("fwd", "bwd", "readout"))
                merge(worst, err)
                same_bits(first, again)
        report("rounds H=%d %s" % (H, cases.FORM_NAMES[agg]), worst)


@pytest.mark.parametrize("H,kernels", [(H, ("cell_fwd", "cell_bwd")) for H in cases.CELL_OWN_WIDTHS] +
                         [(H, ("readout_fwd", "readout_bwd")) for H in cases.READOUT_OWN_WIDTHS], ids=lambda v: v if isinstance(v, int) else v[0])
def test_the_levels_own_two_rounds(gf, H, kernels):
    """rounds = 0 at the smallest vertex count where vertices_per_group itself picks two rounds, and three vertices: a last workgroup
    whose first round is ragged and whose second round is dead.  The count follows from each kernel's LDS bytes (the cells' images leave
    one workgroup per CU at 64 channels, the read-out's four)"""
    nV = cases.own_rounds(H, kernels)
    per = cases.own_round(kernels, H)
    assert -(-nV // per) == 2 and 0 < nV - per < cases.slots(H)
    cell = kernels[0] == "cell_fwd"
    for agg in (SUM, PAIRS) if cell else (SUM,):
        err, _ = cases.check_chain(cases.own_rounds_case(H, nV, agg), DEVICE, rounds=0, what=("fwd", "bwd") if cell else ("readout",))
        report("the level's own grid H=%d nV=%d %s %s" % (H, nV, kernels[0], cases.FORM_NAMES[agg]), err)


@pytest.mark.parametrize("H", cases.RANGE_WIDTHS)
def test_gate_range(gf, H):
    """arguments that are exact in fp32 and far outside what expf takes: one channel at +-30, +-90, +-120 or +-80 among moderate ones,
    all +120, all -120, all 0 (c's and t's: +-7.5, +-22.5, +-30, +-20, 0).  Every stored value finite, every row within its measure, a
    gate below 2^-126 a small non-negative number; h = hp where z = 0 and h = c where z = 1, bit for bit; on those stored gates dz', dc',
    dr', ds and dt are exactly 0 at the saturated ends and nothing is NaN"""
    c = cases.range_case(H)
    err, f, rf = cases.range_checks(c, DEVICE)
    for gate in (f["z"], f["r"], rf["s"]):
        assert (gate == 0).any() and (gate == 1).any() and (gate == 0.5).any()
    for gate in (f["c"], rf["t"]):
        assert (gate == 1).any() and (gate == -1).any() and (gate == 0).any()
    assert np.abs(rf["g"]).max() == 1
    report("gate range H=%d" % H, err)


@pytest.mark.parametrize("H", cases.LONG_WIDTHS)
def test_long_lists(gf, H):
    """a hub of 300 members (301 with the shared source), lists of 63, 64 and 65, a source with 301 consumers, ten sources with none
    (pairs: their gathered gradient is exactly 0): forward, backward and gather plus the direct part, both forms"""
    for agg in (SUM, PAIRS):
        err, _ = cases.check_chain(cases.long_case(H, agg), DEVICE, what=("fwd", "bwd", "gather"))
        report("long lists H=%d %s" % (H, cases.FORM_NAMES[agg]), err)


@pytest.mark.parametrize("nMol", cases.READOUT_MOLS)
@pytest.mark.parametrize("H", cases.READOUT_WIDTHS)
def test_readout(gf, H, nMol):
    """fewer molecules than the 16 rows of the dU fold, exactly 16, 17 and 33; molecules of 1 and of 300 vertices and an empty one (g
    exactly 0); dU from a non-zero prefill; without targets and without a loss buffer, which stays untouched"""
    c = cases.readout_case(H, nMol)
    worst = {}
    for target, loss in ((False, True), (True, False)):
        merge(worst, cases.check_readout_forward(c, c.hprev, DEVICE.readout_fwd(c, c.hprev, 0, target, loss), target, loss))
    err, _ = cases.check_chain(c, DEVICE, what=("readout",))
    merge(worst, err)
    report("read-out H=%d nMol=%d (%d vertices)" % (H, nMol, c.nV), worst)


@pytest.mark.parametrize("case", ["H=5 sum", "H=64 given", "two rounds H=20 pairs", "long H=64 pairs"])
def test_same_bits_twice(gf, case):
    c, what = {"H=5 sum": (cases.instantiation_case(5, SUM), None), "H=64 given": (cases.instantiation_case(64, GIVEN), None),
               "two rounds H=20 pairs": (cases.own_rounds_case(20, cases.own_rounds(20, ("cell_fwd", "cell_bwd")), PAIRS), ("fwd", "bwd")),
               "long H=64 pairs": (cases.long_case(64, PAIRS), None)}[case]
    what = what or ("fwd", "bwd", "gather", "readout")
    same_bits(cases.check_chain(c, DEVICE, what=what)[1], cases.check_chain(c, DEVICE, what=what)[1])


def test_parity_under_poison(gf):
    """GF_POISON=1: no kernel of the level reads memory nobody wrote -- the instantiation and rounds tests in a fresh child process"""
    kit.run_under_poison(__file__, "every_instantiation or rounds_and_ragged")


def test_refusals_leave_the_context_usable(gf):
    """every refusal answers GF_ERR_INVALID, names its reason and writes nothing; then the same context serves a call"""
    from graphflow_amd import _lib
    c = cases.instantiation_case(9, PAIRS)
    g = cases.instantiation_case(9, GIVEN)
    b = cases.Numpy32()
    f = b.cell_fwd(c)
    rf = b.readout_fwd(c, f["h"])
    i64, i32 = (lambda a: np.asarray(a, dtype=np.int64)), (lambda a: np.asarray(a, dtype=np.int32))

    def refused(answer, why=None):
        st, untouched, prefilled = answer
        assert st == _lib.GF_ERR_INVALID, (st, why)
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

    shapes = [dict(H=0), dict(H=65), dict(H=-1), dict(nV=0), dict(nV=-3), dict(rounds=-1)]
    lists = [dict(ptr=i64(bad(c.ptr, 0, 1))), dict(ptr=i64(bad(c.ptr, 5, c.ptr[4] - 1))), dict(idx=i32(bad(np.append(c.idx, 0), 3, c.nV))),
             dict(idx=i32(bad(np.append(c.idx, 0), 0, -1)))]
    required = [{k: None} for k in ("M6", "hprev", "h", "n", "z", "r", "c")]
    for kw in shapes + [dict(aggregate=3), dict(aggregate=-1)] + required + [{k: None} for k in ("ptr", "idx", "Tprev", "A", "T", "Tt")] + lists:
        refused(DEVICE.cell_fwd(c, status=True, over=kw), kw)
    for kw in required + [dict(ptr=None), dict(idx=None)] + lists:
        refused(DEVICE.cell_fwd(c, agg=SUM, status=True, over=kw), kw)
    for kw in shapes + required:
        refused(DEVICE.cell_fwd(g, status=True, over=kw), kw)
    given = DEVICE.cell_fwd(g, over=dict(ptr=None, idx=None, Tprev=None, A=None, T=None, Tt=None))   # (the given form needs none of them)
    same_bits([given[k] for k in ("h", "z", "r", "c")], [DEVICE.cell_fwd(g)[k] for k in ("h", "z", "r", "c")])
    still_works()
    every = [{k: None} for k in ("M6", "hprev", "dh", "z", "r", "c", "dzp", "drp", "dcp", "q", "dn", "direct")]
    for kw in shapes + every + [{k: None} for k in ("A", "Tt", "gTt", "sA")]:
        refused(DEVICE.cell_bwd(c, f["z"], f["r"], f["c"], f["A"], f["Tt"], status=True, over=kw), kw)
    for kw in every:
        refused(DEVICE.cell_bwd(c, f["z"], f["r"], f["c"], None, None, pairs=False, status=True, over=kw), kw)
    still_works()
    for kw in shapes + [dict(nMol=0), dict(nMol=-2)] + [{k: None} for k in ("M2", "U", "hL", "mol_ptr", "s", "t", "g", "yhat", "dy")] + [
            dict(mol_ptr=i32(bad(c.mol_ptr, 0, 1))), dict(mol_ptr=i32(bad(c.mol_ptr, 2, c.mol_ptr[1] - 1))),
            dict(mol_ptr=i32(bad(c.mol_ptr, c.nMol, c.nV + 1)))]:
        refused(DEVICE.readout_fwd(c, f["h"], status=True, over=kw), kw)
    still_works()
    for kw in shapes + [dict(nMol=0)] + [{k: None} for k in ("M2", "U", "s", "t", "g", "dy", "vmol", "ds", "dt", "dh", "dU")] + [
            dict(vmol=i32(bad(c.vmol, 2, c.nMol))), dict(vmol=i32(bad(c.vmol, c.nV - 1, -1)))]:
        refused(DEVICE.readout_bwd(c, rf["s"], rf["t"], rf["g"], rf["dy"], status=True, over=kw), kw)
    still_works()
