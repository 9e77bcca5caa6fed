"""CPU suite for the per-kernel tests of the gated neighbourhood level (tests/test_smp_gru_ops_gpu.py): (a) the operator references of
tests/gru_ops_ref.py, chained over a golden molecule's lists, give what tests/gru_gcn_ref.py gives at 1e-12 and so the real classes'
numbers at 1e-9; (b) a numpy float32 evaluation of every case the GPU suite runs stays within TOL / 2 of the fp64 one by every measure,
so fp32 can hold the bound the device is held to; (c) outside the gate-range cases at least half of the entries of each of z, r and c
is unsaturated -- a suite whose gates are all 0 or 1 tests nothing downstream.  The worst float32 figure per test group is printed
(NOTES.md has them beside the device's)."""
import numpy as np
import pytest

import gru_gcn_ref as gref
import gru_ops_cases as cases
import gru_ops_ref as ops
import neighbourhood_ops_ref as nops
from field_suite import TOL, blockwise, load_golden
from util import rel_err


def composed(form, adj, feat, target, params, L, H, D, R):
    """one molecule through the operator references alone: {h, n, predict, loss, graph_feature, grads}"""
    pairs = form == 5
    sp = gref.hop_distances(np.asarray(adj))
    x = gref.shell_features(np.asarray(feat, dtype=np.float64), sp, D)
    V, FD = x.shape
    P = gref.split(np.asarray(params, dtype=np.float64), H, FD)
    M6 = np.stack([P[m] for m in gref.MATRICES[:6]])
    M2 = np.stack([P[m] for m in gref.MATRICES[6:]])
    N = gref.neighbourhoods(adj, L, R, sp)
    lists = [None] + [ops.csr(N[l]) for l in range(1, L + 1)]
    h0 = gref.softmax(x @ P["W"].T)
    fwd = [{"h": h0, "T": h0.sum(axis=1)}]
    for l in range(1, L + 1):
        fwd.append(ops.cell_forward(M6, fwd[l - 1]["h"], fwd[l - 1]["T"], *lists[l], ops.PAIRS if pairs else ops.SUM))
    mol_ptr, vmol = np.array([0, V]), np.zeros(V, dtype=np.int64)
    grads = np.zeros(params.size)
    G = gref.split(grads, H, FD)
    rf = ops.readout_forward(M2, P["U"], fwd[L]["h"], mol_ptr, np.array([target]))
    rb = ops.readout_backward(M2, P["U"], rf["s"], rf["t"], rf["g"], rf["dy"], vmol, np.zeros(H))
    G["U"] += rb["dU"]
    G["W_g"] += rb["ds"].T @ fwd[L]["h"]
    G["U_g"] += rb["dt"].T @ fwd[L]["h"]
    dh = rb["dh"]
    for l in range(L, 0, -1):
        f, hp = fwd[l], fwd[l - 1]["h"]
        b = ops.cell_backward(M6, hp, dh, f["z"], f["r"], f["c"], f["A"], f["Tt"], pairs)
        for name, lhs, rhs in (("W_z", "dzp", f["n"]), ("U_z", "dzp", hp), ("W_r", "drp", f["n"]), ("U_r", "drp", hp), ("W_h", "dcp", f["n"]),
                               ("U_h", "dcp", b["q"])):
            G[name] += b[lhs].T @ rhs
        tptr, tidx = ops.transpose(*lists[l], V)
        dh = nops.gather_backward(tptr, tidx, b["dn"], hp, fwd[l - 1]["T"], pairs) + b["direct"]
    G["W"] += (dh * h0 * (1 - h0)).T @ x
    return {"h": [f["h"] for f in fwd], "n": [None] + [f["n"] for f in fwd[1:]], "predict": rf["yhat"][0], "loss": rf["loss"][0],
            "graph_feature": rf["g"][0], "grads": grads}


@pytest.mark.parametrize("mol", ["CH4", "star8_far", "syn12"])
@pytest.mark.parametrize("form", [4, 5])
def test_composed_operators_are_the_model(form, mol):
    gz = load_golden("smp_gru_gcn.npz")
    tag = "n%d_%s" % (form, mol)
    _, L, H, D, R, V = (int(v) for v in gz[tag + "__cfg"])
    adj, feat, result, params = gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"], gz[tag + "__params"].astype(np.float64)
    assert L >= 1
    r = gref.run(form, adj, feat, result[2], params, L, H, D, R)
    c = composed(form, adj, feat, result[2], params, L, H, D, R)
    blocks = gref.blocks(H, feat.shape[1] * (D + 1))
    assert max(rel_err(a, b) for a, b in zip(c["h"], r["h"])) <= 1e-12
    assert max(rel_err(a, b) if np.abs(b).max() > 0 else np.abs(a).max() for a, b in zip(c["n"][1:], r["n"][1:])) <= 1e-12
    assert rel_err([c["predict"], c["loss"]], [r["predict"], r["loss"]]) <= 1e-12 and rel_err(c["graph_feature"], r["graph_feature"]) <= 1e-12
    assert blockwise(c["grads"], r["grads"], blocks)[0] <= 1e-12
    assert rel_err([c["predict"], c["loss"]], result[:2]) <= 1e-9 and rel_err(c["graph_feature"], gz[tag + "__graph_feature"]) <= 1e-9
    assert blockwise(c["grads"], gz[tag + "__grads"], blocks)[0] <= 1e-9


def test_the_cases_are_what_the_gpu_tests_say():
    assert [cases.own_rounds(H, ("cell_fwd", "cell_bwd")) for H in cases.CELL_OWN_WIDTHS] == [1027, 8195]
    assert cases.own_rounds(64, ("readout_fwd", "readout_bwd")) == 4099
    assert [cases.slots(H) for H in (1, 8, 9, 16, 17, 32, 33, 64)] == [32, 32, 16, 16, 8, 8, 4, 4]
    c = cases.long_case(20, cases.PAIRS)
    n, t = np.diff(c.ptr), np.diff(c.tptr)
    assert list(n[:4]) == [301, 63, 64, 65] and t[399] == 301 and not t[380:390].any()
    c = cases.instantiation_case(33, cases.PAIRS)
    n = np.diff(c.ptr)
    assert c.nV == 13 and {0, 1, 2, 12} <= set(int(v) for v in n) and any(v in c.idx[c.ptr[v]:c.ptr[v + 1]] for v in range(c.nV))
    assert c.hprev.min() < -0.9 and c.hprev.max() > 0.9 and np.abs(c.hprev).max() <= 1
    for H in cases.READOUT_WIDTHS:
        sizes = set(int(v) for v in np.diff(cases.readout_case(H, 33).mol_ptr))
        assert {0, 1, 300} <= sizes
        assert [cases.readout_case(H, m).nMol for m in cases.READOUT_MOLS] == list(cases.READOUT_MOLS)
    for H in cases.RANGE_WIDTHS:   # the arguments are the intended numbers, exactly, in fp32 as in fp64; every saturated end occurs
        c = cases.range_case(H)
        rows = np.stack([a for _, a in cases.range_rows(H)])
        R = len(rows)
        for dt in (np.float64, np.float32):
            n = ops.aggregate(c.hprev, None, c.ptr, c.idx, False, dt=dt)["n"]
            M = c.M6.astype(dt)
            assert np.array_equal((n @ M[0].T)[:R], rows) and np.array_equal((n @ M[2].T)[:R], np.roll(rows, 1, axis=1))
            assert np.array_equal((n @ M[4].T)[:R], np.roll(rows, 2, axis=1) / 4) and not (n[R:].any() or M[1::2].any())
            assert np.array_equal((c.hprev.astype(dt) @ c.M2[0].astype(dt).T)[R:2 * R], rows)
        f = cases.Numpy32().cell_fwd(c)
        rf = cases.Numpy32().readout_fwd(c, c.hprev)
        for g in (f["z"], f["r"], rf["s"]):
            assert (g == 0).any() and (g == 1).any() and (g == 0.5).any()
        for g in (f["c"], rf["t"]):
            assert (g == 1).any() and (g == -1).any() and (g == 0).any()
        assert np.abs(rf["g"]).max() == 1
        names = [k for k, _ in cases.range_rows(H)]
        assert {"+30 at 0", "-90 at 0", "+120 at %d" % (H - 1), "-80 at 0", "all +120", "all -120", "all 0"} <= set(names)


def test_the_gates_of_the_main_cases_are_not_saturated():
    """at least half of the entries of each of z, r and c of every case outside the gate-range test lies in [0.05, 0.95] (|c| < 0.95)"""
    worst = (1.0, None)
    for group, label, c, what in cases.every_case():
        if "fwd" not in what:
            continue
        assert not c.saturating
        f = ops.cell_forward(c.M6, c.hprev, c.Tprev, c.ptr, c.idx, c.agg, c.n_given)
        share = ops.unsaturated(f["z"], f["r"], f["c"])
        assert min(share) >= 0.5, (group, label, share)
        worst = min(worst, (min(share), (group, label)))
    print("the smallest unsaturated share: %.2f (%s)" % worst)


def test_float32_stays_inside_half_the_bound_on_every_gpu_case():
    """a correct fp32 evaluation has room: every measure of every case at TOL / 2, no row excused"""
    b = cases.Numpy32()
    worst = {}

    def note(group, label, err):
        for k, v in err.items():
            assert v <= TOL / 2, (group, label, k, v)
            if group not in worst or v > worst[group][0]:
                worst[group] = (v, k, label)

    for group, label, c, what in cases.every_case():
        if group == "readout":
            for target, loss in ((True, True), (False, True), (True, False)):
                note(group, label, cases.check_readout_forward(c, c.hprev, b.readout_fwd(c, c.hprev, 0, target, loss), target, loss))
        note(group, label, cases.check_chain(c, b, what=what)[0])
    for H in cases.RANGE_WIDTHS:
        note("gate_range", H, cases.range_checks(cases.range_case(H), b)[0])
    for group, (v, k, label) in sorted(worst.items()):
        print("float32 %-28s %.2e (%s of %s)" % (group, v, k, label))
    assert set(worst) == {"every_instantiation", "rounds_and_ragged_tails", "the_levels_own_two_rounds", "long_lists", "readout", "gate_range"}


def test_the_measure_of_a_gate_below_the_normal_range():
    ref, den = np.array([[1e-50, 1e-45], [0.5, 0.25]]), np.array([1e-45, 0.5])
    assert cases.gate_err(np.array([[0.0, 2.0 ** -127], [0.5, 0.25]]), ref, den) == 0
    for bad in (-1e-45, 2.0 ** -125, np.nan):
        with pytest.raises(AssertionError):
            cases.gate_err(np.array([[0.0, bad], [0.5, 0.25]]), ref, den)
    assert cases.gate_err(np.array([[0.0, 0.0], [0.5, 0.25 + 1e-6]]), ref, den) == pytest.approx(2e-6, rel=1e-3)
