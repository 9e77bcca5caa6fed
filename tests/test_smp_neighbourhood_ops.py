"""CPU suite for the per-kernel tests of the neighbourhood level (tests/test_smp_neighbourhood_ops_gpu.py): (a) the operator references
of tests/neighbourhood_ops_ref.py, composed over a golden molecule's lists, give what tests/neighbourhood_ref.py gives at 1e-12 and so
the real classes' numbers at 1e-9, and the vectorised pair aggregate and its reverse are risi2d_closed / risi2d_closed_backward per
vertex; (b) a numpy float32 evaluation of every case the GPU suite runs stays within TOL / 2 of the fp64 one by every measure, so fp32
can hold the bound the device is held to.  The worst float32 figure per test group is printed (NOTES.md has them beside the device's)."""
import numpy as np
import pytest

import neighbourhood_ops_cases as cases
import neighbourhood_ops_ref as ops
import neighbourhood_ref as nref
from field_suite import TOL, blockwise, load_golden
from util import rel_err


def composed(form, adj, feat, target, params, L, H, D, R):
    """one molecule through the operator references alone: {h, predict, loss, final_feature, grads, per level (lists, fwd, dn)}"""
    pairs = form == 3
    x = nref.shell_features(np.asarray(feat, dtype=np.float64), nref.hop_distances(np.asarray(adj)), D)
    V, FD = x.shape
    W1, W2, W = nref.split(np.asarray(params, dtype=np.float64), H, FD, L)
    N = nref.neighbourhoods(form, np.asarray(adj), L, R)
    lists = [None] + [ops.csr(N[l]) for l in range(1, L + 1)]
    fwd = [ops.forward(W1[0], x, None, None, None, None, None, pairs)]
    for l in range(1, L + 1):
        fwd.append(ops.forward(W1[l], x, W2[l], fwd[l - 1]["h"], fwd[l - 1]["T"], *lists[l], pairs))
    mol_ptr = np.array([0, V])
    grads = np.zeros(params.size)
    gW1, gW2, gW = nref.split(grads, H, FD, L)
    r = ops.readout(fwd[L]["h"], mol_ptr, W, np.array([target]), gW.copy())
    gW += r["dW"]
    dh, dns = None, {}
    for l in range(L, -1, -1):
        nb = ops.node_backward(W2[l], fwd[l]["h"], dh, r["dy"] if l == L else None, W, np.zeros(V, dtype=np.int64), fwd[l]["A"],
                               fwd[l]["Tt"], pairs)
        gW1[l] += nb["dz"].T @ x
        if l == 0:
            break
        gW2[l] += nb["dz"].T @ fwd[l]["n"]
        tptr, tidx = ops.transpose(*lists[l], V)
        dh = ops.gather_backward(tptr, tidx, nb["dn"], fwd[l - 1]["h"], fwd[l - 1]["T"], pairs)
        dns[l] = (nb["dn"], dh)
    return {"h": [f["h"] for f in fwd], "predict": r["yhat"][0], "loss": r["loss"][0], "final_feature": r["g"][0], "grads": grads, "N": N,
            "fwd": fwd, "dn": dns}


@pytest.mark.parametrize("mol", ["CH4", "star8", "syn12"])
@pytest.mark.parametrize("form", [1, 2, 3])
def test_composed_operators_are_the_model(form, mol):
    gz = load_golden("smp_neighbourhood.npz")
    tag = "n%d_%s" % (form, mol)
    _, L, H, D, R, V = (int(v) for v in gz[tag + "__cfg"])
    adj, feat, result, params = gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"], gz[tag + "__params"].astype(np.float64)
    assert L >= 1
    r = nref.run(form, adj, feat, result[2], params, L, H, D, R)
    c = composed(form, adj, feat, result[2], params, L, H, D, R)
    blocks = nref.blocks(H, feat.shape[1] * (D + 1), L)
    assert max(rel_err(a, b) for a, b in zip(c["h"], r["h"])) <= 1e-12
    assert rel_err([c["predict"], c["loss"]], [r["predict"], r["loss"]]) <= 1e-12 and rel_err(c["final_feature"], r["final_feature"]) <= 1e-12
    assert blockwise(c["grads"], r["grads"], blocks)[0] <= 1e-12
    assert rel_err([c["predict"], c["loss"]], result[:2]) <= 1e-9 and rel_err(c["final_feature"], gz[tag + "__final_feature"]) <= 1e-9
    assert blockwise(c["grads"], gz[tag + "__grads"], blocks)[0] <= 1e-9
    if form != 3:
        return
    for l in range(1, L + 1):   # the vectorised pair aggregate and its reverse, per vertex / per consumer, from the definitions
        a, (dn, dh) = c["fwd"][l - 1]["h"], c["dn"][l]
        want = np.zeros_like(dh)
        for v, mem in enumerate(c["N"][l]):
            assert rel_err(c["fwd"][l]["n"][v], nref.risi2d_closed(a[mem])) <= 1e-12
            want[mem] += nref.risi2d_closed_backward(a[mem], dn[v])
        assert rel_err(dh, want) <= 1e-12


def test_the_cases_are_what_the_gpu_tests_say():
    for H, nV in cases.OWN_ROUNDS:   # the smallest vertex count at which the level itself takes two rounds, and fewer vertices than
        q, r = divmod(nV, cases.slots(H) * 256)   # one round of slots more: the last workgroup's first round ragged, its second dead
        assert q == 2 and 0 < r < cases.slots(H)
    assert [cases.slots(H) for H in (8, 9, 16, 17, 32, 33, 128)] == [32, 16, 16, 8, 8, 4, 4]
    c = cases.long_case(20, True)
    n, t = np.diff(c.ptr), np.diff(c.tptr)
    assert list(n[:4]) == [301, 63, 64, 65]
    assert t[399] == 301 and not t[380:390].any()
    c = cases.instantiation_case(33, 4, True)
    n = np.diff(c.ptr)
    assert c.nV == 13 and {0, 1, 2, 12} <= set(int(v) for v in n) and any(v in c.idx[c.ptr[v]:c.ptr[v + 1]] for v in range(c.nV))
    for H in cases.ROUND_WIDTHS:
        assert {1, 40} <= set(int(v) for v in np.diff(cases.node_case(H, "top", True)[0].mol_ptr))
    _, h, _, _ = cases.node_case(64, "inner", True)
    assert (h == 1).any() and (h == 0).any() and ((h > 0) & (h < 1)).any()
    for H in cases.RANGE_WIDTHS:
        names = [n for n, _ in cases.range_rows(H)]
        assert ("peak at 64" in names) == (H > 64) and "all +120" in names and "all -120" in names and "all equal" in names
    assert abs(c.Tprev - 1).max() > 0.3


def test_float32_stays_inside_half_the_bound_on_every_gpu_case():
    """a correct fp32 evaluation has room: every measure of every case at TOL / 2, no row excused"""
    b = cases.Numpy32()
    worst = {}
    what = {"softmax_range": ("fwd",), "long_lists": ("fwd", "node", "gather")}

    def note(group, label, err):
        for k, v in err.items():
            assert v <= TOL / 2, (group, label, k, v)
            if group not in worst or v > worst[group][0]:
                worst[group] = (v, k, label)

    for group, label, c in cases.every_case():
        if group == "readout":
            for target, loss in ((True, True), (False, True), (True, False)):
                note(group, label, cases.check_readout(c, c.hprev, b.readout(c, c.hprev, target, loss), target, loss))
        else:
            note(group, label, cases.check_chain(c, b, what=what.get(group, ("fwd", "node", "gather", "readout")))[0])
    for H in cases.ROUND_WIDTHS:
        for kind in ("top", "inner", "level0"):
            for pairs in (False, True):
                c, h, A, Tt = cases.node_case(H, kind, pairs)
                note("node_backward", (H, kind, pairs), cases.check_node(c, h, A, Tt, kind == "top", b.node(c, h, A, Tt, kind == "top")))
    for group, (v, k, label) in sorted(worst.items()):
        print("float32 %-28s %.2e (%s of %s)" % (group, v, k, label))
    assert set(worst) == {"every_instantiation", "rounds_and_ragged_tails", "the_levels_own_two_rounds", "softmax_range", "long_lists",
                          "readout", "node_backward"}


def test_row_err_excuses_nothing():
    ref, den = np.ones((3, 2)), np.array([1.0, 1.0, 0.0])
    x = ref.copy()
    assert ops.row_err(x, ref, np.ones(3)) == 0
    x[1, 1] = np.nan
    assert ops.row_err(x, ref, np.ones(3)) == np.inf
    x[1, 1] = 1 + 1e-6
    assert ops.row_err(x, ref, den) == pytest.approx(1e-6, rel=1e-3)   # (row 2 has no magnitude and is met exactly)
    x[2, 0] = 1 + 1e-30 + 1e-12
    assert ops.row_err(x, ref, den) == np.inf
