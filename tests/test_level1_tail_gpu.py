"""The two kernels of a level whose sources are all single vertices (level 1) -- tables-forward on smp_tables_fwd_single, a lane group per
(node, b) pair, and the backward gather on smp_bwd_gather_single, several sources per wave -- against the general kernels
(GF_SMP_LEVEL1=0: smp_tables_fwd_w, smp_bwd_gather_all): every output bit for bit, with the handle's count of single-vertex launches
as the evidence of which ran (the launch names are the same).  And the read-out's weight gradient, whose thread runs are requested
sixteen molecules at a time, against the same sums written out in numpy."""
import os

import numpy as np
import pytest

from field_suite import dev, run_under_poison
from inputs import edge_molecules, smp_params, synthetic_molecule
from util import golden_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F, D, CAP = 5, 2, 12


def graph(V, edges, seed):
    adj = np.zeros((V, V), dtype=np.int32)
    for u, v in edges:
        adj[u, v] = adj[v, u] = 1
    rng = np.random.default_rng(seed)
    feat = np.zeros((V, F))
    feat[np.arange(V), rng.integers(0, F, V)] = 1.0
    return adj, feat


ATOM, PAIR, PATH3, TRIANGLE = graph(1, [], 1), graph(2, [(0, 1)], 2), graph(3, [(0, 1), (1, 2)], 3), graph(3, [(0, 1), (1, 2), (0, 2)], 4)
STAR5 = graph(6, [(0, k) for k in range(1, 6)], 5)
# a vertex of degree 8 (level-1 field of 9 positions: the widest size class of tables-forward below 17), a ring through four of its
# neighbours and a tail of two
DEG8 = graph(11, [(0, k) for k in range(1, 9)] + [(1, 2), (2, 3), (3, 4), (8, 9), (9, 10)], 6)


def batches(golden):
    syn12 = golden_cases(golden, "smp_syn12")["smp_syn12"]
    edge = {name: (adj, feat) for name, adj, feat, _ in edge_molecules(F)}
    mixed = [(syn12["adj"], syn12["feature"]), STAR5, edge["two_fragments"], edge["isolated_vertex"], ATOM, DEG8, synthetic_molecule(77, nV=9)[:2]]
    out = {"one, two and three vertices": [ATOM, PAIR, PATH3, TRIANGLE, ATOM],   # 10 vertices
           "5-star": [STAR5],
           "degree 8": [DEG8],
           "mixed batch of 7": mixed,
           "4k+1 vertices": [ATOM, PAIR, PATH3, TRIANGLE],    # 9
           "4k+2 vertices": [ATOM, PAIR, PATH3],              # 6
           "4k+3 vertices": [PAIR, PATH3, PAIR],              # 7
           "one vertex": [ATOM]}
    assert [sum(len(a) for a, _ in out[k]) % 4 for k in ("4k+1 vertices", "4k+2 vertices", "4k+3 vertices")] == [1, 2, 3]
    assert len(mixed) == 7 and len(mixed[0][0]) == 12
    return out


def run(mols, L, C, seed=3, counts=None):
    """predict, loss, feature, gradients and every f_l the handle exposes, as the device's float32; counts (a list): the handle's
    single-vertex launches and the number this batch should give are appended"""
    from graphflow_amd.smp import SMPOmega
    net = SMPOmega(L, C, F, D, CAP, True)
    net.prepare(mols)
    p = dev(smp_params(C, F, D, L, seed))
    tg = np.array([float(len(a)) for a, _ in mols])
    pred, loss, feat = net.forward(p, dev(tg))
    acts = [net.activation(m, l, v) for m, (a, _) in enumerate(mols) for l in range(L + 1) for v in range(len(a))]
    grads = torch.empty(net.n_params, device="cuda")
    net.backward(p, grads)
    out = [pred.cpu().numpy(), loss.cpu().numpy(), feat.cpu().numpy(), grads.cpu().numpy()] + acts
    if counts is not None:
        # expected: for every level whose SOURCES (the nodes of the level below) all have one position -- level 1 always, a further level
        # only in a batch of isolated vertices -- one launch per size class of tables-forward (fields up to 64 / (C / 4) positions,
        # twice, four times, eight times that) and one of the gather
        ppw, expect = 64 // (C // 4), 0
        sizes = [{len(net.receptive_field(m, l, v)) for m, (a, _) in enumerate(mols) for v in range(len(a))} for l in range(L + 1)]
        for l in range(1, L + 1):
            if max(sizes[l - 1]) == 1:
                expect += len({min(k for k in (1, 2, 4, 8) if s <= k * ppw) for s in sizes[l]}) + 1
        counts.append((net.single_vertex_launches(), expect))
    net.close()
    return out


def blocks(C, L):
    """name -> slice of the parameter vector (inputs.smp_param_count)"""
    b, o = {"H": slice(0, C * F * (D + 1))}, C * F * (D + 1)
    for l in range(1, L + 1):
        b["K%d" % l], b["b%d" % l] = slice(o, o + 18 * C * C), slice(o + 18 * C * C, o + 18 * C * C + C)
        o += 18 * C * C + C
    b["W"] = slice(o, o + C)
    return b


@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("C", [64, 32, 16])
def test_single_vertex_sources_gather_gives_the_general_kernels_bits(gf, golden, monkeypatch, C, L):
    """tables-forward AND the backward gather of level 1 (the name dates from the gather alone): the switch moves both, and a forward
    and backward pass launch the single-vertex kernels once per size class plus once for the gather at every level whose sources are
    single vertices (level 1; also level 2 of the batch that is one isolated vertex) -- or never"""
    for name, mols in batches(golden).items():
        monkeypatch.delenv("GF_SMP_LEVEL1", raising=False)
        n_on, n_off = [], []
        on = run(mols, L, C, counts=n_on)
        again = run(mols, L, C)
        monkeypatch.setenv("GF_SMP_LEVEL1", "0")
        off = run(mols, L, C, counts=n_off)
        assert n_on[0][0] == n_on[0][1] >= 2 and n_off[0][0] == 0, (name, n_on, n_off)
        assert np.isfinite(on[3]).all() and np.abs(on[3]).max() > 0, name
        for k, what in enumerate(("predict", "loss", "feature")):
            assert np.array_equal(on[k], off[k]), (name, what)
        for blk, sl in blocks(C, L).items():
            assert np.array_equal(on[3][sl], off[3][sl]), (name, blk, np.abs(on[3][sl].astype(np.float64) - off[3][sl]).max())
        assert len(on) == len(off) and all(np.array_equal(x, y) for x, y in zip(on[4:], off[4:])), name
        assert all(np.array_equal(x, y) for x, y in zip(on, again)), name   # two runs: identical bits


def test_level1_under_poison():
    """GF_POISON=1 (NaN patterns in every buffer handed out without contents; read once per process): one case in a fresh process"""
    run_under_poison(os.path.abspath(__file__), "general_kernels_bits and 64-1")


def fma32(a, b, c):
    """fl32(a b + c) for float32 arrays: the product is exact in float64, the sum is rounded there first (a double rounding changes
    the float32 result only on an exact tie of the float64 sum: not with these inputs, see the test)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("nMol", [1, 33, 1024])
def test_readout_dW_is_the_ordered_sum_of_its_runs(gf, nMol):
    """dW[f] = sum over 16 runs r, in order, of (the sum over m = r, r + 16, .. in order of dy[m] g[m][f]) at C = 64: 1,024 threads =
    16 runs x 64 channels.  The device contracts dy g + acc into one fused multiply-add or not as the compiler chose: the result has
    to be one of the two, bit for bit, whatever the number of molecules a run requests together."""
    C, L = 64, 1
    kinds = [ATOM, PAIR, PATH3, TRIANGLE]
    mols = [kinds[(m * 7 + m // 5) % 4] for m in range(nMol)]
    from graphflow_amd.smp import SMPOmega
    net = SMPOmega(L, C, F, D, CAP, True)
    net.prepare(mols)
    p = dev(smp_params(C, F, D, L, 11))
    tg = np.array([0.25 * (m % 9) for m in range(nMol)], dtype=np.float32)
    pred, _, feat = net.forward(p, dev(tg))
    grads = torch.empty(net.n_params, device="cuda")
    net.backward(p, grads)
    dW = grads.cpu().numpy()[blocks(C, L)["W"]]
    g, dy = feat.cpu().numpy().reshape(nMol, C), pred.cpu().numpy() - tg   # (SquaredLoss::backward: y - t, in float32)
    net.close()
    expect = []
    for fused in (True, False):
        t = np.zeros(C, dtype=np.float32)
        for r in range(16):
            acc = np.zeros(C, dtype=np.float32)
            for m in range(r, nMol, 16):
                acc = fma32(np.full(C, dy[m], dtype=np.float32), g[m], acc) if fused else acc + dy[m] * g[m]
            t = t + acc
        expect.append(t)
    assert np.abs(dW).max() > 0
    assert np.array_equal(dW, expect[0]) or np.array_equal(dW, expect[1]), (np.abs(dW - expect[0]).max(), np.abs(dW - expect[1]).max())
