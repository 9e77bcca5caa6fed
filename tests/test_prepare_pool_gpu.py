"""GPU suite for what a handle keeps from one prepared batch to the next (smp_prepare.hip: the pool of device blocks, gf_smp_batch): one
handle per prepare path and variant runs the batches A, B, A, A, A, A -- four toy molecules, eight larger ones, then A four times, which is
the "idle for three prepares, then freed" rule of the pool -- with a forward and a backward after every prepare.
  * gf_smp_device_bytes after every step equals tests/golden/prepare_pool_bytes.json, recorded on the commit that file names (the pool's
    arithmetic is integer: which block backs which request, how far the pool grows and what it frees are decided by the order, element
    type and count of the requests alone);
  * predictions and gradients of every A batch have the bits of the first;
  * a prepare refused before the old batch is let go (a molecule above max_nVertices) leaves that batch usable: a forward straight after
    the refusal gives the previous predictions bit for bit.
The gated handle takes its accumulate = 1 sweep buffer lazily: on B and on the last A, into zeroed gradients.  No test reads the reference tree."""
import json
import os

import numpy as np
import pytest

from inputs import synthetic_molecule, toy_molecules

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "prepare_pool_bytes.json")
F, D, MAXV, NCLASS = 5, 1, 14, 3   # (no molecule of A or B has MAXV vertices: LCNN's sequences never need its padding row)
SEQUENCE = "ABAAAA"
ACCUMULATE_AT = (1, 5)             # the gated handle's steps with accumulate = 1


def make_nets():
    """name -> (constructor, kind of batch)"""
    from graphflow_amd import GCA1D, GCNMW, LCNN, SMPDistance, SMPGatedNeighbourhood, SMPKernelPairs, SMPNeighbourhood
    from graphflow_amd.smp import SMP1D, SMP2D, SMPClassifier, SMPGamma, SMPOmega, SMPTheta, SMPUnrestricted
    return {
        "omega_c16": (lambda: SMPOmega(2, 16, F, D, 6, True), "plain"),
        "gamma": (lambda: SMPGamma(2, 8, F, D, MAXV, True), "plain"),
        "classifier_ver6": (lambda: SMPClassifier(NCLASS, 2, 8, F, D, 6), "labels"),
        "theta": (lambda: SMPTheta(MAXV, MAXV, 2, 8, F, D), "plain"),
        "smp_1d_ver3": (lambda: SMP1D(3, MAXV, 2, 4, F, D), "plain"),
        "smp_2d": (lambda: SMP2D("2d", MAXV, 2, 5, F, D), "plain"),
        "smp_2d_ver5": (lambda: SMP2D("ver5", MAXV, 2, 8, F, D), "plain"),
        "unrestricted_2d": (lambda: SMPUnrestricted("2d", MAXV, 2, 4, F, D), "plain"),
        "gcn_2d": (lambda: SMPNeighbourhood("gcn_2d", 2, 8, F, D, MAXV, 2), "plain"),
        "gru_gcn_2d": (lambda: SMPGatedNeighbourhood("gru_gcn_2d", 2, 8, F, D, MAXV, 2), "plain"),
        "gcn_3d": (lambda: SMPNeighbourhood("gcn_3d", 2, 8, F, D, MAXV, 2), "plain"),
        "gcn_1d_distance": (lambda: SMPDistance("gcn_1d_distance", 2, 8, F, D, MAXV, 2), "distance"),
        "gcn_1d_kernel": (lambda: SMPKernelPairs("gcn_1d_kernel", 2, MAXV, F, 8, D, 2), "pairs"),
        "gca_1d": (lambda: GCA1D(2, MAXV, F, 8, D, 2), "gram"),
        "lcnn": (lambda: LCNN(MAXV, F, 3, D, 4, 3, 4), "plain"),
        "gcn_mw": (lambda: GCNMW(2, MAXV, F, 8, D), "plain"),
    }


def molecules(which):
    """A: the four toy molecules (their four features and a column of zeros); B: eight synthetic molecules of 6 .. 13 vertices"""
    if which == "A":
        return [(adj, np.concatenate([feat, np.zeros((len(adj), 1))], axis=1), t) for _, adj, feat, t in toy_molecules()]
    return [synthetic_molecule(400 + i, nV=n) for i, n in enumerate((9, 13, 6, 11, 8, 12, 7, 10))]


def distances(adj):
    """a distance matrix for a distance handle: |i - j| + 1/2 off the diagonal (finite, symmetric)"""
    i = np.arange(len(adj), dtype=np.float64)
    d = np.abs(i[:, None] - i[None, :])
    return np.where(d > 0, d + 0.5, 0.0)


def batch_of(kind, which):
    """(arguments of net.prepare, targets or None)"""
    mols = molecules(which)
    graphs = [(a, f) for a, f, _ in mols]
    targets = np.array([t for *_, t in mols])
    if kind == "labels":
        return (graphs,), np.arange(len(mols)) % NCLASS
    if kind == "distance":
        return ([(a, f, distances(a)) for a, f in graphs],), targets
    if kind == "pairs":   # X_p with the molecule after it as Y_p
        return (graphs, graphs[1:] + graphs[:1]), targets
    if kind == "gram":
        return (graphs,), None
    return (graphs,), targets


def run_sequence(name):
    """The batches of SEQUENCE through one handle: ([(in_use, reserved)] per step, [(predictions, gradients)] per step, bit patterns)"""
    make, kind = make_nets()[name]
    net = make()
    params = torch.as_tensor(np.random.default_rng(7).uniform(-0.3, 0.3, net.n_params).astype(np.float32)).cuda()
    sizes, results = [], []
    for step, which in enumerate(SEQUENCE):
        args, targets = batch_of(kind, which)
        net.prepare(*args)
        tg = None if targets is None else torch.as_tensor(targets.astype(np.float32)).cuda()
        out = net.forward(params) if kind == "gram" else net.forward(params, tg)
        pred = (out if kind == "gram" else out[0]).cpu().numpy().copy()
        grads = torch.zeros(net.n_params, device="cuda")
        net.backward(params, grads, accumulate=name == "gru_gcn_2d" and step in ACCUMULATE_AT)
        torch.cuda.synchronize()
        sizes.append(list(net.device_bytes()))
        results.append((pred, grads.cpu().numpy()))
    net.close()
    return sizes, results


def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["omega_c16", "gamma", "classifier_ver6", "theta", "smp_1d_ver3", "smp_2d", "smp_2d_ver5", "unrestricted_2d",
                                  "gcn_2d", "gru_gcn_2d", "gcn_3d", "gcn_1d_distance", "gcn_1d_kernel", "gca_1d", "lcnn", "gcn_mw"])
def test_pool_bytes_and_repeated_batches(gf, name):
    sizes, results = run_sequence(name)
    print(name, sizes)
    assert sizes == recorded()["bytes"][name]
    first = results[0]
    assert np.isfinite(first[0]).all() and np.isfinite(first[1]).all() and np.abs(first[1]).max() > 0
    for step, which in enumerate(SEQUENCE):
        if which == "A":
            assert np.array_equal(results[step][0], first[0]), (name, step)
            assert np.array_equal(results[step][1], first[1]), (name, step)
    assert not np.array_equal(results[1][1], first[1])


@pytest.mark.parametrize("name", ["theta", "gcn_2d"])
def test_a_prepare_refused_early_keeps_the_previous_batch(gf, name):
    """molecule 1 of the refused batch has MAXV + 1 vertices: refused before the handle lets go of anything"""
    from graphflow_amd.ops import GraphFlowHipError
    make, kind = make_nets()[name]
    net = make()
    params = torch.as_tensor(np.random.default_rng(7).uniform(-0.3, 0.3, net.n_params).astype(np.float32)).cuda()
    args, targets = batch_of(kind, "A")
    net.prepare(*args)
    tg = torch.as_tensor(targets.astype(np.float32)).cuda()
    before = [t.cpu().numpy().copy() for t in net.forward(params, tg)]
    held = net.device_bytes()
    too_big = (np.zeros((MAXV + 1, MAXV + 1), dtype=np.int32), np.zeros((MAXV + 1, F)))
    with pytest.raises(GraphFlowHipError, match="molecule 1 has %d vertices, the model was created with max_nVertices = %d" % (MAXV + 1, MAXV)):
        net.prepare([args[0][0], too_big])
    assert net.device_bytes() == held
    after = [t.cpu().numpy() for t in net.forward(params, tg)]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    grads = torch.zeros(net.n_params, device="cuda")
    net.backward(params, grads)
    assert np.isfinite(grads.cpu().numpy()).all()
    net.close()
