"""GPU suite for GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (gf_smp_create, readout = 1 with neighbourhood = 2, 3, 6) and GCA_1D (readout = 2
with neighbourhood = 2) on the softmax neighbourhood level with the read-outs of smp_level_readouts.hip.  Checked against the real
classes' numbers (tests/golden/smp_pair_gram.npz), block by block of the parameter vector, and at shapes without a golden against
tests/pair_gram_ref.py, which tests/test_smp_pair_gram.py pins to the real classes at 1e-9.  Tolerance: the suite's 1e-5 (tests/util.py:
rel_err) for the final feature or G, the prediction, the loss and every parameter block; no element is excused.  Inputs of the 3D class
satisfy the gap condition of tests/third_order_ref.py on both graphs of a pair, decided on the CPU before any device runs; its packed inputs
are admitted at a quarter of the tolerance, as GCN_3D_Distance's (tests/test_smp_distance_gpu.py says why).  No test reads the reference
tree."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import neighbourhood_ref as nref
import pair_gram_ref as pref
from field_suite import TOL, blockwise, dev, f64
from test_smp_pair_gram import CHECKPOINTS, FORMS, gca_case, gca_config, gca_tags, pair_case, pair_config, pair_tags, refused_configs, train_batch
from third_order_ref import GAP
from unrestricted_cases import packing_batch
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PACK_L, PACK_R, PACK_MAXV, PACK_D, PACK_F = 3, 2, 12, 0, 5
WIDTHS = (5, 8, 17, 32, 33, 64)   # every class; lane groups of 8, 32, 64
WIDE = (65, 128)                  # the 1D / 2D pair classes and GCA: two channels per lane
_PACK = {}


def golden():
    return kit.load_golden("smp_pair_gram.npz")


def pair_net(form, L, H, F, D, maxV, R=1):
    from graphflow_amd import SMPKernelPairs
    return SMPKernelPairs(FORMS[form], L, maxV, F, H, D, R)


def gca_net(L, H, F, D, maxV, R=1):
    from graphflow_amd import GCA1D
    return GCA1D(L, maxV, F, H, D, R)


def run_pairs(form, graphs, targets, params, L, H, D, maxV, R=1, **kw):
    """graphs = (X's, Y's): [predict, loss, final_feature, grads (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: pair_net(form, L, H, graphs[0][0][1].shape[1], D, maxV, R), graphs, targets, params, **kw)


def run_gca(mols, params, L, H, D, maxV, R=1, inspect=None):
    """[loss, the Gram matrices, grads (, inspect(net))]"""
    net = gca_net(L, H, mols[0][1].shape[1], D, maxV, R)
    assert net.n_params == np.asarray(params).size
    net.prepare(mols)
    p = dev(params)
    out = [f64(net.forward(p)), [g.astype(np.float64) for g in net.gram()]]
    grads = torch.full((net.n_params,), float("nan"), device="cuda")
    net.backward(p, grads)
    out.append(f64(grads))
    if inspect:
        out.append(inspect(net))
    net.close()
    return out


def lists_of(net, graph, V, L):
    return [[net.receptive_field(graph, l, v) for v in range(V)] for l in range(L + 1)]


@pytest.mark.parametrize("form", list(FORMS))
def test_pairs_match_the_real_classes(gf, form):
    """Every pair of tests/golden/smp_pair_gram.npz: CH4 with a one-vertex graph, X identical to Y, an isolated vertex on one side, the
    6-cycle with the 12-vertex molecule at 0 and 3 levels, max_Radius = 0, and for the 2D class max_Radius = 1 at three levels.  The lists
    N_l(v) of graph 2 p and 2 p + 1 through gf_smp_receptive_field, for the small case every h_l[v] through gf_smp_read_activation."""
    gz = golden()
    for tag in pair_tags(gz, form):
        _, L, H, D, R, M, gx, gy, (pred_ref, loss_ref, target), params = pair_case(gz, tag)

        def inspect(net):
            acts = [np.concatenate([net.activation(g, l, v) for l in range(L + 1) for v in range(len(a))]) for g, (a, _) in enumerate((gx, gy))]
            return (acts, [lists_of(net, g, len(a), L) for g, (a, _) in enumerate((gx, gy))], net.level_sizes(L),
                    int(net.lib.gf_smp_feature_width(net.handle)))

        pred, loss, feat, grads, (acts, lists, sizes, width) = run_pairs(form, ([gx], [gy]), [target], params, L, H, D, M, R, inspect=inspect)
        e = blockwise(grads, gz[tag + "__grads"], pref.blocks(H, gx[1].shape[1] * (D + 1), L, 1))
        print(tag, rel_err(pred, [pred_ref]), rel_err(feat[0], gz[tag + "__final_feature"]), rel_err(loss, [loss_ref]), e)
        assert pred.shape == (1,) and feat.shape == (1, 2 * H)
        assert rel_err(pred, [pred_ref]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__final_feature"]) <= TOL, tag
        assert rel_err(loss, [loss_ref]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        for side, name in enumerate(("x", "y")):
            assert np.array_equal(pref.lists_flat(lists[side], L), gz["%s__lists_%s" % (tag, name)]), tag
            assert lists[side][0] == [[v] for v in range(len((gx, gy)[side][0]))], tag
            if "%s__activations_%s" % (tag, name) in gz:
                assert rel_err(acts[side], gz["%s__activations_%s" % (tag, name)]) <= TOL, tag
        nV = len(gx[0]) + len(gy[0])
        assert sizes == (nV, nV, 0) and width == 2 * H, tag


def test_gca_matches_the_real_class(gf):
    """Every molecule of the golden: one vertex, CH4 (V = max_nVertices), an isolated vertex (V < max_nVertices), an asymmetric adjacency,
    an entry of 2, the 12-vertex molecule at 0 and 3 levels: G, the loss, every parameter block, the lists, CH4's h_l[v]."""
    gz = golden()
    for tag in gca_tags(gz):
        L, H, D, R, M, (adj, feat), loss_ref, params = gca_case(gz, tag)
        V = len(adj)

        def inspect(net):
            return (np.concatenate([net.activation(0, l, v) for l in range(L + 1) for v in range(V)]), lists_of(net, 0, V, L),
                    int(net.lib.gf_smp_feature_width(net.handle)))

        loss, gram, grads, (act, lists, width) = run_gca([(adj, feat)], params, L, H, D, M, R, inspect=inspect)
        e = blockwise(grads, gz[tag + "__grads"], pref.blocks(H, feat.shape[1] * (D + 1), L, 2))
        print(tag, rel_err(gram[0], gz[tag + "__gram"]), rel_err(loss, [loss_ref]), e)
        assert gram[0].shape == (V, V) and rel_err(gram[0], gz[tag + "__gram"]) <= TOL, tag
        assert rel_err(loss, [loss_ref]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        assert np.array_equal(pref.lists_flat(lists, L), gz[tag + "__lists"]) and width == 0, tag
        if tag + "__activations" in gz:
            assert rel_err(act, gz[tag + "__activations"]) <= TOL, tag


class GcaTrajectory:
    """GCA1D under field_suite.check_momentum_trajectory, which hands every forward the recorded targets: the auto-encoder has none"""

    def __init__(self, net):
        self.net, self.n_params, self.uniform_init, self.backward, self.prepare = net, net.n_params, net.uniform_init, net.backward, net.prepare

    def forward(self, p, targets):
        return None, self.net.forward(p)


@pytest.mark.parametrize("form", [2, 3, 6, 0])
def test_momentum_steps_match_the_real_classes(gf, form):
    """Three BatchLearn steps of the real class (pairs of the four toy molecules; GCA_1D on the four molecules): initial weights from
    gf_smp_uniform_init_host after the same srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    p_ = "train_%s__" % ("p%d" % form if form else "g")
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in z[p_ + "cfg"])
    batch = train_batch(z, form)
    lr, gamma = float(z[p_ + "lr"][0]), float(z[p_ + "momentum"][0])
    net = pair_net(form, L, H, 4, D, maxV, R) if form else gca_net(L, H, 4, D, maxV, R)
    mols = ([x for x, _ in batch], [y for _, y in batch]) if form else batch
    kit.check_momentum_trajectory(net if form else GcaTrajectory(net), lambda p, g: net.step(p, g, lr, len(batch), gamma), z, p_, mols, seed, nIter, lr)
    net.close()


@pytest.mark.parametrize("kind", CHECKPOINTS)
def test_checkpoint_round_trip(gf, kind, tmp_path):
    """Every class's file (GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel, GCA_1D).  The reference's own save_model file loads to the float32 of its values in registration order (GCA_1D's holds no W); a saved file
    equals the reference's token for token and reloads to the same bits; the loaded model gives what the golden says."""
    gz = golden()
    tag = str(gz["checkpoint_%s__tag" % kind])
    ref_file = tmp_path / "reference.txt"
    ref_file.write_bytes(bytes(gz["checkpoint_%s__text" % kind]))
    tokens = ref_file.read_text().split()
    if kind != "g":
        form, L, H, D, R, M, gx, gy, result, params = pair_case(gz, tag)
        net = pair_net(form, L, H, 4, D, M, R)
    else:
        L, H, D, R, M, mol, loss_ref, params = gca_case(gz, tag)
        net = gca_net(L, H, 4, D, M, R)
    assert len(tokens) == net.n_params
    loaded = net.load_model(torch.zeros(net.n_params, device="cuda"), ref_file)
    assert np.array_equal(loaded.cpu().numpy(), np.array([float(t) for t in tokens], dtype=np.float32))
    net.save_model(dev(params), tmp_path / "ours.txt")
    assert (tmp_path / "ours.txt").read_text().split() == tokens
    q = net.load_model(torch.zeros(net.n_params, device="cuda"), tmp_path / "ours.txt")
    assert np.array_equal(q.cpu().numpy(), loaded.cpu().numpy())
    if kind != "g":
        net.prepare([gx], [gy])
        pred = f64(net.forward(q, dev(result[2:3]))[0])
        assert rel_err(pred, result[:1]) <= TOL
    else:
        net.prepare([mol])
        assert rel_err(f64(net.forward(q)), [loss_ref]) <= TOL
        assert rel_err(net.gram()[0], gz[tag + "__gram"]) <= TOL
    net.close()


# ---- the 70-molecule packing batch: 35 pairs of unequal sizes, and the same 70 molecules for GCA_1D ----
def pack_pairs():
    """X_p = molecule 2 p, Y_p = molecule 2 p + 1 of the packing batch (5 and 4, 3 and 6 vertices seventeen times, 12 and 7): the X / Y
    boundaries fall inside a workgroup's vertices"""
    if "pairs" not in _PACK:
        mols, tg = packing_batch()
        _PACK["pairs"] = (([mols[2 * p] for p in range(35)], [mols[2 * p + 1] for p in range(35)]), np.array([tg[2 * p] - tg[2 * p + 1] + 0.1 * (p % 3) for p in range(35)]))
    return _PACK["pairs"]


def reference_pairs(form, graphs, tg, params, H, dtype=np.float64):
    """pair_gram_ref over the batch, one evaluation per DISTINCT pair: the prediction does not depend on the target and the gradient is
    linear in dy = predict - target, so a copy's result is its original's with the gradient scaled by the ratio of the two dy"""
    first, res = {}, []
    for gx, gy, t in zip(graphs[0], graphs[1], tg):
        key = (gx[0].tobytes(), gx[1].tobytes(), gy[0].tobytes(), gy[1].tobytes())
        if key not in first:   # (the base evaluation: at a target one away where the pair's own would leave dy near zero)
            r0 = pref.run_pair(form, gx, gy, t, params, PACK_L, H, PACK_D, PACK_R, dtype=dtype)
            first[key] = (r0, t) if abs(r0["predict"] - dtype(t)) >= 0.01 else (pref.run_pair(form, gx, gy, t + 1, params, PACK_L, H, PACK_D, PACK_R, dtype=dtype), t + 1)
        r0, t0 = first[key]
        dy0, dy = r0["predict"] - dtype(t0), r0["predict"] - dtype(t)
        res.append(r0 if t0 == t else dict(r0, loss=0.5 * dy * dy, grads=r0["grads"] * (dy / dy0)))
    return res, sum(r["grads"] for r in res)


def smooth_params(form, H, readout, rng, scale):
    """float32-exact parameters in registration order, uniform in [-scale, scale] (W2 of the 2D class divided by H, as the goldens')"""
    parts = []
    for name, n in pref.blocks(H, PACK_F, PACK_L, readout):
        w = rng.uniform(-1.0, 1.0, n) * scale
        parts.append(w / H if name.startswith("W2") and form == 3 else w)
    return np.concatenate(parts).astype(np.float32).astype(np.float64)


def admissible(H, seed):
    """the 3D class's draw of `seed`, or None: every vertex-level of both graphs of every pair satisfies the gap condition, and (the scale
    halved until it does) a numpy float32 evaluation of the restatement, selection included, meets the fp64 one within a QUARTER of the
    tolerance block by block"""
    graphs, tg = pack_pairs()
    scale = 0.5
    while scale > 0.01:
        params = smooth_params(6, H, 1, np.random.default_rng(1000 * H + seed), scale)
        res, rg = reference_pairs(6, graphs, tg, params, H)
        if min(r["gap"] for r in res) < GAP:
            return None
        rg32 = reference_pairs(6, graphs, tg, params, H, dtype=np.float32)[1]
        if blockwise(rg32.astype(np.float64), rg, pref.blocks(H, PACK_F, PACK_L, 1))[0] <= 0.25 * TOL:
            _PACK[("reference", H)] = (res, rg)   # (the fp64 expectation at these parameters: packed_pairs takes it from here)
            return params
        scale *= 0.5
    return None


def pair_params(form, H):
    if form != 6:
        return smooth_params(form, H, 1, np.random.default_rng(H + 4), 0.5)
    for seed in range(50):
        params = admissible(H, seed)
        if params is not None:
            return params
    raise AssertionError(("no admissible draw", H))


def run_packed_pairs(form, H):
    return lambda graphs, tg, params, **kw: run_pairs(form, graphs, tg, params, PACK_L, H, PACK_D, PACK_MAXV, PACK_R, **kw)


def packed_pairs(form, H):
    """the 35 pairs on the device beside their fp64 expectation, once per (class, width)"""
    def reference(graphs, tg, params, out):
        return (_PACK.get(("reference", H)) if form == 6 else None) or reference_pairs(form, graphs, tg, params, H)

    return kit.packed_case(("pairs", form, H), pack_pairs, lambda: pair_params(form, H), run_packed_pairs(form, H), reference)


@pytest.mark.parametrize("form,H", [(f, H) for f in FORMS for H in WIDTHS + (WIDE if f != 6 else ())])
def test_pairs_across_the_widths(gf, form, H):
    """35 pairs of unequal graphs against pair_gram_ref, per pair (prediction, loss, final feature) and per block of the summed gradient:
    more vertices than a workgroup's slots, every lane-group width, both channel counts per lane, more pairs than the 16 rows of the dW fold"""
    graphs, tg, params, out, (res, rg) = packed_pairs(form, H)
    assert len(graphs[0]) == 35 and all(len(x[0]) != len(y[0]) for x, y in zip(*graphs)) and sum(len(g[0]) for g in graphs[0] + graphs[1]) > 256
    e = blockwise(out[3], rg, pref.blocks(H, PACK_F, PACK_L, 1))
    worst_feat = max(rel_err(out[2][p], res[p]["final_feature"]) for p in range(35))
    print(form, H, rel_err(out[0], [r["predict"] for r in res]), worst_feat, e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert rel_err(out[1], np.array([r["loss"] for r in res])) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e


def packed_gca(H):
    """the 70 molecules under GCA_1D beside their fp64 expectation, once per width"""
    if ("gca", H) not in _PACK:
        mols = packing_batch()[0]
        params = smooth_params(2, H, 2, np.random.default_rng(H + 9), 0.5)
        out = run_gca(mols, params, PACK_L, H, PACK_D, PACK_MAXV, PACK_R)
        first, res = {}, []
        for a, f in mols:   # (no targets: a copy's result is its original's)
            key = (a.tobytes(), f.tobytes())
            if key not in first:
                first[key] = pref.run_gca(a, f, params, PACK_L, H, PACK_D, PACK_R)
            res.append(first[key])
        _PACK[("gca", H)] = (mols, params, out, res, sum(r["grads"] for r in res))
    return _PACK[("gca", H)]


@pytest.mark.parametrize("H", WIDTHS + WIDE)
def test_gca_across_the_widths(gf, H):
    """the 70 molecules against pair_gram_ref: every G, every loss, every block of the summed gradient"""
    mols, params, (loss, gram, grads), res, rg = packed_gca(H)
    e = blockwise(grads, rg, pref.blocks(H, PACK_F, PACK_L, 2))
    worst_gram = max(rel_err(gram[m], res[m]["gram"]) for m in range(len(mols)))
    print(H, worst_gram, rel_err(loss, [r["loss"] for r in res]), e)
    assert worst_gram <= TOL
    assert rel_err(loss, np.array([r["loss"] for r in res])) <= TOL
    assert e[0] <= TOL, e


@pytest.mark.parametrize("form,H", [(2, 33), (3, 65), (6, 17)])
def test_one_pair_isolated_inside_the_batch(gf, form, H):
    """With every other target equal to its prediction only pair 34 (12 and 7 vertices) has a loss gradient: the batch gradient is then
    that pair's own, and its prediction and final feature are those it has alone."""
    kit.check_isolated(packed_pairs(form, H), 34, run_packed_pairs(form, H), pref.blocks(H, PACK_F, PACK_L, 1), outputs=True)


def test_one_molecule_alone_gives_its_gram_and_loss(gf):
    """GCA_1D: a molecule's G and loss inside the batch are those it has alone"""
    mols, params, (loss, gram, _), _, _ = packed_gca(17)
    for m in (0, 68, 69):
        alone = run_gca(mols[m:m + 1], params, PACK_L, 17, PACK_D, PACK_MAXV, PACK_R)
        assert rel_err(alone[0], loss[m:m + 1]) <= TOL and rel_err(alone[1][0], gram[m]) <= TOL


@pytest.mark.parametrize("form,H", [(2, 8), (3, 128), (6, 32)])
def test_two_runs_give_the_same_bits(gf, form, H):
    kit.check_same_bits(packed_pairs(form, H), run_packed_pairs(form, H))


def test_two_gca_runs_give_the_same_bits(gf):
    mols, params, out = packed_gca(33)[:3]
    again = run_gca(mols, params, PACK_L, 33, PACK_D, PACK_MAXV, PACK_R)
    assert np.array_equal(out[0], again[0]) and np.array_equal(out[2], again[2])
    assert all(np.array_equal(a, b) for a, b in zip(out[1], again[1]))


@pytest.mark.parametrize("form,H", [(2, 5), (3, 65), (6, 17)])
def test_accumulate_and_a_second_sweep(gf, form, H):
    """pairs: after one forward a second backward gives the bits of the first (the read-out's reverse rebuilds dh_L from dy), and
    backward(accumulate=True) onto the first result gives twice the first result, which is exact in fp32"""
    graphs, tg, params = packed_pairs(form, H)[:3]
    net = pair_net(form, PACK_L, H, PACK_F, PACK_D, PACK_MAXV, PACK_R)
    net.prepare(*graphs)
    p = dev(params)
    net.forward(p, dev(tg))
    first, again = torch.full((net.n_params,), float("nan"), device="cuda"), torch.full((net.n_params,), float("nan"), device="cuda")
    net.backward(p, first)
    net.backward(p, again)
    twice = first.clone()
    net.backward(p, twice, accumulate=True)
    net.close()
    a, b, c = (t.cpu().numpy() for t in (first, again, twice))
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(c, 2 * a)


def test_gca_backward_follows_any_forward_once(gf):
    """GCA_1D: backward works after a forward that asked for nothing (Predict), needs no second Gram launch, and a second reverse sweep
    asks for a new forward (dz_L has replaced dh_L in place)"""
    from graphflow_amd.ops import GraphFlowHipError
    mols, params, (_, _, grads), _, _ = packed_gca(8)
    net = gca_net(PACK_L, 8, PACK_F, PACK_D, PACK_MAXV, PACK_R)
    net.prepare(mols)
    p, g = dev(params), torch.full((net.n_params,), float("nan"), device="cuda")
    net.ctx.check(net.lib.gf_smp_forward(net.handle, C.c_void_p(p.data_ptr()), None, None, None, None))   # (not even the loss)
    counts = kit.traced_counts(net, lambda: net.backward(p, g))
    assert "gram_readout" not in counts and counts["nbh_node_bwd"] == PACK_L + 1, counts
    assert np.array_equal(f64(g), grads)
    with pytest.raises(GraphFlowHipError, match="second reverse sweep of a Gram handle"):
        net.backward(p, g)
    net.forward(p)
    net.backward(p, g)
    assert np.array_equal(f64(g), grads)
    net.close()


@pytest.mark.parametrize("kind", ["gcn_1d_kernel", "gcn_2d_kernel", "gcn_3d_kernel", "gca_1d"])
def test_kernel_table(gf, kind):
    """The launches of one step are fixed: the levels' own (one forward and one node launch per level, one gather or third-order pool
    per level from 1 on, the TN products), and the read-out's: pair_readout, pair_readout_dW and pair_dh, or ONE gram_readout.  Neither
    nbh_readout nor nbh_readout_dW."""
    L, H = PACK_L, 20
    if kind == "gca_1d":
        net, mols = gca_net(L, H, PACK_F, PACK_D, PACK_MAXV, PACK_R), packing_batch()[0]
        net.prepare(mols)
        p = dev(smooth_params(2, H, 2, np.random.default_rng(1), 0.5))
        fwd = lambda: net.forward(p)   # noqa: E731
        expect = {"gram_readout": 1}
    else:
        form = {v: k for k, v in FORMS.items()}[kind]
        graphs, tg = pack_pairs()
        net = pair_net(form, L, H, PACK_F, PACK_D, PACK_MAXV, PACK_R)
        net.prepare(*graphs)
        p = dev(smooth_params(form, H, 1, np.random.default_rng(1), 0.5))
        fwd = lambda: net.forward(p, dev(tg))   # noqa: E731
        expect = {"pair_readout": 1, "pair_readout_dW": 1, "pair_dh": 1}
    grads = torch.empty(net.n_params, device="cuda")
    counts = kit.traced_counts(net, lambda: (fwd(), net.backward(p, grads)))
    net.close()
    expect.update({"nbh_level_fwd": L + 1, "nbh_node_bwd": L + 1, "gemm_tn": 2 * L + 1})
    expect.update({"third_pool_fwd": L, "third_pool_bwd": L} if kind == "gcn_3d_kernel" else {"nbh_gather_bwd": L})
    print(kind, counts)
    assert counts == expect, counts


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of these models reads memory
    nobody wrote.  The golden cases, the trajectories and the isolated-pair shapes in a fresh child process."""
    kit.run_under_poison(__file__, "real_class or momentum_steps or isolated_inside or alone_gives")


def test_a_zero_readout_is_inert(gf):
    """Existing behaviour: a readout = 0 GCN_1D handle, built through the Python structure with the new field, on the packing batch against
    neighbourhood_ref at TOL (the existing suites pin its bits)"""
    from graphflow_amd import SMPNeighbourhood
    mols, tg = packing_batch()
    L, H, D, R = 3, 17, 1, 2
    net = SMPNeighbourhood("gcn_1d", L, H, PACK_F, D, PACK_MAXV, R)
    assert net.cfg.readout == 0
    net.close()
    rng = np.random.default_rng(3)
    params = (rng.uniform(-0.5, 0.5, nref.n_params(H, PACK_F * (D + 1), L))).astype(np.float32).astype(np.float64)
    out = kit.run_net(lambda: SMPNeighbourhood("gcn_1d", L, H, PACK_F, D, PACK_MAXV, R), mols, tg, params)
    res = [nref.run(2, a, f, t, params, L, H, D, R) for (a, f), t in zip(mols, tg)]
    rg = sum(r["grads"] for r in res)
    e = blockwise(out[3], rg, nref.blocks(H, PACK_F * (D + 1), L))
    print(rel_err(out[0], [r["predict"] for r in res]), e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert rel_err(out[1], np.array([r["loss"] for r in res])) <= TOL
    assert max(rel_err(out[2][m], res[m]["final_feature"]) for m in range(len(mols))) <= TOL
    assert e[0] <= TOL, e


def test_refusals_leave_the_context_usable(gf):
    """The GF_ERR_UNSUPPORTED answers, the prepare-call mismatches, gf_smp_gram before a forward, targets on a Gram handle and the refused
    configurations, each followed by a call that succeeds on the same context"""
    from graphflow_amd import SMPNeighbourhood, _lib
    from graphflow_amd.ops import GraphFlowHipError
    gz = golden()
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def packed(net, mols):
        pk = net.pack(mols)
        return (len(pk["nV"]), pk["nV"].ctypes.data_as(IP), pk["adj"].ctypes.data_as(IP), pk["feature"].ctypes.data_as(DP)), pk

    def five_unsupported(net, p, grads, works):
        lib, ctx, h = net.lib, net.ctx, C.c_void_p()
        assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
        works()
        assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
        works()
        masks = (C.c_uint * 64)()
        assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
        works()
        dfeat = torch.zeros(64, device="cuda")
        assert lib.gf_smp_backward_features(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(grads.data_ptr()), C.c_void_p(dfeat.data_ptr()),
                                            0) == _lib.GF_ERR_UNSUPPORTED
        works()
        y = np.zeros(8)
        assert lib.gf_smp_forward_host(net.handle, None, y.ctypes.data_as(DP), None, None) == _lib.GF_ERR_UNSUPPORTED   # by name, also without a model
        assert b"read-out (readout = " in lib.gf_last_error(ctx.handle)
        host = np.zeros(net.n_params, dtype=np.float32)
        assert lib.gf_smp_parameters_upload(net.handle, host.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
        assert lib.gf_smp_forward_host(net.handle, None, y.ctypes.data_as(DP), None, None) == _lib.GF_ERR_UNSUPPORTED
        assert b"read-out (readout = " in lib.gf_last_error(ctx.handle)
        works()

    for form in FORMS:   # ---- the pair handles
        tag = "p%d_CH4_one" % form
        _, L, H, D, R, M, gx, gy, result, params = pair_case(gz, tag)
        net = pair_net(form, L, H, 4, D, M, R)
        lib, ctx = net.lib, net.ctx
        p, grads, target = dev(params), torch.empty(net.n_params, device="cuda"), dev(result[2:3])

        def works():
            net.prepare([gx], [gy])
            pred, _, feat = net.forward(p, target)
            net.backward(p, grads)
            assert rel_err(pred.cpu().numpy(), result[:1]) <= TOL
            assert rel_err(feat.cpu().numpy()[0], gz[tag + "__final_feature"]) <= TOL

        works()
        five_unsupported(net, p, grads, works)
        ptrs, pk = packed(net, [gx])
        cm = np.zeros(pk["adj"].size)
        assert lib.gf_smp_prepare(net.handle, *ptrs) == _lib.GF_ERR_INVALID                   # a pair handle without its second batch
        assert b"gf_smp_prepare_pairs" in lib.gf_last_error(ctx.handle)
        works()
        assert lib.gf_smp_prepare_coulomb(net.handle, *ptrs, cm.ctypes.data_as(DP)) == _lib.GF_ERR_INVALID
        works()
        assert lib.gf_smp_prepare_distance(net.handle, *ptrs, cm.ctypes.data_as(DP)) == _lib.GF_ERR_INVALID
        works()
        assert lib.gf_smp_gram(net.handle, C.c_void_p(grads.data_ptr())) == _lib.GF_ERR_UNSUPPORTED
        works()
        big = (np.zeros((M + 1, M + 1), dtype=np.int32), np.zeros((M + 1, 4)))
        with pytest.raises(GraphFlowHipError, match="graph Y of pair 1 has %d vertices" % (M + 1)):   # the pair and the side are named
            net.prepare([gx, gx], [gy, big])
        works()
        with pytest.raises(GraphFlowHipError, match="graph X of pair 0"):
            net.prepare([big], [gy])
        works()
        plain = SMPNeighbourhood({2: "gcn_1d", 3: "gcn_2d", 6: "gcn_3d"}[form], L, H, 4, D, M, R)   # any other handle
        assert lib.gf_smp_prepare_pairs(plain.handle, *ptrs, *ptrs[1:]) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_gram(plain.handle, C.c_void_p(grads.data_ptr())) == _lib.GF_ERR_UNSUPPORTED
        plain.prepare([gx])
        plain.close()
        works()
        net.close()
    # ---- the Gram handle
    L, H, D, R, M, mol, loss_ref, params = gca_case(gz, "g_CH4")
    net = gca_net(L, H, 4, D, M, R)
    lib, ctx = net.lib, net.ctx
    p, grads = dev(params), torch.empty(net.n_params, device="cuda")

    def works():
        net.prepare([mol])
        loss = net.forward(p)
        net.backward(p, grads)
        assert rel_err(f64(loss), [loss_ref]) <= TOL and rel_err(net.gram()[0], gz["g_CH4__gram"]) <= TOL

    flat = torch.zeros(len(mol[0]) ** 2, device="cuda")
    net.prepare([mol])
    assert lib.gf_smp_gram(net.handle, C.c_void_p(flat.data_ptr())) == _lib.GF_ERR_INVALID        # before a forward
    assert b"before gf_smp_forward" in lib.gf_last_error(ctx.handle)
    works()
    five_unsupported(net, p, grads, works)
    one = torch.zeros(1, device="cuda")
    for args in ((C.c_void_p(one.data_ptr()), None, None, None), (None, C.c_void_p(one.data_ptr()), None, None),
                 (None, None, None, C.c_void_p(one.data_ptr()))):                                  # targets, predict, graph_feature: all NULL
        assert lib.gf_smp_forward(net.handle, C.c_void_p(p.data_ptr()), *args) == _lib.GF_ERR_INVALID
        assert b"a Gram handle (readout = 2) has no targets" in lib.gf_last_error(ctx.handle)
        works()
    ptrs, pk = packed(net, [mol])
    assert lib.gf_smp_prepare_pairs(net.handle, *ptrs, *ptrs[1:]) == _lib.GF_ERR_UNSUPPORTED
    works()
    assert lib.gf_smp_prepare_coulomb(net.handle, *ptrs, np.zeros(pk["adj"].size).ctypes.data_as(DP)) == _lib.GF_ERR_UNSUPPORTED
    works()
    with pytest.raises(GraphFlowHipError):   # a molecule above max_nVertices
        net.prepare([(np.zeros((M + 1, M + 1), dtype=np.int32), np.zeros((M + 1, 4)))])
    works()
    h = C.c_void_p()
    for bad, _ in refused_configs():
        assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID
    works()
    net.close()
    assert pair_config(2, 1, 4, 4, 0, 5).readout == 1 and gca_config(1, 4, 4, 0, 5).readout == 2
