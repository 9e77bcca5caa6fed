"""GPU suite for GCN_1D_Distance, GCN_2D_Distance and GCN_3D_Distance (gf_smp_create, distance_channel = 1 with neighbourhood = 2, 3, 6)
on the two-channel level of smp_level_neighbourhood.hip / smp_level_distance.hip.  Checked against the real classes' numbers
(tests/golden/smp_distance.npz), block by block of the parameter vector, and at shapes without a golden against tests/distance_ref.py,
which tests/test_smp_distance.py pins to the real classes at 1e-9.  Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the final
feature, the prediction, the loss and every parameter block; no element is excused.  Inputs of the 3D class satisfy the gap condition of
tests/third_order_ref.py (adjacent classes around the KMax cut 1e-5 max|T| apart in both channels), decided on the CPU before any
device runs.  No test reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as dref
import field_suite as kit
from field_suite import TOL, blockwise, dev
from make_distance_golden import point_distances, random_params
from test_smp_distance import FORMS, case, refused_configs, train_molecules
from third_order_ref import GAP
from unrestricted_cases import packing_batch
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PACK_L, PACK_R, PACK_MAXV, PACK_D = 3, 2, 13, 0   # (M = 13: every row of the batch is padded, the 12-vertex molecule by one zero)
WIDTHS = (5, 8, 17, 32, 33, 64)                    # every class; lane groups of 8, 32, 64
WIDE = (65, 128)                                   # the 1D / 2D classes: two channels per lane
_PACK = {}


def golden():
    return kit.load_golden("smp_distance.npz")


def net_of(form, L, H, F, D, maxV, R=1):
    from graphflow_amd import SMPDistance
    return SMPDistance(FORMS[form], L, H, F, D, maxV, R)


def run_net(form, mols, targets, params, L, H, D, maxV, R=1, **kw):
    """[predict, loss, final_feature, grads (, lists) (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: net_of(form, L, H, mols[0][1].shape[1], D, maxV, R), mols, targets, params, **kw)


def radj_code(net):
    buf = np.empty(64, dtype=np.float32)
    return net.lib.gf_smp_read_reduced_adjacency(net.handle, 0, min(1, net.cfg.nLevels), 0, buf.ctypes.data_as(C.c_void_p), buf.size)


@pytest.mark.parametrize("form", list(FORMS))
def test_device_matches_the_real_classes(gf, form):
    """Every case of tests/golden/smp_distance.npz: CH4, one vertex, an isolated vertex, the 6-cycle, the 12-vertex molecule at 0 and 3
    levels, V < M, the asymmetric matrix (the column convention), tied and negative distances.  The lists N_l(v) through
    gf_smp_receptive_field everywhere, for CH4 every [h^v_l[v] | h^d_l[v]] through gf_smp_read_activation."""
    gz = golden()
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        _, L, H, D, R, M, mol, (pred_ref, loss_ref, target), params = case(gz, tag)
        V = len(mol[0])

        def inspect(net):
            act = np.concatenate([net.activation(0, l, v) for l in range(L + 1) for v in range(V)])
            return act, net.level_sizes(L), int(net.lib.gf_smp_feature_width(net.handle)), radj_code(net)

        pred, loss, feat, grads, lists, (act, sizes, width, radj) = run_net(form, [mol], [target], params, L, H, D, M, R, want_fields=True,
                                                                         inspect=inspect)
        e = blockwise(grads, gz[tag + "__grads"], dref.blocks(H, mol[1].shape[1] * (D + 1), M, L))
        print(tag, rel_err(pred, [pred_ref]), rel_err(feat[0], gz[tag + "__final_feature"]), rel_err(loss, [loss_ref]), e)
        assert rel_err(pred, [pred_ref]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__final_feature"]) <= TOL, tag
        assert rel_err(loss, [loss_ref]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        assert np.array_equal(dref.lists_flat(lists[0], L), gz[tag + "__lists"]) and lists[0][0] == [[v] for v in range(V)], tag
        assert sizes == (V, V, 0) and width == 2 * H and radj == -1, tag
        if tag + "__activations" in gz:
            assert rel_err(act, gz[tag + "__activations"]) <= TOL, tag


# ---- the 70-molecule packing batch with distances attached ----
def pack_batch():
    """the packing batch's molecules with four feature columns (the fifth folded into them at half weight, so that no vertex has a row of
    zeros) and a distance matrix each: one matrix per distinct molecule (the 17 copies of a toy molecule share it and differ in their
    targets), the seven-vertex molecule's asymmetric"""
    if "batch" not in _PACK:
        mols, tg = packing_batch()
        rng, dist = np.random.default_rng(70), {}
        out = []
        for m, (a, x) in enumerate(mols):
            key = (len(a), a.tobytes())
            if key not in dist:
                dist[key] = point_distances(len(a), rng, asymmetric=len(a) == 7)
            out.append((a, np.ascontiguousarray(x[:, :4] + 0.5 * x[:, 4:5]), dist[key]))
        _PACK["batch"] = (out, tg)
    return _PACK["batch"]


def reference_batch(form, mols, tg, params, L, H, D, M, R, dtype=np.float64):
    """distance_ref over the batch, one evaluation per DISTINCT molecule: the prediction does not depend on the target and the gradient is
    linear in dy = predict - target, so a copy's result is its original's with the gradient scaled by the ratio of the two dy"""
    first, res = {}, []
    for (a, f, d), t in zip(mols, tg):
        key = (len(a), a.tobytes(), f.tobytes(), np.asarray(d).tobytes())
        if key not in first:   # (the base evaluation: at a target one away where the molecule's own would leave dy near zero)
            r0 = dref.run(form, a, f, d, t, params, L, H, D, M, R, dtype=dtype)
            first[key] = (r0, t) if abs(r0["predict"] - dtype(t)) >= 0.01 else (dref.run(form, a, f, d, t + 1, params, L, H, D, M, R, dtype=dtype), t + 1)
        r0, t0 = first[key]
        dy0, dy = r0["predict"] - dtype(t0), r0["predict"] - dtype(t)
        res.append(r0 if t0 == t else dict(r0, loss=0.5 * dy * dy, grads=r0["grads"] * (dy / dy0)))
    return res, sum(r["grads"] for r in res)


def smooth_params(form, H, FD, M, L, rng, scale):
    """float32-exact parameters in registration order, uniform in [-scale, scale] (W2 of the 2D class divided by H, as the goldens').  Not
    the goldens' multiples of 1 / 64: on one-hot features those give two channels of a wide level the same pre-activations at level 0 with
    a few per cent probability per draw, hence classes of RisiLayer3D that tie exactly -- a degenerate input, not a rounding question."""
    parts = []
    for name, n in dref.blocks(H, FD, M, L):
        w = rng.uniform(-1.0, 1.0, n) * scale
        parts.append(w / H if name.startswith("W2") and form == 3 else w)
    return np.concatenate(parts).astype(np.float32).astype(np.float64)


# The 3D class: where the search for an admissible draw starts (an admissible seed of each width, found by pack_params' own loop; the
# loop still checks the draw it is pointed at, so a wrong entry costs time, not correctness)
FIRST_SEED = {5: 0, 8: 0, 17: 3, 32: 1, 33: 9, 64: 7}


def admissible(form, H, seed):
    """the draw of `seed`, or None: every vertex-level of both channels satisfies the gap condition, and (the scale halved until it does) a
    numpy float32 evaluation of the restatement, selection included, meets the fp64 one within a QUARTER of the tolerance block by block.
    A quarter, not the half of tests/test_smp_third_order.py: the distance channel's softmax over rows of values up to 5 is peaked, the
    closed form of RisiLayer3D cancels, and one fp32 evaluation order is only a sample of what another order (the device sums A and B
    member by member and contracts into fmas) may round to -- at half, numpy's own fp32 error on a W2 block of the 8-channel case was
    3.5e-6, sixty times the unit roundoff, which leaves a factor of 1.4 for any other order (NOTES.md)."""
    mols, tg = pack_batch()
    scale = 0.5
    while scale > 0.01:
        params = smooth_params(form, H, 4, PACK_MAXV, PACK_L, np.random.default_rng(1000 * H + seed), scale)
        res, rg = reference_batch(form, mols, tg, params, PACK_L, H, PACK_D, PACK_MAXV, PACK_R)
        if min(r["gap"] for r in res) < GAP:
            return None
        rg32 = reference_batch(form, mols, tg, params, PACK_L, H, PACK_D, PACK_MAXV, PACK_R, dtype=np.float32)[1]
        if blockwise(rg32.astype(np.float64), rg, dref.blocks(H, 4, PACK_MAXV, PACK_L))[0] <= 0.25 * TOL:
            _PACK[("reference", form, H)] = (res, rg)   # (the fp64 expectation at these parameters: packed_case takes it from here)
            return params
        scale *= 0.5
    return None


def pack_params(form, H):
    """float32-exact parameters of the packed case; for the 3D class an admissible draw (tests/test_smp_third_order.py: model_case),
    decided on the CPU before any device runs"""
    if form != 6:
        return smooth_params(form, H, 4, PACK_MAXV, PACK_L, np.random.default_rng(H + 4), 0.5)
    seed = FIRST_SEED.get(H, 0)
    for seed in range(seed, seed + 50):
        params = admissible(form, H, seed)
        if params is not None:
            return params
    raise AssertionError(("no admissible draw", form, H))


def run_packed(form, H):
    return lambda mols, tg, params, **kw: run_net(form, mols, tg, params, PACK_L, H, PACK_D, PACK_MAXV, PACK_R, **kw)


def packed_case(form, H):
    """the packing batch on the device beside its fp64 expectation, once per (class, width)"""
    def reference(mols, tg, params, out):
        res, rg = _PACK.get(("reference", form, H)) or reference_batch(form, mols, tg, params, PACK_L, H, PACK_D, PACK_MAXV, PACK_R)
        assert out[4] == [r["N"] for r in res]
        return res, rg

    return kit.packed_case(("distance", form, H), pack_batch, lambda: pack_params(form, H), run_packed(form, H), reference, want_fields=True)


@pytest.mark.parametrize("form,H", [(f, H) for f in FORMS for H in WIDTHS + (WIDE if f != 6 else ())])
def test_batch_across_the_widths(gf, form, H):
    """the 70-molecule packing batch against distance_ref, per molecule (prediction, loss, final feature) and per block of the summed
    gradient: more vertices than a workgroup's slots, a ragged last workgroup, every lane-group width, both channel counts per lane, and
    two operand widths (F' = 4 beside M = 13) in every launch"""
    mols, tg, params, out, (res, rg) = packed_case(form, H)
    assert len(mols) == 70 and sum(len(m[0]) for m in mols) > 256 and max(len(m[0]) for m in mols) < PACK_MAXV
    e = blockwise(out[3], rg, dref.blocks(H, 4, PACK_MAXV, PACK_L))
    worst_feat = max(rel_err(out[2][m], res[m]["final_feature"]) for m in range(len(mols)))
    print(form, H, rel_err(out[0], [r["predict"] for r in res]), worst_feat, e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert rel_err(out[1], np.array([r["loss"] for r in res])) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e


@pytest.mark.parametrize("form,H", [(2, 33), (3, 65), (6, 17)])
def test_one_molecule_isolated_inside_the_batch(gf, form, H):
    """With every other target equal to its prediction only molecule 68 (the 12-vertex one) has a loss gradient: the batch gradient is
    then that molecule's single-molecule gradient, and its prediction and final feature are those it has alone."""
    kit.check_isolated(packed_case(form, H), 68, run_packed(form, H), dref.blocks(H, 4, PACK_MAXV, PACK_L), outputs=True)


@pytest.mark.parametrize("form,H", [(2, 8), (3, 128), (6, 32)])
def test_two_runs_give_the_same_bits(gf, form, H):
    kit.check_same_bits(packed_case(form, H), run_packed(form, H))


@pytest.mark.parametrize("form,H", [(2, 5), (3, 65), (6, 17)])
def test_accumulate_and_a_second_sweep(gf, form, H):
    """after one forward a second backward gives the bits of the first, and backward(accumulate=True) onto the first result gives twice
    the first result, which is exact in fp32"""
    mols, tg, params = packed_case(form, H)[:3]
    net = net_of(form, PACK_L, H, 4, PACK_D, PACK_MAXV, PACK_R)
    net.prepare(mols)
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


@pytest.mark.parametrize("form", list(FORMS))
def test_launches_per_channel_give_the_same_bits(gf, form, monkeypatch):
    """GF_SMP_DISTANCE_LAUNCHES=2 (every level kernel once per channel, what tools/distance_time.py compares with): the same bits"""
    case_ = packed_case(form, 17)
    monkeypatch.setenv("GF_SMP_DISTANCE_LAUNCHES", "2")
    kit.check_same_bits(case_, run_packed(form, 17))


@pytest.mark.parametrize("form", list(FORMS))
def test_batch_of_one_vertex_molecules(gf, form):
    """five molecules of one vertex: every neighbourhood is the vertex itself (2D and 3D: n = 0 exactly), a row is the diagonal entry
    and two zeros"""
    rng = np.random.default_rng(7)
    mols = [(np.zeros((1, 1), dtype=np.int32), np.round(rng.random((1, 4)) * 8) / 8, np.array([[0.25 * (m - 1)]])) for m in range(5)]
    tg = np.arange(5) * 0.25
    L, H, D, M = 2, 6, 1, 3
    params = random_params(form, H, 4 * (D + 1), M, L, rng, 0.5)
    out = run_net(form, mols, tg, params, L, H, D, M, 1)
    res, rg = dref.run_batch(form, mols, tg, params, L, H, D, M, 1)
    blocks = dref.blocks(H, 4 * (D + 1), M, L)
    e = blockwise(out[3], rg, blocks)
    print(form, rel_err(out[0], [r["predict"] for r in res]), e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert max(rel_err(out[2][m], res[m]["final_feature"]) for m in range(5)) <= TOL
    assert e[0] <= TOL, e
    if form != 2:   # (W2 sees n = 0 everywhere: its gradient is exactly zero, in both channels)
        off = 0
        for name, n in blocks:
            assert name[:2] != "W2" or not out[3][off:off + n].any(), name
            off += n


@pytest.mark.parametrize("form", list(FORMS))
def test_permutation_invariance(gf, form):
    """these models have no vertex ordering: the final feature of the 12-vertex molecule does not depend on the numbering, when the
    distance matrix is renumbered with the adjacency"""
    gz = golden()
    _, L, H, D, R, M, (adj, x, dist), _, params = case(gz, "n%d_syn12" % form)
    perm = np.random.default_rng(0).permutation(len(adj))
    padj, px, pdist = adj[np.ix_(perm, perm)], x[perm], dist[np.ix_(perm, perm)]
    a = run_net(form, [(adj, x, dist)], np.array([1.0]), params, L, H, D, M, R)
    b = run_net(form, [(padj, px, pdist)], np.array([1.0]), params, L, H, D, M, R)
    ra = dref.run(form, adj, x, dist, 1.0, params, L, H, D, M, R)
    rb = dref.run(form, padj, px, pdist, 1.0, params, L, H, D, M, R)
    assert rb["gap"] >= GAP and ra["gap"] >= GAP
    assert rel_err(rb["final_feature"], ra["final_feature"]) <= 1e-12
    assert rel_err(b[2], a[2]) <= TOL
    assert rel_err(a[2][0], ra["final_feature"]) <= TOL


@pytest.mark.parametrize("form", list(FORMS))
def test_momentum_steps_match_the_real_classes(gf, form):
    """Three BatchLearn steps of the real class on the four toy molecules: initial weights from gf_smp_uniform_init_host after the same
    srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    p_ = "train_n%d__" % form
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in z[p_ + "cfg"])
    mols = train_molecules(z)
    lr, gamma = float(z[p_ + "lr"][0]), float(z[p_ + "momentum"][0])
    net = net_of(form, L, H, 4, D, maxV, R)
    kit.check_momentum_trajectory(net, lambda p, g: net.step(p, g, lr, len(mols), gamma), z, p_, mols, seed, nIter, lr)
    net.close()


def test_checkpoint_round_trip(gf, tmp_path):
    """The reference's own save_model file -- channel by channel, not in registration order -- loads to the float32 of its values at their
    registration-order places; a saved file equals the reference's token for token and reloads to the same bits; the loaded model
    predicts what the golden and the restatement at the loaded values say."""
    gz = golden()
    tag = str(gz["checkpoint__tag"])
    form, L, H, D, R, M, mol, result, params = case(gz, tag)
    FD = mol[1].shape[1] * (D + 1)
    ref_file = tmp_path / "reference.txt"
    ref_file.write_bytes(bytes(gz["checkpoint__text"]))
    tokens = ref_file.read_text().split()
    net = net_of(form, L, H, 4, D, M, R)
    loaded = net.load_model(torch.zeros(net.n_params, device="cuda"), ref_file).cpu().numpy()
    assert np.array_equal(loaded, dref.from_checkpoint(np.array([float(t) for t in tokens], dtype=np.float32), H, FD, M, L))
    assert rel_err(loaded, params) <= 1e-5 and not np.array_equal(dref.to_checkpoint(loaded, H, FD, M, L), loaded)
    net.save_model(dev(params), tmp_path / "ours.txt")
    assert (tmp_path / "ours.txt").read_text().split() == tokens
    q = net.load_model(torch.zeros(net.n_params, device="cuda"), tmp_path / "ours.txt")
    assert np.array_equal(q.cpu().numpy(), loaded)
    net.prepare([mol])
    pred = kit.f64(net.forward(q, dev(result[2:3]))[0])
    net.close()
    r = dref.run(form, mol[0], mol[1], mol[2], float(result[2]), loaded.astype(np.float64), L, H, D, M, R)["predict"]
    print(tag, pred, r, result[0])
    assert rel_err(pred, [r]) <= TOL and rel_err(pred, result[:1]) <= TOL


@pytest.mark.parametrize("form", list(FORMS))
def test_kernel_table(gf, form):
    """The launches of one step are fixed: per level ONE forward launch and ONE node launch for both channels, one gather per level from 1
    on (the 3D class: third_pool_fwd and third_pool_bwd once per channel and level instead), the read-out and its dW, and the TN products
    dW1 (2 (L + 1)) and dW2 (2 L), unsplit at this batch's 325 vertices.  Nothing else."""
    mols, tg = pack_batch()
    L, H = PACK_L, 20
    net = net_of(form, L, H, 4, PACK_D, PACK_MAXV, PACK_R)
    net.prepare(mols)
    p = dev(random_params(form, H, 4, PACK_MAXV, L, np.random.default_rng(1), 0.5))
    grads = torch.empty(net.n_params, device="cuda")
    counts = kit.traced_counts(net, lambda: (net.forward(p, dev(tg)), net.backward(p, grads)))
    net.close()
    expect = {"nbh_level_fwd": L + 1, "dist_readout": 1, "dist_readout_dW": 1, "nbh_node_bwd": L + 1, "gemm_tn": 2 * (2 * L + 1)}
    expect.update({"third_pool_fwd": 2 * L, "third_pool_bwd": 2 * L} if form == 6 else {"nbh_gather_bwd": L})
    print(form, counts)
    assert counts == expect, counts


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of these models reads memory
    nobody wrote.  The golden cases, the one-vertex batch and the isolated-molecule shapes in a fresh child process."""
    kit.run_under_poison(__file__, "real_classes or one_vertex or isolated_inside")


def test_refusals_leave_the_context_usable(gf):
    """The GF_ERR_UNSUPPORTED answers, the GF_ERR_INVALID inputs and configurations, each followed by a call that succeeds on the same
    context"""
    from graphflow_amd import SMPNeighbourhood, _lib
    from graphflow_amd.ops import GraphFlowHipError
    gz = golden()
    for form in FORMS:
        tag = "n%d_CH4" % form
        _, L, H, D, R, M, mol, result, params = case(gz, tag)
        V = len(mol[0])
        net = net_of(form, L, H, 4, D, M, R)
        lib, ctx = net.lib, net.ctx
        h = C.c_void_p()
        p, grads, target = dev(params), torch.empty(net.n_params, device="cuda"), dev(result[2:3])

        def works():
            net.prepare([mol])
            pred, _, feat = net.forward(p, target)
            net.backward(p, grads)
            assert rel_err(pred.cpu().numpy(), result[:1]) <= TOL
            assert rel_err(feat.cpu().numpy()[0], gz[tag + "__final_feature"]) <= TOL

        works()
        assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
        works()
        assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
        works()
        masks = (C.c_uint * 8)()
        assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
        works()
        dfeat = torch.zeros_like(net.feature)
        assert lib.gf_smp_backward_features(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(grads.data_ptr()), C.c_void_p(dfeat.data_ptr()),
                                            0) == _lib.GF_ERR_UNSUPPORTED
        works()
        pk = net.pack([mol])
        ptrs = (len(pk["nV"]), pk["nV"].ctypes.data_as(C.POINTER(C.c_int)), pk["adj"].ctypes.data_as(C.POINTER(C.c_int)),
                pk["feature"].ctypes.data_as(C.POINTER(C.c_double)))
        dptr = pk["distance"].ctypes.data_as(C.POINTER(C.c_double))
        assert lib.gf_smp_prepare(net.handle, *ptrs) == _lib.GF_ERR_INVALID               # a distance handle without its distances
        works()
        assert lib.gf_smp_prepare_coulomb(net.handle, *ptrs, dptr) == _lib.GF_ERR_INVALID
        works()
        for bad in (np.nan, np.inf):                                                        # an entry that is not finite: the molecule is named
            broken = mol[2].copy()
            broken[V - 1, 0] = bad
            with pytest.raises(GraphFlowHipError, match="molecule 1 .*not finite"):
                net.prepare([mol, (mol[0], mol[1], broken)])
            works()
        with pytest.raises(GraphFlowHipError):   # a molecule above max_nVertices
            net.prepare([(np.zeros((M + 1, M + 1), dtype=np.int32), np.zeros((M + 1, 4)), np.zeros((M + 1, M + 1)))])
        works()
        plain = SMPNeighbourhood({2: "gcn_1d", 3: "gcn_2d", 6: "gcn_3d"}[form], L, H, 4, D, M, R)   # any other handle
        assert lib.gf_smp_prepare_distance(plain.handle, *ptrs, dptr) == _lib.GF_ERR_UNSUPPORTED
        plain.prepare([mol[:2]])
        plain.close()
        works()
        assert radj_code(net) == -1
        net.set_fused(False)   # (no effect: one plan)
        works()
        for bad in refused_configs(form):
            assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID
            works()
        net.close()
