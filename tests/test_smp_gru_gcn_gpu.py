"""GPU suite for GRU_GCN_1D and GRU_GCN_2D (gf_smp_create, neighbourhood = 4, 5) on the gated level of smp_level_gru.hip.  Checked
against the real classes' numbers (tests/golden/smp_gru_gcn.npz), block by block of the parameter vector (ten blocks), and at shapes
without a golden against tests/gru_gcn_ref.py, which tests/test_smp_gru_gcn.py pins to the real classes at 1e-9.  Tolerance: the suite's
1e-5 (tests/util.py: rel_err), for the graph feature, the prediction, the loss, every h_l[v] and every parameter block; no element is
excused."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import gru_gcn_ref as gref
from field_suite import TOL, blockwise, dev
from inputs import synthetic_molecule, toy_molecules
from make_gru_gcn_golden import random_params
from test_smp_gru_gcn import FORMS, WIDTHS, refused_configs
from unrestricted_cases import packing_batch
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PACK_MAXV = 12


def golden():
    return kit.load_golden("smp_gru_gcn.npz")


def net_of(form, L, H, F, D, maxV, R=1):
    from graphflow_amd import SMPGatedNeighbourhood
    return SMPGatedNeighbourhood(FORMS[form], L, H, F, D, maxV, R)


def run_net(form, mols, targets, params, L, H, D, maxV, R=1, **kw):
    """[predict, loss, graph_feature, grads (, lists) (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: net_of(form, L, H, mols[0][1].shape[1], D, maxV, R), mols, targets, params, **kw)


def radj_code(net):
    """what gf_smp_read_reduced_adjacency answers (the models have none: -1)"""
    buf = np.empty(64, dtype=np.float32)
    return net.lib.gf_smp_read_reduced_adjacency(net.handle, 0, min(1, net.cfg.nLevels), 0, buf.ctypes.data_as(C.c_void_p), buf.size)


def case(gz, tag):
    form, L, H, D, R, V = (int(x) for x in gz[tag + "__cfg"])
    return form, L, H, D, R, V, (gz[tag + "__adj"], gz[tag + "__feature"]), gz[tag + "__result"], gz[tag + "__params"]


def all_activations(net, mols, L):
    return np.concatenate([net.activation(m, l, v) for m in range(len(mols)) for l in range(L + 1) for v in range(len(mols[m][0]))])


def expected_activations(res):
    return np.concatenate([gref.activations(r) for r in res])


def check_batch(out, res, rg, H, FD, what):
    """prediction, loss, graph feature per molecule and the ten blocks of the summed gradient at TOL; returns the figures"""
    e = blockwise(out[3], rg, gref.blocks(H, FD))
    worst_feat = max(rel_err(out[2][m], res[m]["graph_feature"]) for m in range(len(res)))
    figures = (rel_err(out[0], np.array([r["predict"] for r in res])), rel_err(out[1], np.array([r["loss"] for r in res])), worst_feat, e)
    print(what, *figures)
    assert figures[0] <= TOL, what
    assert figures[1] <= TOL, what
    assert worst_feat <= TOL, what
    assert e[0] <= TOL, (what, e)
    return figures


@pytest.mark.parametrize("form", [4, 5])
def test_device_matches_the_real_classes(gf, form):
    """Every case of tests/golden/smp_gru_gcn.npz: the four toy molecules, one vertex, an isolated vertex, the disconnected graph, the
    6-cycle, the 8-star at radius 0 and beyond its diameter, the 9 / 12 / 29-vertex molecules, 0, 1 and 3 levels.  The lists N_l(v) through
    gf_smp_receptive_field everywhere, every recorded h_l[v] through gf_smp_read_activation."""
    gz = golden()
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        _, L, H, D, R, V, mol, (pred_ref, loss_ref, target), params = case(gz, tag)

        def inspect(net):
            return all_activations(net, [mol], L), net.level_sizes(L), int(net.lib.gf_smp_feature_width(net.handle)), radj_code(net)

        pred, loss, feat, grads, lists, (act, sizes, width, radj) = run_net(form, [mol], [target], params, L, H, D, V, R, want_fields=True,
                                                                         inspect=inspect)
        blocks = gref.blocks(H, mol[1].shape[1] * (D + 1))
        e = blockwise(grads, gz[tag + "__grads"], blocks)
        print(tag, rel_err(pred, [pred_ref]), rel_err(feat[0], gz[tag + "__graph_feature"]), rel_err(loss, [loss_ref]), e)
        assert len(blocks) == 10
        assert rel_err(pred, [pred_ref]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__graph_feature"]) <= TOL, tag
        assert rel_err(loss, [loss_ref]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        assert np.array_equal(gref.lists_flat(lists[0], L), gz[tag + "__lists"]) and lists[0][0] == [[v] for v in range(V)], tag
        assert sizes == (V, V, 0) and width == H and radj == -1, tag
        if tag + "__activations" in gz:
            assert rel_err(act, gz[tag + "__activations"]) <= TOL, tag


def small_batch():
    """a one-vertex molecule first and last, the four toy molecules (four feature columns) and a nine-vertex one between them: 32 vertices"""
    one = (np.zeros((1, 1), dtype=np.int32), np.array([[0.5, 0.0, 1.0, 0.25]]))
    adj9, x9, _ = synthetic_molecule(3, 9)
    mols = [one] + [(a, f) for _, a, f, _ in toy_molecules()] + [(adj9, x9[:, :4] + 0.5 * x9[:, 4:5])] + [(one[0], one[1][:, ::-1].copy())]
    return mols, np.array([0.5, 5.0, 4.0, 3.0, 6.0, 9.0, -1.0])


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("form", [4, 5])
def test_every_lane_group_width(gf, form, H):
    """H = 1, 5, 8, 9, 16, 17, 32, 33, 64 -- lane groups of 8, 16, 32 and 64 with both edges of each -- in both forms at L = 0, 1, 3 with
    max_Radius = 0 (every neighbourhood one member) and 5 (at least L), nDepth = 1: the small batch against gru_gcn_ref, every h_l[v] included.
    L = 3 is the check of the weight gradients summed over the levels."""
    mols, tg = small_batch()
    D, FD = 1, 8
    for L in (0, 1, 3):
        for R in (0, 5):
            params = random_params(form, H, FD, np.random.default_rng(100 * H + 10 * L + R), 0.5)
            out = run_net(form, mols, tg, params, L, H, D, 9, R, inspect=lambda net: all_activations(net, mols, L))
            res, rg = gref.run_batch(form, mols, tg, params, L, H, D, R)
            check_batch(out, res, rg, H, FD, (form, H, L, R))
            assert rel_err(out[4], expected_activations(res)) <= TOL, (form, H, L, R)
            assert np.abs(rg).max() > 0


def ragged_batch(reps):
    """The 70-molecule packing batch `reps` times over, a molecule of one vertex in front and behind; four feature columns.  The batch's own
    targets (0.15 .. 0.3) lie within 0.1 of what these models predict at the suite's parameter scale: dy = predict - target would lose two
    digits to cancellation and hand that loss to every gradient block, whoever evaluates it in fp32.  Targets 4 lower keep dy near 4."""
    mols, tg = packing_batch()
    mols, tg = [(a, x[:, :4] + 0.5 * x[:, 4:5]) for a, x in mols], tg - 4.0
    one = (np.zeros((1, 1), dtype=np.int32), np.array([[1.0, 0.0, 0.5, 0.0]]))
    return mols, tg, [one] + mols * reps + [one], np.concatenate([[0.25], np.tile(tg, reps), [0.75]])


@pytest.mark.parametrize("form,H,reps", [(4, 64, 4), (5, 64, 4), (4, 8, 101), (5, 8, 101)])
def test_batch_across_workgroups_and_rounds(gf, form, H, reps):
    """A vertex count that is no multiple of the slots per workgroup, several workgroups, two rounds of a slot: at H = 64 (4 slots, one
    workgroup's images per CU: 1024 vertices a round) 1,302 vertices, at H = 8 (32 slots, four workgroups per CU: 32,768 a round) 32,827.
    Molecules of one vertex go first and last.  The reference runs the 70 distinct molecules and the two single vertices once."""
    L, D, R, FD = 3, 0, 2, 4
    base, tg, mols, targets = ragged_batch(reps)
    nV = sum(len(a) for a, _ in mols)
    G = 64 if H > 32 else 8
    slots, lds = 256 // G, 4 * (6 * H * (H | 1) + 3 * (256 // G) * H)
    per_round = slots * 256 * max(1, min(4, 160 * 1024 // lds))
    assert nV % slots and -(-nV // per_round) == 2 and nV // (2 * slots) > 2
    # The parameters are drawn as the golden generator draws them: the scale is halved until a numpy float32 evaluation of the restatement
    # meets the fp64 one within half the tolerance on this batch, block by block (the summed gradient of 70 molecules cancels in places, and
    # rel_err measures a block against its largest entry).  Decided on the CPU, before the device runs.
    rng, scale = np.random.default_rng(H + reps), 0.5
    while True:
        params = random_params(form, H, FD, rng, scale)
        res, rg = gref.run_batch(form, base, tg, params, L, H, D, R)
        ends, gends = gref.run_batch(form, [mols[0], mols[-1]], targets[[0, -1]], params, L, H, D, R)
        rg32 = gref.run_batch(form, base, tg, params, L, H, D, R, dtype=np.float32)[1]
        ge32 = gref.run_batch(form, [mols[0], mols[-1]], targets[[0, -1]], params, L, H, D, R, dtype=np.float32)[1]
        e32 = blockwise(reps * rg32.astype(np.float64) + ge32, reps * rg + gends, gref.blocks(H, FD))
        if e32[0] <= 0.5 * TOL:
            break
        scale *= 0.5
        assert scale > 1e-3, e32
    print("numpy float32 on this batch:", e32, "scale", scale)
    out = run_net(form, mols, targets, params, L, H, D, PACK_MAXV, R)
    full = [ends[0]] + res * reps + [ends[1]]
    check_batch(out, full, reps * rg + gends, H, FD, (form, H, reps, nV))


@pytest.mark.parametrize("form,H", [(4, 33), (5, 17)])
def test_accumulate_adds_exactly_a_second_sweep(gf, form, H):
    """after one forward a second backward gives the bits of the first (every level keeps what a second sweep needs), and
    backward(accumulate=True) onto the first result gives twice the first result, which is exact in fp32"""
    mols, tg = small_batch()
    L, D, R = 3, 1, 2
    net = net_of(form, L, H, 4, D, 9, R)
    net.prepare(mols)
    p = dev(random_params(form, H, 8, np.random.default_rng(H), 0.5))
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


@pytest.mark.parametrize("H", [5, 64])
def test_pair_form_with_one_member_neighbourhoods(gf, H):
    """Form 5 at max_Radius = 0: every neighbourhood is the vertex itself, A Tt - a T is one rounded product minus itself, so n is exactly 0
    -- the gradients of W_z, W_r and W_h (dz'^T n, dr'^T n, dc'^T n) are then exact zeros -- and every h_l[v] is the restatement's."""
    mols, tg = small_batch()
    L, D, FD = 3, 1, 8
    params = random_params(5, H, FD, np.random.default_rng(H), 0.5)
    out = run_net(5, mols, tg, params, L, H, D, 9, 0, inspect=lambda net: all_activations(net, mols, L))
    res, rg = gref.run_batch(5, mols, tg, params, L, H, D, 0)
    assert all(not r["n"][l].any() for r in res for l in range(1, L + 1))
    check_batch(out, res, rg, H, FD, ("one member", H))
    assert rel_err(out[4], expected_activations(res)) <= TOL
    off = 0
    for name, n in gref.blocks(H, FD):
        if name in ("W_z", "W_r", "W_h"):
            assert not out[3][off:off + n].any(), name
        else:
            assert out[3][off:off + n].any(), name
        off += n


@pytest.mark.parametrize("form,H", [(4, 9), (5, 64)])
def test_two_runs_give_the_same_bits(gf, form, H):
    """prediction, loss, graph feature and gradients of two runs from scratch, bit for bit"""
    base, tg, mols, targets = ragged_batch(1)
    params = random_params(form, H, 4, np.random.default_rng(H), 0.5)
    a = run_net(form, mols, targets, params, 3, H, 0, PACK_MAXV, 2)
    b = run_net(form, mols, targets, params, 3, H, 0, PACK_MAXV, 2)
    assert np.abs(a[3]).max() > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of this level reads memory
    nobody wrote.  The golden cases, the one-member form and the bit-identity test in a fresh child process."""
    kit.run_under_poison(__file__, "real_classes or one_member or same_bits")


@pytest.mark.parametrize("form", [4, 5])
def test_momentum_steps_match_the_real_classes(gf, form):
    """Three BatchLearn steps of the real class on the four toy molecules: initial weights from gf_smp_uniform_init_host after the same
    srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    p_ = "train_n%d__" % form
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in z[p_ + "cfg"])
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    lr, gamma = float(z[p_ + "lr"][0]), float(z[p_ + "momentum"][0])
    net = net_of(form, L, H, 4, D, maxV, R)
    kit.check_momentum_trajectory(net, lambda p, g: net.step(p, g, lr, len(mols), gamma), z, p_, mols, seed, nIter, lr)
    net.close()


def test_checkpoint_round_trip(gf, tmp_path):
    """The reference's own save_model file loads to the float32 of its values; a saved file is the reference's text; the loaded model
    predicts what the golden and the restatement at the loaded values say."""
    gz = golden()
    tag = str(gz["checkpoint__tag"])
    form, L, H, D, R, V, mol, result, params = case(gz, tag)
    ref_file = tmp_path / "reference.txt"
    ref_file.write_bytes(bytes(gz["checkpoint__text"]))
    net = net_of(form, L, H, 4, D, V, R)
    loaded = net.load_model(torch.zeros(net.n_params, device="cuda"), ref_file).cpu().numpy()
    assert np.array_equal(loaded, np.array([float(t) for t in ref_file.read_text().split()], dtype=np.float32))
    net.save_model(dev(params), tmp_path / "ours.txt")
    assert (tmp_path / "ours.txt").read_text().split() == ref_file.read_text().split()
    kit.check_checkpoint_round_trip(
        net, tag, mol, params, result[2:3], result[0],
        lambda values, lists: gref.run(form, mol[0], mol[1], float(result[2]), values.astype(np.float64), L, H, D, R, nbh=lists)["predict"], tmp_path)


def test_refusals_leave_the_context_usable(gf):
    """The five GF_ERR_UNSUPPORTED answers and the GF_ERR_INVALID configurations (with their messages), each followed by a call that
    succeeds on the same context"""
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    gz = golden()
    for form in (4, 5):
        tag = "n%d_CH4" % form
        _, L, H, D, R, V, mol, result, params = case(gz, tag)
        net = net_of(form, L, H, 4, D, V, R)
        lib, ctx = net.lib, net.ctx
        h = C.c_void_p()
        p, grads, target = dev(params), torch.empty(net.n_params, device="cuda"), dev(result[2:3])

        def works():
            net.prepare([mol])
            pred, _, feat = net.forward(p, target)
            net.backward(p, grads)
            assert rel_err(pred.cpu().numpy(), result[:1]) <= TOL
            assert rel_err(feat.cpu().numpy()[0], gz[tag + "__graph_feature"]) <= TOL

        assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
        assert b"GRU_GCN_1D / GRU_GCN_2D have no `_classification` class" in lib.gf_last_error(ctx.handle)
        works()
        assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
        works()
        masks = (C.c_uint * 8)()
        assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
        works()
        with pytest.raises(GraphFlowHipError):
            net.prepare([mol], coulomb=[np.ones((V, V))])
        works()
        dfeat = torch.zeros_like(net.feature)
        assert lib.gf_smp_backward_features(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(grads.data_ptr()), C.c_void_p(dfeat.data_ptr()),
                                            0) == _lib.GF_ERR_UNSUPPORTED
        works()
        with pytest.raises(GraphFlowHipError):   # a molecule above max_nVertices
            net.prepare([(np.zeros((V + 1, V + 1), dtype=np.int32), np.zeros((V + 1, 4)))])
        works()
        assert radj_code(net) == -1
        net.set_fused(False)   # (no effect: one plan)
        works()
        for bad, text in refused_configs(form):
            assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID and not h.value
            assert text in lib.gf_last_error(ctx.handle), lib.gf_last_error(ctx.handle)
            works()
        assert lib.gf_smp_param_count(net.handle) == lib.gf_smp_config_param_count(C.byref(net.cfg)) == gref.n_params(H, 4 * (D + 1))
        net.close()
