"""GPU suite for NeuralFingerprint, GCN_1D and GCN_2D (gf_smp_create, neighbourhood = 1, 2, 3) on the level of
smp_level_neighbourhood.hip.  Checked against the real classes' numbers (tests/golden/smp_neighbourhood.npz), block by block of the
parameter vector, and at shapes without a golden against tests/neighbourhood_ref.py, which tests/test_smp_neighbourhood.py pins to the real
classes at 1e-9.  Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the final feature, the prediction, the loss and every
parameter block; no element is excused."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import neighbourhood_ref as nref
from field_suite import TOL, blockwise, dev
from inputs import toy_molecules
from make_neighbourhood_golden import random_params
from unrestricted_cases import packing_batch
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORMS = {1: "fingerprint", 2: "gcn_1d", 3: "gcn_2d"}
PACK_L, PACK_R, PACK_MAXV = 3, 2, 12   # (form 2 then walks two lists: radius 1 at level 1, 2 at levels 2 and 3)
# lane groups of 8 / 16 / 32 / 64 with both edges of the 16-lane group, two channels per lane above 64, the largest LDS image
WIDTHS = (5, 6, 8, 9, 16, 17, 31, 32, 33, 64, 65, 128)


def golden():
    return kit.load_golden("smp_neighbourhood.npz")


def net_of(form, L, H, F, D, maxV, R=1):
    from graphflow_amd import SMPNeighbourhood
    return SMPNeighbourhood(FORMS[form], L, H, F, D, maxV, R)


def run_net(form, mols, targets, params, L, H, D, maxV, R=1, **kw):
    """[predict, loss, final_feature, grads (, lists) (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: net_of(form, L, H, mols[0][1].shape[1], D, maxV, R), mols, targets, params, **kw)


def radj_code(net):
    """what gf_smp_read_reduced_adjacency answers (the models have none: -1)"""
    buf = np.empty(64, dtype=np.float32)
    return net.lib.gf_smp_read_reduced_adjacency(net.handle, 0, min(1, net.cfg.nLevels), 0, buf.ctypes.data_as(C.c_void_p), buf.size)


def case(gz, tag):
    form, L, H, D, R, V = (int(x) for x in gz[tag + "__cfg"])
    return form, L, H, D, R, V, (gz[tag + "__adj"], gz[tag + "__feature"]), gz[tag + "__result"], gz[tag + "__params"]


@pytest.mark.parametrize("form", [1, 2, 3])
def test_device_matches_the_real_classes(gf, form):
    """Every case of tests/golden/smp_neighbourhood.npz: CH4, one vertex, an isolated vertex, the 6-cycle, the 8-star (also with a radius
    beyond its diameter), the 12-vertex molecule at 0 and 3 levels, form 1's directed adjacency.  The lists N_l(v) through
    gf_smp_receptive_field everywhere, for CH4 every h_l[v] through gf_smp_read_activation."""
    gz = golden()
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        _, L, H, D, R, V, mol, (pred_ref, loss_ref, target), params = case(gz, tag)

        def inspect(net):
            act = np.concatenate([net.activation(0, l, v) for l in range(L + 1) for v in range(V)])
            return act, net.level_sizes(L), int(net.lib.gf_smp_feature_width(net.handle)), radj_code(net)

        pred, loss, feat, grads, lists, (act, sizes, width, radj) = run_net(form, [mol], [target], params, L, H, D, V, R, want_fields=True,
                                                                         inspect=inspect)
        e = blockwise(grads, gz[tag + "__grads"], nref.blocks(H, mol[1].shape[1] * (D + 1), L))
        print(tag, rel_err(pred, [pred_ref]), rel_err(feat[0], gz[tag + "__final_feature"]), rel_err(loss, [loss_ref]), e)
        assert rel_err(pred, [pred_ref]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__final_feature"]) <= TOL, tag
        assert rel_err(loss, [loss_ref]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        assert np.array_equal(nref.lists_flat(lists[0], L), gz[tag + "__lists"]) and lists[0][0] == [[v] for v in range(V)], tag
        assert sizes == (V, V, 0) and width == H and radj == -1, tag
        if tag + "__activations" in gz:
            assert rel_err(act, gz[tag + "__activations"]) <= TOL, tag


def wide_features(x, FD):
    """the packing batch's five feature columns as F' = 4 (the first four) or, for form 1, which has no depth, 15 columns"""
    return x[:, :4] if FD == 4 else np.concatenate([x, 0.5 * x, 0.25 * x], axis=1)


def pack_shape(form, FD):
    """(molecules, targets, nDepth) of the packing batch at F' = 4 or 15"""
    mols, tg = packing_batch()
    if FD == 4:
        return [(a, wide_features(x, 4)) for a, x in mols], tg, 0
    return ([(a, wide_features(x, 15)) for a, x in mols], tg, 0) if form == 1 else (mols, tg, 2)


def run_packed(form, H, FD):
    D = pack_shape(form, FD)[2]
    return lambda mols, tg, params, **kw: run_net(form, mols, tg, params, PACK_L, H, D, PACK_MAXV, PACK_R, **kw)


def packed_case(form, H, FD):
    """the packing batch on the device beside its fp64 expectation, once per (form, width, F')"""
    def batch():
        return pack_shape(form, FD)[:2]

    def reference(mols, tg, params, out):
        res, rg = nref.run_batch(form, mols, tg, params, PACK_L, H, pack_shape(form, FD)[2], PACK_R)
        assert out[4] == [r["N"] for r in res]
        return res, rg

    return kit.packed_case(("neighbourhood", form, H, FD), batch, lambda: random_params(form, H, FD, PACK_L, np.random.default_rng(H + FD), 0.5),
                           run_packed(form, H, FD), reference, want_fields=True)


@pytest.mark.parametrize("FD", [4, 15])
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("form", [1, 2, 3])
def test_batch_across_the_widths(gf, form, H, FD):
    """the 70-molecule packing batch against neighbourhood_ref, per molecule (prediction, final feature) and per block of the summed
    gradient: more vertices than a workgroup's slots, a ragged last workgroup, every lane-group width and both channel counts per lane"""
    mols, tg, params, out, (res, rg) = packed_case(form, H, FD)
    assert len(mols) == 70 and sum(len(a) for a, _ in mols) > 256 and mols[0][1].shape[1] * (pack_shape(form, FD)[2] + 1) == FD
    e = blockwise(out[3], rg, nref.blocks(H, FD, PACK_L))
    worst_feat = max(rel_err(out[2][m], res[m]["final_feature"]) for m in range(len(mols)))
    print(form, H, FD, rel_err(out[0], [r["predict"] for r in res]), worst_feat, e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert rel_err(out[1], np.array([r["loss"] for r in res])) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e


@pytest.mark.parametrize("form,H,reps", [(1, 64, 7), (3, 64, 7), (2, 20, 13)])
def test_batch_the_level_runs_in_two_rounds(gf, form, H, reps):
    """The packing batch seven (thirteen) times over: 2,275 vertices at H = 64 (4,225 at H = 20), where a workgroup of nbh_level_fwd and
    nbh_node_bwd takes two rounds of its slots and the TN products of dW1_l / dW2_l split their K (the traced launch table shows the
    fold).  The reference runs the 70 distinct (molecule, target) pairs once: every copy has its molecule's prediction, loss and final
    feature, and the batch gradient is `reps` times the 70's."""
    mols, tg, params, _, (res, rg) = packed_case(form, H, 4)
    G = 64 if H > 32 else 32
    assert sum(len(a) for a, _ in mols) * reps // ((256 // G) * 256) >= 2
    traced = {}

    def inspect(net):
        p, t, grads = dev(params), dev(np.tile(tg, reps)), torch.empty(net.n_params, device="cuda")
        traced.update(kit.traced_counts(net, lambda: (net.forward(p, t), net.backward(p, grads))))

    out = run_packed(form, H, 4)(mols * reps, np.tile(tg, reps), params, inspect=inspect)
    pick = lambda k: np.array([res[m % 70][k] for m in range(70 * reps)])   # noqa: E731
    e = blockwise(out[3], reps * rg, nref.blocks(H, 4, PACK_L))
    worst_feat = max(rel_err(out[2][m], res[m % 70]["final_feature"]) for m in range(70 * reps))
    print(form, H, reps, rel_err(out[0], pick("predict")), rel_err(out[1], pick("loss")), worst_feat, e, traced)
    assert rel_err(out[0], pick("predict")) <= TOL
    assert rel_err(out[1], pick("loss")) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e
    assert traced.get("splitk_reduce", 0) >= 1, traced


@pytest.mark.parametrize("form,H", [(3, 65), (1, 20)])
def test_accumulate_and_a_second_sweep(gf, form, H):
    """after one forward a second backward gives the bits of the first (every level keeps what a second sweep needs), and
    backward(accumulate=True) onto the first result gives twice the first result, which is exact in fp32"""
    mols, tg, D = pack_shape(form, 4)
    net = net_of(form, PACK_L, H, 4, D, PACK_MAXV, PACK_R)
    net.prepare(mols)
    p = dev(random_params(form, H, 4, PACK_L, np.random.default_rng(H), 0.5))
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


@pytest.mark.parametrize("form", [1, 3])
def test_largest_accepted_lds_image(gf, form):
    """H = 128 with F' = 185, the widest level gf_smp_create accepts (163.5 KB of LDS in nbh_level_fwd; F' = 186 is refused): the eight
    smallest molecules of the packing batch with their features spread over 185 columns, against neighbourhood_ref"""
    H, FD, L = 128, 185, 2
    rng = np.random.default_rng(185)
    spread = np.round(rng.random((5, FD)) * 4) / 16
    mols, tg = packing_batch()
    mols, tg = [(a, x @ spread) for a, x in mols[:8]], tg[:8]
    params = random_params(form, H, FD, L, rng, 0.125)
    out = run_net(form, mols, tg, params, L, H, 0, PACK_MAXV, 1)
    res, rg = nref.run_batch(form, mols, tg, params, L, H, 0, 1)
    e = blockwise(out[3], rg, nref.blocks(H, FD, L))
    worst_feat = max(rel_err(out[2][m], res[m]["final_feature"]) for m in range(len(mols)))
    print(form, rel_err(out[0], [r["predict"] for r in res]), worst_feat, e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e


@pytest.mark.parametrize("form,H", [(1, 5), (2, 33), (3, 65)])
def test_one_molecule_isolated_inside_the_batch(gf, form, H):
    """With every other target equal to its prediction only molecule 68 (the 12-vertex one) has a loss gradient: the batch gradient is
    then that molecule's single-molecule gradient, and its prediction and final feature are those it has alone."""
    kit.check_isolated(packed_case(form, H, 4), 68, run_packed(form, H, 4), nref.blocks(H, 4, PACK_L), outputs=True)


@pytest.mark.parametrize("form,H", [(1, 6), (2, 64), (3, 128)])
def test_two_runs_give_the_same_bits(gf, form, H):
    kit.check_same_bits(packed_case(form, H, 15), run_packed(form, H, 15))


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of this level reads memory
    nobody wrote.  The golden cases, the one-vertex batch and three packed shapes in a fresh child process."""
    kit.run_under_poison(__file__, "real_classes or one_vertex or isolated_inside")


@pytest.mark.parametrize("form", [1, 2, 3])
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
    """The reference's own save_model file loads to the float32 of its values; a saved file is the reference's text and reloads to the same
    bits; the loaded model predicts what the golden and the restatement at the loaded values say."""
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
        lambda values, lists: nref.run(form, mol[0], mol[1], float(result[2]), values.astype(np.float64), L, H, D, R, nbh=lists)["predict"], tmp_path)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_permutation_invariance(gf, form):
    """these models have no vertex ordering: the final feature of the 12-vertex molecule does not depend on the numbering"""
    gz = golden()
    _, L, H, D, R, V, (adj, x), _, params = case(gz, "n%d_syn12" % form)
    kit.check_permutation_invariance(
        adj, x, lambda mols, tg: run_net(form, mols, tg, params, L, H, D, V, R, want_fields=True),
        lambda a, f, lists: nref.run(form, a, f, 1.0, params.astype(np.float64), L, H, D, R, nbh=lists)["final_feature"])


@pytest.mark.parametrize("form", [1, 2, 3])
def test_kernel_table(gf, form):
    """The launches of one step are fixed: a forward kernel per level and level 0, the read-out; backward the read-out's dW, a node kernel
    per level and level 0, a gather per level, and the TN products dW1_l (L + 1) and dW2_l (L), unsplit at this batch's 325 vertices.
    Nothing else: none of the other levels' kernels."""
    mols, tg, D = pack_shape(form, 4)
    L, H = PACK_L, 20
    net = net_of(form, L, H, 4, D, PACK_MAXV, PACK_R)
    net.prepare(mols)
    p = dev(random_params(form, H, 4, L, np.random.default_rng(1), 0.5))
    grads = torch.empty(net.n_params, device="cuda")
    counts = kit.traced_counts(net, lambda: (net.forward(p, dev(tg)), net.backward(p, grads)))
    net.close()
    # (the batch has 325 vertices: below the 256 x 2 a split of the products' K takes, so no fold launch -- measured on an MI355X)
    expect = {"nbh_level_fwd": L + 1, "nbh_readout": 1, "nbh_readout_dW": 1, "nbh_node_bwd": L + 1, "nbh_gather_bwd": L, "gemm_tn": 2 * L + 1}
    print(form, counts)
    assert counts == expect, counts


@pytest.mark.parametrize("form", [1, 2, 3])
def test_batch_of_one_vertex_molecules(gf, form):
    """five molecules of one vertex: form 1's neighbourhoods are empty, form 3's hold one member (n = 0)"""
    rng = np.random.default_rng(7)
    mols = [(np.zeros((1, 1), dtype=np.int32), np.round(rng.random((1, 4)) * 8) / 8) for _ in range(5)]
    tg = np.arange(5) * 0.25
    L, H, D = 2, 6, (0 if form == 1 else 1)
    params = random_params(form, H, 4 * (D + 1), L, rng, 0.5)
    out = run_net(form, mols, tg, params, L, H, D, 3, 1)
    res, rg = nref.run_batch(form, mols, tg, params, L, H, D, 1)
    e = blockwise(out[3], rg, nref.blocks(H, 4 * (D + 1), L))
    print(form, rel_err(out[0], [r["predict"] for r in res]), e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert max(rel_err(out[2][m], res[m]["final_feature"]) for m in range(5)) <= TOL
    assert e[0] <= TOL, e
    if form != 2:   # (W2_l sees n = 0 everywhere: its gradient is exactly zero)
        off = 0
        for name, n in nref.blocks(H, 4 * (D + 1), L):
            assert name[:2] != "W2" or not out[3][off:off + n].any(), name
            off += n


def test_refusals_leave_the_context_usable(gf):
    """The GF_ERR_UNSUPPORTED answers and the GF_ERR_INVALID configurations, each followed by a call that succeeds on the same context"""
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    from test_smp_neighbourhood import refused_configs
    gz = golden()
    for form in (1, 2, 3):
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
            assert rel_err(feat.cpu().numpy()[0], gz[tag + "__final_feature"]) <= TOL

        assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
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
        for bad in refused_configs(form):
            assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID
            works()
        net.close()
