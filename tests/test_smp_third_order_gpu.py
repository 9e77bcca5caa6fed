"""GPU suite for GCN_3D and GRU_GCN_3D (gf_smp_create, neighbourhood = 6, 7): the softmax and the gated neighbourhood level with the
third-order pool of smp_level_third.hip as their aggregate.  Checked against the real classes' numbers (tests/golden/smp_third_order.npz),
block by block of the parameter vector (W1_l / W2_l per level and W in form 6, the ten blocks in form 7), and at shapes without a golden
against tests/third_order_ref.py, which tests/test_smp_third_order.py pins to the real classes at 1e-9.  Every input satisfies the gap
condition (checked on the CPU by that file, which builds the inputs).  Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the
graph feature, the prediction, the loss, every h_l[v] and every parameter block; no element and no case is excused."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import third_order_ref as tref
from field_suite import TOL, blockwise, dev
from inputs import toy_molecules
from test_smp_third_order import FORMS, WIDTHS, model_case, refused_configs
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def golden():
    return kit.load_golden("smp_third_order.npz")


def net_of(form, L, H, F, D, maxV, R=1):
    from graphflow_amd import SMPGatedNeighbourhood, SMPNeighbourhood
    return (SMPNeighbourhood if form == 6 else SMPGatedNeighbourhood)(FORMS[form], L, H, F, D, maxV, R)


def run_net(form, mols, targets, params, L, H, D, maxV, R=1, **kw):
    """[predict, loss, graph_feature, grads (, lists) (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: net_of(form, L, H, mols[0][1].shape[1], D, maxV, R), mols, targets, params, **kw)


def radj_code(net):
    buf = np.empty(64, dtype=np.float32)
    return net.lib.gf_smp_read_reduced_adjacency(net.handle, 0, min(1, net.cfg.nLevels), 0, buf.ctypes.data_as(C.c_void_p), buf.size)


def case(gz, tag):
    form, L, H, D, R, V = (int(x) for x in gz[tag + "__cfg"])
    return form, L, H, D, R, V, (gz[tag + "__adj"], gz[tag + "__feature"]), gz[tag + "__result"], gz[tag + "__params"]


def all_activations(net, mols, L):
    return np.concatenate([net.activation(m, l, v) for m in range(len(mols)) for l in range(L + 1) for v in range(len(mols[m][0]))])


def check_batch(out, res, rg, blocks, what):
    """prediction, loss, graph feature per molecule and every block of the summed gradient at TOL; returns the figures"""
    e = blockwise(out[3], rg, blocks)
    worst_feat = max(rel_err(out[2][m], res[m]["graph_feature"]) for m in range(len(res)))
    figures = (rel_err(out[0], np.array([r["predict"] for r in res])), rel_err(out[1], np.array([r["loss"] for r in res])), worst_feat, e)
    print(what, *figures)
    assert figures[0] <= TOL, what
    assert figures[1] <= TOL, what
    assert worst_feat <= TOL, what
    assert e[0] <= TOL, (what, e)
    return figures


@pytest.mark.parametrize("form", [6, 7])
def test_device_matches_the_real_classes(gf, form):
    """Every case of tests/golden/smp_third_order.npz: the four toy molecules, one vertex, an isolated vertex, the disconnected graph, the
    6-cycle, the 8-star at radius 0 and beyond its diameter, the 9 / 12 / 29-vertex molecules, 0, 1 and 3 levels.  The lists N_l(v) through
    gf_smp_receptive_field everywhere, every recorded h_l[v] through gf_smp_read_activation."""
    gz = golden()
    worst = (0.0, "")
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        _, L, H, D, R, V, mol, (pred_ref, loss_ref, target), params = case(gz, tag)

        def inspect(net):
            return all_activations(net, [mol], L), net.level_sizes(L), int(net.lib.gf_smp_feature_width(net.handle)), radj_code(net)

        pred, loss, feat, grads, lists, (act, sizes, width, radj) = run_net(form, [mol], [target], params, L, H, D, V, R, want_fields=True,
                                                                         inspect=inspect)
        blocks = tref.blocks(form, H, mol[1].shape[1] * (D + 1), L)
        e = blockwise(grads, gz[tag + "__grads"], blocks)
        print(tag, rel_err(pred, [pred_ref]), rel_err(feat[0], gz[tag + "__graph_feature"]), rel_err(loss, [loss_ref]), e)
        worst = max(worst, (e[0], tag + " " + e[1]))
        assert len(blocks) == (2 * L + 2 if form == 6 else 10)
        assert rel_err(pred, [pred_ref]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__graph_feature"]) <= TOL, tag
        assert rel_err(loss, [loss_ref]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        assert np.array_equal(tref.lists_flat(lists[0], L), gz[tag + "__lists"]) and lists[0][0] == [[v] for v in range(V)], tag
        assert sizes == (V, V, 0) and width == H and radj == -1, tag
        if tag + "__activations" in gz:
            assert rel_err(act, gz[tag + "__activations"]) <= TOL, tag
    print("form %d: worst block against the real classes" % form, worst)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("form", [6, 7])
def test_every_lane_group_width(gf, form, H):
    """H = 1, 5, 8, 9, 16, 17, 32, 33, 64 in both forms at L = 0, 1, 3 with max_Radius = 0 (every neighbourhood one member: n = 0 exactly)
    and 5 (at least L), nDepth = 1: the small batch (one-vertex molecules first and last) against the restatement, every h_l[v] included."""
    FD = 8
    for L in (0, 1, 3):
        for R in (0, 5):
            mols, tg, params, res, rg, gap = model_case(form, H, L, R)
            out = run_net(form, mols, tg, params, L, H, 1, 9, R, inspect=lambda net: all_activations(net, mols, L))
            check_batch(out, res, rg, tref.blocks(form, H, FD, L), (form, H, L, R, gap))
            assert rel_err(out[4], np.concatenate([tref.activations(r) for r in res])) <= TOL, (form, H, L, R)
            if R == 0 and L:   # n = 0 exactly: the blocks that multiply n are exact zeros, and so is whatever the restatement has at zero
                off = 0        # (form 6: nothing flows below the top level, so only W1_L and W have a gradient)
                for name, n in tref.blocks(form, H, FD, L):
                    if name.startswith("W2") or name in ("W_z", "W_r", "W_h"):
                        assert not out[3][off:off + n].any() and not rg[off:off + n].any(), name
                    assert bool(out[3][off:off + n].any()) == bool(rg[off:off + n].any()), name
                    off += n


@pytest.mark.parametrize("form,H", [(6, 33), (7, 17)])
def test_accumulate_adds_a_sweep_to_the_callers_values(gf, form, H):
    """after one forward a second backward gives the bits of the first (every level keeps what a second sweep needs), and
    backward(accumulate=True) onto the first result gives twice the first result, which is exact in fp32"""
    mols, tg, params, res, rg, gap = model_case(form, H, 3, 2)
    net = net_of(form, 3, H, 4, 1, 9, 2)
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
    assert blockwise(a.astype(np.float64), rg, tref.blocks(form, H, 8, 3))[0] <= TOL
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(c, 2 * a)


@pytest.mark.parametrize("form,H", [(6, 9), (7, 64)])
def test_two_runs_give_the_same_bits(gf, form, H):
    """prediction, loss, graph feature and gradients of two runs from scratch, bit for bit"""
    mols, tg, params, res, rg, gap = model_case(form, H, 3, 2)
    a = run_net(form, mols, tg, params, 3, H, 1, 9, 2)
    b = run_net(form, mols, tg, params, 3, H, 1, 9, 2)
    assert np.abs(a[3]).max() > 0
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of the level reads memory
    nobody wrote.  Forward and backward of the golden cases and the bit-identity test in a fresh child process."""
    kit.run_under_poison(__file__, "real_classes or same_bits")


@pytest.mark.parametrize("form", [6, 7])
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
        lambda values, lists: tref.run(form, mol[0], mol[1], float(result[2]), values.astype(np.float64), L, H, D, R, nbh=lists)["predict"], tmp_path)


def test_refusals_leave_the_context_usable(gf):
    """The five GF_ERR_UNSUPPORTED answers and the GF_ERR_INVALID configurations (with their messages), each followed by a call that
    succeeds on the same context"""
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    gz = golden()
    for form in (6, 7):
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
        assert b"GCN_3D / GRU_GCN_3D have no `_classification` class" in lib.gf_last_error(ctx.handle)
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
        assert lib.gf_smp_param_count(net.handle) == lib.gf_smp_config_param_count(C.byref(net.cfg)) == tref.n_params(form, H, 4 * (D + 1), L)
        net.close()
