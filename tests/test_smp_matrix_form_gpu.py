"""GPU suite for LCNN and GCN_MW (gf_smp_create, matrix_form = 1, 2) on the row-list GEMM level (smp_level_rowlist.hip).  Checked against
the real classes' numbers (tests/golden/smp_matrix_form.npz), block by block of the parameter vector, and for batches against
tests/matrix_form_ref.py, which tests/test_smp_matrix_form.py pins to the real classes at 1e-9.  No pre-activation of a fixture lies
within 1e-3 max|z| of the kink of LeakyReLU.  Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the graph feature, the
prediction, the loss, every recorded activation and every parameter block; no element and no case is excused."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import matrix_form_ref as mref
from field_suite import TOL, blockwise, dev
from inputs import f32exact, toy_molecules
from test_smp_matrix_form import activations, case, refused_configs, tags
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def golden():
    return kit.load_golden("smp_matrix_form.npz")


def net_of(kind, cfg, F, maxV=None):
    from graphflow_amd import GCNMW, LCNN
    if kind == "lcnn":
        V, k, D, C1, C2, nD = cfg
        return LCNN(V, F, k, D, C1, C2, nD)
    L, H, D = cfg
    return GCNMW(L, maxV, F, H, D)


def rows_of(kind, cfg, mol):
    return cfg[0] if kind == "lcnn" else len(mol[0])


def read_structure(kind, cfg, net, m, mol):
    """order and sequence (LCNN) through gf_smp_receptive_field, or the non-zero pattern of A-hat (GCN_MW)"""
    n = rows_of(kind, cfg, mol)
    if kind == "lcnn":
        return np.array([net.receptive_field(m, 0, i)[0] for i in range(n)] + [u for i in range(n) for u in net.receptive_field(m, 1, i)])
    return [net.receptive_field(m, l, v) for l in range(cfg[0] + 1) for v in range(n)]


def read_activations(kind, cfg, net, m, mol):
    n = rows_of(kind, cfg, mol)
    levels = (1, 2) if kind == "lcnn" else range(cfg[0] + 1)
    return np.concatenate([net.activation(m, l, v) for l in levels for v in range(n)])


def run_net(kind, cfg, mols, targets, params, maxV=None, **kw):
    """[predict, loss, graph_feature, grads (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: net_of(kind, cfg, mols[0][1].shape[1], maxV or max(len(a) for a, _ in mols)), mols, targets, params, **kw)


@pytest.mark.parametrize("tag", tags())
def test_device_matches_the_real_class(gf, tag):
    """Every case of tests/golden/smp_matrix_form.npz: feature, prediction, loss, the gradient block by block, order / sequence / the
    pattern of A-hat through gf_smp_receptive_field, every recorded activation through gf_smp_read_activation"""
    gz = golden()
    kind, cfg, adj, feat, (pred_ref, loss_ref, target), params = case(tag)
    mol = (adj, feat)
    n = rows_of(kind, cfg, mol)

    def inspect(net):
        return (read_structure(kind, cfg, net, 0, mol), read_activations(kind, cfg, net, 0, mol), net.level_sizes(cfg[0] if kind == "gcn_mw" else 2),
                int(net.lib.gf_smp_feature_width(net.handle)))

    pred, loss, feature, grads, (struct, act, sizes, width) = run_net(kind, cfg, [mol], [target], params, inspect=inspect)
    e = blockwise(grads, gz[tag + "__grads"], mref.blocks(kind, cfg, feat.shape[1]))
    print(tag, rel_err(pred, [pred_ref]), rel_err(feature[0], gz[tag + "__graph_feature"]), rel_err(loss, [loss_ref]), e)
    assert rel_err(pred, [pred_ref]) <= TOL
    assert rel_err(feature[0], gz[tag + "__graph_feature"]) <= TOL
    assert rel_err(loss, [loss_ref]) <= TOL
    assert e[0] <= TOL, e
    assert sizes == (n, n, 0) and width == gz[tag + "__graph_feature"].size
    if kind == "lcnn":
        assert np.array_equal(struct, gz[tag + "__structure"].astype(np.int64))
    else:
        ah = gz[tag + "__structure"].reshape(n, n)
        assert struct == [list(np.flatnonzero(ah[v])) for _ in range(cfg[0] + 1) for v in range(n)]
    if tag + "__activations" in gz:
        assert rel_err(act, gz[tag + "__activations"]) <= TOL


def batch_of(kind, count):
    """`count` molecules cycling over the class's four demo fixtures, which share their parameters: (cfg, mols, targets, params, the
    per-molecule golden tags)"""
    demo = tags(kind)[:4]
    picked = [demo[i % 4] for i in range(count)]
    cs = [case(t) for t in picked]
    assert all(np.array_equal(c[5], cs[0][5]) and c[1] == cs[0][1] for c in cs)
    return cs[0][1], [(c[2], c[3]) for c in cs], np.array([c[4][2] + 0.125 * i for i, c in enumerate(cs)]), cs[0][5], picked


@pytest.mark.parametrize("kind", ["lcnn", "gcn_mw"])
def test_batch_beyond_one_row_tile(gf, kind):
    """23 molecules (LCNN: 23 x 6 = 138 rows, more than one 128-row tile and no multiple of it; GCN_MW: 104 vertices, with a second batch
    of 61 molecules = 275): features are the goldens', predictions and the summed gradient the restatement's at the shifted targets,
    every activation of the first, the last and a middle molecule"""
    gz = golden()
    for count in (23, 61):
        cfg, mols, tg, params, picked = batch_of(kind, count)
        res = [mref.run(kind, cfg, a, f, t, params) for (a, f), t in zip(mols, tg)]
        rg = sum(r["grads"] for r in res)
        look = (0, count // 2, count - 1)
        out = run_net(kind, cfg, mols, tg, params, maxV=6,
                      inspect=lambda net: [read_activations(kind, cfg, net, m, mols[m]) for m in look])
        e = blockwise(out[3], rg, mref.blocks(kind, cfg, 4))
        feat_err = max(rel_err(out[2][m], gz[picked[m] + "__graph_feature"]) for m in range(count))
        print(kind, count, rel_err(out[0], np.array([r["predict"] for r in res])), feat_err, e)
        assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
        assert rel_err(out[1], np.array([r["loss"] for r in res])) <= TOL
        assert feat_err <= TOL
        assert e[0] <= TOL, e
        for m, act in zip(look, out[4]):
            assert rel_err(act, activations(kind, res[m])) <= TOL, m


@pytest.mark.parametrize("kind", ["lcnn", "gcn_mw"])
def test_isolated_sample_and_same_bits(gf, kind):
    """with every other target equal to its prediction the batch gradient is one sample's own; a second run gives the bits of the first"""
    cfg, mols, tg, params, _ = batch_of(kind, 23)
    run = lambda ms, t, p: run_net(kind, cfg, ms, t, p, maxV=6)   # noqa: E731
    first = run(mols, tg, params)
    assert np.abs(first[3]).max() > 0
    kit.check_same_bits((mols, tg, params, first), run)
    kit.check_isolated((mols, tg, params, first), 22, run, mref.blocks(kind, cfg, 4), outputs=True)


@pytest.mark.parametrize("tag", ["lcnn_syn12", "gcn_mw_disconnected"])
def test_accumulate_adds_a_sweep_to_the_callers_values(gf, tag):
    """after one forward a second backward gives the bits of the first (nothing a second sweep needs is overwritten), and
    backward(accumulate=True) onto the first result gives twice the first result, which is exact in fp32"""
    gz = golden()
    kind, cfg, adj, feat, result, params = case(tag)
    net = net_of(kind, cfg, feat.shape[1], len(adj))
    net.prepare([(adj, feat)])
    p = dev(params)
    net.forward(p, dev(result[2:3]))
    first, again = torch.full((net.n_params,), float("nan"), device="cuda"), torch.full((net.n_params,), float("nan"), device="cuda")
    net.backward(p, first)
    net.backward(p, again)
    twice = first.clone()
    net.backward(p, twice, accumulate=True)
    net.close()
    a, b, c = (t.cpu().numpy() for t in (first, again, twice))
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert blockwise(a.astype(np.float64), gz[tag + "__grads"], mref.blocks(kind, cfg, feat.shape[1]))[0] <= TOL
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(c, 2 * a)


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of the level reads memory
    nobody wrote.  The golden cases and the batches in a fresh child process."""
    kit.run_under_poison(__file__, "real_class or beyond_one_row_tile")


@pytest.mark.parametrize("kind", ["lcnn", "gcn_mw"])
def test_momentum_steps_match_the_real_classes(gf, kind):
    """Three BatchLearn steps of the real class on the four toy molecules: initial weights from gf_smp_uniform_init_host after the same
    srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    p_ = "train_%s__" % kind
    cfg = tuple(int(x) for x in z[p_ + "cfg"])
    seed, nIter, maxV = (int(x) for x in z[p_ + "seed"])
    mols = [(adj, f32exact(feat)) for _, adj, feat, _ in toy_molecules()]
    lr, gamma = float(z[p_ + "lr"][0]), float(z[p_ + "momentum"][0])
    net = net_of(kind, cfg, 4, maxV)
    kit.check_momentum_trajectory(net, lambda p, g: net.step(p, g, lr, len(mols), gamma), z, p_, mols, seed, nIter, lr)
    net.close()


def test_checkpoint_round_trip(gf, tmp_path):
    """The reference's own save_model file loads to the float32 of its values; a saved file is the reference's text; the loaded model
    predicts what the golden and the restatement at the loaded values say."""
    gz = golden()
    tag = str(gz["checkpoint__tag"])
    kind, cfg, adj, feat, result, params = case(tag)
    ref_file = tmp_path / "reference.txt"
    ref_file.write_bytes(bytes(gz["checkpoint__text"]))
    net = net_of(kind, cfg, 4, len(adj))
    loaded = net.load_model(torch.zeros(net.n_params, device="cuda"), ref_file).cpu().numpy()
    assert np.array_equal(loaded, np.array([float(t) for t in ref_file.read_text().split()], dtype=np.float32))
    net.save_model(dev(params), tmp_path / "ours.txt")
    assert (tmp_path / "ours.txt").read_text().split() == ref_file.read_text().split()
    kit.check_checkpoint_round_trip(
        net, tag, (adj, feat), params, result[2:3], result[0],
        lambda values, lists: mref.run(kind, cfg, adj, feat, float(result[2]), values.astype(np.float64))["predict"], tmp_path)


def test_refusals_leave_the_context_usable(gf):
    """The GF_ERR_UNSUPPORTED answers, the molV == V refusal of gf_smp_prepare and the GF_ERR_INVALID configurations (with their
    messages), each followed by a call that succeeds on the same context"""
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    from make_gru_gcn_golden import disconnected_molecule
    gz = golden()
    for tag in ("lcnn_CH4", "gcn_mw_CH4"):
        kind, cfg, adj, feat, result, params = case(tag)
        mol, V = (adj, feat), 6
        net = net_of(kind, cfg, 4, V)
        lib, ctx = net.lib, net.ctx
        h = C.c_void_p()
        p, grads, target = dev(params), torch.empty(net.n_params, device="cuda"), dev(result[2:3])

        def works():
            net.prepare([mol])
            pred, _, feature = net.forward(p, target)
            net.backward(p, grads)
            assert rel_err(pred.cpu().numpy(), result[:1]) <= TOL
            assert rel_err(feature.cpu().numpy()[0], gz[tag + "__graph_feature"]) <= TOL

        assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
        assert b"LCNN / GCN_MW have no `_classification` class" in lib.gf_last_error(ctx.handle)
        works()
        assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
        assert b"matrix-form handle" in lib.gf_last_error(ctx.handle)
        assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
        works()
        masks = (C.c_uint * 8)()
        assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
        assert b"matrix-form handle" in lib.gf_last_error(ctx.handle)
        works()
        with pytest.raises(GraphFlowHipError, match="no Coulomb adjacency"):
            net.prepare([mol], coulomb=[np.ones((len(adj), len(adj)))])
        works()
        dfeat = torch.zeros_like(net.feature)
        assert lib.gf_smp_backward_features(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(grads.data_ptr()), C.c_void_p(dfeat.data_ptr()),
                                            0) == _lib.GF_ERR_UNSUPPORTED
        assert b"is no tower" in lib.gf_last_error(ctx.handle)
        works()
        with pytest.raises(GraphFlowHipError, match="max_nVertices = 6"):   # a molecule above max_nVertices
            net.prepare([(np.zeros((V + 1, V + 1), dtype=np.int32), np.zeros((V + 1, 4)))])
        works()
        if kind == "lcnn":   # a full-size molecule whose fragments hold three vertices each, second in its batch: k = 5 pads with row 6
            dadj, dfeat6, _ = disconnected_molecule()
            with pytest.raises(GraphFlowHipError, match="molecule 1 has max_nVertices = 6 vertices .* past its matrix"):
                net.prepare([mol, (dadj, dfeat6)])
            with pytest.raises(GraphFlowHipError, match="before gf_smp_prepare"):
                net.forward(p, target)
            works()
        buf = np.empty(64, dtype=np.float32)
        assert lib.gf_smp_read_reduced_adjacency(net.handle, 0, 1, 0, buf.ctypes.data_as(C.c_void_p), buf.size) == -1
        net.set_fused(False)   # (no effect: one plan)
        works()
        for bad, text in refused_configs():
            assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID and not h.value
            assert text in lib.gf_last_error(ctx.handle), lib.gf_last_error(ctx.handle)
        works()
        assert lib.gf_smp_param_count(net.handle) == lib.gf_smp_config_param_count(C.byref(net.cfg)) == params.size
        net.close()
