"""GPU suite for CGCN_1D and CGCN_2D (gf_smp_create, covariant = 1, 2) on the whole-network covariant vertex level
(smp_level_covariant.hip), through the Python classes CGCN1D and CGCN2D.  Checked against the real classes' numbers
(tests/golden/smp_cgcn.npz), block by block of the parameter vector, and for batches against tests/cgcn_ref.py, which
tests/test_smp_cgcn.py pins to the real classes at 1e-12.  Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the graph feature,
the prediction, the loss, every recorded activation and every parameter block; no element and no case is excused."""
import ctypes as C

import numpy as np
import pytest

import cgcn_ref as cref
import field_suite as kit
from field_suite import TOL, blockwise, dev
from inputs import f32exact, toy_molecules
from test_smp_cgcn import case, refused_configs, tags
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def golden():
    return kit.load_golden("smp_cgcn.npz")


def net_of(form, L, M, F, D):
    from graphflow_amd import CGCN1D, CGCN2D
    return (CGCN1D if form == 1 else CGCN2D)(L, M, F, D)


def run_net(cfg, mols, targets, params, **kw):
    """[predict, loss, graph_feature, grads (, inspect(net))] as float64 arrays"""
    form, L, M, D = cfg
    return kit.run_net(lambda: net_of(form, L, M, mols[0][1].shape[1], D), mols, targets, params, **kw)


@pytest.mark.parametrize("tag", tags())
def test_device_matches_the_real_class(gf, tag):
    """Every case of tests/golden/smp_cgcn.npz: feature, prediction, loss, the gradient block by block, the masks of every level through
    gf_smp_receptive_field, every h_l[v] through gf_smp_read_activation (against the record where there is one, else the restatement)"""
    gz = golden()
    cfg, adj, feat, (pred_ref, loss_ref, target), params = case(tag)
    form, L, M, D = cfg
    V = len(adj)

    def inspect(net):
        return ([[net.receptive_field(0, l, v) for v in range(V)] for l in range(L + 1)],
                np.array([[net.activation(0, l, v) for v in range(V)] for l in range(L + 1)]), net.level_sizes(L),
                int(net.lib.gf_smp_feature_width(net.handle)))

    pred, loss, feature, grads, (fields, act, sizes, width) = run_net(cfg, [(adj, feat)], [target], params, inspect=inspect)
    e = blockwise(grads, gz[tag + "__grads"], cref.blocks(feat.shape[1] * (D + 1), L, M))
    ref_act = gz[tag + "__activations"] if tag + "__activations" in gz else cref.run(form, adj, feat, target, params, L, M, D)["h"]
    print(tag, rel_err(pred, [pred_ref]), rel_err(feature[0], gz[tag + "__feature_out"]), rel_err(loss, [loss_ref]), e, rel_err(act, ref_act))
    assert rel_err(pred, [pred_ref]) <= TOL
    assert rel_err(feature[0], gz[tag + "__feature_out"]) <= TOL
    assert rel_err(loss, [loss_ref]) <= TOL
    assert e[0] <= TOL, e
    assert rel_err(act, ref_act) <= TOL
    assert sizes == (V, V, 0) and width == M
    assert fields == [[list(np.flatnonzero(gz[tag + "__masks"][l][v])) for v in range(V)] for l in range(L + 1)]


def packed(form):
    """(mols, targets, params, out, ref) of the packing batch: the 12-vertex molecule, the four toy molecules, the molecule with an isolated
    vertex and the 12-vertex one again, at the 12-vertex case's configuration (L = 3, M = 16) and parameters"""
    from make_neighbourhood_golden import isolated_molecule
    cfg, adj, feat, result, params = case("c%d_syn12" % form)

    def batch():
        iso = isolated_molecule()
        mols = [(adj, feat)] + [(a, f32exact(f)) for _, a, f, _ in toy_molecules()] + [(iso[0], f32exact(iso[1])), (adj, feat)]
        return mols, np.array([result[2] + 0.25 * i for i in range(len(mols))])

    def reference(mols, tg, p, out):
        return [cref.run(form, a, f, t, p, *cfg[1:]) for (a, f), t in zip(mols, tg)]

    return cfg, kit.packed_case("cgcn%d" % form, batch, lambda: params, lambda m, t, p: run_net(cfg, m, t, p), reference)


@pytest.mark.parametrize("form", [1, 2])
def test_packed_batch(gf, form):
    """seven molecules of 3 to 12 vertices in one launch: predictions, losses, features and the summed gradient are the restatement's"""
    cfg, (mols, tg, params, out, ref) = packed(form)
    e = blockwise(out[3], sum(r["grads"] for r in ref), cref.blocks(4 * (cfg[3] + 1), cfg[1], cfg[2]))
    print(form, rel_err(out[0], [r["predict"] for r in ref]), rel_err(out[2], [r["feature"] for r in ref]), e)
    assert rel_err(out[0], [r["predict"] for r in ref]) <= TOL
    assert rel_err(out[1], [r["loss"] for r in ref]) <= TOL
    assert rel_err(out[2], [r["feature"] for r in ref]) <= TOL
    assert e[0] <= TOL, e
    assert rel_err(out[0][[0]], out[0][[6]]) == 0   # (the same molecule twice)


@pytest.mark.parametrize("form", [1, 2])
def test_isolated_sample_and_same_bits(gf, form):
    """with every other target equal to its prediction the batch gradient is one sample's own; a second run gives the bits of the first"""
    cfg, c = packed(form)
    run = lambda ms, t, p: run_net(cfg, ms, t, p)   # noqa: E731
    kit.check_same_bits(c, run)
    kit.check_isolated(c, 6, run, cref.blocks(4 * (cfg[3] + 1), cfg[1], cfg[2]), outputs=True)


@pytest.mark.parametrize("form", [1, 2])
def test_accumulate_adds_a_sweep_to_the_callers_values(gf, form):
    """after one forward a second backward gives the bits of the first (nothing a second sweep needs is overwritten), and
    backward(accumulate=True) onto the first result gives twice the first result, which is exact in fp32"""
    gz = golden()
    tag = "c%d_syn12" % form
    (_, L, M, D), adj, feat, result, params = case(tag)
    net = net_of(form, L, M, feat.shape[1], D)
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
    assert blockwise(a.astype(np.float64), gz[tag + "__grads"], cref.blocks(feat.shape[1] * (D + 1), L, M))[0] <= TOL
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(c, 2 * a)


@pytest.mark.parametrize("form", [1, 2])
def test_relabelling_needs_the_matching_permutation_of_F(gf, form):
    """The models are covariant, not invariant: under a relabelling of the vertices the prediction is unchanged only together with the same
    permutation of the rows and columns of every F_l; with F_l left alone it moves.  Both halves, in the restatement first."""
    cfg, adj, feat, result, params = case("c%d_syn12" % form)
    _, L, M, D = cfg
    V, FD = len(adj), feat.shape[1] * (D + 1)
    perm = np.random.default_rng(0).permutation(V)
    ext = np.concatenate([perm, np.arange(V, M)])
    padj, pfeat = adj[np.ix_(perm, perm)], feat[perm]
    moved = params.copy()
    for l in range(L):
        F = params[FD + l * M * M:FD + (l + 1) * M * M].reshape(M, M)
        moved[FD + l * M * M:FD + (l + 1) * M * M] = F[np.ix_(ext, ext)].ravel()
    r0 = cref.run(form, adj, feat, result[2], params, L, M, D)["predict"]
    r_with = cref.run(form, padj, pfeat, result[2], moved, L, M, D)["predict"]
    r_without = cref.run(form, padj, pfeat, result[2], params, L, M, D)["predict"]
    assert abs(r_with - r0) <= 1e-12 * max(1.0, abs(r0)) and abs(r_without - r0) > 1e-3 * max(1.0, abs(r0))
    d0 = run_net(cfg, [(adj, feat)], result[2:3], params)[0][0]
    d_with = run_net(cfg, [(padj, pfeat)], result[2:3], moved)[0][0]
    d_without = run_net(cfg, [(padj, pfeat)], result[2:3], params)[0][0]
    print(form, r0, r_with, r_without, d0, d_with, d_without)
    assert rel_err([d_with], [d0]) <= TOL and rel_err([d0], [r0]) <= TOL
    assert rel_err([d_without], [r_without]) <= TOL and abs(d_without - d0) > 1e-3 * max(1.0, abs(r0))


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of the level reads memory
    nobody wrote.  The golden cases and the packed batch in a fresh child process."""
    kit.run_under_poison(__file__, "real_class or packed_batch")


@pytest.mark.parametrize("form", [1, 2])
def test_momentum_steps_match_the_real_classes(gf, form):
    """Three BatchLearn steps of the real class on the four toy molecules: initial weights from gf_smp_uniform_init_host after the same
    srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    p_ = "train_c%d__" % form
    _, L, M, D, seed, n_iter = (int(x) for x in z[p_ + "cfg"])
    mols = [(adj, f32exact(feat)) for _, adj, feat, _ in toy_molecules()]
    lr, gamma = float(z[p_ + "lr"][0]), float(z[p_ + "momentum"][0])
    net = net_of(form, L, M, 4, D)
    kit.check_momentum_trajectory(net, lambda p, g: net.step(p, g, lr, len(mols), gamma), z, p_, mols, seed, n_iter, lr)
    net.close()


@pytest.mark.parametrize("form", [1, 2])
def test_checkpoint_round_trip(gf, form, tmp_path):
    """The class's own save_model file loads to the float32 of its values; a saved file holds the class's values in the class's order; the
    loaded model predicts what the golden and the restatement at the loaded values say."""
    gz = golden()
    tag = str(gz["checkpoint_c%d__tag" % form])
    (_, L, M, D), adj, feat, result, params = case(tag)
    ref_file = tmp_path / "reference.txt"
    ref_file.write_bytes(bytes(gz["checkpoint_c%d__text" % form]))
    net = net_of(form, L, M, 4, D)
    loaded = net.load_model(torch.zeros(net.n_params, device="cuda"), ref_file).cpu().numpy()
    assert np.array_equal(loaded, np.array([float(t) for t in ref_file.read_text().split()], dtype=np.float32))
    net.save_model(dev(params), tmp_path / "ours.txt")
    assert (tmp_path / "ours.txt").read_text().split() == ref_file.read_text().split()
    kit.check_checkpoint_round_trip(
        net, tag, (adj, feat), params, result[2:3], result[0],
        lambda values, fields: cref.run(form, adj, feat, float(result[2]), values.astype(np.float64), L, M, D)["predict"], tmp_path)


def test_refusals_leave_the_context_usable(gf):
    """The GF_ERR_UNSUPPORTED answers, the molecule above max_nVertices and the GF_ERR_INVALID configurations (with their messages), each
    followed by a call that succeeds on the same context"""
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    gz = golden()
    IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)
    for tag in ("c1_toy_CH4", "c2_toy_CH4"):
        (form, L, M, D), adj, feat, result, params = case(tag)
        mol = (adj, feat)
        net = net_of(form, L, M, 4, D)
        lib, ctx = net.lib, net.ctx
        h = C.c_void_p()
        p, grads, target = dev(params), torch.empty(net.n_params, device="cuda"), dev(result[2:3])

        def works():
            net.prepare([mol])
            pred, _, feature = net.forward(p, target)
            net.backward(p, grads)
            assert rel_err(pred.cpu().numpy(), result[:1]) <= TOL
            assert rel_err(feature.cpu().numpy()[0], gz[tag + "__feature_out"]) <= TOL

        assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
        assert b"CGCN_1D / CGCN_2D have no `_classification` class" in lib.gf_last_error(ctx.handle)
        works()
        assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
        assert b"covariant handle" in lib.gf_last_error(ctx.handle)
        assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
        works()
        masks = (C.c_uint * 8)()
        assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
        assert b"covariant handle" in lib.gf_last_error(ctx.handle)
        works()
        with pytest.raises(GraphFlowHipError, match="no Coulomb adjacency"):
            net.prepare([mol], coulomb=[np.ones((len(adj), len(adj)))])
        works()
        dfeat = torch.zeros_like(net.feature)
        assert lib.gf_smp_backward_features(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(grads.data_ptr()), C.c_void_p(dfeat.data_ptr()),
                                            0) == _lib.GF_ERR_UNSUPPORTED
        assert b"is no tower" in lib.gf_last_error(ctx.handle)
        works()
        nV = np.array([len(adj)], dtype=np.int32)
        a32, f64_ = np.ascontiguousarray(adj, dtype=np.int32), np.ascontiguousarray(feat, dtype=np.float64)
        assert lib.gf_smp_prepare_distance(net.handle, 1, nV.ctypes.data_as(IP), a32.ctypes.data_as(IP), f64_.ctypes.data_as(DP),
                                           np.zeros(adj.size).ctypes.data_as(DP)) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_prepare_pairs(net.handle, 1, nV.ctypes.data_as(IP), a32.ctypes.data_as(IP), f64_.ctypes.data_as(DP), nV.ctypes.data_as(IP),
                                        a32.ctypes.data_as(IP), f64_.ctypes.data_as(DP)) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_forward_host(net.handle, None, None, None, None) == _lib.GF_ERR_UNSUPPORTED
        assert b"covariant handle" in lib.gf_last_error(ctx.handle)
        works()
        with pytest.raises(GraphFlowHipError, match="molecule 0 has 7 vertices, the model was created with max_nVertices = 6"):
            net.prepare([(np.zeros((M + 1, M + 1), dtype=np.int32), np.zeros((M + 1, 4)))])
        works()
        buf = np.empty(64, dtype=np.float32)
        assert lib.gf_smp_read_reduced_adjacency(net.handle, 0, 1, 0, buf.ctypes.data_as(C.c_void_p), buf.size) == -1
        for bad, text in refused_configs():
            assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID and not h.value
            assert text in lib.gf_last_error(ctx.handle), lib.gf_last_error(ctx.handle)
        works()
        assert lib.gf_smp_param_count(net.handle) == lib.gf_smp_config_param_count(C.byref(net.cfg)) == params.size
        net.close()
