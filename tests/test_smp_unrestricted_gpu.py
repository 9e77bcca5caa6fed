"""GPU suite for Unrestricted_SMP_1D, Unrestricted_SMP_1D_ver2 and Unrestricted_SMP_2D (gf_smp_create, unrestricted = 1, 2, 3) on the level
of smp_level_unrestricted.hip.  Checked against the real classes' numbers (tests/golden/smp_unrestricted.npz), block by block of the
parameter vector, and at shapes without a golden against tests/unrestricted_ref.py, which tests/test_smp_unrestricted.py pins to the real
classes at 1e-9.  Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the graph feature, the prediction, the loss and every
parameter block; no element is excused.

There is no permutation-invariance test: a dense W_s depends on the order of the field, and the classes break WL ties by vertex index, so
the reference itself is not invariant on molecules with tied vertices (CH4's hydrogens)."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import unrestricted_cases as cases
import unrestricted_ref as uref
from field_suite import TOL, blockwise, dev
from inputs import toy_molecules
from make_unrestricted_golden import random_params, unrestricted_blocks
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FORM = cases.FORM


def golden():
    return kit.load_golden("smp_unrestricted.npz")


def params_of(gz, tag):
    form, _, Cn = (int(x) for x in gz[tag + "__cfg"][:3])
    return gz["u%d_c%d_f%d__params" % (form, Cn, gz[tag + "__feature"].shape[1])]


def net_of(form, L, Cn, F, D, maxV, wl=True):
    from graphflow_amd.smp import SMPUnrestricted
    return SMPUnrestricted(FORM[form], maxV, L, Cn, F, D, wl)


def run_net(form, mols, targets, params, L, Cn, D, maxV, wl=True, **kw):
    """[predict, loss, feature, grads (, fields) (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: net_of(form, L, Cn, mols[0][1].shape[1], D, maxV, wl), mols, targets, params, **kw)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_device_matches_the_real_classes(gf, form):
    """Every case of tests/golden/smp_unrestricted.npz: the toy molecules, the 4-cycle, the star and the 12-vertex molecule with and
    without WL ordering, at the (C, nLevels) of the generator.  max_nVertices = 14: the blocks of the sizes that do not occur keep exactly
    zero gradients.  For CH4 at two levels also every level activation and, for form 3, the adjacencies, through the introspection calls."""
    gz = golden()
    tags = [t for t in gz["tags"] if t.startswith("u%d_" % form)]
    assert len(tags) == 24
    for tag in tags:
        _, L, Cn, D, wl, maxV = (int(x) for x in gz[tag + "__cfg"])
        V = len(gz[tag + "__adj"])
        pred_ref, loss_ref, target = gz[tag + "__result"][:3]

        def inspect(net):
            act = np.concatenate([net.activation(0, l, v).ravel() for l in range(L + 1) for v in range(V)])
            radj = np.concatenate([net.reduced_adjacency(0, l, v).ravel() for l in range(1, L + 1) for v in range(V)]) if form == 3 else None
            return act, radj, net.level_sizes(L)

        pred, loss, feat, grads, (act, radj, sizes) = run_net(form, [(gz[tag + "__adj"], gz[tag + "__feature"])], [target], params_of(gz, tag), L,
                                                              Cn, D, maxV, bool(wl), inspect=inspect)
        blocks = unrestricted_blocks(form, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV)
        e = blockwise(grads, gz[tag + "__grads"], blocks)
        print(tag, rel_err(pred, [pred_ref]), rel_err(feat[0], gz[tag + "__graph_feature"]), rel_err(loss, [loss_ref]), e)
        assert rel_err(pred, [pred_ref]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__graph_feature"]) <= TOL, tag
        assert rel_err(loss, [loss_ref]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        used, off = {int(s) for s in gz[tag + "__phi"][1:, :, 0].ravel()}, 0
        for name, n in blocks:
            if name[:2] in ("W_", "W1", "W2", "b_") and int(name.rsplit("_", 1)[1]) not in used:
                assert not grads[off:off + n].any(), (tag, name)
            off += n
        s_top = gz[tag + "__phi"][L, :, 0].astype(np.int64)
        assert sizes[0] == V and sizes[1] == int((s_top ** 2).sum() if form == 3 else s_top.sum()), tag
        if tag + "__activations" in gz:
            assert rel_err(act, gz[tag + "__activations"]) <= TOL, tag
            if form == 3:
                assert np.array_equal(radj, gz[tag + "__adjacency"]), tag


@pytest.mark.parametrize("form", [3, 2])
def test_momentum_steps_match_the_real_classes(gf, form):
    """Three BatchLearn steps of the real Unrestricted_SMP_2D / Unrestricted_SMP_1D_ver2 on the four toy molecules: initial weights from
    gf_smp_uniform_init_host after the same srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    p_ = "train_u%d__" % form
    _, L, Cn, D, wl, maxV, seed, nIter = (int(x) for x in z[p_ + "cfg"])
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    lr, gamma = float(z[p_ + "lr"][0]), float(z[p_ + "momentum"][0])
    net = net_of(form, L, Cn, 4, D, maxV, bool(wl))
    kit.check_momentum_trajectory(net, lambda p, g: net.step(p, g, lr, len(mols), gamma), z, p_, mols, seed, nIter, lr)
    net.close()


def test_checkpoint_round_trip_reproduces_the_golden_prediction(gf, tmp_path):
    """save -> load in the reference's text format (six significant digits per value, registration order), then the loaded model's
    prediction against the golden's and against the restatement at the loaded values"""
    gz = golden()
    for tag in ("u1_C2H4_c5", "u2_C2H4_c5", "u3_C2H4_c5"):
        form, L, Cn, D, wl, maxV = (int(x) for x in gz[tag + "__cfg"])
        adj, x, result = gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"]
        kit.check_checkpoint_round_trip(
            net_of(form, L, Cn, 4, D, maxV, bool(wl)), tag, (adj, x), params_of(gz, tag), result[2:3], result[0],
            lambda loaded, fields: uref.run(form, adj, x, float(result[2]), loaded, L, Cn, D, maxV, fields)["predict"], tmp_path)


def run_packed(form, Cn):
    return lambda mols, tg, params, **kw: run_net(form, mols, tg, params, cases.PACK_L, Cn, cases.PACK_D, cases.PACK_MAXV, **kw)


def packed_case(form, Cn):
    """the packing batch on the device beside its fp64 expectation (unrestricted_cases), once per (form, channel count)"""
    mols, tg, params, blocks, phis, res, rg, margin = cases.packed_reference(form, Cn)
    assert margin >= cases.MARGIN   # (before anything is compared)

    def reference(mols, tg, params, out):
        assert out[4] == phis
        return res, rg, phis

    return kit.packed_case(("unrestricted", form, Cn), lambda: (mols, tg), lambda: params, run_packed(form, Cn), reference,
                           want_fields=True) + (blocks,)


@pytest.mark.parametrize("form,Cn", cases.PACKED_SHAPES)
def test_batch_across_the_packing_boundaries(gf, form, Cn):
    """against unrestricted_ref, per molecule (prediction, graph feature) and per block of the summed gradient: packed runs that break
    inside and between molecules, a size bucket with a single node, one with more nodes than a reduction chunk holds"""
    mols, tg, params, out, (res, rg, phis), blocks = packed_case(form, Cn)
    assert len(mols) == 70 and sum(len(a) for a, _ in mols) > 64
    counts = [np.bincount([len(f) for phi in phis for f in phi[l]]) for l in (1, 2)]
    assert (counts[1] == 1).any(), counts   # (level 2: one node of 7 positions, one of 9)
    assert counts[0].max() > 16 * 2 and counts[1].max() > 16 * 2, counts   # (16 chunks per bucket: several nodes per chunk)
    e = blockwise(out[3], rg, blocks)
    worst_feat = max(rel_err(out[2][m], res[m]["graph_feature"]) for m in range(len(mols)))
    print(form, Cn, rel_err(out[0], [r["predict"] for r in res]), worst_feat, e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e


@pytest.mark.parametrize("which", ["below", "above"])
def test_fields_on_both_sides_of_the_lds_limit(gf, which):
    """Unrestricted_SMP_1D_ver2 at C = 16, three levels, one molecule: a level-3 node keeps s x 64 floats of S, one node per workgroup, so
    the forward's LDS variant takes the fields up to 32 positions and the variant that reads the stored S the larger ones."""
    mols, tg, params, blocks, phis, res, rg, margin = cases.lds_reference(which)
    assert margin >= cases.MARGIN
    top = [len(f) for f in phis[0][cases.LDS_L]]
    assert np.mean(top) * (4 * cases.LDS_C // 4) > 128   # (theta_pack: 256 / items per node < 2 -- one node per workgroup)
    if which == "below":
        assert cases.LDS_FLOATS - 2 * 4 * cases.LDS_C < max(top) * 4 * cases.LDS_C <= cases.LDS_FLOATS, top
    else:
        over = [s for s in top if s * 4 * cases.LDS_C > cases.LDS_FLOATS]
        assert over and min(over) * 4 * cases.LDS_C <= cases.LDS_FLOATS + 2 * 4 * cases.LDS_C, top
    out = run_net(cases.LDS_FORM, mols, tg, params, cases.LDS_L, cases.LDS_C, cases.LDS_D, len(mols[0][0]))
    e = blockwise(out[3], rg, blocks)
    print(which, max(top), rel_err(out[0], [res[0]["predict"]]), rel_err(out[2][0], res[0]["graph_feature"]), e)
    assert rel_err(out[0], [res[0]["predict"]]) <= TOL
    assert rel_err(out[2][0], res[0]["graph_feature"]) <= TOL
    assert e[0] <= TOL, e


@pytest.mark.parametrize("form,Cn", [(1, 4), (2, 3), (3, 5)])
def test_one_molecule_isolated_inside_the_batch(gf, form, Cn):
    """With every other target equal to its prediction only molecule 68 (the 12-vertex one) has a loss gradient: the batch gradient is
    then that molecule's single-molecule gradient, and its prediction and graph feature are those it has alone."""
    case = packed_case(form, Cn)
    kit.check_isolated(case, 68, run_packed(form, Cn), case[5], outputs=True)


@pytest.mark.parametrize("form,Cn", [(1, 6), (2, 4), (3, 8)])
def test_two_runs_give_the_same_bits(gf, form, Cn):
    kit.check_same_bits(packed_case(form, Cn), run_packed(form, Cn))


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of these levels reads memory
    nobody wrote.  The golden, packing-boundary and LDS-limit cases in a fresh child process."""
    kit.run_under_poison(__file__, "real_classes or packing_boundaries or lds_limit")


@pytest.mark.parametrize("form", [1, 2, 3])
def test_kernel_table(gf, form):
    """The only GEMMs of a step are level 0's (H x forward, dH backward): the levels launch none.  One forward kernel per level; the
    reverse sweep's four steps once per level; none of the 18-slice, gamma, first-order or steerable level kernels."""
    mols, tg = cases.packing_batch()
    L, Cn = cases.PACK_L, 4
    net = net_of(form, L, Cn, 5, cases.PACK_D, cases.PACK_MAXV)
    net.prepare(mols)
    p = dev(random_params(form, Cn, 5 * (cases.PACK_D + 1), L, cases.PACK_MAXV, np.random.default_rng(1)))
    grads = torch.empty(net.n_params, device="cuda")
    counts = kit.traced_counts(net, lambda: (net.forward(p, dev(tg)), net.backward(p, grads)))
    net.close()
    d = "unres2d_" if form == 3 else "unres1d_"
    for k in (d + "level_fwd", d + "node_bwd", d + "bucket_partials", "unres_grads_finish", "unres_gather_bwd"):
        assert counts.get(k) == L, (k, counts)
    assert sum(n for k, n in counts.items() if k.startswith("gemm_")) == 2, counts
    # (the first-order read-out, smpt_readout_*, is the restricted sibling's and no level kernel)
    assert not [k for k in counts if k.startswith(("smpf_", "r18_", "smpg_", "smpt_", "smp1d_", "smp2d_")) and "readout" not in k], counts
    assert not [k for k in counts if k.startswith("unres") and not k.startswith((d, "unres_"))], counts


def test_refusals_leave_the_context_usable(gf):
    """The GF_ERR_UNSUPPORTED answers and the GF_ERR_INVALID configurations, then a forward on the same handle and context"""
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    from graphflow_amd.smp import SMPConfig
    gz = golden()
    for form in (1, 2, 3):
        tag = "u%d_NH3_c5" % form
        _, L, Cn, D, wl, maxV = (int(x) for x in gz[tag + "__cfg"])
        mol = (gz[tag + "__adj"], gz[tag + "__feature"])
        net = net_of(form, L, Cn, 4, D, maxV)
        lib, ctx = net.lib, net.ctx
        h = C.c_void_p()
        assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
        assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
        masks = (C.c_uint * 8)()
        assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
        with pytest.raises(GraphFlowHipError):
            net.prepare([mol], coulomb=[np.ones((4, 4))])
        net.prepare([mol])
        p, grads = dev(params_of(gz, tag)), torch.empty(net.n_params, device="cuda")
        target = dev(gz[tag + "__result"][2:3])
        net.forward(p, target)
        dfeat = torch.zeros_like(net.feature)
        assert lib.gf_smp_backward_features(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(grads.data_ptr()), C.c_void_p(dfeat.data_ptr()),
                                            0) == _lib.GF_ERR_UNSUPPORTED
        # a cap, a contraction family, a tower, a first-order form, a steerable form: GF_ERR_INVALID
        for bad in (SMPConfig(2, 8, 5, 1, 6, 1, 0, 0, 0, 0, 9, 0, form), SMPConfig(2, 8, 5, 1, 9, 1, 18, 0, 0, 0, 9, 0, form),
                    SMPConfig(2, 8, 5, 0, 9, 1, 0, 0, 1, 0, 9, 0, form), SMPConfig(2, 8, 5, 1, 9, 1, 0, 0, 0, 2, 9, 0, form),
                    SMPConfig(2, 8, 5, 1, 9, 1, 0, 0, 0, 0, 9, 1, form)):
            assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID
        pred, _, feat = net.forward(p, target)
        assert rel_err(pred.cpu().numpy(), gz[tag + "__result"][:1]) <= TOL
        assert rel_err(feat.cpu().numpy()[0], gz[tag + "__graph_feature"]) <= TOL
        net.close()
