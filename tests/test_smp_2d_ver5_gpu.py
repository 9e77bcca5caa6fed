"""GPU suite for SMP_2D_ver5 (gf_smp_create, steerable_2d = 5) on the level of smp_level_2d_ver5.hip.  Checked against the real class's
numbers (tests/golden/smp_2d_ver5.npz), block by block of the parameter vector, and at shapes without a golden against
tests/smp2d_ver5_ref.py, which tests/test_smp_2d_ver5.py pins to the real class at 1e-9.
Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the graph feature, the prediction, the loss and every parameter block."""
import ctypes as C
import os

import numpy as np
import pytest

import field_suite as kit
import smp2d_ver5_ref
from field_suite import TOL, blockwise, dev
from inputs import synthetic_molecule, toy_molecules
from make_smp2d_ver5_golden import random_params, smp2d_ver5_blocks
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DK_CHUNK = 512   # rows per partial image of dK1 (kV5Chunk of smp_level_2d_ver5.hip)


def golden():
    return kit.load_golden("smp_2d_ver5.npz")


def net_of(L, Cn, F, D, maxV, wl=True):
    from graphflow_amd.smp import SMP2D
    return SMP2D("ver5", maxV, L, Cn, F, D, wl)


def run_net(mols, targets, params, L, Cn, D, maxV, wl=True, **kw):
    """[predict, loss, feature, grads (, fields) (, inspect(net))] as float64 arrays"""
    return kit.run_net(lambda: net_of(L, Cn, mols[0][1].shape[1], D, maxV, wl), mols, targets, params, **kw)


def test_device_matches_the_real_class(gf):
    """Every case of tests/golden/smp_2d_ver5.npz: the toy molecules and the 12-vertex molecule with and without WL ordering, at
    (C, nLevels) = (5, 2), (10, 2), (8, 3): padded MFMA tiles with lane vectors of 1, 2 and 4 floats.  For CH4 at two levels also every
    level activation and reduced adjacency, through the introspection calls."""
    gz = golden()
    tags = list(gz["tags"])
    assert len(tags) == 18
    for tag in tags:
        _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        V = len(gz[tag + "__adj"])

        def inspect(net):
            act = np.concatenate([net.activation(0, l, v).ravel() for l in range(L + 1) for v in range(V)])
            radj = np.concatenate([net.reduced_adjacency(0, l, v).ravel() for l in range(1, L + 1) for v in range(V)])
            return act, radj, net.level_sizes(L)

        pred, loss, feat, grads, (act, radj, sizes) = run_net([(gz[tag + "__adj"], gz[tag + "__feature"])], gz[tag + "__target"],
                                                              gz[tag + "__params"], L, Cn, D, maxV, bool(wl), inspect=inspect)
        e = blockwise(grads, gz[tag + "__grads"], smp2d_ver5_blocks(Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV))
        print(tag, rel_err(pred, gz[tag + "__predict"]), rel_err(feat[0], gz[tag + "__graph_feature"]), rel_err(loss, gz[tag + "__loss"]), e)
        assert rel_err(pred, gz[tag + "__predict"]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__graph_feature"]) <= TOL, tag
        assert rel_err(loss, gz[tag + "__loss"]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)
        assert sizes[0] == V and sizes[1] == int((gz[tag + "__phi"][L, :, 0].astype(np.int64) ** 2).sum()), tag
        if tag + "__activations" in gz:
            assert rel_err(act, gz[tag + "__activations"]) <= TOL, tag
            assert rel_err(radj, gz[tag + "__adjacency"]) <= TOL, tag


def test_momentum_steps_match_the_real_class(gf):
    """Three BatchLearn steps of the real SMP_2D_ver5 on the four toy molecules: initial weights from gf_smp_uniform_init_host after the
    same srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    form, L, Cn, D, wl, maxV, _, seed, nIter = (int(x) for x in z["train__cfg"])
    assert form == 5
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    lr, gamma = float(z["train__lr"][0]), float(z["train__momentum"][0])
    net = net_of(L, Cn, 4, D, maxV, bool(wl))
    kit.check_momentum_trajectory(net, lambda p, g: net.step(p, g, lr, len(mols), gamma), z, "train__", mols, seed, nIter, lr)
    net.close()


def test_checkpoint_round_trip_reproduces_the_golden_prediction(gf, tmp_path):
    """save -> load in the reference's text format (six significant digits per value, registration order: K_l in front of scalar_l), then
    the loaded model's prediction against the golden's and against the restatement at the loaded values"""
    gz = golden()
    tag = "f5_C2H4_c5"
    _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
    adj, x, target = gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__target"]
    kit.check_checkpoint_round_trip(
        net_of(L, Cn, 4, D, maxV, bool(wl)), tag, (adj, x), gz[tag + "__params"], target, gz[tag + "__predict"],
        lambda loaded, fields: smp2d_ver5_ref.run(adj, x, float(target[0]), loaded, L, Cn, D, maxV, fields)["predict"], tmp_path)


def packing_batch():
    """The 70 molecules of test_smp_2d_gpu.py: the four toy molecules 17 times (their features in five columns), the 12-vertex synthetic
    molecule and a 7-vertex one -- more nodes than one workgroup packs (64), every size bucket from 2 to 9, so that the 32-row tiles of the
    projection span nodes of different sizes (lambda1_s per ROW), with a ragged last tile"""
    mols, tg = [], []
    for rep in range(17):
        for _, adj, feat, t in toy_molecules():
            mols.append((adj, np.concatenate([feat, np.zeros((len(adj), 1))], axis=1)))
            tg.append(0.05 * t + 0.01 * rep)
    for seed, V in ((5, 12), (7, 7)):
        adj, x, _ = synthetic_molecule(seed, V)
        mols.append((adj, x))
        tg.append(0.05 * V)
    return mols, np.array(tg)


PACK_L, PACK_D, PACK_MAXV = 2, 1, 13


def run_packed(Cn):
    return lambda mols, tg, params, **kw: run_net(mols, tg, params, PACK_L, Cn, PACK_D, PACK_MAXV, **kw)


def packed_case(Cn):
    """the packing batch on the device (with every level's sizes) and its fp64 expectation, computed once per channel count"""
    blocks = smp2d_ver5_blocks(Cn, 5 * (PACK_D + 1), PACK_L, PACK_MAXV)
    return kit.packed_case(("smp_2d_ver5", Cn), packing_batch,
                           lambda: random_params(Cn, 5 * (PACK_D + 1), PACK_L, PACK_MAXV, np.random.default_rng(500 + Cn)), run_packed(Cn),
                           lambda mols, tg, params, out: smp2d_ver5_ref.run_batch(mols, tg, params, PACK_L, Cn, PACK_D, PACK_MAXV, out[4]),
                           want_fields=True, inspect=lambda net: [net.level_sizes(l) for l in range(PACK_L + 1)]) + (blocks,)


@pytest.mark.parametrize("Cn", [5, 8, 32, 40, 66, 72, 100, 128])
def test_batch_across_the_packing_boundaries(gf, Cn):
    """against smp2d_ver5_ref, per molecule (prediction, graph feature) and per block of the summed gradient.  C = 32: exactly one MFMA
    tile, nothing padded; C = 40: a ragged second tile in the output and in the reduction dimension; 5 and 8: one padded tile, scalar
    and 16-byte operand loads; 66 and 72: three tiles, scalar and 16-byte loads; 100 and 128: four tiles, ragged and full (at 128 the
    LDS images of both projections need the opt-in).  Every level has rows for at least two chunks of dK1, and a last 32-row tile that
    is not full.  Every width runs the whole batch: its fp64 reference takes 0.2 s (C = 40) to 0.5 s (C = 128) on the CPU."""
    mols, tg, params, out, (res, rg), blocks = packed_case(Cn)
    assert len(mols) == 70 and sum(len(a) for a, _ in mols) > 64
    sizes = {int(s) for m in out[4] for l in (1, 2) for s in map(len, m[l])}
    assert sizes == set(range(2, 10))   # (two levels above the 12-vertex molecule: its largest field has 9 vertices)
    for l in (1, 2):
        rows = out[5][l][1]
        assert rows >= 2 * DK_CHUNK and rows % 32 != 0, (l, rows)
    e = blockwise(out[3], rg, blocks)
    worst_feat = max(rel_err(out[2][m], res[m]["graph_feature"]) for m in range(len(mols)))
    print(Cn, rel_err(out[0], [r["predict"] for r in res]), worst_feat, e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e


def test_one_molecule_isolated_inside_the_batch(gf):
    """With every other target equal to its prediction only molecule 68 (the 12-vertex one) has a loss gradient: the batch gradient is
    then that molecule's single-molecule gradient, and its prediction and graph feature are those it has alone."""
    case = packed_case(8)
    kit.check_isolated(case, 68, run_packed(8), case[5], outputs=True)


@pytest.mark.parametrize("Cn", [5, 40, 128])
def test_two_runs_give_the_same_bits(gf, Cn):
    kit.check_same_bits(packed_case(Cn), run_packed(Cn))


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of this level reads memory
    nobody wrote.  The golden and packing-boundary cases, and the level's kernels one by one at every width
    (tests/test_smp_2d_ver5_ops_gpu.py), in a fresh child process."""
    kit.run_under_poison([__file__, os.path.join(kit.HERE, "test_smp_2d_ver5_ops_gpu.py")],
                         "real_class or packing_boundaries or every_instantiation")


def test_kernel_table(gf):
    """Forward, per level: the storing gather and the two projections.  Reverse sweep, per level: dz, the two transposed projections, the
    two chunked dK reductions and their fold, combine, then the steerable level's own three steps.  The only GEMMs of a step are level
    0's; none of forms 1 / 2's forward or node kernels, nor any other family's level kernels."""
    mols, tg = packing_batch()
    L, Cn = PACK_L, 8
    net = net_of(L, Cn, 5, PACK_D, PACK_MAXV)
    net.prepare(mols)
    p = dev(random_params(Cn, 5 * (PACK_D + 1), L, PACK_MAXV, np.random.default_rng(1)))
    grads = torch.empty(net.n_params, device="cuda")
    net.ctx.set_timing(True)
    net.forward(p, dev(tg))
    fwd = {k: n for k, (_, n) in net.ctx.timings().items()}
    net.backward(p, grads)
    counts = {k: n for k, (_, n) in net.ctx.timings().items()}
    net.ctx.set_timing(False)
    net.close()
    for k in ("smp2d5_store_S", "smp2d5_col_proj", "smp2d5_row_proj"):
        assert fwd.get(k) == L and counts.get(k) == L, (k, fwd, counts)
    assert not [k for k in fwd if k.endswith("_bwd") or k in ("smp2d5_dz", "smp2d5_wgrad", "smp2d5_combine")], fwd
    for k in ("smp2d5_dz", "smp2d5_row_proj_bwd", "smp2d5_col_proj_bwd", "smp2d5_wgrad_fold", "smp2d5_combine", "smp2d_bucket_partials",
              "smp2d_grads_finish", "smp2d_gather_bwd"):
        assert counts.get(k) == L, (k, counts)
    assert counts.get("smp2d5_wgrad") == 2 * L, counts
    assert sum(n for k, n in counts.items() if k.startswith("gemm_")) == 2, counts
    assert not [k for k in counts if k.startswith(("smpf_", "r18_", "smpg_", "smpt_", "smp1d_", "unres_")) or
                k in ("smp2d_level_fwd", "smp2d_node_bwd")], counts


def test_refusals_leave_the_context_usable(gf):
    """GF_ERR_UNSUPPORTED: a classifier, the all-reduce, dropout masks, backward-features, a Coulomb matrix; GF_ERR_INVALID: 129 channels,
    forms 3 and 4, a cap.  Then a forward on the same handle and context."""
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    from graphflow_amd.smp import SMP2D, SMPConfig
    gz = golden()
    tag = "f5_NH3_c5"
    _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
    mol = (gz[tag + "__adj"], gz[tag + "__feature"])
    net = net_of(L, Cn, 4, D, maxV)
    lib, ctx = net.lib, net.ctx
    h = C.c_void_p()
    ok = SMPConfig(2, 8, 5, 1, 9, 1, 0, 0, 0, 0, 9, 5)
    assert lib.gf_smp_create_classifier(ctx.handle, C.byref(ok), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
    with pytest.raises(GraphFlowHipError):
        SMP2D("ver5", 9, 2, 8, 5, 1, True, 3)
    assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
    assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
    masks = (C.c_uint * 8)()
    assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
    with pytest.raises(GraphFlowHipError):
        net.prepare([mol], coulomb=[np.ones((4, 4))])
    net.prepare([mol])
    p, grads = dev(gz[tag + "__params"]), torch.empty(net.n_params, device="cuda")
    net.forward(p, dev(gz[tag + "__target"]))
    dfeat = torch.zeros_like(net.feature)
    assert lib.gf_smp_backward_features(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(grads.data_ptr()), C.c_void_p(dfeat.data_ptr()),
                                        0) == _lib.GF_ERR_UNSUPPORTED
    for bad in (SMPConfig(2, 129, 5, 1, 9, 1, 0, 0, 0, 0, 9, 5), SMPConfig(2, 8, 5, 1, 9, 1, 0, 0, 0, 0, 9, 3),
                SMPConfig(2, 8, 5, 1, 9, 1, 0, 0, 0, 0, 9, 4), SMPConfig(2, 8, 5, 1, 6, 1, 0, 0, 0, 0, 9, 5),
                SMPConfig(2, 8, 5, 1, 9, 1, 18, 0, 0, 0, 9, 5), SMPConfig(2, 8, 5, 1, 9, 1, 0, 0, 0, 2, 9, 5)):
        assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID
    pred, _, feat = net.forward(p, dev(gz[tag + "__target"]))
    assert rel_err(pred.cpu().numpy(), gz[tag + "__predict"]) <= TOL
    assert rel_err(feat.cpu().numpy()[0], gz[tag + "__graph_feature"]) <= TOL
    net.close()


def test_feature_is_invariant_under_vertex_permutation(gf):
    """WL ordering on: Feature of the 12-vertex molecule under a random vertex permutation.  The fp64 restatement's own difference under
    the same permutation is at rounding level first, so the property holds for the inputs chosen."""
    adj, x, _ = synthetic_molecule(5, 12)
    L, Cn, D, maxV = 2, 4, 2, 12
    params = random_params(Cn, 5 * (D + 1), L, maxV, np.random.default_rng(9))
    kit.check_permutation_invariance(adj, x, lambda mols, tg: run_net(mols, tg, params, L, Cn, D, maxV, want_fields=True),
                                     lambda a, f, fields: smp2d_ver5_ref.run(a, f, 1.0, params, L, Cn, D, maxV, fields)["graph_feature"])
