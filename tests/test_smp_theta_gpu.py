"""GPU suite for the first-order models: SMP_theta through gf_smp_create (first_order = 1) and SMP_theta_physics / SMP_theta_pairgraphs
through gf_smp_model_create, on the level of smp_level_theta.hip.  Checked against the real classes' numbers (tests/golden/smp_theta.npz,
smp_theta_physics.npz), block by block of the parameter vector, and at shapes without a golden against tests/theta_ref.py, which
tests/test_smp_theta.py pins to the real classes.  Tolerances: those of tests/test_smp_gamma_gpu.py / test_gamma_physics_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import theta_ref
from field_suite import TOL, blockwise, dev, load_golden as load
from inputs import synthetic_molecule
from make_theta_golden import model_blocks, random_params, small_molecules, theta_blocks
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def theta_net(L, Cn, F, D, cap, maxV, wl=True):
    from graphflow_amd.smp import SMPTheta
    return SMPTheta(maxV, cap, L, Cn, F, D, wl)


def run_theta(mols, targets, params, L, Cn, D, cap, maxV, wl=True, want_fields=False):
    return kit.run_net(lambda: theta_net(L, Cn, mols[0][1].shape[1], D, cap, maxV, wl), mols, targets, params, want_fields=want_fields)


def test_device_matches_the_real_smp_theta(gf):
    """Every case of tests/golden/smp_theta.npz (1 / 2 / 5 / 9 vertices at C = 8, 10, 1; the capped star; the capped 12-vertex
    molecule at L = 3), one molecule per batch."""
    gz = load("smp_theta.npz")
    for tag in gz["tags"]:
        p = "theta_%s__" % tag
        L, Cn, D, wl, cap, maxV = (int(x) for x in gz[p + "cfg"])
        pred, loss, feat, grads = run_theta([(gz[p + "adj"], gz[p + "feature"])], gz[p + "target"], gz[p + "params"], L, Cn, D, cap, maxV, bool(wl))
        e = blockwise(grads, gz[p + "grads"], theta_blocks(Cn, gz[p + "feature"].shape[1] * (D + 1), L, maxV))
        print(tag, rel_err(pred, gz[p + "predict"]), rel_err(feat[0], gz[p + "graph_feature"]), rel_err(loss, gz[p + "loss"]), e)
        assert rel_err(pred, gz[p + "predict"]) <= TOL, tag
        assert rel_err(feat[0], gz[p + "graph_feature"]) <= TOL, tag
        assert rel_err(loss, gz[p + "loss"]) <= 2 * TOL, tag
        assert e[0] <= TOL, (tag, e)


def test_towers_match_the_real_classes(gf):
    """SMP_theta_physics (16 -> 8 -> 4 and 10 -> 5 -> 2) and SMP_theta_pairgraphs through gf_smp_model_create."""
    from graphflow_amd.smp import SMPModel
    pz = load("smp_theta_physics.npz")
    for tag in pz["tags"]:
        p = "tphys_%s__" % tag
        towers, L, Cn, cap, maxV1, maxV2 = (int(x) for x in pz[p + "cfg"])
        F = [pz[p + "feature"].shape[1]] + ([pz[p + "feature2"].shape[1]] if towers == 2 else [])
        net = SMPModel(L, Cn, cap, F, first_order=True, max_nVertices=[maxV1, maxV2][:towers])
        assert net.n_params == pz[p + "params"].size, tag
        net.prepare([(pz[p + "adj"], pz[p + "feature"])], [(pz[p + "adj2"], pz[p + "feature2"])] if towers == 2 else None)
        prm = dev(pz[p + "params"])
        pred, loss = net.forward(prm, dev(pz[p + "target"]))
        grads = torch.empty(net.n_params, device="cuda")
        net.backward(prm, grads)
        e = blockwise(grads.cpu().numpy().astype(np.float64), pz[p + "grads"], model_blocks(towers, Cn, L, F + [0], [maxV1, maxV2]))
        print(tag, rel_err(pred.cpu().numpy(), pz[p + "predict"]), rel_err(loss.cpu().numpy(), pz[p + "loss"]), e)
        assert rel_err(pred.cpu().numpy(), pz[p + "predict"]) <= TOL, tag
        assert rel_err(loss.cpu().numpy(), pz[p + "loss"]) <= 2 * TOL, tag
        assert e[0] <= TOL, (tag, e)
        net.close()


def test_tower_initial_weights_match_the_real_class(gf):
    from graphflow_amd.smp import SMPModel
    pz = load("smp_theta_physics.npz")
    _, L, Cn, cap, maxV, seed, _ = (int(x) for x in pz["train__cfg"])
    net = SMPModel(L, Cn, cap, [4], first_order=True, max_nVertices=maxV)
    C.CDLL(None).srand(seed)
    assert np.array_equal(net.uniform_init_host(), pz["train__params0"].astype(np.float32))
    net.close()


def test_batchlearn_steps_match_the_real_smp_theta(gf):
    """Three BatchLearn steps of the real SMP_theta on the four small molecules: initial weights from gf_smp_uniform_init_host after the
    same srand, gf_smp_adam_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = load("smp_theta.npz")
    L, Cn, D, cap, maxV, seed, nIter = (int(x) for x in z["train__cfg"])
    mols = [(adj, feat) for _, adj, feat, _ in small_molecules()]
    lr = float(z["train__lr"][0])
    net = theta_net(L, Cn, 4, D, cap, maxV)
    kit.check_momentum_trajectory(net, lambda p, g: net.adam_step(p, g, lr, len(mols)), z, "train__", mols, seed, nIter, lr, show=None)
    net.close()


def packing_batch():
    """70 molecules of 1 to 9 vertices, several 1-vertex molecules (fields of one position) at both ends: more nodes than one workgroup
    packs (64), with a ragged last workgroup, and size buckets from 1 up"""
    rng = np.random.default_rng(70)
    sizes = [1, 1, 1] + [int(v) for v in rng.integers(2, 10, 64)] + [1, 1, 1]
    mols, tg = [], []
    for i, V in enumerate(sizes):
        if V == 1:
            adj, x = np.zeros((1, 1), dtype=np.int32), np.eye(5)[[i % 5]]
        else:
            adj, x, _ = synthetic_molecule(7000 + i, V)
        mols.append((adj, x))
        tg.append(0.25 * V - 1.0)
    return mols, np.array(tg)


PACK_L, PACK_D, PACK_MAXV = 2, 1, 9


def run_packed(Cn):
    return lambda mols, tg, params, **kw: run_theta(mols, tg, params, PACK_L, Cn, PACK_D, PACK_MAXV, PACK_MAXV, **kw)


def packed_case(Cn):
    """the packing batch on the device and its fp64 expectation, computed once per channel count"""
    blocks = theta_blocks(Cn, 5 * (PACK_D + 1), PACK_L, PACK_MAXV)
    return kit.packed_case(("theta", Cn), packing_batch, lambda: random_params(blocks, np.random.default_rng(100 + Cn)),
                           run_packed(Cn), lambda mols, tg, params, out: theta_ref.run_batch(mols, tg, params, PACK_L, Cn, PACK_D, PACK_MAXV, out[4]),
                           want_fields=True) + (blocks,)


@pytest.mark.parametrize("Cn", [10, 8])
def test_batch_across_the_packing_boundaries(gf, Cn):
    mols, tg, params, out, (rp, rf, rg), blocks = packed_case(Cn)
    assert sum(len(a) for a, _ in mols) > 64
    e = blockwise(out[3], rg, blocks)
    print(Cn, rel_err(out[0], rp), rel_err(out[2], rf), e)
    assert rel_err(out[0], rp) <= TOL
    assert rel_err(out[2], rf) <= TOL
    assert e[0] <= TOL, e


def test_one_molecule_isolated_inside_the_batch(gf):
    """With every other target equal to its prediction only molecule 37 has a loss gradient: the batch gradient is then that molecule's
    single-molecule gradient."""
    case = packed_case(10)
    kit.check_isolated(case, 37, run_packed(10), case[5])


def test_two_runs_give_the_same_bits(gf):
    kit.check_same_bits(packed_case(8), run_packed(8))


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no first-order kernel reads memory
    nobody wrote.  The golden and packing-boundary cases in a child process."""
    kit.run_under_poison(__file__, "real_smp_theta or real_classes or packing_boundaries")


def test_only_the_first_order_kernels_run(gf):
    mols, tg = packing_batch()
    L, Cn, D, maxV = 2, 8, 1, 9
    net = theta_net(L, Cn, 5, D, maxV, maxV)
    net.prepare(mols)
    p = dev(random_params(theta_blocks(Cn, 5 * (D + 1), L, maxV), np.random.default_rng(1)))
    grads = torch.empty(net.n_params, device="cuda")
    counts = kit.traced_counts(net, lambda: (net.forward(p, dev(tg)), net.backward(p, grads)))
    nodes, rows, ppos = net.level_sizes(L)
    assert nodes == sum(len(a) for a, _ in mols) and ppos == 0
    assert rows == sum(len(net.receptive_field(m, L, v)) for m in range(len(mols)) for v in range(len(mols[m][0])))
    net.close()
    for k in ("smpt_level_fwd", "smpt_node_bwd", "smpt_size_grads", "smpt_gather_bwd"):
        assert counts.get(k) == L, (k, counts)
    assert not [k for k in counts if k.startswith(("smpf_", "r18_", "smpg_"))], counts


def test_refusals_and_device_bytes(gf):
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    from graphflow_amd.smp import SMPOmega, SMPTheta
    net = theta_net(2, 8, 5, 1, 9, 9)
    lib, ctx = net.lib, net.ctx
    h = C.c_void_p()
    assert lib.gf_smp_create_classifier(ctx.handle, C.byref(net.cfg), 3, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
    assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
    assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
    masks = (C.c_uint * 4)()
    assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
    with pytest.raises(GraphFlowHipError, match="max_nVertices"):
        SMPTheta(4, 6, 2, 8, 5, 1)
    mols, _ = packing_batch()
    net.prepare(mols)
    used, _ = net.device_bytes()
    omega = SMPOmega(2, 8, 5, 1, 9)
    omega.prepare(mols)
    used18, _ = omega.device_bytes()
    assert used < used18 / 4, (used, used18)   # (none of the 18-slice level's rows x 18 C scratch and s^2-sized tables)
    net.set_fused(False)   # (one plan: no effect)
    net.close()
    omega.close()


def test_feature_is_invariant_under_vertex_permutation(gf):
    """No cap: Feature of the 9-vertex molecule under a random vertex permutation.  The fp64 restatement's own difference under the same
    permutation is at rounding level first, so the property holds for the inputs chosen."""
    _, adj, x, _ = small_molecules()[3]
    L, Cn, D, maxV = 2, 8, 2, 9
    params = random_params(theta_blocks(Cn, 4 * (D + 1), L, maxV), np.random.default_rng(9))
    kit.check_permutation_invariance(adj, x, lambda mols, tg: run_theta(mols, tg, params, L, Cn, D, maxV, maxV, want_fields=True),
                                     lambda a, f, fields: theta_ref.run(a, f, 1.0, params, L, Cn, D, maxV, fields)["graph_feature"])
