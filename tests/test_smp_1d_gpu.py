"""GPU suite for SMP_1D, SMP_1D_ver2, SMP_1D_ver3 (gf_smp_create, first_order = 2, 3, 4) and their classifiers (gf_smp_create_classifier)
on the level of smp_level_1d.hip.  Checked against the real classes' numbers (tests/golden/smp_1d.npz), block by block of the parameter
vector, and at shapes without a golden against tests/smp1d_ref.py, which tests/test_smp_1d.py pins to the real classes at 1e-9.
Tolerance: the suite's 1e-5 (tests/util.py: rel_err), for the graph feature, the prediction, the loss and every parameter block."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
import smp1d_ref
from field_suite import TOL, blockwise
from inputs import synthetic_molecule, toy_molecules
from make_smp1d_golden import random_params, smp1d_blocks
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def golden():
    return kit.load_golden("smp_1d.npz")


def net_of(version, L, Cn, F, D, maxV, wl=True, nClass=0):
    from graphflow_amd.smp import SMP1D
    return SMP1D(version, maxV, L, Cn, F, D, wl, nClass)


def run_net(version, mols, targets, params, L, Cn, D, maxV, wl=True, nClass=0, want_fields=False):
    """[predict, loss, feature, grads (, scores, probability) (, fields)] as float64 arrays"""
    return kit.run_net(lambda: net_of(version, L, Cn, mols[0][1].shape[1], D, maxV, wl, nClass), mols, targets, params, n_class=nClass,
                       want_fields=want_fields)


@pytest.mark.parametrize("version", [1, 2, 3])
def test_device_matches_the_real_classes(gf, version):
    """Every regression case of tests/golden/smp_1d.npz: the toy molecules, the 4-cycle, the star and the 12-vertex molecule with and
    without WL ordering, at 4 and 3 channels (3: the two halves of a row start at an odd column) and, for SMP_1D, 5."""
    gz = golden()
    tags = [t for t in gz["tags"] if t.startswith("v%d_" % version)]
    assert len(tags) >= 16
    for tag in tags:
        _, L, Cn, D, wl, maxV, _ = (int(x) for x in gz[tag + "__cfg"])
        pred, loss, feat, grads = run_net(version, [(gz[tag + "__adj"], gz[tag + "__feature"])], gz[tag + "__target"], gz[tag + "__params"], L, Cn,
                                          D, maxV, bool(wl))
        e = blockwise(grads, gz[tag + "__grads"], smp1d_blocks(version, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV))
        print(tag, rel_err(pred, gz[tag + "__predict"]), rel_err(feat[0], gz[tag + "__graph_feature"]), rel_err(loss, gz[tag + "__loss"]), e)
        assert rel_err(pred, gz[tag + "__predict"]) <= TOL, tag
        assert rel_err(feat[0], gz[tag + "__graph_feature"]) <= TOL, tag
        assert rel_err(loss, gz[tag + "__loss"]) <= TOL, tag
        assert e[0] <= TOL, (tag, e)


def test_classifiers_match_the_real_classes(gf):
    """SMP_1D_classification and SMP_1D_ver3_classification at nClass = 5 on the 12-vertex molecule: scores, probabilities, loss, the
    arg-max label and every gradient block; a first_order = 1 classifier is still refused."""
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPTheta
    gz = golden()
    for tag in gz["class_tags"]:
        version, L, Cn, D, wl, maxV, nClass = (int(x) for x in gz[tag + "__cfg"])
        pred, loss, feat, grads, scores, prob = run_net(version, [(gz[tag + "__adj"], gz[tag + "__feature"])], gz[tag + "__target"],
                                                        gz[tag + "__params"], L, Cn, D, maxV, bool(wl), nClass)
        e = blockwise(grads, gz[tag + "__grads"], smp1d_blocks(version, Cn, gz[tag + "__feature"].shape[1] * (D + 1), L, maxV, nClass))
        print(tag, rel_err(scores[0], gz[tag + "__scores"]), rel_err(prob[0], gz[tag + "__probability"]), rel_err(loss, gz[tag + "__loss"]), e)
        assert rel_err(feat[0], gz[tag + "__graph_feature"]) <= TOL, tag
        assert rel_err(scores[0], gz[tag + "__scores"]) <= TOL, tag
        assert rel_err(prob[0], gz[tag + "__probability"]) <= TOL, tag
        assert rel_err(loss, gz[tag + "__loss"]) <= TOL, tag
        assert int(pred[0]) == int(gz[tag + "__label"][0]), tag
        assert e[0] <= TOL, (tag, e)
    theta = SMPTheta(9, 9, 2, 8, 5, 1)
    h = C.c_void_p()
    assert theta.lib.gf_smp_create_classifier(theta.ctx.handle, C.byref(theta.cfg), 5, C.byref(h)) == _lib.GF_ERR_UNSUPPORTED
    theta.close()


def test_version2_classifier_matches_the_restatement(gf):
    """The reference has no SMP_1D_ver2_classification; the handle is the ver2 levels under the same read-out, held to smp1d_ref."""
    adj, x, _ = synthetic_molecule(5, 12)
    L, Cn, D, maxV, nClass = 2, 3, 1, 12, 5
    blocks = smp1d_blocks(2, Cn, 5 * (D + 1), L, maxV, nClass)
    params = random_params(blocks, np.random.default_rng(52), nClass)
    out = run_net(2, [(adj, x)], np.array([3.0]), params, L, Cn, D, maxV, True, nClass, want_fields=True)
    r = smp1d_ref.run(2, adj, x, 3.0, params, L, Cn, D, maxV, out[6][0], nClass)
    assert rel_err(out[4][0], r["scores"]) <= TOL and rel_err(out[5][0], r["probability"]) <= TOL
    assert rel_err(out[1], [r["loss"]]) <= TOL and int(out[0][0]) == r["label"]
    e = blockwise(out[3], r["grads"], blocks)
    assert e[0] <= TOL, e


def test_momentum_steps_match_the_real_smp_1d_ver3(gf):
    """Three BatchLearn steps of the real SMP_1D_ver3 on the four toy molecules: initial weights from gf_smp_uniform_init_host after the
    same srand, gf_smp_momentum_step.  The bounds are field_suite.check_momentum_trajectory's."""
    z = golden()
    version, L, Cn, D, wl, maxV, _, seed, nIter = (int(x) for x in z["train__cfg"])
    mols = [(adj, feat) for _, adj, feat, _ in toy_molecules()]
    lr, gamma = float(z["train__lr"][0]), float(z["train__momentum"][0])
    net = net_of(version, L, Cn, 4, D, maxV, bool(wl))
    kit.check_momentum_trajectory(net, lambda p, g: net.step(p, g, lr, len(mols), gamma), z, "train__", mols, seed, nIter, lr)
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


def run_packed(version, Cn):
    return lambda mols, tg, params, **kw: run_net(version, mols, tg, params, PACK_L, Cn, PACK_D, PACK_MAXV, **kw)


def packed_case(version, Cn):
    """the packing batch on the device and its fp64 expectation (per molecule, summed gradient), computed once per (form, channel count)"""
    blocks = smp1d_blocks(version, Cn, 5 * (PACK_D + 1), PACK_L, PACK_MAXV)
    return kit.packed_case(("smp_1d", version, Cn), packing_batch, lambda: random_params(blocks, np.random.default_rng(100 * version + Cn)),
                           run_packed(version, Cn),
                           lambda mols, tg, params, out: smp1d_ref.run_batch(version, mols, tg, params, PACK_L, Cn, PACK_D, PACK_MAXV, out[4]),
                           want_fields=True) + (blocks,)


PACKED_SHAPES = [(1, 5), (2, 3), (2, 4), (3, 3), (3, 4)]


@pytest.mark.parametrize("version,Cn", PACKED_SHAPES)
def test_batch_across_the_packing_boundaries(gf, version, Cn):
    """against smp1d_ref, per molecule (prediction, graph feature) and per block of the summed gradient"""
    mols, tg, params, out, (res, rg), blocks = packed_case(version, Cn)
    assert sum(len(a) for a, _ in mols) > 64
    e = blockwise(out[3], rg, blocks)
    worst_feat = max(rel_err(out[2][m], res[m]["graph_feature"]) for m in range(len(mols)))
    print(version, Cn, rel_err(out[0], [r["predict"] for r in res]), worst_feat, e)
    assert rel_err(out[0], np.array([r["predict"] for r in res])) <= TOL
    assert worst_feat <= TOL
    assert e[0] <= TOL, e


@pytest.mark.parametrize("version,Cn", [(1, 5), (2, 3), (3, 4)])
def test_one_molecule_isolated_inside_the_batch(gf, version, Cn):
    """With every other target equal to its prediction only molecule 37 has a loss gradient: the batch gradient is then that molecule's
    single-molecule gradient."""
    case = packed_case(version, Cn)
    kit.check_isolated(case, 37, run_packed(version, Cn), case[5])


@pytest.mark.parametrize("version,Cn", [(1, 5), (2, 4), (3, 3)])
def test_two_runs_give_the_same_bits(gf, version, Cn):
    kit.check_same_bits(packed_case(version, Cn), run_packed(version, Cn))


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel of these levels reads memory
    nobody wrote.  The golden, classifier and packing-boundary cases in a fresh child process."""
    kit.run_under_poison(__file__, "real_classes or packing_boundaries")


@pytest.mark.parametrize("version", [1, 2, 3])
def test_kernel_table(gf, version):
    """SMP_1D / ver2: the only GEMMs of a step are level 0's (H x forward, dH backward) -- the levels launch none; ver3: three per level
    on top.  None of the 18-slice, gamma or theta level kernels; the per-size reduction is the theta level's."""
    mols, tg = packing_batch()
    L, Cn = PACK_L, 4
    net = net_of(version, L, Cn, 5, PACK_D, PACK_MAXV)
    net.prepare(mols)
    p = kit.dev(random_params(smp1d_blocks(version, Cn, 5 * (PACK_D + 1), L, PACK_MAXV), np.random.default_rng(1)))
    grads = torch.empty(net.n_params, device="cuda")
    counts = kit.traced_counts(net, lambda: (net.forward(p, kit.dev(tg)), net.backward(p, grads)))
    nodes, rows, ppos = net.level_sizes(L)
    assert nodes == sum(len(a) for a, _ in mols) and ppos == 0
    net.close()
    for k in ("smp1d_level_fwd", "smp1d_node_bwd", "smpt_size_grads", "smp1d_gather_bwd"):
        assert counts.get(k) == L, (k, counts)
    gemms = sum(n for k, n in counts.items() if k.startswith("gemm_"))
    assert gemms == 2 + (3 * L if version == 3 else 0), counts
    assert (counts.get("smpt_weight_views", 0), counts.get("smpt_wgrad_fold", 0)) == ((2 * L, L) if version == 3 else (0, 0)), counts
    assert not [k for k in counts if k.startswith(("smpf_", "r18_", "smpg_", "smpt_level", "smpt_node", "smpt_gather"))], counts


def test_refusals_and_device_bytes(gf):
    from graphflow_amd import _lib
    from graphflow_amd.ops import GraphFlowHipError
    from graphflow_amd.smp import SMP1D, SMPConfig, SMPTheta
    mols, _ = packing_batch()
    net = net_of(1, 2, 8, 5, 1, 9)
    lib, ctx = net.lib, net.ctx
    assert lib.gf_smp_set_grad_allreduce(net.handle, 1) == _lib.GF_ERR_UNSUPPORTED
    assert lib.gf_smp_set_grad_allreduce(net.handle, 0) == _lib.GF_OK
    masks = (C.c_uint * 4)()
    assert lib.gf_smp_dropout_masks(net.handle, masks, C.c_float(1.0)) == _lib.GF_ERR_UNSUPPORTED
    h = C.c_void_p()
    for form in (2, 3, 4):   # a cap, a contraction family, a tower: GF_ERR_INVALID, from either constructor
        for bad in (SMPConfig(2, 8, 5, 1, 6, 1, 0, 0, 0, form, 9), SMPConfig(2, 8, 5, 1, 9, 1, 18, 0, 0, form, 9),
                    SMPConfig(2, 8, 5, 0, 9, 1, 0, 0, 1, form, 9)):
            assert lib.gf_smp_create(ctx.handle, C.byref(bad), C.byref(h)) == _lib.GF_ERR_INVALID
            assert lib.gf_smp_create_classifier(ctx.handle, C.byref(bad), 3, C.byref(h)) == _lib.GF_ERR_INVALID
    with pytest.raises(GraphFlowHipError):
        SMP1D(1, 9, 2, 8, 5, 1, True, 1)   # nClass = 1
    net.prepare(mols)
    used, _ = net.device_bytes()
    theta = SMPTheta(9, 9, 2, 8, 5, 1)
    theta.prepare(mols)
    used_theta, _ = theta.device_bytes()
    assert used <= used_theta, (used, used_theta)   # (the same tables, A and B; no G / dG, no weight views)
    net.close()
    theta.close()


@pytest.mark.parametrize("version", [1, 2, 3])
def test_feature_is_invariant_under_vertex_permutation(gf, version):
    """WL ordering on: Feature of the 12-vertex molecule under a random vertex permutation.  The fp64 restatement's own difference under
    the same permutation is at rounding level first, so the property holds for the inputs chosen."""
    adj, x, _ = synthetic_molecule(5, 12)
    L, Cn, D, maxV = 2, 4, 2, 12
    params = random_params(smp1d_blocks(version, Cn, 5 * (D + 1), L, maxV), np.random.default_rng(9))
    kit.check_permutation_invariance(adj, x, lambda mols, tg: run_net(version, mols, tg, params, L, Cn, D, maxV, want_fields=True),
                                     lambda a, f, fields: smp1d_ref.run(version, a, f, 1.0, params, L, Cn, D, maxV, fields)["graph_feature"])
