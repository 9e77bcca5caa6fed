"""GPU suite for CCN_1D through gf_smp_model_create (gf_smp_model_config.ccn_1d), on the first-order level of smp_level_theta.hip at widths
it had not seen (27 -> 22 -> 18 -> 16, seven levels of 16) and the head at widths set by the decay.  Checked against the real class's
numbers (tests/golden/ccn_1d.npz, ccn_1d_demo.npz, ccn_1d_checkpoint.dat), block by block of the parameter vector, and at a batch
without a golden against tests/ccn1d_ref.py, which tests/test_ccn_1d.py pins to the real class.  Tolerances: those of
tests/test_smp_theta_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import ccn1d_ref
import field_suite as kit
from field_suite import TOL, blockwise, dev, load_golden as load
from make_ccn1d_golden import demo_pairs, model_blocks, random_params
from theta_ref import fields_of
from test_smp_theta_gpu import packing_batch
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def golden_cases():
    out = {}
    for name in ("ccn_1d.npz", "ccn_1d_demo.npz"):
        z = load(name)
        for tag in z["tags"]:
            p = "ccn_%s__" % tag
            out[str(tag)] = {k[len(p):]: v for k, v in z.items() if k.startswith(p)}
    return out


def settings(c):
    maxV1, maxV2, cap, L, Cn = (int(x) for x in c["cfg"])
    return maxV1, maxV2, cap, L, Cn, float(c["decay"][0]), [c["feature"].shape[1], c["feature2"].shape[1]]


def run_pairs(cfg, g1, g2, targets, params, ctx=None):
    """prediction, loss and the batch gradient of CCN1D(*cfg) on the pairs (g1[i], g2[i]), as float64 arrays"""
    from graphflow_amd.smp import CCN1D
    return kit.run_net(lambda: CCN1D(*cfg, ctx=ctx), (g1, g2), targets, params)


def check_case(tag, c, ctx=None):
    maxV1, maxV2, cap, L, Cn, decay, F = settings(c)
    pred, loss, grads = run_pairs((maxV1, maxV2, cap, L, Cn, F[0], F[1], decay), [(c["adj"], c["feature"])], [(c["adj2"], c["feature2"])],
                                  c["target"], c["params"], ctx)
    e = blockwise(grads, c["grads"], model_blocks(Cn, L, F, [maxV1, maxV2], decay))
    print(tag, rel_err(pred, c["predict"]), rel_err(loss, c["loss"]), e)
    assert rel_err(pred, c["predict"]) <= TOL, tag
    assert rel_err(loss, c["loss"]) <= 2 * TOL, tag
    assert e[0] <= TOL, (tag, e)


@pytest.mark.parametrize("tag", ["toy_L7", "toy_L3", "asym_c27", "decay1", "star5_cap4", "negative"])
def test_device_matches_the_real_ccn_1d(gf, tag):
    check_case(tag, golden_cases()[tag])


def demo_net(L):
    from graphflow_amd.smp import CCN1D
    return CCN1D(10, 10, 6, L, 16, 4, 4, 0.5)


def test_initial_weights_match_the_real_class(gf):
    z = load("ccn_1d_demo.npz")
    *_, L, _, seed, _ = (int(x) for x in z["train__cfg"])
    net = demo_net(L)
    C.CDLL(None).srand(seed)
    w = net.uniform_init_host()
    net.close()
    assert z["train__params0"].dtype == np.float32 and np.array_equal(w, z["train__params0"])


def test_batchlearn_steps_match_the_real_ccn_1d(gf):
    """Three BatchLearn steps of the real class on the 16 toy pairs at the demo's settings (L = 3): initial weights after the same srand,
    Adam over the whole vector; then Predict.  The bounds are field_suite.check_momentum_trajectory's."""
    z = load("ccn_1d_demo.npz")
    *_, L, _, seed, nIter = (int(x) for x in z["train__cfg"])
    pairs = demo_pairs()
    g1, g2 = [a for a, _, _ in pairs], [b for _, b, _ in pairs]
    assert np.array_equal(z["train__targets"], [t for *_, t in pairs])
    lr = float(z["train__lr"][0])
    net = demo_net(L)
    p = kit.check_momentum_trajectory(net, lambda p, g: net.adam_step(p, g, lr, len(pairs)), z, "train__", (g1, g2), seed, nIter, lr,
                                      init=net.uniform_init_host, show="%s %s")
    pred, _ = net.forward(p)
    assert rel_err(pred.cpu().numpy(), z["train__predict"]) <= TOL
    net.close()


def test_checkpoints(gf, tmp_path):
    """The text checkpoint the real class's save_model wrote after the three steps loads and predicts what the real class predicted from
    it; a checkpoint saved here reloads to the same bits."""
    z = load("ccn_1d_demo.npz")
    *_, L, _, seed, _ = (int(x) for x in z["train__cfg"])
    pairs = demo_pairs()
    net = demo_net(L)
    p = net.load_model(os.path.join(kit.HERE, "golden", "ccn_1d_checkpoint.dat"))
    assert rel_err(p.cpu().numpy(), z["train__params"]) <= 1e-6   # (six printed digits of values below 0.1)
    net.prepare([a for a, _, _ in pairs], [b for _, b, _ in pairs])
    pred, _ = net.forward(p)
    assert rel_err(pred.cpu().numpy(), z["train__checkpoint_predict"]) <= TOL
    C.CDLL(None).srand(seed)
    w = dev(net.uniform_init_host())
    net.save_model(w, tmp_path / "ccn.dat")
    again = net.load_model(tmp_path / "ccn.dat")
    assert np.array_equal(again.cpu().numpy().view(np.uint32), w.cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError, match="parameters"):
        demo_net(L + 1).load_model(tmp_path / "ccn.dat")
    net.close()


# ---- a batch across the packing boundaries: 70 pairs, tower 2 sees the list reversed -------------------------------------------------
PACK = (9, 9, 6, 2, 18, 5, 5, 0.9)   # widths 18 -> 17 -> 16: lane vectors of 2, 1 and 4 floats; the cap of 6 bites on the 7- to 9-vertex molecules


def host_fields(lib, maxV, cap, L, Cn, adj, feat):
    """phi_l(v) from gf_smp_prepare_molecule_host (tests/test_ccn_1d.py holds it against the real class's fields)"""
    from graphflow_amd.smp import SMPTheta
    adj, feat = np.ascontiguousarray(adj, dtype=np.int32), np.ascontiguousarray(feat, dtype=np.float64)
    cfg = SMPTheta.config(maxV, cap, L, Cn, feat.shape[1], 0, False)
    cfg.physics = 1
    phi = np.zeros((L + 1, len(adj), cap + 1), dtype=np.int32)
    assert lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(adj), adj.ctypes.data_as(C.POINTER(C.c_int)), feat.ctypes.data_as(C.POINTER(C.c_double)),
                                            phi.ctypes.data_as(C.POINTER(C.c_int)), None) == 0
    return fields_of(phi)


def run_packed(pairs, tg, params):
    return run_pairs(PACK, pairs[0], pairs[1], tg, params)


def packed_case():
    """((g1, g2), targets, params, out, ref): the 70-pair batch on the device and its fp64 expectation, computed once"""
    maxV1, maxV2, cap, L, Cn, F1, F2, decay = PACK

    def batch():
        mols, tg = packing_batch()
        return (mols, mols[::-1]), tg

    def reference(pairs, tg, params, out):
        from graphflow_amd import _lib
        lib = _lib.load()
        phis = [(host_fields(lib, maxV1, cap, L, Cn, *a), host_fields(lib, maxV2, cap, L, Cn, *b)) for a, b in zip(*pairs)]
        return ccn1d_ref.run_batch(list(zip(*pairs)), tg, params, L, Cn, [maxV1, maxV2], decay, phis)

    return kit.packed_case("ccn_1d", batch, lambda: random_params(Cn, L, [F1, F2], [maxV1, maxV2], decay, [np.ones(F1), np.ones(F2)],
                                                                  np.random.default_rng(118)), run_packed, reference)


def pack_blocks():
    maxV1, maxV2, cap, L, Cn, F1, F2, decay = PACK
    return model_blocks(Cn, L, [F1, F2], [maxV1, maxV2], decay)


def test_batch_across_the_packing_boundaries(gf):
    (g1, _), tg, _, (pred, loss, grads), (rp, rg) = packed_case()
    assert len(g1) == 70 and sum(len(a) for a, _ in g1) > 64
    e = blockwise(grads, rg, pack_blocks())
    print(rel_err(pred, rp), e)
    assert rel_err(pred, rp) <= TOL
    assert rel_err(loss, 0.5 * (rp - tg) ** 2) <= 2 * TOL
    assert e[0] <= TOL, e


def test_one_pair_isolated_inside_the_batch(gf):
    """With every other target equal to its prediction only pair 37 has a loss gradient: the batch gradient is then that pair's own."""
    kit.check_isolated(packed_case(), 37, run_packed, pack_blocks(), outputs=True)


def test_two_runs_give_the_same_bits(gf):
    kit.check_same_bits(packed_case(), run_packed)


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel reads memory nobody wrote at
    the new widths.  The golden and packing-boundary cases in a child process."""
    kit.run_under_poison(__file__, "real_ccn_1d or packing_boundaries")


def test_only_the_first_order_kernels_run(gf):
    from graphflow_amd.smp import CCN1D
    (g1, g2), tg, params = packed_case()[:3]
    L = PACK[3]
    net = CCN1D(*PACK)
    net.prepare(g1, g2)
    p = dev(params)
    grads = torch.empty(net.n_params, device="cuda")
    counts = kit.traced_counts(net, lambda: (net.forward(p, dev(tg)), net.backward(p, grads)))
    net.close()
    for name in ("smpt_level_fwd", "smpt_node_bwd", "smpt_size_grads", "smpt_gather_bwd"):
        assert counts.get(name) == 2 * L, (name, counts)   # (two towers)
    assert not [name for name in counts if name.startswith(("smpf_", "r18_", "r10_", "r4_", "fam", "smpg_", "smp1d_", "smp2d", "unres"))], counts


def test_refusals_leave_the_context_usable(gf):
    """nChanels = 15, decay 0 and 1.5 and one tower are refused at create, a zero feature row at prepare, each with GF_ERR_INVALID; the
    same context then runs a golden case."""
    from graphflow_amd import _lib
    from graphflow_amd.ops import Context, GraphFlowHipError
    from graphflow_amd.smp import CCN1D, SMPModel
    ctx = Context(0)
    for args in ((10, 10, 6, 3, 15, 4, 4, 0.5), (10, 10, 6, 3, 16, 4, 4, 0.0), (10, 10, 6, 3, 16, 4, 4, 1.5)):
        with pytest.raises(GraphFlowHipError, match="ccn_1d") as e:
            CCN1D(*args, ctx=ctx)
        assert e.value.status == _lib.GF_ERR_INVALID
    with pytest.raises(GraphFlowHipError, match="nTowers = 2") as e:
        SMPModel(3, 16, 6, [4], ctx=ctx, first_order=True, max_nVertices=10, ccn_1d=True, nChanels_decay=0.5)
    assert e.value.status == _lib.GF_ERR_INVALID
    c = golden_cases()["negative"]
    maxV1, maxV2, cap, L, Cn, decay, F = settings(c)
    net = CCN1D(maxV1, maxV2, cap, L, Cn, F[0], F[1], decay, ctx=ctx)
    zero = c["feature2"].copy()
    zero[3] = 0.0
    with pytest.raises(GraphFlowHipError, match="sample 1, tower 2, vertex 3") as e:
        net.prepare([(c["adj"], c["feature"])] * 2, [(c["adj2"], c["feature2"]), (c["adj2"], zero)])
    assert e.value.status == _lib.GF_ERR_INVALID
    net.close()
    check_case("negative", c, ctx)
    ctx.close()
