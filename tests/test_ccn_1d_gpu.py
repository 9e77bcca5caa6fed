"""GPU suite for CCN_1D through gf_smp_model_create (gf_smp_model_config.ccn_1d), on the first-order level of smp_level_theta.hip at widths
it had not seen (27 -> 22 -> 18 -> 16, seven levels of 16) and the head at widths set by the decay.  Checked against the real class's
numbers (tests/golden/ccn_1d.npz, ccn_1d_demo.npz, ccn_1d_checkpoint.dat), block by block of the parameter vector, and at a batch
without a golden against tests/ccn1d_ref.py, which tests/test_ccn_1d.py pins to the real class.  Tolerances: those of
tests/test_smp_theta_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ccn1d_ref
from make_ccn1d_golden import demo_pairs, model_blocks, random_params
from theta_ref import fields_of
from test_smp_theta_gpu import packing_batch
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TOL = 1e-5   # the suite's end-to-end tolerance (tests/util.py)
HERE = os.path.dirname(os.path.abspath(__file__))


def dev(x, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype)).cuda()


def load(name):
    with np.load(os.path.join(HERE, "golden", name)) as z:
        return {k: z[k] for k in z.files}


def golden_cases():
    out = {}
    for name in ("ccn_1d.npz", "ccn_1d_demo.npz"):
        z = load(name)
        for tag in z["tags"]:
            p = "ccn_%s__" % tag
            out[str(tag)] = {k[len(p):]: v for k, v in z.items() if k.startswith(p)}
    return out


def blockwise(x, ref, blocks):
    """the largest rel_err over the parameter blocks: one norm over the whole vector cannot see an error confined to a small block"""
    off, worst = 0, (0.0, "")
    for name, n in blocks:
        worst = max(worst, (rel_err(x[off:off + n], ref[off:off + n]), name))
        off += n
    assert off == ref.size
    return worst


def settings(c):
    maxV1, maxV2, cap, L, Cn = (int(x) for x in c["cfg"])
    return maxV1, maxV2, cap, L, Cn, float(c["decay"][0]), [c["feature"].shape[1], c["feature2"].shape[1]]


def run_pairs(cfg, g1, g2, targets, params, ctx=None):
    """prediction, loss and the batch gradient of CCN1D(*cfg) on the pairs (g1[i], g2[i]), as float64 arrays"""
    from graphflow_amd.smp import CCN1D
    net = CCN1D(*cfg, ctx=ctx)
    assert net.n_params == len(params)
    net.prepare(g1, g2)
    p = dev(params)
    pred, loss = net.forward(p, dev(targets))
    grads = torch.empty(net.n_params, device="cuda")
    net.backward(p, grads)
    out = [x.cpu().numpy().astype(np.float64) for x in (pred, loss, grads)]
    net.close()
    return out


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
    Adam over the whole vector; then Predict.  Bounds of test_batchlearn_steps_match_the_real_smp_theta."""
    z = load("ccn_1d_demo.npz")
    *_, L, _, seed, nIter = (int(x) for x in z["train__cfg"])
    pairs = demo_pairs()
    g1, g2 = [a for a, _, _ in pairs], [b for _, b, _ in pairs]
    assert np.array_equal(z["train__targets"], [t for *_, t in pairs])
    tg = dev(z["train__targets"])
    lr = float(z["train__lr"][0])
    net = demo_net(L)
    C.CDLL(None).srand(seed)
    p = dev(net.uniform_init_host())
    net.prepare(g1, g2)
    grads = torch.empty(net.n_params, device="cuda")
    for it in range(nIter):
        _, loss = net.forward(p, tg)
        before = float(loss.sum())
        net.backward(p, grads)
        net.adam_step(p, grads, lr, len(pairs))
        _, loss = net.forward(p, tg)
        after = float(loss.sum())
        print(it, before, z["train__losses"][it, 0], after, z["train__losses"][it, 1])
        assert abs(before - z["train__losses"][it, 0]) <= TOL * max(1.0, before), it
        assert abs(after - z["train__losses"][it, 1]) <= 5 * TOL * max(1.0, after), it
    err = np.abs(p.cpu().numpy().astype(np.float64) - z["train__params"])
    print(err.max(), np.median(err))
    assert err.max() <= 0.005 * lr
    assert np.median(err) <= 1e-6
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
    p = net.load_model(os.path.join(HERE, "golden", "ccn_1d_checkpoint.dat"))
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
_PACKED = {}


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


def packed_case(gf):
    """the 70-pair batch on the device and its fp64 expectation, computed once"""
    if not _PACKED:
        from graphflow_amd import _lib
        mols, tg = packing_batch()
        g1, g2 = mols, mols[::-1]
        maxV1, maxV2, cap, L, Cn, F1, F2, decay = PACK
        params = random_params(Cn, L, [F1, F2], [maxV1, maxV2], decay, [np.ones(F1), np.ones(F2)], np.random.default_rng(118))
        out = run_pairs(PACK, g1, g2, tg, params)
        lib = _lib.load()
        phis = [(host_fields(lib, maxV1, cap, L, Cn, *a), host_fields(lib, maxV2, cap, L, Cn, *b)) for a, b in zip(g1, g2)]
        ref = ccn1d_ref.run_batch(list(zip(g1, g2)), tg, params, L, Cn, [maxV1, maxV2], decay, phis)
        _PACKED.update(g1=g1, g2=g2, tg=tg, params=params, out=out, ref=ref)
    return _PACKED


def pack_blocks():
    maxV1, maxV2, cap, L, Cn, F1, F2, decay = PACK
    return model_blocks(Cn, L, [F1, F2], [maxV1, maxV2], decay)


def test_batch_across_the_packing_boundaries(gf):
    k = packed_case(gf)
    assert len(k["g1"]) == 70 and sum(len(a) for a, _ in k["g1"]) > 64
    (pred, loss, grads), (rp, rg) = k["out"], k["ref"]
    e = blockwise(grads, rg, pack_blocks())
    print(rel_err(pred, rp), e)
    assert rel_err(pred, rp) <= TOL
    assert rel_err(loss, 0.5 * (rp - k["tg"]) ** 2) <= 2 * TOL
    assert e[0] <= TOL, e


def test_one_pair_isolated_inside_the_batch(gf):
    """With every other target equal to its prediction only pair 37 has a loss gradient: the batch gradient is then that pair's own."""
    k = packed_case(gf)
    i = 37
    t2 = k["out"][0].astype(np.float32).astype(np.float64).copy()   # (the device's own fp32 predictions: y - t is exactly 0)
    t2[i] = k["tg"][i]
    batch = run_pairs(PACK, k["g1"], k["g2"], t2, k["params"])
    alone = run_pairs(PACK, k["g1"][i:i + 1], k["g2"][i:i + 1], k["tg"][i:i + 1], k["params"])
    assert np.abs(alone[2]).max() > 0
    e = blockwise(batch[2], alone[2], pack_blocks())
    assert e[0] <= TOL, e
    assert rel_err(batch[0][i:i + 1], alone[0]) <= TOL


def test_two_runs_give_the_same_bits(gf):
    k = packed_case(gf)
    again = run_pairs(PACK, k["g1"], k["g2"], k["tg"], k["params"])
    for x, y in zip(k["out"], again):
        assert np.array_equal(x, y)


def test_parity_under_poison(gf):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): no kernel reads memory nobody wrote at
    the new widths.  The golden and packing-boundary cases in a child process."""
    env = dict(os.environ, GF_POISON="1")
    sel = "real_ccn_1d or packing_boundaries"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", sel, "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail


def test_only_the_first_order_kernels_run(gf):
    from graphflow_amd.smp import CCN1D
    k = packed_case(gf)
    L = PACK[3]
    net = CCN1D(*PACK)
    net.prepare(k["g1"], k["g2"])
    p = dev(k["params"])
    grads = torch.empty(net.n_params, device="cuda")
    net.ctx.set_timing(True)
    net.forward(p, dev(k["tg"]))
    net.backward(p, grads)
    counts = {name: n for name, (_, n) in net.ctx.timings().items()}
    net.ctx.set_timing(False)
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
