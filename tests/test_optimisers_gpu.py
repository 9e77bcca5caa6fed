"""GPU suite for graphflow_amd/csrc/smp_optimisers.hip: SGD, AdaMax, AdaDelta and the L1 / L2 regularisers, from the stand-alone operators
(gf_optimiser_step_f32, gf_regularise_f32) up to the handle entries, the fit loop and the host drop-in classes.

Yardsticks.  (1) tests/optim_ref.py with storage = float32 -- the reference's expressions in double on fp32 storage, which is what the
kernels are: parameters and every state array BIT FOR BIT, infinity_norm and beta1_t equal as doubles.  A condition, not a tolerance.
(2) tests/golden/optimisers.npz, recorded from the real fp64 classes (make_optimiser_golden.py).  The bound against it cannot be derived
in advance, so it was measured on the CPU as the deviation of the float32 restatement -- the reference plus a rounding model, not the
code under test -- from the record over Part A's six steps, largest absolute difference at the recorded indices:

    MEASURED = parameters 1.16e-07 (SGD), 1.33e-07 (AdaMax, all three cases), 1.28e-07 (AdaDelta);
               first_order 6.61e-09; E[g^2] 1.56e-09; E[dx^2] 1.23e-12; infinity_norm and beta1_t 0 (they never pass through fp32)

and the tests assert twice that.  (3) Part C: four BatchLearn steps of four real classes with each optimiser, held to
field_suite.check_momentum_trajectory's bounds (losses TOL before / 5 TOL after a step; final weights max <= 0.005 s, median <= 1e-6, s
= the rate for SGD and AdaMax, the record's largest single step for AdaDelta, which has no rate).  No test reads the reference tree."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import field_suite as kit
import optim_ref
from field_suite import dev, f64
from make_neighbourhood_golden import graph_text
from make_optimiser_golden import (A_KIND, A_LR, BLOCKS, N_BATCH, N_STEPS, REG_LAMBDA, REG_TIMES, TRAJ_KIND, TRAJ_STEPS, a_index, case_grads,
                                   offsets_of, part_a_inputs, traj_batch)
from test_optimisers import run_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "graphflow_amd", "host")
# the float32 restatement's largest deviation from the fp64 record, measured on the CPU (see above), per case and array
MEASURED = {"sgd": {"p": 1.16e-7}, "adamax": {"p": 1.33e-7, "s0": 6.61e-9}, "adamax_zero": {"p": 1.33e-7, "s0": 6.61e-9},
            "adamax_zero1": {"p": 1.33e-7, "s0": 6.61e-9}, "adadelta": {"p": 1.28e-7, "s0": 1.56e-9, "s1": 1.23e-12}}
_CACHE = {}


def golden():
    return kit.load_golden("optimisers.npz")


def restated(case):
    if case not in _CACHE:
        _CACHE[case] = run_case(case, np.float32)
    return _CACHE[case]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """bit for bit -- except that a NaN is a NaN: IEEE 754 leaves the sign and payload of the NaN an invalid operation (0 / 0) returns to
    the implementation (x86 sets the sign bit, the GPU does not), so NaN must sit in the same places, every other element has equal bits"""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def context():
    from graphflow_amd.ops import default_context
    return default_context()


def optim_config(kind, nBatch, lr, **kw):
    from graphflow_amd import _lib
    return _lib.OptimConfig(kind, nBatch, lr, kw.get("gamma", 0.0), kw.get("beta1", 0.0), kw.get("beta2", 0.0), kw.get("rho", 0.0), kw.get("epsilon", 0.0))


def device_case(case, offsets=None):
    """the six steps of a Part A case through gf_optimiser_step_f32: per step (p, s0, s1, norms, beta1_t) as host arrays"""
    ctx = context()
    params, grads, _ = part_a_inputs()
    g = case_grads(case, grads)
    off = (C.c_size_t * (len(BLOCKS) + 1))(*[int(x) for x in (offsets_of(BLOCKS) if offsets is None else offsets)])
    p, s0, s1 = dev(params), torch.zeros(params.size, device="cuda"), torch.zeros(params.size, device="cuda")
    norms = torch.zeros(len(BLOCKS), dtype=torch.float64, device="cuda")
    beta1_t = C.c_double(1.0)
    cfg = optim_config(A_KIND[case], N_BATCH, A_LR[case])
    vp = C.c_void_p
    steps = []
    for s in range(N_STEPS):
        gs = dev(g[s])
        ctx.check(ctx.lib.gf_optimiser_step_f32(ctx.handle, C.byref(cfg), vp(p.data_ptr()), vp(gs.data_ptr()), params.size, off, len(BLOCKS),
                                                vp(s0.data_ptr()), vp(s1.data_ptr()), vp(norms.data_ptr()), C.byref(beta1_t)))
        torch.cuda.synchronize()
        steps.append((p.cpu().numpy(), s0.cpu().numpy(), s1.cpu().numpy(), norms.cpu().numpy(), beta1_t.value))
    return steps


@pytest.mark.parametrize("case", list(A_KIND))
def test_operator_is_the_restatement_bit_for_bit_and_near_the_record(gf, case):
    z, idx = golden(), a_index()
    got, want = device_case(case), restated(case)
    worst = {}
    for s in range(N_STEPS):
        for k, tag in enumerate(("p", "s0", "s1")):
            same = same_bits(got[s][k], want[s][k])
            if not same:
                bad = np.flatnonzero((bits(got[s][k]) != bits(want[s][k])) & ~(np.isnan(got[s][k]) & np.isnan(want[s][k])))
                print(case, "step", s, tag, "differs at", bad[:8], got[s][k][bad[:8]], want[s][k][bad[:8]], "of", bad.size)
            assert same, (case, s, tag)
            key = "a_%s__%s" % (case, tag)
            if key in z:
                x, ref = got[s][k][idx].astype(np.float64), z[key][s]
                assert np.array_equal(np.isnan(x), np.isnan(ref)), (case, s, tag)
                ok = ~np.isnan(ref)
                worst[tag] = max(worst.get(tag, 0.0), float(np.abs(x[ok] - ref[ok]).max()))
        assert np.array_equal(got[s][3], want[s][3]) and got[s][4] == want[s][4], (case, s)
        if A_KIND[case] == optim_ref.ADAMAX:
            assert np.array_equal(got[s][3], z["a_%s__norms" % case][s]) and got[s][4] == z["a_%s__beta1_t" % case][s][0], (case, s)
    print(case, "largest deviation from the fp64 record:", worst, "measured for the restatement:", MEASURED[case])
    for tag, w in worst.items():
        assert w <= 2.0 * MEASURED[case][tag], (case, tag, w)


@pytest.mark.parametrize("case", ["adamax_zero", "adamax_zero1"])
def test_a_block_without_gradient_is_the_references_nan_and_stays_alone(gf, case):
    """0 / 0 in the block whose norm is still 0: NaN in exactly its elements (in case two on every step; in case three from step 1 on --
    the record says a NaN parameter stays NaN -- with finite state from step 2 on), and every other block bit-equal to the plain run"""
    z, idx = golden(), a_index()
    off = offsets_of(BLOCKS)
    got, plain = device_case(case), device_case("adamax")
    inside = np.zeros(int(off[-1]), dtype=bool)
    inside[off[4]:off[5]] = True
    for s in range(N_STEPS):
        p = got[s][0]
        assert np.isnan(p[inside]).all() and np.isfinite(p[~inside]).all(), (case, s)
        assert np.array_equal(np.isnan(p[idx]), np.isnan(z["a_%s__p" % case][s])), (case, s)
        assert np.array_equal(bits(p[~inside]), bits(plain[s][0][~inside])) and np.array_equal(bits(got[s][1][~inside]), bits(plain[s][1][~inside]))
        assert np.isfinite(got[s][1]).all() and np.isfinite(got[s][3]).all()
        assert np.array_equal(np.delete(got[s][3], 4), np.delete(plain[s][3], 4))
        assert (got[s][3][4] == 0.0) == (case == "adamax_zero" or s == 0)


@pytest.mark.parametrize("norm", [1, 2])
def test_regulariser_operator(gf, norm):
    z, idx = golden(), a_index()
    ctx = context()
    _, grads, reg = part_a_inputs()
    n = reg.shape[1]
    vp = C.c_void_p
    for s in range(N_STEPS):
        p, g = dev(reg[s]), dev(grads[s])
        value, again = C.c_double(0.0), C.c_double(0.0)
        ctx.check(ctx.lib.gf_regularise_f32(ctx.handle, vp(p.data_ptr()), vp(g.data_ptr()), n, norm, REG_LAMBDA, REG_TIMES, C.byref(value)))
        want_value, want_g = optim_ref.regularise(norm, reg[s].astype(np.float32), grads[s].astype(np.float32), REG_LAMBDA, REG_TIMES, np.float32)
        assert np.array_equal(bits(g.cpu().numpy()), bits(want_g)), (norm, s)
        ref = z["a_l%d__value" % norm][s]
        print(norm, s, value.value, ref, abs(value.value - ref) / ref)
        assert abs(value.value - ref) <= n * 2.0 ** -52 * ref   # (every term is non-negative: the bound of ANY summation order)
        g2 = dev(grads[s])
        ctx.check(ctx.lib.gf_regularise_f32(ctx.handle, vp(p.data_ptr()), vp(g2.data_ptr()), n, norm, REG_LAMBDA, REG_TIMES, C.byref(again)))
        assert again.value == value.value and torch.equal(g, g2)
        assert np.all(np.abs(f64(g)[idx] - z["a_l%d__g" % norm][s]) <= 2.0 ** -23 * np.maximum(np.abs(z["a_l%d__g" % norm][s]), np.abs(grads[s][idx])))
    assert ctx.lib.gf_regularise_f32(ctx.handle, vp(p.data_ptr()), vp(g.data_ptr()), n, 3, 0.1, 1, C.byref(value)) == 1   # GF_ERR_INVALID


def test_operator_refusals(gf):
    ctx = context()
    p, g, s0, s1 = (torch.ones(8, device="cuda") for _ in range(4))
    norms = torch.zeros(2, dtype=torch.float64, device="cuda")
    b = C.c_double(1.0)
    vp = C.c_void_p
    call = lambda cfg, off, nb: ctx.lib.gf_optimiser_step_f32(ctx.handle, C.byref(cfg) if cfg else None, vp(p.data_ptr()), vp(g.data_ptr()), 8, off, nb,  # noqa: E731
                                                              vp(s0.data_ptr()), vp(s1.data_ptr()), vp(norms.data_ptr()), C.byref(b))
    good = (C.c_size_t * 3)(0, 3, 8)
    assert call(optim_config(3, 4, 0.1), good, 2) == 0
    for kind in (0, 1, 5, -1):
        assert call(optim_config(kind, 4, 0.1), good, 2) == 1
    assert call(optim_config(3, 0, 0.1), good, 2) == 1 and call(None, good, 2) == 1
    for off in ((0, 3, 7), (1, 3, 8), (0, 8, 8), (0, 9, 8)):   # not to n, not from 0, an empty block, descending
        assert call(optim_config(3, 4, 0.1), (C.c_size_t * 3)(*off), 2) == 1
    assert call(optim_config(3, 4, 0.1), None, 2) == 1 and call(optim_config(3, 4, 0.1), good, 0) == 1
    assert call(optim_config(2, 4, 0.1), None, 0) == 0   # SGD reads no table


# ---- the handle entries ----------------------------------------------------------------------------------------------------------------
def make_net(name):
    from graphflow_amd import smp as gfa
    if name == "SMP_omega":
        net = gfa.SMPOmega(2, 4, 4, 1, 6)
    elif name == "GCN_1D":
        net = gfa.SMPNeighbourhood("gcn_1d", 2, 5, 4, 1, 6, 1)
    elif name == "SMP_2D_ver6_classification":
        net = gfa.SMPClassifier(3, 2, 4, 4, 1, 6)
    else:
        net = gfa.SMPModel(2, 4, 6, 4)
        return net, net.uniform_init_host
    return net, net.uniform_init


def start(name, seed=23):
    net, init = make_net(name)
    C.CDLL(None).srand(seed)
    p = dev(init())
    x, t = traj_batch(name)
    net.prepare(x)
    return net, p, dev(np.array(t)), len(x)


def three_steps(name, step):
    net, p, tg, n = start(name)
    g = torch.empty_like(p)
    for _ in range(3):
        net.forward(p, tg)
        net.backward(p, g)
        step(net, p, g, n)
    net.close()
    return p


@pytest.mark.parametrize("name", ["SMP_omega", "SMP_omega_physics"])
def test_kinds_0_and_1_are_the_old_entries_bit_for_bit(gf, name):
    new0 = three_steps(name, lambda net, p, g, n: net.optimiser_step(p, g, "adam", 0.01, n))
    if name == "SMP_omega":
        old0 = three_steps(name, lambda net, p, g, n: net.adam_step(p, g, 0.01, n))
        old1 = three_steps(name, lambda net, p, g, n: net.momentum_step(p, g, 0.01, n, 0.8))
        new1 = three_steps(name, lambda net, p, g, n: net.optimiser_step(p, g, "momentum", 0.01, n, gamma=0.8))
        assert torch.equal(new1, old1) and not torch.equal(new1, new0)
    else:   # gf_smp_model_adam_step works on the handle-owned model
        def owned(net, p, g, n):
            host, hg = p.cpu().numpy(), g.cpu().numpy()
            fp = C.POINTER(C.c_float)
            net.ctx.check(net.lib.gf_smp_model_parameters_upload(net.handle, host.ctypes.data_as(fp)))
            net.ctx.check(net.lib.gf_smp_model_backward(net.handle, None, None, 0))   # the same gradient into the handle's own buffer
            own_g = np.empty_like(hg)
            net.ctx.check(net.lib.gf_smp_model_adam_step(net.handle, 0.01, n))
            net.ctx.check(net.lib.gf_smp_model_parameters_download(net.handle, host.ctypes.data_as(fp), own_g.ctypes.data_as(fp)))
            assert np.array_equal(own_g, hg)
            p.copy_(torch.as_tensor(host))
        old0 = three_steps(name, owned)
        # Momentum on the composite handle has no older entry: the kernel of gf_smp_momentum_step, restated in double (test_fit_gpu's bound)
        net, p, tg, n = start(name)
        g, m = torch.empty_like(p), torch.zeros_like(p)
        for _ in range(3):
            net.forward(p, tg)
            net.backward(p, g)
            md = 0.8 * m.double() + 0.01 * g.double() * (1.0 / n)
            want = p.double() - md
            m = md.float()
            net.optimiser_step(p, g, "momentum", 0.01, n, gamma=0.8)
            step = float(md.abs().max())
            assert float((p.double() - want).abs().max()) <= 1e-6 * step + 1e-7 * float(want.abs().max())
            assert step > 0.0
        net.close()
    assert torch.equal(new0, old0)


def test_kind_changes_need_a_reset(gf):
    net, p, tg, n = start("GCN_1D")
    g = torch.empty_like(p)
    net.forward(p, tg)
    net.backward(p, g)
    p0 = p.clone()
    net.optimiser_step(p, g, "adadelta", 0.0, n)
    first = p.clone()
    for other in ("adam", "momentum", "sgd", "adamax"):
        with pytest.raises(gf.GraphFlowHipError):
            net.optimiser_step(p, g, other, 0.01, n)
    assert torch.equal(p, first)
    net.momentum_step(p, g, 0.01, n, 0.9)   # the old entries never refuse; they record their kind
    with pytest.raises(gf.GraphFlowHipError):
        net.optimiser_step(p, g, "adadelta", 0.0, n)
    net.adam_reset()
    p.copy_(p0)
    net.optimiser_step(p, g, "adadelta", 0.0, n)   # accepted, and from zero state: the first step again
    assert torch.equal(p, first)
    net.adam_reset()
    net.optimiser_step(p, g, "adamax", 0.01, n)
    net.adam_reset()
    p.copy_(p0)
    net.optimiser_step(p, g, "adamax", 0.01, n)    # beta1_t and the norms start over too
    again = p.clone()
    p.copy_(p0)
    net.adam_reset()
    net.optimiser_step(p, g, "adamax", 0.01, n)
    assert torch.equal(p, again)
    for bad in (dict(kind=7, nBatch=n), dict(kind="sgd", nBatch=0), dict(kind=-1, nBatch=n)):
        with pytest.raises(gf.GraphFlowHipError):
            net.optimiser_step(p, g, bad["kind"], 0.01, bad["nBatch"])
    assert net.lib.gf_smp_optimiser_step(net.handle, C.c_void_p(p.data_ptr()), C.c_void_p(g.data_ptr()), None) == 1
    net.close()


@pytest.mark.parametrize("name", ["GCN_1D", "SMP_omega_physics"])
@pytest.mark.parametrize("opt", list(TRAJ_KIND))
def test_handle_step_is_the_operator_on_the_handles_blocks(gf, name, opt):
    ctx = context()
    net, p, tg, n = start(name)
    g = torch.empty_like(p)
    blocks = net.param_blocks()
    assert blocks[-1] == net.n_params
    off = (C.c_size_t * len(blocks))(*blocks)
    q, s0, s1 = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    norms, beta1_t = torch.zeros(len(blocks) - 1, dtype=torch.float64, device="cuda"), C.c_double(1.0)
    vp = C.c_void_p
    for _ in range(3):
        net.forward(p, tg)
        net.backward(p, g)
        net.optimiser_step(p, g, opt, 0.01, n)
        cfg = optim_config(TRAJ_KIND[opt], n, 0.01)
        ctx.check(ctx.lib.gf_optimiser_step_f32(ctx.handle, C.byref(cfg), vp(q.data_ptr()), vp(g.data_ptr()), net.n_params, off, len(blocks) - 1,
                                                vp(s0.data_ptr()), vp(s1.data_ptr()), vp(norms.data_ptr()), C.byref(beta1_t)))
        assert torch.equal(p, q) and bool(torch.isfinite(p).all())
    net.close()


def test_handle_regulariser_is_the_operator(gf):
    ctx = context()
    for name in ("GCN_1D", "SMP_omega_physics"):
        net, p, tg, n = start(name)
        g = torch.empty_like(p)
        net.forward(p, tg)
        net.backward(p, g)
        g2 = g.clone()
        want_value, want_g = optim_ref.regularise(1, p.cpu().numpy(), g.cpu().numpy(), 0.02, n, np.float32)
        value = net.regularise(p, g, 1, 0.02, n)
        v2 = C.c_double(0.0)
        ctx.check(ctx.lib.gf_regularise_f32(ctx.handle, C.c_void_p(p.data_ptr()), C.c_void_p(g2.data_ptr()), net.n_params, 1, 0.02, n, C.byref(v2)))
        assert value == v2.value and torch.equal(g, g2) and np.array_equal(bits(g.cpu().numpy()), bits(want_g))
        assert abs(value - want_value) <= net.n_params * 2.0 ** -52 * want_value and value > 0.0
        net.close()


# ---- Part C: the real classes' trajectories ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["SMP_omega", "GCN_1D", "SMP_2D_ver6_classification", "SMP_omega_physics"])
@pytest.mark.parametrize("opt", list(TRAJ_KIND))
def test_trajectories_of_the_real_classes(gf, name, opt):
    z = dict(golden())
    prefix = "c_%s__%s__" % (name, opt)
    x, t = traj_batch(name)
    z[prefix + "targets"] = np.array(t)
    lr, n = float(z[prefix + "lr"][0]), len(x)
    scale = float(z[prefix + "step_max"][0]) if opt == "adadelta" else lr
    net, init = make_net(name)
    kit.check_momentum_trajectory(net, lambda p, g: net.optimiser_step(p, g, opt, lr, n), z, prefix, x, int(z[prefix + "seed"][0]), TRAJ_STEPS, scale,
                                  init=init, show=name + " " + opt + ": final weights max %s median %s")
    net.close()


# ---- fit with optimiser 2, 3, 4 is the hand-rolled loop ----------------------------------------------------------------------------------
def host_sum(loss):
    total = 0.0
    for v in loss.cpu().numpy():
        total += float(v)
    return total


@pytest.mark.parametrize("name", ["GCN_1D", "SMP_omega_physics"])
@pytest.mark.parametrize("opt,lr", [("sgd", 2.0), ("adamax", 0.5), ("adadelta", 0.1)])
def test_fit_is_the_hand_rolled_loop_bit_for_bit(gf, name, opt, lr):
    """gf::fit_run (kind 0) written out from forward / backward / optimiser_step / torch copies as the cache, at rates large enough that
    steps are kept AND restored where the optimiser reads the rate: the same calls in the same order, hence the same bits"""
    nIter = 10
    net, p, tg, n = start(name)
    g = torch.empty_like(p)
    rep, dec = net.fit(p, g, tg, nIter, lr, 0.0, 0, optimiser=opt)
    net.close()
    net, q, tg, n = start(name)
    g2 = torch.empty_like(q)
    cache = q.clone()
    first = second = host_sum(net.forward(q, tg)[1])
    dec2, rate, stale = [], lr, False
    for _ in range(nIter):
        if stale:
            net.forward(q, tg)
        stale = False
        net.backward(q, g2)
        net.optimiser_step(q, g2, opt, rate, n)
        loss = host_sum(net.forward(q, tg)[1])
        if loss > second:
            q.copy_(cache)
            stale = True
            rate *= 0.5
            dec2.append(3 if rate < 1e-6 else 2)
            if dec2[-1] == 3:
                break
        else:
            second = loss
            cache.copy_(q)
            dec2.append(1)
    net.close()
    print(name, opt, rep, dec)
    assert dec == dec2 and [float(rep[k]).hex() for k in ("first", "second", "learning_rate")] == [float(v).hex() for v in (first, second, rate)]
    assert bool(torch.isfinite(p).all()) and torch.equal(p, q) and torch.equal(g, g2)
    assert 1 in dec


def test_fit_refuses_a_kind_change_and_unknown_optimisers(gf):
    from graphflow_amd import _lib
    net, p, tg, n = start("GCN_1D")
    g = torch.empty_like(p)
    net.fit(p, g, tg, 1, 0.01, optimiser="momentum")
    with pytest.raises(gf.GraphFlowHipError):
        net.fit(p, g, tg, 1, 0.01, optimiser="sgd")        # the handle's state is Momentum's
    net.fit(p, g, tg, 1, 0.01, optimiser="adam")           # (the old kinds never refuse)
    net.adam_reset()
    net.fit(p, g, tg, 1, 0.01, optimiser="sgd")
    with pytest.raises(ValueError):
        net.fit(p, g, tg, 1, 0.01, optimiser="rmsprop")
    cfg, rep = _lib.FitConfig(0, 5, 1, 0.1, 0.0, 0.9), _lib.FitReport()
    vp = C.c_void_p
    assert net.lib.gf_smp_fit(net.handle, vp(p.data_ptr()), vp(g.data_ptr()), vp(tg.data_ptr()), C.byref(cfg), C.byref(rep), None) == _lib.GF_ERR_INVALID
    net.close()


# ---- the host drop-in classes ------------------------------------------------------------------------------------------------------------
def test_use_optimiser_of_the_host_classes(gf, tmp_path):
    """tests/cpp/test_optimisers_hip.cpp: two classes of the shared skeleton's kind and one composite, use_optimiser, BatchLearn -- the
    Part C record within the trajectory bounds, and the constructor's weights bit for bit"""
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine: the host C++ test program cannot be compiled")
    exe = str(tmp_path / "test_optimisers_hip")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_optimisers_hip.cpp"), "-L" + os.path.join(ROOT, "graphflow_amd", "csrc"), "-lgf_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "graphflow_amd", "csrc"), "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    z = golden()
    cases = [("GCN_1D", "adamax"), ("SMP_omega_physics", "adadelta"), ("SMP_omega", "sgd")]
    text = ""
    for name, opt in cases:
        p_ = "c_%s__%s__" % (name, opt)
        x, t = traj_batch(name)
        text += "case %s %s %d %d %.17g %d %d 4\n" % (name + "-" + opt, name, int(z[p_ + "seed"][0]), TRAJ_KIND[opt], float(z[p_ + "lr"][0]), TRAJ_STEPS, len(x))
        text += "".join(graph_text(a, f) for a, f in x) + " ".join("%.17g" % v for v in t) + "\n"
    (tmp_path / "cases.txt").write_text(text)
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), r.stdout[-1500:] + r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stdout.split("\n"):
        tok = line.split()
        if not tok or tok[0] == "DONE":
            continue
        if tok[0] == "case":
            cur = out.setdefault(tok[1], {"pair": []})
        elif tok[0] == "pair":
            cur["pair"].append([float.fromhex(v) for v in tok[1:]])
        else:
            cur[tok[0]] = np.array([float.fromhex(v) for v in tok[1:]])
    for name, opt in cases:
        p_, got = "c_%s__%s__" % (name, opt), out[name + "-" + opt]
        assert np.array_equal(got["params0"], z[p_ + "params0"].astype(np.float32).astype(np.float64))
        scale = float(z[p_ + "step_max"][0]) if opt == "adadelta" else float(z[p_ + "lr"][0])
        for (before, after), (b, a) in zip(got["pair"], z[p_ + "losses"]):
            assert abs(before - b) <= kit.TOL * max(1.0, abs(b)) and abs(after - a) <= 5 * kit.TOL * max(1.0, abs(a)), (name, opt)
        err = np.abs(got["params"] - z[p_ + "params"])
        print(name, opt, "final weights: max %.3g median %.3g (scale %.3g)" % (err.max(), np.median(err), scale))
        assert len(got["pair"]) == TRAJ_STEPS and err.max() <= 0.005 * scale and np.median(err) <= 1e-6
