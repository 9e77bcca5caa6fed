"""GPU suite for the iterative training calls of the C ABI -- gf_smp_fit / gf_smp_model_fit (the classes' BatchLearn with nIterations and
Learn), gf_smp_parameters_snapshot / _rollback, gf_smp_forward_host_samples, gf_smp_gram_host -- through SMPOmega.fit / SMPModel.fit.

Two yardsticks.  (1) tests/golden/smp_iterative.npz, recorded from the real classes by tests/golden/make_iterative_golden.py: the decision
of every iteration and the iteration count exactly (every recorded comparison has a gap of 1e-3, twenty times what an fp32 loss may be
off), the returned pair within field_suite's bounds before / after a step (TOL, 5 TOL), the final weights within
check_momentum_trajectory's (max <= 0.005 lr, median <= 1e-6).  (2) Without any golden: the same loop written out here from the calls
that existed before -- forward, backward, the optimiser step, a host sum in double, torch copies as the cache -- gives the same losses,
decisions and final weights BIT FOR BIT, because the calls, their order and their arguments are the same and every one is deterministic.
The one step without an earlier call is Adam's Learn(alpha) overload (kind 1 on an Adam class): restated in torch in double, compared at
1e-6 of the step.  All on the four toy molecules (3 to 6 atoms) at 4 / 5 channels.  No test reads the reference tree."""
import ctypes as C

import numpy as np
import pytest

import field_suite as kit
from field_suite import TOL, dev, f64
from make_iterative_golden import ACCEPT, CLASSES, LEAVE, REJECT, REJECT_LEAVE, batch_of
from test_fit_policy import RUNS, recorded_runs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ADAM = ("SMP_omega", "SMP_omega_physics")


def golden():
    return kit.load_golden("smp_iterative.npz")


def all_runs():
    return recorded_runs(golden())


def make_net(name):
    """(net, init): the Python wrapper of the class at the generator's constructor arguments, and what draws its initial weights"""
    from graphflow_amd import smp as gfa
    c = CLASSES[name][1]
    if name == "SMP_omega":
        net = gfa.SMPOmega(c[2], c[3], c[4], c[5], c[1])
    elif name == "GCN_1D":
        net = gfa.SMPNeighbourhood("gcn_1d", c[0], c[3], c[2], c[4], c[1], c[5])
    elif name == "SMP_2D_ver6_classification":
        net = gfa.SMPClassifier(c[0], c[2], c[3], c[4], c[5], c[1])
    elif name == "SMP_omega_physics":
        net = gfa.SMPModel(c[2], c[3], c[1], c[4])
        return net, net.uniform_init_host
    elif name == "GCN_1D_Kernel":
        net = gfa.SMPKernelPairs("gcn_1d_kernel", c[0], c[1], c[2], c[3], c[4], c[5])
    else:
        net = gfa.GCA1D(c[0], c[1], c[2], c[3], c[4], c[5])
    return net, net.uniform_init


def start(name, kind, z, seed=None):
    """the class as the generator built it: srand(seed), the constructor's weights, the run's batch prepared"""
    net, init = make_net(name)
    C.CDLL(None).srand(int(z[name + "__batch_mixed__seed"][0]) if seed is None else seed)
    p = dev(init())
    x, y, t = batch_of(name, kind)
    if y:
        net.prepare(x, y)
    else:
        net.prepare(x)
    return net, p, (dev(np.array(t)) if t else None), len(x)


def fit(net, name, p, g, tg, kind, nIter, lr, eps, gamma):
    if name == "SMP_omega_physics":
        return net.fit(p, g, tg, nIter, lr, eps, kind)
    return net.fit(p, g, tg, nIter, lr, eps, kind, "adam" if name in ADAM else "momentum", gamma)


def run_config(z, name, run):
    p_ = "%s__%s__" % (name, run)
    return p_, int(z[p_ + "cfg"][0]), int(z[p_ + "cfg"][1]), float(z[p_ + "lr"][0]), float(z[p_ + "eps"][0]), float(z[p_ + "momentum"][0])


@pytest.mark.parametrize("name,run", all_runs())
def test_fit_reproduces_the_real_classes(gf, name, run):
    z = golden()
    p_, kind, nIter, lr, eps, gamma = run_config(z, name, run)
    net, p, tg, n = start(name, kind, z, int(z[p_ + "seed"][0]))
    assert np.array_equal(p.cpu().numpy(), z[p_ + "params0"].astype(np.float32))
    g = torch.empty_like(p)
    rep, dec = fit(net, name, p, g, tg, kind, nIter, lr, eps, gamma)
    want, pair = list(z[p_ + "decisions"]), z[p_ + "pair"]
    err = np.abs(f64(p) - z[p_ + "params"])
    print(p_, rep, dec, pair, "final weights: max %.3g median %.3g" % (err.max(), np.median(err)))
    assert dec == want and rep["iterations"] == len(want)
    assert rep["accepted"] == want.count(ACCEPT) and rep["rejected"] == want.count(REJECT) + want.count(REJECT_LEAVE)
    assert rep["left_early"] == int(run == "learn_immediate" or (len(want) > 0 and want[-1] in (REJECT_LEAVE, LEAVE)))
    assert rep["learning_rate"] == z[p_ + "final_lr"][0]
    assert abs(rep["first"] - pair[0]) <= TOL * max(1.0, abs(pair[0]))
    assert abs(rep["second"] - pair[1]) <= 5 * TOL * max(1.0, abs(pair[1]))
    assert err.max() <= 0.005 * lr
    assert np.median(err) <= 1e-6
    net.close()


def host_sum(loss):
    """the classes' `total += loss[i]`: doubles, ascending"""
    total = 0.0
    for x in loss.cpu().numpy():
        total += float(x)
    return total


def hand_rolled(net, name, p, g, tg, n, kind, nIter, lr, eps, gamma):
    """gf::fit_run from the calls that were there before it; returns (losses, decisions, first, second, rate)"""
    adam = name in ADAM
    moments = [torch.zeros_like(p), torch.zeros_like(p), 0]   # (Adam's Learn(alpha), restated: the one step without an earlier call)

    def forward():
        if name == "GCA_1D":
            return host_sum(net.forward(p))
        return host_sum(net.forward(p, tg)[1])

    def step(rate):
        net.backward(p, g)
        if not adam:
            net.momentum_step(p, g, rate, 1 if kind else n, gamma)
        elif kind == 0:
            net.adam_step(p, g, rate, n)
        else:
            m, v, t = moments
            moments[2] = t = t + 1
            gd = g.double()
            md = 0.9 * m.double() + (1.0 - 0.9) * gd   # (the update reads the moments before they are rounded for storage, as the kernel does)
            vd = 0.999 * v.double() + (1.0 - 0.999) * gd * gd
            m.copy_(md.float())
            v.copy_(vd.float())
            p.copy_((p.double() - rate * (md / (1.0 - 0.9 ** t)) / (torch.sqrt(vd / (1.0 - 0.999 ** t)) + 1e-8)).float())

    cache = p.clone()
    first = second = forward()
    losses, dec, stale = [], [], False
    if not (kind == 1 and first < eps):
        for _ in range(nIter):
            if stale:
                forward()
            stale = False
            step(lr)
            loss = forward()
            losses.append(loss)
            if kind == 1 and loss < eps:
                dec.append(LEAVE)
                break
            if (loss > second) if kind == 0 else (loss >= second):
                p.copy_(cache)
                stale = True
                lr = lr * 0.5 if kind == 0 else max(lr * 0.5, 1e-6)
                dec.append(REJECT_LEAVE if kind == 0 and lr < 1e-6 else REJECT)
                if dec[-1] == REJECT_LEAVE:
                    break
            else:
                second = loss
                cache.copy_(p)
                dec.append(ACCEPT)
    if stale:
        forward()
    return losses, dec, first, second, lr


@pytest.mark.parametrize("name,run", all_runs())
def test_fit_is_the_hand_rolled_loop_bit_for_bit(gf, name, run):
    z = golden()
    p_, kind, nIter, lr, eps, gamma = run_config(z, name, run)
    net, p, tg, n = start(name, kind, z, int(z[p_ + "seed"][0]))
    g = torch.empty_like(p)
    rep, dec = fit(net, name, p, g, tg, kind, nIter, lr, eps, gamma)
    net.close()
    net2, q, tg2, _ = start(name, kind, z, int(z[p_ + "seed"][0]))
    g2 = torch.empty_like(q)
    losses, dec2, first, second, rate = hand_rolled(net2, name, q, g2, tg2, n, kind, nIter, lr, eps, gamma)
    net2.close()
    print(p_, rep, dec, losses)
    assert dec == dec2 and rep["learning_rate"] == rate
    if name in ADAM and kind == 1 and dec:
        step = np.abs(f64(p) - z[p_ + "params0"]).max() + lr
        assert abs(rep["first"] - first) == 0.0 and abs(rep["second"] - second) <= 1e-5 * max(1.0, abs(second))
        assert np.abs(f64(p) - f64(q)).max() <= 1e-6 * step
        return
    assert rep["first"] == first and rep["second"] == second
    assert torch.equal(p, q) and (not dec or torch.equal(g, g2))


def momentum_step_once(net, p, g, tg, lr, n, gamma):
    net.forward(p, tg)
    net.backward(p, g)
    net.momentum_step(p, g, lr, n, gamma)


def test_snapshot_and_rollback_copy_values_and_leave_the_optimiser_alone(gf):
    z = golden()
    lr, gamma = 0.05, 0.9
    net, p, tg, n = start("GCN_1D", 0, z)
    g = torch.empty_like(p)
    p0 = p.clone()
    with pytest.raises(gf.GraphFlowHipError):
        net.parameters_rollback(p)   # nothing cached yet
    net.parameters_snapshot(p)
    momentum_step_once(net, p, g, tg, lr, n, gamma)   # velocity v1 = lr g0 / n
    p1 = p.clone()
    assert not torch.equal(p1, p0)
    p.add_(1.0)
    net.parameters_rollback(p)
    assert torch.equal(p, p0)
    momentum_step_once(net, p, g, tg, lr, n, gamma)   # the same gradient g0: the step is gamma v1 + lr g0 / n
    p2 = p.clone()
    net.close()
    fresh, q, tg2, _ = start("GCN_1D", 0, z)
    momentum_step_once(fresh, q, torch.empty_like(q), tg2, lr, n, gamma)
    fresh.close()
    assert torch.equal(q, p1)   # (a first step is a first step)
    v1 = f64(p0) - f64(p1)
    want = f64(p0) - (1.0 + gamma) * v1
    assert np.abs(v1).max() > 1e-4
    assert np.abs(f64(p2) - want).max() <= 1e-6 * np.abs(v1).max() + 2e-7 * np.abs(want).max()
    assert np.abs(f64(p2) - f64(q)).max() >= 0.5 * gamma * np.abs(v1).max()


def test_adam_state_survives_a_rollback(gf):
    """snapshot / rollback copy values only: Adam's moments and its element counter stay.  A step, a rollback, a second step from the same
    weights and gradient: the second step is the one Adam takes with the first step's moments and the bias-correction powers continued
    (element i of the second call: beta^(n + i + 1)), restated here in double; a fresh handle's first step is a different one."""
    z = golden()
    lr = 0.01
    net, p, tg, n = start("SMP_omega", 0, z)
    g = torch.empty_like(p)
    p0 = p.clone()
    net.parameters_snapshot(p)
    net.forward(p, tg)
    net.backward(p, g)
    net.adam_step(p, g, lr, n)
    p1 = p.clone()
    net.parameters_rollback(p)
    assert torch.equal(p, p0)
    net.forward(p, tg)
    net.backward(p, g)
    net.adam_step(p, g, lr, n)
    net.close()
    gd = f64(g) / n
    m1, v1 = np.float32(0.1 * gd).astype(np.float64), np.float32(0.001 * gd * gd).astype(np.float64)   # (stored as fp32 between the calls)
    m2, v2 = 0.9 * m1 + 0.1 * gd, 0.999 * v1 + 0.001 * gd * gd
    t = net.n_params + np.arange(net.n_params) + 1.0
    want = f64(p0) - lr * (m2 / (1.0 - 0.9 ** t)) / (np.sqrt(v2 / (1.0 - 0.999 ** t)) + 1e-8)
    step = np.abs(want - f64(p0)).max()
    assert step > 1e-4
    assert np.abs(f64(p) - want).max() <= 1e-5 * step + 1e-7 * np.abs(want).max()
    assert np.abs(f64(p) - f64(p1)).max() >= 0.05 * step   # not a first step: the moments and the counter were kept


@pytest.mark.parametrize("n", [1, 5, 257, 2048, 2049, 5000])
def test_loss_sum_adds_in_order_in_double(gf, n):
    """the loop's sum kernel on its own (gf_smp_loss_sum_f32): every lane stages, more than one chunk of 2048, and values spread over 40
    binary orders, where the order of the additions shows in the last bits: the bits of the host loop"""
    from graphflow_amd.ops import default_context
    ctx = default_context()
    rng = np.random.default_rng(n)
    loss = (rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(-20, 21, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    total = 0.0
    for x in loss:
        total += float(x)
    out = C.c_double(float("nan"))
    ctx.check(ctx.lib.gf_smp_loss_sum_f32(ctx.handle, C.c_void_p(dev(loss).data_ptr()), n, C.byref(out)))
    assert out.value == total


def test_gram_host_reuses_its_staging_block(gf):
    z = golden()
    net, p, _, n = start("GCA_1D", 0, z)
    own_model(net, p)
    net.forward(p)
    size = sum(len(a) ** 2 for a, _ in batch_of("GCA_1D", 0)[0])
    out = np.empty(size)
    net.ctx.check(net.lib.gf_smp_gram_host(net.handle, dptr(out)))
    held = net.device_bytes()
    for _ in range(3):
        net.ctx.check(net.lib.gf_smp_gram_host(net.handle, dptr(out)))
    assert net.device_bytes() == held
    net.close()


def test_model_snapshot_and_rollback(gf):
    z = golden()
    net, p, tg, n = start("SMP_omega_physics", 0, z)
    lib, vp = net.lib, C.c_void_p
    assert lib.gf_smp_model_parameters_rollback(net.handle, vp(p.data_ptr())) == 1   # GF_ERR_INVALID: nothing cached yet
    net.ctx.check(lib.gf_smp_model_parameters_snapshot(net.handle, vp(p.data_ptr())))
    p0 = p.clone()
    p.mul_(3.0).add_(1.0)
    net.ctx.check(lib.gf_smp_model_parameters_rollback(net.handle, vp(p.data_ptr())))
    torch.cuda.synchronize()
    assert torch.equal(p, p0)
    net.close()


def own_model(net, p):
    host = p.cpu().numpy()
    net.ctx.check(net.lib.gf_smp_parameters_upload(net.handle, host.ctypes.data_as(C.POINTER(C.c_float))))


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_host_samples_on_pair_gram_and_covariant_handles(gf):
    """gf_smp_forward_host_samples / gf_smp_gram_host are gf_smp_forward / gf_smp_gram converted to double; gf_smp_forward_host still refuses"""
    from graphflow_amd import _lib, smp as gfa
    z = golden()
    # pairs
    net, p, tg, n = start("GCN_1D_Kernel", 0, z)
    own_model(net, p)
    pred, loss, feat = (f64(t) for t in net.forward(p, tg))
    t64 = f64(tg)
    y, l, f = np.full(n, np.nan), np.full(n, np.nan), np.full(feat.shape, np.nan)
    assert net.lib.gf_smp_forward_host(net.handle, dptr(t64), dptr(y), dptr(l), None) == _lib.GF_ERR_UNSUPPORTED
    net.ctx.check(net.lib.gf_smp_forward_host_samples(net.handle, dptr(t64), dptr(y), dptr(l), dptr(f)))
    assert np.array_equal(y, pred) and np.array_equal(l, loss) and np.array_equal(f, feat) and feat.shape == (n, 10)
    net.close()
    # Gram
    net, p, _, n = start("GCA_1D", 0, z)
    own_model(net, p)
    loss = f64(net.forward(p))
    grams = np.concatenate([gm.astype(np.float64).ravel() for gm in net.gram()])
    l, gh = np.full(n, np.nan), np.full(grams.size, np.nan)
    assert net.lib.gf_smp_forward_host(net.handle, None, None, dptr(l), None) == _lib.GF_ERR_UNSUPPORTED
    assert net.lib.gf_smp_forward_host_samples(net.handle, None, dptr(l), dptr(l), None) == _lib.GF_ERR_INVALID   # no predict on a Gram handle
    net.ctx.check(net.lib.gf_smp_forward_host_samples(net.handle, None, None, dptr(l), None))
    net.ctx.check(net.lib.gf_smp_gram_host(net.handle, dptr(gh)))
    assert np.array_equal(l, loss) and np.array_equal(gh, grams)
    net.close()
    # covariant
    for cls in (gfa.CGCN1D, gfa.CGCN2D):
        net = cls(2, 6, 4, 1)
        C.CDLL(None).srand(5)
        p = dev(net.uniform_init())
        x, _, t = batch_of("GCN_1D", 0)
        net.prepare(x)
        own_model(net, p)
        tg = dev(np.array(t))
        pred, loss, feat = (f64(t_) for t_ in net.forward(p, tg))
        y, l, f = np.full(len(x), np.nan), np.full(len(x), np.nan), np.full(feat.shape, np.nan)
        assert net.lib.gf_smp_forward_host(net.handle, None, dptr(y), None, None) == _lib.GF_ERR_UNSUPPORTED
        assert net.lib.gf_smp_gram_host(net.handle, dptr(y)) == _lib.GF_ERR_UNSUPPORTED
        net.ctx.check(net.lib.gf_smp_forward_host_samples(net.handle, dptr(np.array(t)), dptr(y), dptr(l), dptr(f)))
        assert np.array_equal(y, pred) and np.array_equal(l, loss) and np.array_equal(f, feat) and feat.shape == (len(x), 6)
        net.close()


def test_fit_refuses_what_it_cannot_run(gf):
    z = golden()
    net, p, tg, n = start("GCN_1D", 0, z)
    g = torch.empty_like(p)
    with pytest.raises(gf.GraphFlowHipError):
        net.fit(p, g, tg, 3, 0.1, kind=1, optimiser="momentum")   # Learn on a batch of four
    with pytest.raises(gf.GraphFlowHipError):
        net.fit(p, g, tg, -1, 0.1, optimiser="momentum")
    with pytest.raises(gf.GraphFlowHipError):
        net.fit(p, g, None, 3, 0.1, optimiser="momentum")      # a regression handle needs targets
    rep, dec = net.fit(p, g, tg, 0, 0.1, optimiser="momentum")   # no iterations: the loss alone
    assert dec == [] and rep["first"] == rep["second"] == host_sum(net.forward(p, tg)[1]) and not rep["left_early"]
    net.close()
    net, p, tg, n = start("SMP_omega_physics", 0, z)
    from graphflow_amd import _lib
    cfg, rep = _lib.FitConfig(0, 1, 2, 0.1, 0.0, 0.9), _lib.FitReport()
    vp = C.c_void_p
    g = torch.empty_like(p)
    assert net.lib.gf_smp_model_fit(net.handle, vp(p.data_ptr()), vp(g.data_ptr()), vp(tg.data_ptr()), C.byref(cfg), C.byref(rep), None) == _lib.GF_ERR_UNSUPPORTED
    net.close()


def test_one_fit_under_poison(gf):
    kit.run_under_poison(__file__, "hand_rolled and GCN_1D-batch_mixed")
