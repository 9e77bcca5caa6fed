"""Data-parallel entry points of the C ABI (gf_dist_*) on one GPU: RCCL with a one-rank communicator.  The two-rank logic
(sharding, the launcher, the single gradient exchange) is covered on CPU by tests/test_dist_cpu.py; a communicator with more
than one rank needs more than one GPU (RCCL refuses two ranks on one device)."""
import numpy as np
import pytest

from inputs import smp_params, synthetic_molecule

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def test_one_rank_collectives_through_rccl(gf):
    ctx = gf.Context(0)
    assert (ctx.dist_rank, ctx.dist_world) == (0, 1)
    t = torch.arange(1000, dtype=torch.float32, device="cuda")
    with pytest.raises(gf.GraphFlowHipError):
        ctx.allreduce_sum_(t)                      # no communicator yet: refused, not silently skipped
    uid = ctx.dist_unique_id()
    assert len(uid) == 128 and any(uid)
    ctx.dist_init(uid, 0, 1)
    assert (ctx.dist_rank, ctx.dist_world) == (0, 1)
    with pytest.raises(gf.GraphFlowHipError):
        ctx.dist_init(uid, 0, 1)                   # one communicator per context
    ref = t.clone()
    ctx.allreduce_sum_(t)
    ctx.broadcast_(t, 0)
    ctx.synchronize()
    assert torch.equal(t, ref)
    with pytest.raises(gf.GraphFlowHipError):
        ctx.broadcast_(t, 3)
    ctx.dist_finalize()
    assert ctx.dist_world == 1
    ctx.close()


@pytest.mark.parametrize("fused", [True, False])
def test_smp_backward_reduces_its_gradient_segments_on_the_communicator(gf, fused):
    """With a communicator on the context, gf_smp_backward all-reduces [K_L b_L W], [K_l b_l], ..., [H] on the communicator's
    stream as the reverse sweep produces them and joins before returning: with one rank the result must be bit-identical to
    the plain sweep (every segment reduced exactly once, none missed, ordering against the sweep correct)."""
    from graphflow_amd.smp import SMPOmega
    L, C, F, D, cap = 3, 64, 5, 3, 29
    mols, tg = [], []
    for seed in range(24):
        a, f, t = synthetic_molecule(4100 + seed)
        mols.append((a, f))
        tg.append(t)
    p = torch.as_tensor(smp_params(C, F, D, L, 8).astype(np.float32)).cuda()
    t = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()

    def grads(ctx, allreduce=True):
        net = SMPOmega(L, C, F, D, cap, True, ctx=ctx)
        net.set_fused(fused)
        net.set_grad_allreduce(allreduce)
        net.prepare(mols)
        g = torch.full((net.n_params,), float("nan"), device="cuda")
        for _ in range(3):   # re-running must not double-reduce anything
            net.forward(p, t)
            net.backward(p, g)
        torch.cuda.synchronize()
        return g.clone(), net

    plain, _ = grads(gf.Context(0))
    ctx = gf.Context(0)
    ctx.dist_init(ctx.dist_unique_id(), 0, 1)
    reduced, net = grads(ctx)
    local, _ = grads(ctx, allreduce=False)
    assert torch.equal(plain, reduced) and torch.equal(plain, local)
    with pytest.raises(gf.GraphFlowHipError, match="accumulate"):
        net.backward(p, reduced, accumulate=True)
    net.close()
    ctx.close()


@pytest.mark.parametrize("nK", [10, 50])
def test_padded_and_embedded_models_reduce_their_segments_too(gf, nK):
    """The SMP_2D_ver6 / ver7 wirings run as an 18-slice model on padded [f | f^T] channels: the gradient segments that are
    all-reduced are those of the PADDED vector, ver7's extra products' blocks behind it included ([X_1 .. X_L], its own segment).  One rank:
    bit-identical to the plain sweep, every caller-side gradient written."""
    from graphflow_amd.smp import SMPOmega
    L, C, F, D, cap = 3, 10, 5, 2, 12
    mols, tg = [], []
    for seed in range(16):
        a, f, t = synthetic_molecule(4300 + seed, nV=3 + seed % 10)
        mols.append((a, f))
        tg.append(t)
    t = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()

    def grads(ctx):
        net = SMPOmega(L, C, F, D, cap, True, ctx=ctx, nContractions=nK, custom_matmul=True)
        p = torch.as_tensor((np.random.default_rng(3).uniform(-1, 1, net.n_params) / np.sqrt(nK * C)).astype(np.float32)).cuda()
        net.prepare(mols)
        g = torch.full((net.n_params,), float("nan"), device="cuda")
        for _ in range(2):
            net.forward(p, t)
            net.backward(p, g)
        torch.cuda.synchronize()
        net.close()
        return g.clone()

    plain = grads(gf.Context(0))
    ctx = gf.Context(0)
    ctx.dist_init(ctx.dist_unique_id(), 0, 1)
    reduced = grads(ctx)
    assert bool(torch.isfinite(plain).all()) and float(plain.abs().max()) > 0
    assert torch.equal(plain, reduced)
    ctx.close()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: arms itself on a multi-GPU node")
def test_ranks_on_separate_gpus_sum_their_gradients(gf, tmp_path):
    """N = min(4, GPUs) ranks, one per GPU, through RCCL over xGMI: every rank's gf_smp_backward returns the SAME gradient, equal
    (to fp32 summation order) to the single-GPU gradient of the whole batch -- and the real `bench.py --gpus 2` prints one line
    with n_gpus 2 and the RCCL world in it.  Skipped on one-GPU boxes."""
    import json
    import os
    import subprocess
    import sys
    from graphflow_amd.smp import SMPOmega
    from util import rel_err
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = min(4, torch.cuda.device_count())
    out = str(tmp_path / "g.npy")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n, "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port()), os.path.join(root, "tools", "dist_check.py"), out],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out).astype(np.float64)
    L, C, F, D, cap = 3, 64, 5, 3, 29
    mols, tg = [], []
    for seed in range(32):
        a, f, t = synthetic_molecule(4100 + seed)
        mols.append((a, f))
        tg.append(t)
    net = SMPOmega(L, C, F, D, cap, True)
    net.prepare(mols)
    p = torch.as_tensor(smp_params(C, F, D, L, 8).astype(np.float32)).cuda()
    g = torch.empty(net.n_params, device="cuda")
    net.forward(p, torch.as_tensor(np.array(tg, dtype=np.float32)).cuda())
    net.backward(p, g)
    assert rel_err(got, g.cpu().numpy().astype(np.float64)) <= 2e-6
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--batch", "64",
                        "--no-cpu-baseline", "--no-extra"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and "world 2" in line["config"]["collective"]


def test_a_rank_whose_peer_never_arrives_times_out_with_its_rank_and_world(tmp_path):
    """Watchdog (round 5): gf_dist_init for rank 0 of a world of TWO, with no second rank anywhere.  ncclCommInitRank would block for
    ever; the call must come back with GF_ERR_TIMEOUT after GF_DIST_TIMEOUT_S and name the rank, the world and the call.  In a
    subprocess: the helper thread stays inside RCCL's bootstrap."""
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "lonely_rank.py"
    script.write_text(textwrap.dedent("""
        import sys, time
        sys.path.insert(0, %r)
        import graphflow_amd as gf
        from graphflow_amd import _lib
        ctx = gf.Context(0)
        uid = ctx.dist_unique_id()
        t0 = time.time()
        try:
            ctx.dist_init(uid, 0, 2)
        except gf.GraphFlowHipError as e:
            msg = str(e)
            assert "rank 0 of 2" in msg and "ncclCommInitRank" in msg and "GF_DIST_TIMEOUT_S" in msg, msg
            assert 2.0 < time.time() - t0 < 60.0, time.time() - t0
            assert ctx.dist_world == 1            # no half-made communicator left on the context
            ctx.dist_quiesce()                    # a no-op without a communicator
            print("timed out as it should:", msg)
            sys.stdout.flush()
            import os
            os._exit(0)                           # (the helper thread is still blocked in RCCL's bootstrap)
        raise SystemExit("gf_dist_init returned without its peer")
    """ % root))
    env = dict(os.environ, GF_DIST_TIMEOUT_S="4")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, env=env, timeout=180)
    assert r.returncode == 0 and "timed out as it should" in r.stdout, r.stdout + r.stderr


def test_after_a_collective_timeout_the_context_tears_down_instead_of_hanging(tmp_path):
    """Round-5 advice (medium): GF_ERR_TIMEOUT was reported but gf_dist_finalize / gf_ctx_destroy then drained the very stream the stuck
    collective sat on -- the hang the watchdog exists to prevent.  Now a timeout POISONS the communicator: later waits fail at once,
    finalize aborts it (ncclCommAbort) instead of synchronizing, and the context is usable again.  One GPU: the limit is set below the
    time the device needs for the work queued in front of the join (the wait is what times out, as it would behind a peer that never
    joins); a subprocess, so that a hang here costs a timeout and not the suite."""
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "poisoned.py"
    script.write_text(textwrap.dedent("""
        import os, sys, time
        sys.path.insert(0, %r)
        sys.path.insert(0, os.path.join(%r, "tests", "golden"))
        import numpy as np, torch
        import graphflow_amd as gf
        from graphflow_amd.smp import SMPOmega
        from inputs import smp_params, synthetic_molecule
        L, C, F, D, cap = 3, 64, 5, 3, 29
        mols = [synthetic_molecule(5000 + i)[:2] for i in range(256)]
        t = torch.as_tensor(np.array([len(a) for a, _ in mols], dtype=np.float32)).cuda()
        p = torch.as_tensor(smp_params(C, F, D, L, 8).astype(np.float32)).cuda()
        ctx = gf.Context(0)
        ctx.dist_init(ctx.dist_unique_id(), 0, 1)
        net = SMPOmega(L, C, F, D, cap, True, ctx=ctx)
        net.prepare(mols)
        g = torch.empty(net.n_params, device="cuda")
        net.forward(p, t); net.backward(p, g); ctx.dist_quiesce()      # warm, healthy
        os.environ["GF_DIST_TIMEOUT_S"] = "0.000001"
        for _ in range(8):
            net.forward(p, t)                                           # milliseconds of queued work ...
        try:
            ctx.dist_quiesce()                                          # ... in front of a wait that gives up after a microsecond
        except gf.GraphFlowHipError as e:
            assert "waited" in str(e) and "rank 0 of 1" in str(e), str(e)
        else:
            raise SystemExit("the wait did not time out")
        try:
            ctx.dist_quiesce()
        except gf.GraphFlowHipError as e:
            assert "timed out" in str(e), str(e)                        # poisoned: refuses at once
        else:
            raise SystemExit("a poisoned communicator accepted another wait")
        t0 = time.time()
        ctx.dist_finalize()                                             # aborts; must not wait for the communicator's streams
        assert time.time() - t0 < 30.0 and ctx.dist_world == 1
        os.environ["GF_DIST_TIMEOUT_S"] = "60"
        ctx.synchronize()
        ctx.dist_init(ctx.dist_unique_id(), 0, 1)                       # and the context takes a new communicator
        g2 = torch.empty_like(g)
        net.forward(p, t); net.backward(p, g2); ctx.dist_quiesce(); ctx.synchronize()
        assert torch.equal(g, g2)
        net.close(); ctx.close()
        print("poisoned communicator torn down and replaced")
    """ % (root, root)))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "torn down and replaced" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: arms itself on a multi-GPU node")
def test_a_rank_that_skips_an_allreduce_makes_its_peer_time_out_and_tear_down(tmp_path):
    """Two ranks on two GPUs; rank 1 skips one all-reduce.  Rank 0 must come back from gf_dist_quiesce with GF_ERR_TIMEOUT naming the
    exchange, and its gf_dist_finalize / context close must return (ncclCommAbort) instead of hanging behind the stuck collective."""
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    idf = tmp_path / "uid.bin"
    script = tmp_path / "skipper.py"
    script.write_text(textwrap.dedent("""
        import os, sys, time
        sys.path.insert(0, %r)
        import torch
        import graphflow_amd as gf
        rank = int(sys.argv[1]); idf = sys.argv[2]
        ctx = gf.Context(rank)
        if rank == 0:
            uid = ctx.dist_unique_id()
            open(idf + ".tmp", "wb").write(bytes(uid)); os.rename(idf + ".tmp", idf)
        else:
            while not os.path.exists(idf): time.sleep(0.05)
            uid = open(idf, "rb").read()
        ctx.dist_init(uid, rank, 2)
        x = torch.ones(1 << 20, device="cuda:%%d" %% rank)
        ctx.allreduce_sum_(x); ctx.dist_quiesce(); ctx.synchronize()
        assert float(x[0]) == 2.0
        if rank == 0:
            ctx.allreduce_sum_(x)                      # the peer never joins this one
            t0 = time.time()
            try:
                ctx.dist_quiesce()
            except gf.GraphFlowHipError as e:
                assert "rank 0 of 2" in str(e) and "all-reduce #2" in str(e), str(e)
            else:
                raise SystemExit("no timeout")
            ctx.dist_finalize(); ctx.close()
            print("rank 0 timed out after %%.1f s and tore down" %% (time.time() - t0))
        else:
            time.sleep(20)                             # alive, but not in the collective
            os._exit(0)
    """ % root))
    env = dict(os.environ, GF_DIST_TIMEOUT_S="5", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(idf)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert procs[0].returncode == 0 and "tore down" in outs[0], outs[0][-2000:]


MOCK_RCCL = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "cpp", "bin", "libmock_rccl.so")


@pytest.mark.parametrize("world,C", [(2, 64), (4, 64), (2, 10)])
def test_world_of_several_ranks_on_one_gpu_through_the_mock_transport(gf, tmp_path, world, C):
    """RCCL refuses two ranks on one device, so on a one-GPU box the path's own exchange never ran with a world above one (round-5 review,
    missing #1).  tests/cpp/mock_rccl.cpp is a shared-memory stand-in for the six RCCL entry points gf_dist.hip binds (GF_RCCL_LIBRARY
    selects it): `world` rank PROCESSES on device 0, each with its contiguous shard of a 48-molecule batch (graphflow_amd.dist.shard),
    broadcast the parameters from rank 0 (Threaded_BatchLearn's copy_value, SMP_omega.h:771-773), run forward + backward with the
    per-level gradient segments all-reduced inside gf_smp_backward (add_gradient, :784-786) -- three steps, so a segment reduced
    twice or not at all shows -- and every rank must hold the SAME gradient, equal to the one-context gradient of the whole batch to
    fp32 summation order; then Adam steps on every rank leave identical parameters.  Exercises OUR side of the exchange (segments,
    offsets, stream choreography, join, teardown), not RCCL's transport."""
    import os
    import subprocess
    import sys
    import textwrap
    from graphflow_amd.smp import SMPOmega
    from util import rel_err
    assert os.path.exists(MOCK_RCCL), "tests/cpp/bin/libmock_rccl.so is built by __graft_entry__.build() (make -C tests/cpp)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "rank.py"
    script.write_text(textwrap.dedent("""
        import os, sys, time
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests", "golden"))
        import numpy as np, torch
        import graphflow_amd as gf
        from graphflow_amd.dist import shard
        from graphflow_amd.smp import SMPOmega
        from inputs import smp_params, synthetic_molecule
        rank, world, C, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
        ctx = gf.Context(0)
        idf = os.path.join(out, "uid.bin")
        if rank == 0:
            uid = ctx.dist_unique_id()
            open(idf + ".tmp", "wb").write(bytes(uid)); os.rename(idf + ".tmp", idf)
        else:
            while not os.path.exists(idf): time.sleep(0.02)
            uid = open(idf, "rb").read()
        ctx.dist_init(uid, rank, world)
        assert (ctx.dist_rank, ctx.dist_world) == (rank, world)
        L, F, D, cap = 3, 5, 3, 29
        mols, tg = [], []
        for seed in range(48):
            a, f, t = synthetic_molecule(4100 + seed); mols.append((a, f)); tg.append(t)
        lo, hi = shard(len(mols), rank, world)
        net = SMPOmega(L, C, F, D, cap, True, ctx=ctx)
        net.prepare(mols[lo:hi])
        # every rank starts from ITS OWN parameters; rank 0's are broadcast (the reference copies the master's values into the clones)
        p = torch.as_tensor(smp_params(C, F, D, L, 8 + rank).astype(np.float32)).cuda()
        ctx.broadcast_(p, 0)
        t = torch.as_tensor(np.array(tg[lo:hi], dtype=np.float32)).cuda()
        g = torch.full((net.n_params,), float("nan"), device="cuda")
        for _ in range(3):
            net.forward(p, t); net.backward(p, g)
        ctx.dist_quiesce(); ctx.synchronize()
        np.save(os.path.join(out, "g%%d.npy" %% rank), g.cpu().numpy())
        for _ in range(2):   # two training steps: identical parameters on every rank afterwards
            net.forward(p, t); net.backward(p, g); net.adam_step(p, g, 1e-4, len(mols))
        ctx.dist_quiesce(); ctx.synchronize()
        np.save(os.path.join(out, "p%%d.npy" %% rank), p.cpu().numpy())
        net.close(); ctx.dist_finalize(); ctx.close()
        print("rank %%d of %%d done" %% (rank, world))
    """ % (root, root)))
    env = dict(os.environ, GF_RCCL_LIBRARY=MOCK_RCCL, GF_DIST_TIMEOUT_S="120")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), str(C), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True, env=env) for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "done" in o, "rank %d:\n%s" % (r, o[-3000:])
    gs = [np.load(tmp_path / ("g%d.npy" % r)) for r in range(world)]
    ps = [np.load(tmp_path / ("p%d.npy" % r)) for r in range(world)]
    for r in range(1, world):
        assert np.array_equal(gs[0], gs[r]) and np.array_equal(ps[0], ps[r]), r   # the same sum, the same step, bit for bit
    L, F, D, cap = 3, 5, 3, 29
    mols, tg = [], []
    for seed in range(48):
        a, f, t = synthetic_molecule(4100 + seed)
        mols.append((a, f))
        tg.append(t)
    net = SMPOmega(L, C, F, D, cap, True)
    net.prepare(mols)
    p = torch.as_tensor(smp_params(C, F, D, L, 8).astype(np.float32)).cuda()
    g = torch.empty(net.n_params, device="cuda")
    net.forward(p, torch.as_tensor(np.array(tg, dtype=np.float32)).cuda())
    net.backward(p, g)
    e = rel_err(gs[0].astype(np.float64), g.cpu().numpy().astype(np.float64))
    print("world %d on one GPU (mock transport), C = %d: summed gradient vs one context: %.2e" % (world, C, e))
    assert np.isfinite(gs[0]).all() and e <= 2e-6
    net.close()


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_entry_point_with_two_ranks_on_one_gpu(gf, scaling):
    """`python bench.py --gpus 2` -- the driver's multi-GPU entry point: self-spawn through torch.distributed.run, the unique id's
    broadcast, gf_dist_init on every rank, sharding, the timed region with the bounded waits, max over ranks, the end-to-end loop with
    its loader threads and collectives inside backward, the `collective` block of the line, teardown -- with both ranks on device 0
    (GF_BENCH_ONE_GPU, torch's side channel on gloo) and the exchange on the mock transport.  One JSON line, n_gpus 2, the library's
    communicator reporting a world of two, four all-reduces per step."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GF_BENCH_ONE_GPU="1", GF_RCCL_LIBRARY=MOCK_RCCL, GF_DIST_TIMEOUT_S="120", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--repeats", "2", "--batch",
                        "96" if scaling == "weak" else "192", "--scaling", scaling, "--no-cpu-baseline", "--full"], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == scaling and line["value"] > 0
    assert "world 2" in line["config"]["collective"] and "TEST HOOK" in line["data"]
    c = line["collective"]
    assert c["rccl_ranks_seen"] == 2 and c["expected"] == 2 and abs(c["allreduces_per_step"] - 4.0) < 1e-9   # [K_3 b_3 W], [K_2 b_2], [K_1 b_1], [H]
    assert line["end_to_end"]["value"] > 0 and "all 2 GPUs" in line["end_to_end"]["unit"]
    assert "96 synthetic" in line["config"]["workload"]   # weak: 96 per rank; strong: 192 split over the two


def test_a_rank_that_skips_an_allreduce_on_one_gpu_through_the_mock_transport(tmp_path):
    """Round-5 advice (medium), the scenario it asked for, on ONE GPU: two rank processes on device 0 over the mock transport (whose
    collectives hold their stream until every rank has joined, as RCCL's kernels do).  Rank 1 skips an all-reduce.  Rank 0 must come back
    from gf_dist_quiesce with GF_ERR_TIMEOUT naming the exchange, and gf_dist_finalize / gf_ctx_destroy must RETURN -- ncclCommAbort frees
    the stuck stream -- instead of hanging behind the collective; the context then still computes."""
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(MOCK_RCCL)
    idf = tmp_path / "uid.bin"
    script = tmp_path / "skipper.py"
    script.write_text(textwrap.dedent("""
        import os, sys, time
        sys.path.insert(0, %r)
        import torch
        import graphflow_amd as gf
        rank = int(sys.argv[1]); idf = sys.argv[2]
        ctx = gf.Context(0)
        if rank == 0:
            uid = ctx.dist_unique_id()
            open(idf + ".tmp", "wb").write(bytes(uid)); os.rename(idf + ".tmp", idf)
        else:
            while not os.path.exists(idf): time.sleep(0.02)
            uid = open(idf, "rb").read()
        ctx.dist_init(uid, rank, 2)
        x = torch.ones(1 << 16, device="cuda")
        ctx.allreduce_sum_(x); ctx.dist_quiesce(); ctx.synchronize()
        assert float(x[0]) == 2.0
        if rank == 0:
            ctx.allreduce_sum_(x)                      # the peer never joins this one: the context's stream is stuck behind it
            t0 = time.time()
            try:
                ctx.dist_quiesce()
            except gf.GraphFlowHipError as e:
                assert "rank 0 of 2" in str(e) and "all-reduce #2" in str(e), str(e)
            else:
                raise SystemExit("no timeout")
            waited = time.time() - t0
            t1 = time.time()
            ctx.dist_finalize()                        # aborts the communicator: must not wait for the stuck stream
            ctx.synchronize()                          # ... which drains once the collective has been released
            assert time.time() - t1 < 20.0
            y = (torch.arange(8, device="cuda") * 2).sum()
            assert int(y) == 56
            ctx.close()
            print("rank 0 timed out after %%.1f s, tore down in %%.2f s" %% (waited, time.time() - t1))
        else:
            time.sleep(12)                             # alive, but not in the collective
            os._exit(0)
    """ % root))
    env = dict(os.environ, GF_DIST_TIMEOUT_S="4", GF_RCCL_LIBRARY=MOCK_RCCL)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(idf)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert procs[0].returncode == 0 and "tore down" in outs[0], outs[0][-3000:]
