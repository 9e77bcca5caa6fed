"""The harness of the step-timing tools (theta_time, smp1d_time, smp2d_time, smp2d_ver5_time, unrestricted_time, ccn1d_time, gamma_time,
gamma_physics_time): the cfg3 batch, the command line, the timed regions and the traced step, written once so that every
parent-against-new comparison made with these tools measures the same way.  A tool keeps its models, its parameters, its `step(name)`
and the fields it alone reports.  Importing this module puts the repository and tests/golden on sys.path."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from inputs import synthetic_molecule  # noqa: E402


def parse_args(argv, regions=5, steps=10, batch=1024):
    """[regions] [steps per region] [batch] [--out file.json] (other --flags are the tool's): regions, steps, batch, out path or None"""
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    n = [int(a) for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--out")]
    n += [regions, steps, batch][len(n):]
    return n[0], n[1], n[2], out_path


def cfg3_batch(B):
    """bench.py cfg3's first B synthetic molecules: [(adjacency, features)], their targets on the device, the largest vertex count"""
    mols, tg = [], []
    for i in range(B):
        adj, feat, t = synthetic_molecule(i)
        mols.append((adj, feat))
        tg.append(t)
    return mols, torch.as_tensor(np.array(tg, dtype=np.float32)).cuda(), max(len(a) for a, _ in mols)


def device_state(modes):
    """{name: (parameters on the device, an empty gradient)} for modes = {name: (net, host parameters, ...)}"""
    return {k: (torch.as_tensor(np.asarray(m[1], dtype=np.float32)).cuda(), torch.empty(m[0].n_params, device="cuda")) for k, m in modes.items()}


def time_handles(modes, step, regions, steps):
    """{name: [ms per step of each region]}: three warm-up steps of every mode (pools, workspaces, code objects), a synchronise, then
    `regions` rounds over the modes, each one untimed step after the switch of handle or plan and `steps` steps between two HIP events"""
    for name in modes:
        for _ in range(3):
            step(name)
    torch.cuda.synchronize()
    times = {k: [] for k in modes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(regions):
        for name in modes:
            step(name)
            e0.record()
            for _ in range(steps):
                step(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)
    return times


def summary(times):
    """the median and min .. max ms per step of each mode's regions, under the keys every tool reports"""
    return {"ms_per_step_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
            "ms_per_step_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}}


def trace_one_step(nets, step):
    """{name: {kernel: [ms, launches]}}, slowest kernel first, of one step(name) per net under gf_ctx_set_timing: the kernels run one by
    one, so the table says where the time goes, not what the step costs"""
    kernels = {}
    for name, net in nets.items():
        net.ctx.set_timing(True)
        step(name)
        kernels[name] = {k: [round(ms, 4), int(n)] for k, (ms, n) in sorted(net.ctx.timings().items(), key=lambda kv: -kv[1][0])}
        net.ctx.set_timing(False)
    return kernels


def emit(record, out_path=None):
    """one JSON line on stdout, and in out_path when given"""
    line = json.dumps(record)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
