"""One training step (forward + backward + Adam) of CCN_1D at the reference demo's settings -- 10 / 10 vertices, cap 6, 7 levels, 16
channels, decay 0.5 (tests/test_CCN_1D.cpp) -- on a synthetic batch of 1024 pairs of 3- to 10-vertex molecules (F = 5), with
SMP_theta_pairgraphs at 16 channels (16 -> 8 -> 4 -> 2 -> 1 ..) on the same pairs in the same process for scale.  Five timed regions per
model, alternated, HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step, and of one traced step
per model (gf_ctx_set_timing) the per-kernel table, the number of launches and the sum of the kernel times: a step much longer than its
kernels' sum is bound by its launches.  `--kernels-only` runs a few CCN_1D steps and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --` for the profiler's own per-kernel table.
usage: python tools/ccn1d_time.py [regions] [steps per region] [batch] [--kernels-only]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from inputs import synthetic_molecule  # noqa: E402
from make_ccn1d_golden import random_params  # noqa: E402
from make_theta_golden import model_blocks  # noqa: E402
from make_theta_golden import random_params as theta_params  # noqa: E402
from graphflow_amd.smp import CCN1D, SMPModel  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
kernels_only = "--kernels-only" in sys.argv
regions = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 10
B = int(args[2]) if len(args) > 2 else 1024
maxV, cap, L, Cn, F, decay = 10, 6, 7, 16, 5, 0.5
g1, g2, tg = [], [], []
for i in range(B):
    a, fa, ta = synthetic_molecule(i, 3 + i % 8)
    b, fb, tb = synthetic_molecule(50000 + i, 3 + (i // 8) % 8)
    g1.append((a, fa))
    g2.append((b, fb))
    tg.append(ta - tb)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
ccn = CCN1D(maxV, maxV, cap, L, Cn, F, F, decay)
ccn.prepare(g1, g2)
modes = {"ccn_1d": (ccn, random_params(Cn, L, [F, F], [maxV, maxV], decay, [np.ones(F), np.ones(F)], np.random.default_rng(1)))}
if not kernels_only:
    pair = SMPModel(L, Cn, cap, [F, F], first_order=True, max_nVertices=[maxV, maxV])
    pair.prepare(g1, g2)
    modes["theta_pairgraphs"] = (pair, theta_params(model_blocks(2, Cn, L, [F, F], [maxV, maxV]), np.random.default_rng(1)))
state = {k: (torch.as_tensor(np.asarray(p, dtype=np.float32)).cuda(), torch.empty(net.n_params, device="cuda")) for k, (net, p) in modes.items()}
for k, (net, p) in modes.items():
    assert len(p) == net.n_params, k


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    net.adam_step(p, g, 1e-6, B)


for name in modes:   # warm-up: pools, workspaces, code objects
    for _ in range(3):
        step(name)
torch.cuda.synchronize()
if kernels_only:
    for _ in range(steps):
        step("ccn_1d")
    torch.cuda.synchronize()
    ccn.close()
    sys.exit(0)
times = {k: [] for k in modes}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(regions):
    for name in modes:
        step(name)   # (one untimed step after a switch of handle)
        e0.record()
        for _ in range(steps):
            step(name)
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) / steps)
traced = {}
for name, (net, _) in modes.items():
    net.ctx.set_timing(True)
    step(name)
    t = net.ctx.timings()
    net.ctx.set_timing(False)
    traced[name] = {"launches": int(sum(n for _, n in t.values())), "kernel_ms_sum": round(sum(ms for ms, _ in t.values()), 4),
                    "kernels_ms_launches": {k: [round(ms, 4), int(n)] for k, (ms, n) in sorted(t.items(), key=lambda kv: -kv[1][0])}}
print(json.dumps({"tool": "ccn1d_time", "batch": B, "L": L, "C": Cn, "F": F, "cap": cap, "max_nVertices": maxV, "decay": decay,
                  "regions": regions, "steps": steps, "vertices": [int(sum(len(a) for a, _ in g)) for g in (g1, g2)],
                  "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()},
                  "ms_per_step_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
                  "ms_per_step_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                  "one_traced_step": traced}), flush=True)
for net, _ in modes.values():
    net.close()
