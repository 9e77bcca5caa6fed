"""One training step (forward + backward + Adam) of SMP_theta on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, C = 64, F = 5,
D = 5, cap 29 -- with SMP_gamma and SMP_omega (cap 29) steps on the same molecules in the same process for scale.  Five timed regions per
model, alternated, HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step and the per-kernel table of
one traced SMP_theta step (gf_ctx_set_timing).  `--kernels-only` runs a few SMP_theta steps and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --` for the profiler's own per-kernel table.
usage: python tools/theta_time.py [regions] [steps per region] [batch] [--kernels-only]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from inputs import smp_params, synthetic_molecule  # noqa: E402
from make_theta_golden import random_params, theta_blocks  # noqa: E402
from graphflow_amd.smp import SMPGamma, SMPOmega, SMPTheta  # noqa: E402
from make_gamma_golden import gamma_params  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
kernels_only = "--kernels-only" in sys.argv
regions = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 10
B = int(args[2]) if len(args) > 2 else 1024
L, Cn, F, D, cap = 3, 64, 5, 5, 29
mols, tg = [], []
for i in range(B):
    adj, feat, t = synthetic_molecule(i)   # (bench.py cfg3's molecules)
    mols.append((adj, feat))
    tg.append(t)
maxV = max(len(a) for a, _ in mols)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
theta = SMPTheta(maxV, cap, L, Cn, F, D)
theta.prepare(mols)
modes = {"theta": (theta, random_params(theta_blocks(Cn, F * (D + 1), L, maxV), np.random.default_rng(1)))}
if not kernels_only:
    gamma = SMPGamma(L, Cn, F, D, maxV)
    gamma.prepare(mols)
    omega = SMPOmega(L, Cn, F, D, cap, True)
    omega.prepare(mols)
    modes["gamma"] = (gamma, gamma_params(Cn, F, D, L, 1))
    modes["omega_cap29"] = (omega, smp_params(Cn, F, D, L, 1))
state = {k: (torch.as_tensor(np.asarray(p, dtype=np.float32)).cuda(), torch.empty(net.n_params, device="cuda")) for k, (net, p) in modes.items()}


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
        step("theta")
    torch.cuda.synchronize()
    theta.close()
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
theta.ctx.set_timing(True)
step("theta")
kernels = {k: [round(ms, 4), int(n)] for k, (ms, n) in sorted(theta.ctx.timings().items(), key=lambda kv: -kv[1][0])}
theta.ctx.set_timing(False)
sizes = {l: theta.level_sizes(l) for l in range(L + 1)}
print(json.dumps({"tool": "theta_time", "batch": B, "L": L, "C": Cn, "F": F, "D": D, "cap": cap, "max_nVertices": maxV, "regions": regions,
                  "steps": steps, "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()},
                  "ms_per_step_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
                  "ms_per_step_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                  "theta_level_nodes_rows": {str(l): [int(s[0]), int(s[1])] for l, s in sizes.items()},
                  "theta_device_bytes": theta.device_bytes()[0],
                  "theta_kernels_ms_launches_one_step": kernels}), flush=True)
for net, _ in modes.values():
    net.close()
