"""One training step (forward + backward + Momentum) of SMP_1D, SMP_1D_ver2 and SMP_1D_ver3 on the cfg3 batch -- 1024 synthetic QM9-size
molecules, L = 3, nChanels = 16 (the concatenating forms end at 128 channels), F = 5, D = 5, no cap -- with an SMP_theta step (forward +
backward + Adam) at the same settings on the same molecules in the same process.  Regions alternate between the four handles; HIP events
after a warm-up; prints one JSON line with the median and min .. max ms per step, and the per-kernel table of one traced step of each form
(gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not what the step costs).
usage: python tools/smp1d_time.py [regions] [steps per region] [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from inputs import synthetic_molecule  # noqa: E402
from make_smp1d_golden import random_params as params_1d, smp1d_blocks  # noqa: E402
from make_theta_golden import random_params as params_theta, theta_blocks  # noqa: E402
from graphflow_amd.smp import SMP1D, SMPTheta  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
regions = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 10
B = int(args[2]) if len(args) > 2 else 1024
L, Cn, F, D = 3, 16, 5, 5
mols, tg = [], []
for i in range(B):
    adj, feat, t = synthetic_molecule(i)   # (bench.py cfg3's molecules)
    mols.append((adj, feat))
    tg.append(t)
maxV = max(len(a) for a, _ in mols)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
modes = {}
for version, name in ((1, "smp_1d"), (2, "smp_1d_ver2"), (3, "smp_1d_ver3")):
    net = SMP1D(version, maxV, L, Cn, F, D)
    net.prepare(mols)
    modes[name] = (net, params_1d(smp1d_blocks(version, Cn, F * (D + 1), L, maxV), np.random.default_rng(version)))
theta = SMPTheta(maxV, maxV, L, Cn, F, D)
theta.prepare(mols)
modes["theta"] = (theta, params_theta(theta_blocks(Cn, F * (D + 1), L, maxV), np.random.default_rng(1)))
state = {k: (torch.as_tensor(np.asarray(p, dtype=np.float32)).cuda(), torch.empty(net.n_params, device="cuda")) for k, (net, p) in modes.items()}


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    if name == "theta":
        net.adam_step(p, g, 1e-6, B)
    else:
        net.step(p, g, 1e-6, B)


for name in modes:   # warm-up: pools, workspaces, code objects
    for _ in range(3):
        step(name)
torch.cuda.synchronize()
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
kernels = {}
for name, (net, _) in modes.items():
    net.ctx.set_timing(True)
    step(name)
    kernels[name] = {k: [round(ms, 4), int(n)] for k, (ms, n) in sorted(net.ctx.timings().items(), key=lambda kv: -kv[1][0])}
    net.ctx.set_timing(False)
sizes = {l: theta.level_sizes(l) for l in range(L + 1)}
print(json.dumps({"tool": "smp1d_time", "batch": B, "L": L, "C": Cn, "F": F, "D": D, "max_nVertices": maxV, "regions": regions, "steps": steps,
                  "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()},
                  "ms_per_step_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
                  "ms_per_step_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                  "level_nodes_rows": {str(l): [int(s[0]), int(s[1])] for l, s in sizes.items()},
                  "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
                  "kernels_ms_launches_one_step": kernels}), flush=True)
for net, _ in modes.values():
    net.close()
