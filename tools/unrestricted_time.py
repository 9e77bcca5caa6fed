"""One training step (forward + backward + Momentum) of Unrestricted_SMP_1D (nChanels = 64), Unrestricted_SMP_1D_ver2 (nChanels = 16,
ending at 128) and Unrestricted_SMP_2D (nChanels = 64) on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, F = 5, D = 5 --
alternated in one process with steps of their restricted siblings on the same molecules: SMP_1D and SMP_2D at 64 channels.  Regions
alternate between the five handles; HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step and the
per-kernel table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not
what the step costs).
usage: python tools/unrestricted_time.py [regions] [steps per region] [batch] [--out file.json]"""
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
from make_smp2d_golden import random_params as params_2d  # noqa: E402
from make_unrestricted_golden import random_params as params_un  # noqa: E402
from graphflow_amd.smp import SMP1D, SMP2D, SMPUnrestricted  # noqa: E402

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--out"]
regions = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 10
B = int(args[2]) if len(args) > 2 else 1024
L, F, D = 3, 5, 5
CH = {"unrestricted_1d": 64, "unrestricted_1d_ver2": 16, "unrestricted_2d": 64, "smp_1d": 64, "smp_2d": 64}
mols, tg = [], []
for i in range(B):
    adj, feat, t = synthetic_molecule(i)   # (bench.py cfg3's molecules)
    mols.append((adj, feat))
    tg.append(t)
maxV = max(len(a) for a, _ in mols)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
modes = {}
for form, name in (("1d", "unrestricted_1d"), ("1d_ver2", "unrestricted_1d_ver2"), ("2d", "unrestricted_2d")):
    net = SMPUnrestricted(form, maxV, L, CH[name], F, D)
    net.prepare(mols)
    modes[name] = (net, params_un(SMPUnrestricted.FORMS[form], CH[name], F * (D + 1), L, maxV, np.random.default_rng(len(name))))
one = SMP1D(1, maxV, L, CH["smp_1d"], F, D)
one.prepare(mols)
modes["smp_1d"] = (one, params_1d(smp1d_blocks(1, CH["smp_1d"], F * (D + 1), L, maxV), np.random.default_rng(1)))
two = SMP2D("2d", maxV, L, CH["smp_2d"], F, D)
two.prepare(mols)
modes["smp_2d"] = (two, params_2d(1, CH["smp_2d"], F * (D + 1), L, maxV, np.random.default_rng(2)))
state = {k: (torch.as_tensor(np.asarray(p, dtype=np.float32)).cuda(), torch.empty(net.n_params, device="cuda")) for k, (net, p) in modes.items()}


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
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
sizes = {name: {l: modes[name][0].level_sizes(l) for l in range(L + 1)} for name in ("unrestricted_1d", "unrestricted_2d")}
line = json.dumps({"tool": "unrestricted_time", "batch": B, "L": L, "channels": CH, "F": F, "D": D, "max_nVertices": maxV, "regions": regions,
                   "steps": steps, "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()},
                   "ms_per_step_median": {k: round(float(np.median(v)), 4) for k, v in times.items()},
                   "ms_per_step_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                   "level_nodes_rows": {k: {str(l): [int(s[0]), int(s[1])] for l, s in v.items()} for k, v in sizes.items()},
                   "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
                   "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()},
                   "kernels_ms_launches_one_step": kernels})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
for net, _ in modes.values():
    net.close()
