"""One training step (forward + backward + Momentum) of SMP_2D_ver5 beside SMP_2D (form 1), both at 64 channels, on the cfg3 batch -- 1024
synthetic QM9-size molecules, L = 3, F = 5, D = 5, no cap -- in one process, the regions alternating between the two handles.  HIP events
after a warm-up; prints one JSON line with the median and min .. max ms per step, the ver5 / form-1 ratio, device_bytes, the per-kernel
table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not what the step
costs), and for the two row projections of ver5 the bytes they must move (S read + f_l written, dz read + dE written; fp32) over the
traced time, beside gf_hbm_copy_probe_f32 (a 1 GiB float4 copy, read + written bytes) in the same process.
usage: python tools/smp2d_ver5_time.py [regions] [steps per region] [batch] [--out file.json]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from inputs import synthetic_molecule  # noqa: E402
from make_smp2d_golden import random_params as params_2d  # noqa: E402
from make_smp2d_ver5_golden import random_params as params_ver5  # noqa: E402
from graphflow_amd.smp import SMP2D  # noqa: E402

out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] != "--out"]
regions = int(args[0]) if len(args) > 0 else 5
steps = int(args[1]) if len(args) > 1 else 10
B = int(args[2]) if len(args) > 2 else 1024
L, F, D, CH = 3, 5, 5, 64
mols, tg = [], []
for i in range(B):
    adj, feat, t = synthetic_molecule(i)   # (bench.py cfg3's molecules)
    mols.append((adj, feat))
    tg.append(t)
maxV = max(len(a) for a, _ in mols)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
modes = {}
for form, name in (("2d", "smp_2d"), ("ver5", "smp_2d_ver5")):
    net = SMP2D(form, maxV, L, CH, F, D)
    net.prepare(mols)
    p = params_2d(1, CH, F * (D + 1), L, maxV, np.random.default_rng(6)) if form == "2d" else \
        params_ver5(CH, F * (D + 1), L, maxV, np.random.default_rng(5))
    modes[name] = (net, p)
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
v5 = modes["smp_2d_ver5"][0]
sizes = {l: v5.level_sizes(l) for l in range(L + 1)}
rows = sum(int(sizes[l][1]) for l in range(1, L + 1))
proj_bytes = 2 * 4 * rows * CH   # one [rows][C] operand read, one written, over the L levels
n = 1 << 28
a, b = torch.ones(n, device="cuda"), torch.empty(n, device="cuda")
probe = v5.ctx.hbm_copy_probe(b, a, 0, 5)
proj = {k: {"bytes": int(proj_bytes), "GBps": round(proj_bytes / (kernels["smp_2d_ver5"][k][0] * 1e-3) / 1e9, 1)}
        for k in ("smp2d5_row_proj", "smp2d5_row_proj_bwd")}
for k in proj:
    proj[k]["fraction_of_copy_probe"] = round(proj[k]["GBps"] / probe, 4)
med = {k: float(np.median(v)) for k, v in times.items()}
line = json.dumps({"tool": "smp2d_ver5_time", "batch": B, "L": L, "channels": CH, "F": F, "D": D, "max_nVertices": maxV, "regions": regions,
                   "steps": steps, "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()},
                   "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
                   "ms_per_step_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
                   "ver5_over_form1": round(med["smp_2d_ver5"] / med["smp_2d"], 4),
                   "level_nodes_rows": {str(l): [int(s[0]), int(s[1])] for l, s in sizes.items()},
                   "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
                   "hbm_copy_probe_GBps": round(probe, 1), "row_projections": proj,
                   "kernels_ms_launches_one_step": kernels})
print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
for net, _ in modes.values():
    net.close()
