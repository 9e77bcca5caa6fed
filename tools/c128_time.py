"""Forward + backward of SMP_omega at 128 channels on the cfg3 batch -- 256 synthetic QM9-size molecules, L = 3, F = 5, D = 5, cap 29 --
on the dedicated block-product kernels (four 64-channel sub-block passes per product, smp_level_c64_split.hip: GF_SMP_C128=1) and on the
grouped tiled GEMMs (GF_SMP_C128=0), alternately (A/B/A/B) in one process on one handle.  Step times with HIP events after a warm-up; then one
step of each with the per-kernel timing table, written to profiles/c128_kernels.json.  Prints one JSON line.
usage: python tools/c128_time.py [rounds] [steps per round] [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from inputs import smp_params, synthetic_molecule  # noqa: E402
from graphflow_amd.smp import SMPOmega  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
B = int(sys.argv[3]) if len(sys.argv) > 3 else 256
L, Cn, F, D, cap = 3, 128, 5, 5, 29
mols, tg = [], []
for i in range(B):
    adj, feat, t = synthetic_molecule(i)   # (bench.py cfg3's molecules)
    mols.append((adj, feat))
    tg.append(t)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
os.environ["GF_SMP_C128"] = "1"   # (the tables and image sets of the sub-block passes are taken when the batch is prepared)
net = SMPOmega(L, Cn, F, D, cap, True)
net.prepare(mols)
p = torch.as_tensor(smp_params(Cn, F, D, L, 1).astype(np.float32)).cuda()
g = torch.empty(net.n_params, device="cuda")
MODES = {"c128_kernels": "1", "GF_SMP_C128=0": "0"}


def step(mode):
    os.environ["GF_SMP_C128"] = MODES[mode]
    net.forward(p, targets)   # (the reverse sweep follows the forward's layout: one value of the switch per step)
    net.backward(p, g)


times = {k: [] for k in MODES}
for mode in MODES:   # warm-up: pools, workspaces, code objects
    for _ in range(2):
        step(mode)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(rounds):
    for mode in MODES:
        step(mode)   # (one untimed step after a switch of plan)
        e0.record()
        for _ in range(steps):
            step(mode)
        e1.record()
        e1.synchronize()
        times[mode].append(e0.elapsed_time(e1) / steps)
kernels = {}
for mode in MODES:
    step(mode)
    net.ctx.set_timing(True)
    step(mode)
    kernels[mode] = {k: {"ms": round(ms, 4), "launches": int(n)} for k, (ms, n) in sorted(net.ctx.timings().items())}
    net.ctx.set_timing(False)
os.environ.pop("GF_SMP_C128", None)
med = {k: float(np.median(v)) for k, v in times.items()}
three = ("smpf_products_fwd", "smpf_products_bwd", "smpf_wgrad")
out = {"tool": "c128_time", "batch": B, "L": L, "C": Cn, "F": F, "D": D, "cap": cap, "rounds": rounds, "steps": steps,
       "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
       "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
       "new_over_old": round(med["c128_kernels"] / med["GF_SMP_C128=0"], 3),
       "dedicated_kernels_ms": {k: kernels["c128_kernels"].get(k, {}).get("ms") for k in three},
       "generic_gemms_ms": {k: kernels["GF_SMP_C128=0"].get(k, {}).get("ms") for k in ("gemm_nn", "gemm_nt", "gemm_tn", "splitk_reduce")}}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "c128_kernels.json"), "w") as f:
    json.dump({"summary": out, "kernels": kernels}, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(out), flush=True)
net.close()
