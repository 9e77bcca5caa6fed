"""One training step (forward + backward + Adam) of SMP_gamma on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, C = 64, F = 5,
D = 5 -- with its fused level, op by op (gf_smp_set_fused(0) on the same handle and batch), and SMP_omega with cap 29 on the same molecules
(the bench.py cfg3 model).  The three run alternately in one process, timed with HIP events after a warm-up; prints one JSON line with the
median ms per step of each.
usage: python tools/gamma_time.py [rounds] [steps per round] [batch]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from inputs import smp_params, synthetic_molecule  # noqa: E402
from graphflow_amd.smp import SMPGamma, SMPOmega  # noqa: E402


def gamma_params(C, F, D, L, seed):
    """Random parameters in SMP_gamma's registration order H[C, F(D+1)], (K_l[4C, C], b_l[C]) x L, W[C], sized like uniform_init's range."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-1, 1, C * F * (D + 1)) / np.sqrt(F * (D + 1))]
    for _ in range(L):
        parts += [rng.uniform(-1, 1, 4 * C * C) / np.sqrt(4 * C), rng.uniform(-0.1, 0.1, C)]
    parts.append(rng.uniform(-1, 1, C) / np.sqrt(C))
    return np.concatenate(parts).astype(np.float32)

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
B = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
L, Cn, F, D, cap = 3, 64, 5, 5, 29
mols, tg = [], []
for i in range(B):
    adj, feat, t = synthetic_molecule(i)   # (bench.py cfg3's molecules)
    mols.append((adj, feat))
    tg.append(t)
maxV = max(len(a) for a, _ in mols)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
gamma = SMPGamma(L, Cn, F, D, maxV)
gamma.prepare(mols)
omega = SMPOmega(L, Cn, F, D, cap, True)
omega.prepare(mols)
modes = {
    "gamma_fused": (gamma, True, gamma_params(Cn, F, D, L, 1)),
    "gamma_op_by_op": (gamma, False, gamma_params(Cn, F, D, L, 1)),
    "omega_cap29": (omega, True, smp_params(Cn, F, D, L, 1)),
}
state = {k: (torch.as_tensor(p.astype(np.float32)).cuda(), torch.empty(net.n_params, device="cuda")) for k, (net, _, p) in modes.items()}


def step(name):
    net, fused, _ = modes[name]
    p, g = state[name]
    net.set_fused(fused)
    net.forward(p, targets)
    net.backward(p, g)
    net.adam_step(p, g, 1e-6, B)


times = {k: [] for k in modes}
for name in modes:   # warm-up: pools, workspaces, code objects
    for _ in range(3):
        step(name)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(rounds):
    for name in modes:
        step(name)   # (one untimed step after a switch of handle or plan)
        e0.record()
        for _ in range(steps):
            step(name)
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) / steps)
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps({"tool": "gamma_time", "batch": B, "L": L, "C": Cn, "F": F, "D": D, "max_nVertices": maxV, "rounds": rounds, "steps": steps,
                  "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
                  "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
                  "fused_speedup_vs_op_by_op": round(med["gamma_op_by_op"] / med["gamma_fused"], 3),
                  "gamma_fused_vs_omega": round(med["gamma_fused"] / med["omega_cap29"], 3)}), flush=True)
gamma.close()
omega.close()
