"""Forward + backward of SMP_gamma_physics / SMP_gamma_pairgraphs (gf_smp_model_*, nContractions = 4) on the cfg3 batch -- 1024 synthetic
QM9-size molecules, L = 3, cap 29, F = 5 (the second tower sees the same molecules, as tools/physics_time.py) -- for 1 and 2 towers at
C = 16 and 32, three ways: the packed gamma tower level (fused), op by op (set_fused(False) on the same handle and batch), and
SMP_omega_physics / _pairgraphs (nContractions = 18) on the same batch.  All configurations run alternately in one process, timed with
HIP events after a warm-up; prints one JSON line with the median ms per step of each.
usage: python tools/gamma_physics_time.py [rounds] [steps per round] [batch] [--out file.json]"""
import sys

import numpy as np
import torch

import step_timing as st
from graphflow_amd.smp import SMPModel

rounds, steps, B, out_path = st.parse_args(sys.argv[1:])
L, cap, F = 3, 29, 5
mols, targets, _ = st.cfg3_batch(B)

nets, modes = [], {}
for towers in (1, 2):
    for Cn in (16, 32):
        gamma = SMPModel(L, Cn, cap, [F] * towers, nContractions=4)
        gamma.prepare(mols, mols if towers == 2 else None)
        omega = SMPModel(L, Cn, cap, [F] * towers)
        omega.prepare(mols, mols if towers == 2 else None)
        nets += [gamma, omega]
        key = "t%d_C%d" % (towers, Cn)
        for name, net, fused in (("gamma_fused", gamma, True), ("gamma_op_by_op", gamma, False), ("omega", omega, True)):
            p = torch.as_tensor(np.random.default_rng(1).uniform(-0.2, 0.2, net.n_params).astype(np.float32)).cuda()
            modes[key + "_" + name] = (net, fused, p, torch.empty(net.n_params, device="cuda"))


def step(name):
    net, fused, p, g = modes[name]
    if net.__dict__.get("_fused") != fused:   # (set_fused drops the forward state: only on a switch)
        net.set_fused(fused)
        net.__dict__["_fused"] = fused
    net.forward(p, targets)
    net.backward(p, g)


times = st.time_handles(modes, step, rounds, steps)
med = {k: float(np.median(v)) for k, v in times.items()}
keys = sorted({k.rsplit("_gamma", 1)[0].rsplit("_omega", 1)[0] for k in modes})
st.emit({"tool": "gamma_physics_time", "batch": B, "L": L, "cap": cap, "F": F, "rounds": rounds, "steps": steps,
         "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
         "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
         "fused_speedup_vs_op_by_op": {k: round(med[k + "_gamma_op_by_op"] / med[k + "_gamma_fused"], 3) for k in keys},
         "gamma_fused_vs_omega": {k: round(med[k + "_gamma_fused"] / med[k + "_omega"], 3) for k in keys}}, out_path)
for net in nets:
    net.close()
