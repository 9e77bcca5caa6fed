"""One training step (forward + backward + Adam) of SMP_gamma on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, C = 64, F = 5,
D = 5 -- with its fused level, op by op (gf_smp_set_fused(0) on the same handle and batch), and SMP_omega with cap 29 on the same molecules
(the bench.py cfg3 model).  The three run alternately in one process, timed with HIP events after a warm-up; prints one JSON line with the
median ms per step of each.
usage: python tools/gamma_time.py [rounds] [steps per round] [batch] [--out file.json]"""
import sys

import numpy as np

import step_timing as st
from inputs import smp_params
from graphflow_amd.smp import SMPGamma, SMPOmega


def gamma_params(C, F, D, L, seed):
    """Random parameters in SMP_gamma's registration order H[C, F(D+1)], (K_l[4C, C], b_l[C]) x L, W[C], sized like uniform_init's range."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-1, 1, C * F * (D + 1)) / np.sqrt(F * (D + 1))]
    for _ in range(L):
        parts += [rng.uniform(-1, 1, 4 * C * C) / np.sqrt(4 * C), rng.uniform(-0.1, 0.1, C)]
    parts.append(rng.uniform(-1, 1, C) / np.sqrt(C))
    return np.concatenate(parts).astype(np.float32)


rounds, steps, B, out_path = st.parse_args(sys.argv[1:], regions=7)
L, Cn, F, D, cap = 3, 64, 5, 5, 29
mols, targets, maxV = st.cfg3_batch(B)
gamma = SMPGamma(L, Cn, F, D, maxV)
gamma.prepare(mols)
omega = SMPOmega(L, Cn, F, D, cap, True)
omega.prepare(mols)
modes = {   # name: (net, parameters, fused)
    "gamma_fused": (gamma, gamma_params(Cn, F, D, L, 1), True),
    "gamma_op_by_op": (gamma, gamma_params(Cn, F, D, L, 1), False),
    "omega_cap29": (omega, smp_params(Cn, F, D, L, 1), True),
}
state = st.device_state(modes)


def step(name):
    net, _, fused = modes[name]
    p, g = state[name]
    net.set_fused(fused)
    net.forward(p, targets)
    net.backward(p, g)
    net.adam_step(p, g, 1e-6, B)


times = st.time_handles(modes, step, rounds, steps)
med = {k: float(np.median(v)) for k, v in times.items()}
st.emit({"tool": "gamma_time", "batch": B, "L": L, "C": Cn, "F": F, "D": D, "max_nVertices": maxV, "rounds": rounds, "steps": steps,
         "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
         "ms_per_step_all": {k: [round(x, 4) for x in v] for k, v in times.items()},
         "fused_speedup_vs_op_by_op": round(med["gamma_op_by_op"] / med["gamma_fused"], 3),
         "gamma_fused_vs_omega": round(med["gamma_fused"] / med["omega_cap29"], 3)}, out_path)
gamma.close()
omega.close()
