"""One training step (forward + backward + Adam) of SMP_theta on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, C = 64, F = 5,
D = 5, cap 29 -- with SMP_gamma and SMP_omega (cap 29) steps on the same molecules in the same process for scale.  Five timed regions per
model, alternated, HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step and the per-kernel table of
one traced SMP_theta step (gf_ctx_set_timing).  `--kernels-only` runs a few SMP_theta steps and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --` for the profiler's own per-kernel table.
usage: python tools/theta_time.py [regions] [steps per region] [batch] [--out file.json] [--kernels-only]"""
import sys

import numpy as np
import torch

import step_timing as st
from inputs import smp_params
from make_theta_golden import random_params, theta_blocks
from graphflow_amd.smp import SMPGamma, SMPOmega, SMPTheta
from make_gamma_golden import gamma_params

kernels_only = "--kernels-only" in sys.argv
regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, Cn, F, D, cap = 3, 64, 5, 5, 29
mols, targets, maxV = st.cfg3_batch(B)
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
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    net.adam_step(p, g, 1e-6, B)


if kernels_only:
    for _ in range(3 + steps):   # (three of them the warm-up)
        step("theta")
    torch.cuda.synchronize()
    theta.close()
    sys.exit(0)
times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({"theta": theta}, step)["theta"]
sizes = {l: theta.level_sizes(l) for l in range(L + 1)}
st.emit({"tool": "theta_time", "batch": B, "L": L, "C": Cn, "F": F, "D": D, "cap": cap, "max_nVertices": maxV, "regions": regions,
         "steps": steps, "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "theta_level_nodes_rows": {str(l): [int(s[0]), int(s[1])] for l, s in sizes.items()},
         "theta_device_bytes": theta.device_bytes()[0], "slowest_kernel": next(iter(kernels)),
         "theta_kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
