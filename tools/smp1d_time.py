"""One training step (forward + backward + Momentum) of SMP_1D, SMP_1D_ver2 and SMP_1D_ver3 on the cfg3 batch -- 1024 synthetic QM9-size
molecules, L = 3, nChanels = 16 (the concatenating forms end at 128 channels), F = 5, D = 5, no cap -- with an SMP_theta step (forward +
backward + Adam) at the same settings on the same molecules in the same process.  Regions alternate between the four handles; HIP events
after a warm-up; prints one JSON line with the median and min .. max ms per step, and the per-kernel table of one traced step of each form
(gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not what the step costs).
usage: python tools/smp1d_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np

import step_timing as st
from make_smp1d_golden import random_params as params_1d, smp1d_blocks
from make_theta_golden import random_params as params_theta, theta_blocks
from graphflow_amd.smp import SMP1D, SMPTheta

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, Cn, F, D = 3, 16, 5, 5
mols, targets, maxV = st.cfg3_batch(B)
modes = {}
for version, name in ((1, "smp_1d"), (2, "smp_1d_ver2"), (3, "smp_1d_ver3")):
    net = SMP1D(version, maxV, L, Cn, F, D)
    net.prepare(mols)
    modes[name] = (net, params_1d(smp1d_blocks(version, Cn, F * (D + 1), L, maxV), np.random.default_rng(version)))
theta = SMPTheta(maxV, maxV, L, Cn, F, D)
theta.prepare(mols)
modes["theta"] = (theta, params_theta(theta_blocks(Cn, F * (D + 1), L, maxV), np.random.default_rng(1)))
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    if name == "theta":
        net.adam_step(p, g, 1e-6, B)
    else:
        net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)
sizes = {l: theta.level_sizes(l) for l in range(L + 1)}
st.emit({"tool": "smp1d_time", "batch": B, "L": L, "C": Cn, "F": F, "D": D, "max_nVertices": maxV, "regions": regions, "steps": steps,
         "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "level_nodes_rows": {str(l): [int(s[0]), int(s[1])] for l, s in sizes.items()},
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
