"""One training step (forward + backward + Momentum) of SMP_2D_ver5 beside SMP_2D (form 1), both at 64 channels, on the cfg3 batch -- 1024
synthetic QM9-size molecules, L = 3, F = 5, D = 5, no cap -- in one process, the regions alternating between the two handles.  HIP events
after a warm-up; prints one JSON line with the median and min .. max ms per step, the ver5 / form-1 ratio, device_bytes, the per-kernel
table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not what the step
costs), and for the two row projections of ver5 the bytes they must move (S read + f_l written, dz read + dE written; fp32) over the
traced time, beside gf_hbm_copy_probe_f32 (a 1 GiB float4 copy, read + written bytes) in the same process.
usage: python tools/smp2d_ver5_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np
import torch

import step_timing as st
from make_smp2d_golden import random_params as params_2d
from make_smp2d_ver5_golden import random_params as params_ver5
from graphflow_amd.smp import SMP2D

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, F, D, CH = 3, 5, 5, 64
mols, targets, maxV = st.cfg3_batch(B)
modes = {}
for form, name in (("2d", "smp_2d"), ("ver5", "smp_2d_ver5")):
    net = SMP2D(form, maxV, L, CH, F, D)
    net.prepare(mols)
    p = params_2d(1, CH, F * (D + 1), L, maxV, np.random.default_rng(6)) if form == "2d" else \
        params_ver5(CH, F * (D + 1), L, maxV, np.random.default_rng(5))
    modes[name] = (net, p)
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)
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
st.emit({"tool": "smp2d_ver5_time", "batch": B, "L": L, "channels": CH, "F": F, "D": D, "max_nVertices": maxV, "regions": regions,
         "steps": steps, "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "ver5_over_form1": round(med["smp_2d_ver5"] / med["smp_2d"], 4),
         "level_nodes_rows": {str(l): [int(s[0]), int(s[1])] for l, s in sizes.items()},
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "hbm_copy_probe_GBps": round(probe, 1), "row_projections": proj,
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
