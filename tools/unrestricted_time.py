"""One training step (forward + backward + Momentum) of Unrestricted_SMP_1D (nChanels = 64), Unrestricted_SMP_1D_ver2 (nChanels = 16,
ending at 128) and Unrestricted_SMP_2D (nChanels = 64) on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, F = 5, D = 5 --
alternated in one process with steps of their restricted siblings on the same molecules: SMP_1D and SMP_2D at 64 channels.  Regions
alternate between the five handles; HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step and the
per-kernel table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not
what the step costs).
usage: python tools/unrestricted_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np

import step_timing as st
from make_smp1d_golden import random_params as params_1d, smp1d_blocks
from make_smp2d_golden import random_params as params_2d
from make_unrestricted_golden import random_params as params_un
from graphflow_amd.smp import SMP1D, SMP2D, SMPUnrestricted

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, F, D = 3, 5, 5
CH = {"unrestricted_1d": 64, "unrestricted_1d_ver2": 16, "unrestricted_2d": 64, "smp_1d": 64, "smp_2d": 64}
mols, targets, maxV = st.cfg3_batch(B)
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
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)
sizes = {name: {l: modes[name][0].level_sizes(l) for l in range(L + 1)} for name in ("unrestricted_1d", "unrestricted_2d")}
st.emit({"tool": "unrestricted_time", "batch": B, "L": L, "channels": CH, "F": F, "D": D, "max_nVertices": maxV, "regions": regions,
         "steps": steps, "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "level_nodes_rows": {k: {str(l): [int(s[0]), int(s[1])] for l, s in v.items()} for k, v in sizes.items()},
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
