"""One training step (forward + backward + Momentum) of SMP_2D (nChanels = 64) and SMP_2D_ver4 (nChanels = 16, ending at 128) on the cfg3
batch -- 1024 synthetic QM9-size molecules, L = 3, F = 5, D = 5, no cap -- framed by two steps on the same molecules in the same process:
SMP_1D at 64 channels (the same structure on sum-s rows, Momentum) and SMP_omega at 64 channels without a cap (second order on the same
sum-s^2 rows, Adam).  Regions alternate between the four handles; HIP events after a warm-up; prints one JSON line with the median and
min .. max ms per step, the per-kernel table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table
says where the time goes, not what the step costs), and for the three kernels of the steerable level the bytes they must move at least
(every input once, every output once, fp32) with the fraction of 8 TB/s that makes in the traced time.
usage: python tools/smp2d_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np

import step_timing as st
from inputs import smp_params
from make_smp1d_golden import random_params as params_1d, smp1d_blocks
from make_smp2d_golden import random_params as params_2d
from graphflow_amd.smp import SMP1D, SMP2D, SMPOmega

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, F, D = 3, 5, 5
CH = {"smp_2d": 64, "smp_2d_ver4": 16, "smp_1d": 64, "smp_omega": 64}
mols, targets, maxV = st.cfg3_batch(B)
modes = {}
for form, name in (("2d", "smp_2d"), ("ver4", "smp_2d_ver4")):
    net = SMP2D(form, maxV, L, CH[name], F, D)
    net.prepare(mols)
    modes[name] = (net, params_2d(SMP2D.FORMS[form], CH[name], F * (D + 1), L, maxV, np.random.default_rng(len(name))))
one = SMP1D(1, maxV, L, CH["smp_1d"], F, D)
one.prepare(mols)
modes["smp_1d"] = (one, params_1d(smp1d_blocks(1, CH["smp_1d"], F * (D + 1), L, maxV), np.random.default_rng(1)))
omega = SMPOmega(L, CH["smp_omega"], F, D, maxV)
omega.prepare(mols)
modes["smp_omega"] = (omega, smp_params(CH["smp_omega"], F, D, L, 3))
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    if name == "smp_omega":
        net.adam_step(p, g, 1e-6, B)
    else:
        net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)


def level_bytes(name):
    """the least the three kernels of the steerable level move over the L levels of one step, in bytes"""
    net = modes[name][0]
    sz = [net.level_sizes(l) for l in range(L + 1)]
    fwd = node = gather = 0
    for l in range(1, L + 1):
        rows, rows_p, Cp, Cc = sz[l][1], sz[l - 1][1], net.level_channels(l - 1), net.level_channels(l)
        fwd += 4 * (rows_p * Cp + rows + rows * Cp + rows * Cc)                               # f_{l-1}, adj -> S, f_l
        node += 4 * (rows * Cc + (rows * Cc if l < L else 0) + rows * Cp + rows + rows * Cp)   # f_l, df_l, S, adj -> dS
        gather += 4 * (rows * Cp + rows_p * Cp)                                                # dS -> df_{l-1}
    return {"smp2d_level_fwd": fwd, "smp2d_node_bwd": node, "smp2d_gather_bwd": gather}


traffic = {}
for name in ("smp_2d", "smp_2d_ver4"):
    traffic[name] = {k: {"min_bytes": int(b), "fraction_of_8TBps": round(b / (kernels[name][k][0] * 1e-3) / 8e12, 4)}
                     for k, b in level_bytes(name).items()}
sizes = {l: modes["smp_2d"][0].level_sizes(l) for l in range(L + 1)}
st.emit({"tool": "smp2d_time", "batch": B, "L": L, "channels": CH, "F": F, "D": D, "max_nVertices": maxV, "regions": regions, "steps": steps,
         "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "level_nodes_rows": {str(l): [int(s[0]), int(s[1])] for l, s in sizes.items()},
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "level_kernel_traffic": traffic,
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
