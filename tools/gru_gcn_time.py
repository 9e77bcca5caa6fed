"""One forward + backward step of GRU_GCN_1D and GRU_GCN_2D on the cfg3 batch -- 1024 synthetic QM9-size molecules, H = 64, L = 3, F = 5,
D = 5 (F' = 30), max_Radius = 2 -- alternated in one process with GCN_1D and GCN_2D at the same shape: the gated level does about four
times the products of a GCN level, so the ratio of the two is what the tool is for.  Regions alternate between the four handles; HIP
events after a warm-up; prints one JSON line with the median and min .. max ms per step, the gated forms' multiple of their GCN
siblings, and the per-kernel table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where
the time goes, not what the step costs).
usage: python tools/gru_gcn_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np

import step_timing as st
from make_gru_gcn_golden import random_params as params_gru
from make_neighbourhood_golden import random_params as params_nb
from graphflow_amd.smp import SMPGatedNeighbourhood, SMPNeighbourhood

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, H, F, D, R = 3, 64, 5, 5, 2
FD = F * (D + 1)
mols, targets, maxV = st.cfg3_batch(B)
modes = {}
for form in ("gcn_1d", "gcn_2d"):
    net = SMPNeighbourhood(form, L, H, F, D, maxV, R)
    net.prepare(mols)
    modes[form] = (net, params_nb(SMPNeighbourhood.FORMS[form], H, FD, L, np.random.default_rng(H + len(form)), 0.5))
for form in ("gru_gcn_1d", "gru_gcn_2d"):
    net = SMPGatedNeighbourhood(form, L, H, F, D, maxV, R)
    net.prepare(mols)
    modes[form] = (net, params_gru(SMPGatedNeighbourhood.FORMS[form], H, FD, np.random.default_rng(H + len(form)), 0.5))
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)
summary = st.summary(times)
med = summary["ms_per_step_median"]
st.emit({"tool": "gru_gcn_time", "batch": B, "L": L, "H": H, "F": F, "D": D, "max_Radius": R, "max_nVertices": maxV,
         "vertices": int(modes["gru_gcn_1d"][0].level_sizes(0)[0]), "regions": regions, "steps": steps,
         "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **summary,
         "gated_over_gcn": {"1d": round(med["gru_gcn_1d"] / med["gcn_1d"], 3), "2d": round(med["gru_gcn_2d"] / med["gcn_2d"], 3)},
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
