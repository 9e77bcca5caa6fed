"""One forward + backward step of GCN_3D and GRU_GCN_3D on the cfg3 batch -- 1024 synthetic QM9-size molecules, H = 64, L = 3, F = 5,
D = 5 (F' = 30), max_Radius = 2 -- alternated in one process with GCN_2D and GRU_GCN_2D at the same shape: the third-order forms are
their siblings' update kernels behind the pool of smp_level_third.hip (45,760 classes of m multiply-adds per vertex and level, in every
pass of the radix select), so the ratio of the two and the share of the two pool kernels is what the tool is for.  Regions alternate
between the four handles; HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step, the third-order
forms' multiple of their second-order siblings, the pool kernels' share of one traced step (gf_ctx_set_timing: the kernels run one by one,
so the table says where the time goes, not what the step costs) and the per-kernel table.
usage: python tools/third_order_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np

import step_timing as st
from make_gru_gcn_golden import random_params as params_gru
from make_neighbourhood_golden import random_params as params_nb
from make_third_order_golden import random_params as params_third
from graphflow_amd.smp import SMPGatedNeighbourhood, SMPNeighbourhood

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, H, F, D, R = 3, 64, 5, 5, 2
FD = F * (D + 1)
mols, targets, maxV = st.cfg3_batch(B)
modes = {}
for form, cls in (("gcn_2d", SMPNeighbourhood), ("gcn_3d", SMPNeighbourhood), ("gru_gcn_2d", SMPGatedNeighbourhood), ("gru_gcn_3d", SMPGatedNeighbourhood)):
    net = cls(form, L, H, F, D, maxV, R)
    net.prepare(mols)
    rng, code = np.random.default_rng(H + len(form)), cls.FORMS[form]
    modes[form] = (net, params_third(code, H, FD, L, rng, 0.5) if code >= 6 else params_nb(code, H, FD, L, rng, 0.5) if code == 3 else
                   params_gru(code, H, FD, rng, 0.5))
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


def pool_share(table):
    total = sum(ms for ms, _ in table.values())
    return {k: round(table[k][0] / total, 4) for k in ("third_pool_fwd", "third_pool_bwd") if k in table}


st.emit({"tool": "third_order_time", "batch": B, "L": L, "H": H, "F": F, "D": D, "max_Radius": R, "max_nVertices": maxV,
         "vertices": int(modes["gcn_3d"][0].level_sizes(0)[0]), "regions": regions, "steps": steps,
         "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **summary,
         "third_over_second": {"gcn": round(med["gcn_3d"] / med["gcn_2d"], 3), "gru_gcn": round(med["gru_gcn_3d"] / med["gru_gcn_2d"], 3)},
         "pool_share_of_traced_step": {k: pool_share(kernels[k]) for k in ("gcn_3d", "gru_gcn_3d")},
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
