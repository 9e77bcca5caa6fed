"""One training step (forward + backward + Momentum) of GCN_1D_Distance, GCN_2D_Distance and GCN_3D_Distance on the cfg3 batch -- 1024
synthetic QM9-size molecules with a distance matrix each (pairwise distances of random points, rounded to 1/16), L = 3, F = 5, D = 5
(F' = 30), max_Radius = 2, M = the batch's largest vertex count -- at H = 64 and at H = 20, alternated in one process with GCN_1D,
GCN_2D and GCN_3D at the same shapes, and with the same distance handles under GF_SMP_DISTANCE_LAUNCHES=2 (every level kernel once
per channel instead of one launch for both: the comparison the two-channel launch has to win or lose).  Regions alternate between the
handles; HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step and the per-kernel table of one
traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not what the step costs).
usage: python tools/distance_time.py [regions] [steps per region] [batch] [--out file.json]"""
import os
import sys

import numpy as np

import step_timing as st
from make_distance_golden import point_distances, random_params as params_dist
from make_neighbourhood_golden import random_params as params_nb
from graphflow_amd.smp import SMPDistance, SMPNeighbourhood

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, F, D, R = 3, 5, 5, 2
mols, targets, maxV = st.cfg3_batch(B)
rng = np.random.default_rng(3)
with_dist = [(a, f, point_distances(len(a), rng)) for a, f in mols]
SWITCH = "GF_SMP_DISTANCE_LAUNCHES"
modes, per_channel = {}, set()
for H in (64, 20):
    for dim, form in ((1, 2), (2, 3), (3, 6)):
        plain = SMPNeighbourhood("gcn_%dd" % dim, L, H, F, D, maxV, R)
        plain.prepare(mols)
        modes["gcn_%dd_h%d" % (dim, H)] = (plain, params_nb(form, H, F * (D + 1), L, np.random.default_rng(H + dim), 0.5))
        for suffix in ("", "_per_channel"):   # (two handles on the same weights, so that neither mode inherits the other's warm state)
            net = SMPDistance("gcn_%dd_distance" % dim, L, H, F, D, maxV, R)
            net.prepare(with_dist)
            key = "gcn_%dd_distance_h%d%s" % (dim, H, suffix)
            modes[key] = (net, params_dist(form, H, F * (D + 1), maxV, L, np.random.default_rng(H + dim), 0.5))
            if suffix:
                per_channel.add(key)
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    if name in per_channel:
        os.environ[SWITCH] = "2"
    net.forward(p, targets)
    net.backward(p, g)
    os.environ.pop(SWITCH, None)
    net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)
med = st.summary(times)["ms_per_step_median"]
ratio = {k: round(med[k + "_per_channel"] / med[k], 4) for k in med if k + "_per_channel" in med}
st.emit({"tool": "distance_time", "batch": B, "L": L, "F": F, "D": D, "max_Radius": R, "max_nVertices": maxV,
         "vertices": int(modes["gcn_1d_distance_h64"][0].level_sizes(0)[0]), "regions": regions, "steps": steps,
         "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "per_channel_over_two_channel": ratio, "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
