"""One training step (forward + backward + Momentum) of NeuralFingerprint, GCN_1D (max_Radius = 2) and GCN_2D on the cfg3 batch -- 1024
synthetic QM9-size molecules, L = 3, F = 5, D = 5 for the two GCNs (F' = 30), D = 0 for the fingerprint -- at H = 64 and at H = 20, the
demo's width, alternated in one process with steps of SMP_1D at 64 channels on the same molecules as context.  Regions alternate
between the seven handles; HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step, the per-kernel
table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes, not what the
step costs), and for the three level kernels the bytes they must move (every operand once, fp32, summed over the levels) over the
traced time, beside gf_hbm_copy_probe_f32 (a 1 GiB float4 copy, read + written bytes) in the same process.
usage: python tools/neighbourhood_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np
import torch

import step_timing as st
from make_neighbourhood_golden import random_params as params_nb
from make_smp1d_golden import random_params as params_1d, smp1d_blocks
from graphflow_amd.smp import SMP1D, SMPNeighbourhood

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, F, D, R = 3, 5, 5, 2
mols, targets, maxV = st.cfg3_batch(B)
modes, shape = {}, {}
for H in (64, 20):
    for form, name in (("fingerprint", "fingerprint"), ("gcn_1d", "gcn_1d"), ("gcn_2d", "gcn_2d")):
        d = 0 if form == "fingerprint" else D
        net = SMPNeighbourhood(form, L, H, F, d, maxV, R)
        net.prepare(mols)
        key = "%s_h%d" % (name, H)
        modes[key] = (net, params_nb(SMPNeighbourhood.FORMS[form], H, F * (d + 1), L, np.random.default_rng(H + len(name)), 0.5))
        shape[key] = (SMPNeighbourhood.FORMS[form], H, F * (d + 1))
one = SMP1D(1, maxV, L, 64, F, D)
one.prepare(mols)
modes["smp_1d"] = (one, params_1d(smp1d_blocks(1, 64, F * (D + 1), L, maxV), np.random.default_rng(1)))
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)
a = torch.empty(1 << 28, device="cuda")
b = torch.empty(1 << 28, device="cuda")
probe = one.ctx.hbm_copy_probe(b, a, 0, 5)
nV = int(modes["gcn_1d_h64"][0].level_sizes(0)[0])


def level_bytes(form, H, FD):
    """bytes one step's launches of each level kernel must move, every operand once: forward h_{l-1} and x read, h_l and n_l written
    (level 0: x read, h_0 written); node backward h_l and dh_l read (the top level reads no dh), dz and dn written (level 0: dz only);
    the gather dn read and dh_{l-1} written.  Form 3 adds A (written / read), dn Tt (written / read) and h_{l-1} in the gather."""
    vec = 4 * nV * H
    pairs = form == 3
    fwd = (L + 1) * (4 * nV * FD + vec) + L * (2 + pairs) * vec
    node = (L + 1) * 2 * vec + L * vec + L * (2 * vec if pairs else 0)   # (h, dz) everywhere, dh below the top, dn (, A, dn Tt) above level 0
    gather = L * (2 + 2 * pairs) * vec
    return {"nbh_level_fwd": fwd, "nbh_node_bwd": node, "nbh_gather_bwd": gather}


moved = {}
for key, (form, H, FD) in shape.items():
    moved[key] = {}
    for k, nbytes in level_bytes(form, H, FD).items():
        gbps = nbytes / (kernels[key][k][0] * 1e-3) / 1e9
        moved[key][k] = {"bytes": int(nbytes), "GBps": round(gbps, 1), "fraction_of_copy_probe": round(gbps / probe, 4)}
st.emit({"tool": "neighbourhood_time", "batch": B, "L": L, "F": F, "D_gcn": D, "max_Radius": R, "max_nVertices": maxV, "vertices": nV,
         "regions": regions, "steps": steps, "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()}, "hbm_copy_probe_GBps": round(probe, 1),
         "level_kernels": moved, "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()},
         "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
