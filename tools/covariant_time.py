"""CGCN_1D and CGCN_2D (gf_smp_config.covariant = 1, 2) on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, F = 5, D = 5
(F' = 30), M = max_nVertices = the batch's largest molecule (29) -- in one process, alternating:
  step    one training step (forward + backward + Momentum) of CGCN_1D and CGCN_2D beside GCN_1D and GCN_2D at H = 64, max_Radius = 2;
  sweeps  forward + backward of the covariant handles alone (cov_network_fwd, cov_network_bwd, cov_fold and the two small copies of a
          forward: everything a step launches but the optimiser) beside the same arithmetic written level by level in torch on
          zero-padded [nMol][M][M] tensors -- per level one bmm for the aggregate, one matmul with F_l, the mask as a multiply, LeakyReLU;
          the reverse through torch's autograd.  The padding is built beforehand and not timed.  Both between HIP events.
The claim under test: one launch per direction beats a per-level formulation.  The ratio is reported whatever it is, with the agreement
of the two results (prediction and the gradient of every F_l, relative to the largest entry).
Regions alternate between the handles; HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step and
the per-kernel table of one traced step of each.
usage: python tools/covariant_time.py [regions] [steps per region] [batch] [--out file.json]"""
import sys

import numpy as np
import torch

import step_timing as st
from make_neighbourhood_golden import random_params as params_nb
from graphflow_amd.smp import CGCN1D, CGCN2D, SMPNeighbourhood

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, F, D, R, H = 3, 5, 5, 2, 64
FD = F * (D + 1)
mols, targets, M = st.cfg3_batch(B)
modes = {}
rng = np.random.default_rng(29)
for form, cls in ((1, CGCN1D), (2, CGCN2D)):
    # (weights that keep the activations of three levels within fp32's normal range: uniform_init's shrink a 2D network by the square per level)
    p = np.concatenate([rng.uniform(0.25, 1.0, FD)] + [rng.uniform(0.2, 1.0, M * M) / (4.0 if form == 1 else 16.0) for _ in range(L)])
    net = cls(L, M, F, D)
    net.prepare(mols)
    modes["cgcn_%dd" % form] = (net, p, targets)
for dim, form in ((1, 2), (2, 3)):
    net = SMPNeighbourhood("gcn_%dd" % dim, L, H, F, D, M, R)
    net.prepare(mols)
    modes["gcn_%dd" % dim] = (net, params_nb(form, H, FD, L, np.random.default_rng(H + dim), 0.5), targets)
state = st.device_state(modes)


def step(name):
    net, _, tg = modes[name]
    p, g = state[name]
    net.forward(p, tg)
    net.backward(p, g)
    net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: m[0] for k, m in modes.items()}, step)
med = st.summary(times)["ms_per_step_median"]

# ---- the two network kernels against the level-by-level formulation in torch ----
sizes = np.array([len(a) for a, _ in mols])
AT = torch.zeros((B, M, M), device="cuda")            # AT[m][v][u] = 1 where u in N(v), i.e. adj[u][v] > 0
masks = torch.zeros((L + 1, B, M, M), device="cuda")   # masks[l][m][v][i] = 1 where sp[i][v] <= l
x0 = torch.zeros((B, M, FD), device="cuda")            # the shell sums, as the handle's preparation derives them
sys.path.insert(0, st.os.path.join(st.ROOT, "tests"))
import cgcn_ref as cref  # noqa: E402
from neighbourhood_ref import hop_distances, shell_features  # noqa: E402
for m, (a, f) in enumerate(mols):
    V = len(a)
    sp = hop_distances(a)
    AT[m, :V, :V] = torch.as_tensor((np.asarray(a).T > 0).astype(np.float32)).cuda()
    masks[:, m, :V] = torch.as_tensor(cref.masks(a, L, M, sp).astype(np.float32)).cuda()
    x0[m, :V] = torch.as_tensor(shell_features(np.asarray(f, dtype=np.float64), sp, D).astype(np.float32)).cuda()
eye = torch.eye(M, device="cuda")


def torch_sweeps(form, p):
    Hw = p[:FD]
    Fs = [p[FD + l * M * M:FD + (l + 1) * M * M].reshape(M, M).clone().requires_grad_(True) for l in range(L)]
    h = eye * (x0 @ Hw)[:, :, None]
    for l in range(L):
        if form == 1:
            n = torch.bmm(AT, h)
        else:
            s = h.sum(dim=2)
            S = torch.bmm(AT, s[:, :, None])
            n = torch.bmm(AT * (S - s[:, None, :]), h)
        z = (n @ Fs[l].T) * masks[l + 1]
        h = torch.nn.functional.leaky_relu(z, 0.01)
    y = h.sum(dim=(1, 2))
    loss = 0.5 * ((y - targets) ** 2).sum()
    grads = torch.autograd.grad(loss, Fs)
    return y, grads


sweeps = {}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for form in (1, 2):
    name = "cgcn_%dd" % form
    net = modes[name][0]
    p, g = torch.as_tensor(np.asarray(modes[name][1], dtype=np.float32)).cuda(), torch.empty(net.n_params, device="cuda")

    def ours():
        net.forward(p, targets)
        net.backward(p, g)

    for _ in range(3):
        ours()
        torch_sweeps(form, p)
    torch.cuda.synchronize()
    y_t, g_t = torch_sweeps(form, p)
    ours()
    torch.cuda.synchronize()
    agree = {"predict": float((net.predict - y_t).abs().max() / y_t.abs().max())}
    for l in range(L):
        ours_F = g[FD + l * M * M:FD + (l + 1) * M * M].reshape(M, M)
        agree["dF_%d" % (l + 1)] = float((ours_F - g_t[l]).abs().max() / g_t[l].abs().max())
    ours_ms, torch_ms = [], []
    for r in range(regions):
        for fn, rec in ((ours, ours_ms), (lambda: torch_sweeps(form, p), torch_ms)):
            fn()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            rec.append(e0.elapsed_time(e1) / steps)
    sweeps[name] = {"one_launch_per_direction_ms_median": round(float(np.median(ours_ms)), 5),
                    "one_launch_per_direction_ms_min_max": [round(min(ours_ms), 5), round(max(ours_ms), 5)],
                    "torch_per_level_ms_median": round(float(np.median(torch_ms)), 5),
                    "torch_per_level_ms_min_max": [round(min(torch_ms), 5), round(max(torch_ms), 5)],
                    "ours_over_torch": round(float(np.median(ours_ms) / np.median(torch_ms)), 4), "agreement_with_torch": agree}

st.emit({"tool": "covariant_time", "batch": B, "L": L, "F": F, "D": D, "H_of_gcn": H, "max_Radius_of_gcn": R, "max_nVertices": int(M),
         "vertices": int(sizes.sum()), "regions": regions, "steps": steps, "n_params": {k: int(m[0].n_params) for k, m in modes.items()},
         **st.summary(times), "cgcn_over_gcn": {"1d": round(med["cgcn_1d"] / med["gcn_1d"], 4), "2d": round(med["cgcn_2d"] / med["gcn_2d"], 4)},
         "forward_backward_alone": sweeps, "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()},
         "kernels_ms_launches_one_step": kernels}, out_path)
for net, *_ in modes.values():
    net.close()
