"""The two read-outs of gf_smp_config.readout on the cfg3 batch -- 1024 synthetic QM9-size molecules, L = 3, F = 5, D = 5 (F' = 30),
max_Radius = 2, H = 64 -- in one process, alternating:
  pairs   one training step (forward + backward + Momentum) of GCN_1D_Kernel, GCN_2D_Kernel and GCN_3D_Kernel on the batch taken as 512
          pairs (X_p = molecule 2 p, Y_p = molecule 2 p + 1) beside GCN_1D, GCN_2D and GCN_3D on the same 1024 graphs: only the read-out
          differs;
  GCA     one step of GCA_1D beside GCN_1D's;
  Gram    gram_readout alone (gf_smp_gram_readout_ex_f32 on the batch's vertex counts, adjacency values and random h_L; the kernel's own
          time from the context's kernel timing) beside the same arithmetic in torch on zero-padded [nMol][M][H] tensors: bmm for G, the
          loss, bmm for (E + E^T) h, between HIP events.
Regions alternate between the handles; HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step and
the per-kernel table of one traced step of each (gf_ctx_set_timing: the kernels run one by one, so the table says where the time goes,
not what the step costs).
usage: python tools/pair_gram_time.py [regions] [steps per region] [batch] [--out file.json]"""
import ctypes as C
import sys

import numpy as np
import torch

import step_timing as st
from make_neighbourhood_golden import random_params as params_nb
from graphflow_amd.smp import GCA1D, SMPKernelPairs, SMPNeighbourhood

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
L, F, D, R, H = 3, 5, 5, 2, 64
mols, targets, maxV = st.cfg3_batch(B)
pair_targets = (targets[0::2] - targets[1::2]).contiguous()
xs, ys = mols[0::2], mols[1::2]
modes = {}
for dim, form in ((1, 2), (2, 3), (3, 6)):
    base = params_nb(form, H, F * (D + 1), L, np.random.default_rng(H + dim), 0.5)   # W1_0; W1_l, W2_l; W [H]
    plain = SMPNeighbourhood("gcn_%dd" % dim, L, H, F, D, maxV, R)
    plain.prepare(mols)
    modes["gcn_%dd" % dim] = (plain, base, targets)
    pairs = SMPKernelPairs("gcn_%dd_kernel" % dim, L, maxV, F, H, D, R)
    pairs.prepare(xs, ys)
    modes["gcn_%dd_kernel" % dim] = (pairs, np.concatenate([base, base[-H:]]), pair_targets)   # (the same levels; W [2 H])
    if dim == 1:
        gca = GCA1D(L, maxV, F, H, D, R)
        gca.prepare(mols)
        modes["gca_1d"] = (gca, base[:-H], None)
state = st.device_state(modes)


def step(name):
    net, _, tg = modes[name]
    p, g = state[name]
    net.forward(p, tg) if tg is not None else net.forward(p)
    net.backward(p, g)
    net.step(p, g, 1e-6, B)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: m[0] for k, m in modes.items()}, step)
med = st.summary(times)["ms_per_step_median"]

# ---- gram_readout alone against the torch formulation ----
ctx = modes["gca_1d"][0].ctx
sizes = np.array([len(a) for a, _ in mols])
mp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
nV, nG = int(mp[-1]), int((sizes * sizes).sum())
rng = np.random.default_rng(1)
hL = torch.as_tensor(rng.random((nV, H)).astype(np.float32) * np.float32(2.0 / H)).cuda()
adj = torch.as_tensor(np.concatenate([np.asarray(a, dtype=np.float32).ravel() for a, _ in mols])).cuda()
mol_ptr = torch.as_tensor(mp).cuda()
gram, loss, dh = torch.empty(nG, device="cuda"), torch.empty(B, device="cuda"), torch.empty((nV, H), device="cuda")


def gram_kernel():
    ctx.check(ctx.lib.gf_smp_gram_readout_ex_f32(ctx.handle, H, nV, B, C.c_void_p(hL.data_ptr()), C.c_void_p(mol_ptr.data_ptr()), C.c_void_p(adj.data_ptr()),
                                                 C.c_void_p(gram.data_ptr()), C.c_void_p(loss.data_ptr()), C.c_void_p(dh.data_ptr())))


hp = torch.zeros((B, maxV, H), device="cuda")     # the zero-padded operands of the torch formulation, built once (not timed)
ap = torch.zeros((B, maxV, maxV), device="cuda")   # (padded rows of h are zero, so G and E vanish outside a molecule's block: no mask)
for m, (a, _) in enumerate(mols):
    V = len(a)
    hp[m, :V] = hL[mp[m]:mp[m + 1]]
    ap[m, :V, :V] = torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda()


def gram_torch():
    G = torch.bmm(hp, hp.transpose(1, 2))
    E = G - ap
    return G, 0.5 * (E * E).sum(dim=(1, 2)), torch.bmm(E + E.transpose(1, 2), hp)


for _ in range(3):
    gram_kernel()
    gram_torch()
torch.cuda.synchronize()
G_t, loss_t, dh_t = gram_torch()
gram_kernel()
torch.cuda.synchronize()
agree = {"loss": float((loss - loss_t).abs().max() / loss_t.abs().max()),
         "dh": float(max((dh[mp[m]:mp[m + 1]] - dh_t[m, :sizes[m]]).abs().max() for m in range(0, B, 37)) / dh_t.abs().max())}
kernel_ms, torch_ms = [], []
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for r in range(regions):
    ctx.set_timing(True)
    for _ in range(steps):
        gram_kernel()
    ms, n = ctx.timings()["gram_readout"]
    ctx.set_timing(False)
    kernel_ms.append(ms / n)
    gram_torch()
    e0.record()
    for _ in range(steps):
        gram_torch()
    e1.record()
    e1.synchronize()
    torch_ms.append(e0.elapsed_time(e1) / steps)
gram_record = {"H": H, "vertices": nV, "gram_floats": nG, "max_nVertices": maxV,
               "gram_readout_ms_median": round(float(np.median(kernel_ms)), 5), "gram_readout_ms_min_max": [round(min(kernel_ms), 5), round(max(kernel_ms), 5)],
               "torch_bmm_ms_median": round(float(np.median(torch_ms)), 5), "torch_bmm_ms_min_max": [round(min(torch_ms), 5), round(max(torch_ms), 5)],
               "kernel_over_torch": round(float(np.median(kernel_ms) / np.median(torch_ms)), 4), "agreement_with_torch": agree}

st.emit({"tool": "pair_gram_time", "batch": B, "pairs": B // 2, "L": L, "F": F, "D": D, "H": H, "max_Radius": R, "max_nVertices": maxV, "vertices": nV,
         "regions": regions, "steps": steps, "n_params": {k: int(m[0].n_params) for k, m in modes.items()}, **st.summary(times),
         "pair_over_single": {"gcn_%dd" % d: round(med["gcn_%dd_kernel" % d] / med["gcn_%dd" % d], 4) for d in (1, 2, 3)},
         "gca_over_gcn_1d": round(med["gca_1d"] / med["gcn_1d"], 4), "gram_alone": gram_record,
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, *_ in modes.values():
    net.close()
