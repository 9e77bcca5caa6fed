"""One forward + backward + Momentum step of LCNN and GCN_MW on the cfg3 batch -- 1024 synthetic QM9-size molecules, F = 5 -- LCNN at
V = 29, k = 10, D = 1, C1 = C2 = 64, nDense = 128 and GCN_MW at L = 3, H = 64, D = 1, alternated in one process: HIP events after a
warm-up, five regions of ten steps, median and min .. max ms per step, and the per-kernel table of one traced step (gf_ctx_set_timing:
the kernels run one by one, so the table says where the time goes, not what the step costs) beside the least bytes each kernel of the
row-list level must move.

In the same process, alternating with it region by region: what the row-list product replaces, on LCNN's two forward products -- the A
operand [nMol V][k Cin] gathered into a buffer by a plain copy kernel (torch.index_select over the sequence) and then the library's tiled
GEMM operator (gf_matmul_forward_f32) -- against gf_smp_rowlist_product_ex_f32 on the same operands.  The operator checks its list on the
host before it launches, so its kernel is timed by the context's per-kernel events (gf_ctx_set_timing), and so is the GEMM of the
alternative; the copy kernel between two HIP events around ten back-to-back launches.
usage: python tools/matrix_form_time.py [regions] [steps per region] [batch] [--out file.json]"""
import ctypes as C
import sys

import numpy as np
import torch

import step_timing as st
from graphflow_amd.ops import matmul_forward
from graphflow_amd.smp import GCNMW, LCNN

regions, steps, B, out_path = st.parse_args(sys.argv[1:])
F, D = 5, 1
FD = F * (D + 1)
mols, targets, maxV = st.cfg3_batch(B)
V, K_NB, C1, C2, ND = max(29, maxV), 10, 64, 64, 128
L, H = 3, 64
LR, GAMMA = 1e-4, 0.9


def small_params(n, seed):
    return (np.random.default_rng(seed).integers(-64, 65, n) / 64.0 * 0.05).astype(np.float32)


modes = {}
for name, net in (("lcnn", LCNN(V, F, K_NB, D, C1, C2, ND)), ("gcn_mw", GCNMW(L, maxV, F, H, D))):
    net.prepare(mols)
    modes[name] = (net, small_params(net.n_params, len(name)))
state = st.device_state(modes)


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    net.step(p, g, LR, B, GAMMA)


times = st.time_handles(modes, step, regions, steps)
kernels = st.trace_one_step({k: net for k, (net, _) in modes.items()}, step)

# ---- the alternative: copy kernel + tiled GEMM, against the row-list product, on LCNN's two forward products ----
lcnn = modes["lcnn"][0]
ctx = lcnn.ctx
R = B * V
seq = np.array([lcnn.receptive_field(m, 1, i) for m in range(B) for i in range(V)], dtype=np.int64)   # [R][k] vertex ids of the molecule
src = (seq + (np.arange(R)[:, None] // V) * V).ravel()
d_ptr = torch.as_tensor(np.arange(R + 1, dtype=np.int64) * K_NB).cuda()
d_src = torch.as_tensor(src.astype(np.int32)).cuda()
d_slot = torch.as_tensor(np.tile(np.arange(K_NB, dtype=np.int32), R)).cuda()
d_idx = torch.as_tensor(src).cuda()
rng = np.random.default_rng(7)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
compare = {}
for label, Cin, N in (("layer1", FD, C1), ("layer2", C1, C2)):
    X = torch.as_tensor(rng.uniform(-1, 1, (R, Cin)).astype(np.float32)).cuda()
    Bm = torch.as_tensor(rng.uniform(-1, 1, (K_NB * Cin, N)).astype(np.float32)).cuda()
    out_new, out_old = torch.empty((R, N), device="cuda"), torch.empty((R, N), device="cuda")
    A = torch.empty((R, K_NB * Cin), device="cuda")

    def new():
        ctx.check(ctx.lib.gf_smp_rowlist_product_ex_f32(ctx.handle, 0, R, K_NB, Cin, N, R, C.c_void_p(d_ptr.data_ptr()), C.c_void_p(d_src.data_ptr()),
                                                        C.c_void_p(d_slot.data_ptr()), None, C.c_void_p(X.data_ptr()), C.c_void_p(Bm.data_ptr()), None,
                                                        0, C.c_void_p(out_new.data_ptr())))

    def gather():
        torch.index_select(X, 0, d_idx, out=A.view(R * K_NB, Cin))

    def kernel_ms(fn):
        """the context's per-kernel events over `steps` calls: ms per call, summed over the kernels the calls launched"""
        ctx.set_timing(True)
        for _ in range(steps):
            fn()
        ms = sum(t for t, _ in ctx.timings().values()) / steps
        ctx.set_timing(False)
        return ms

    new(), gather()
    torch.cuda.synchronize()
    matmul_forward(A, Bm, out=out_old, ctx=ctx)
    torch.cuda.synchronize()
    assert torch.allclose(out_new, out_old, rtol=1e-4, atol=1e-4)
    t = {"rowlist_product": [], "copy": [], "gemm": []}
    for _ in range(regions):
        t["rowlist_product"].append(kernel_ms(new))
        e0.record()
        for _ in range(steps):
            gather()
        e1.record()
        e1.synchronize()
        t["copy"].append(e0.elapsed_time(e1) / steps)
        t["gemm"].append(kernel_ms(lambda: matmul_forward(A, Bm, out=out_old, ctx=ctx)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    compare[label] = {"rows": R, "K": K_NB * Cin, "N": N, "ms_median": {k: round(v, 4) for k, v in med.items()},
                      "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
                      "copy_plus_gemm_ms": round(med["copy"] + med["gemm"], 4),
                      "rowlist_over_copy_plus_gemm": round(med["rowlist_product"] / (med["copy"] + med["gemm"]), 3),
                      "operand_bytes_never_written": 4 * R * K_NB * Cin}

# the least bytes the row-list kernels of one step must move: the source rows once, the matrix or the gradient once, the output; fp32
nV = int(modes["gcn_mw"][0].level_sizes(0)[0])
least = {"lcnn": {"rowlist_gemm layer 1": 4 * (R * FD + K_NB * FD * C1 + R * C1), "rowlist_gemm layer 2": 4 * (R * C1 + K_NB * C1 * C2 + R * C2),
                  "rowlist_gemm_t da1": 4 * (R * C2 + K_NB * C1 * C2 + R * C1), "rowlist_wgrad dF2": 4 * (R * C1 + R * C2 + K_NB * C1 * C2),
                  "rowlist_wgrad dF1": 4 * (R * FD + R * C1 + K_NB * FD * C1)},
         "gcn_mw": {"rowlist_gemm level 0": 4 * (nV * FD + FD * H + nV * H), "rowlist_gemm level l": 4 * (2 * nV * H + H * H),
                    "rowlist_gemm_t level l": 4 * (2 * nV * H + H * H), "rowlist_wgrad level l": 4 * (2 * nV * H + H * H)}}
st.emit({"tool": "matrix_form_time", "batch": B, "F": F, "D": D, "lcnn": {"V": V, "k": K_NB, "C1": C1, "C2": C2, "nDense": ND, "rows": R},
         "gcn_mw": {"L": L, "H": H, "vertices": nV}, "regions": regions, "steps": steps,
         "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "rowlist_product_against_copy_plus_gemm": compare, "least_bytes": least,
         "device_bytes": {k: net.device_bytes()[0] for k, (net, _) in modes.items()},
         "slowest_kernel": {k: next(iter(v)) for k, v in kernels.items()}, "kernels_ms_launches_one_step": kernels}, out_path)
for net, _ in modes.values():
    net.close()
