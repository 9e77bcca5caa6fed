"""One training step (forward + backward + Adam) of CCN_1D at the reference demo's settings -- 10 / 10 vertices, cap 6, 7 levels, 16
channels, decay 0.5 (tests/test_CCN_1D.cpp) -- on a synthetic batch of 1024 pairs of 3- to 10-vertex molecules (F = 5), with
SMP_theta_pairgraphs at 16 channels (16 -> 8 -> 4 -> 2 -> 1 ..) on the same pairs in the same process for scale.  Five timed regions per
model, alternated, HIP events after a warm-up; prints one JSON line with the median and min .. max ms per step, and of one traced step
per model (gf_ctx_set_timing) the per-kernel table, the number of launches and the sum of the kernel times: a step much longer than its
kernels' sum is bound by its launches.  `--kernels-only` runs a few CCN_1D steps and nothing else: the program to put behind
`rocprofv3 --kernel-trace --stats --` for the profiler's own per-kernel table.
usage: python tools/ccn1d_time.py [regions] [steps per region] [batch] [--out file.json] [--kernels-only]"""
import sys

import numpy as np
import torch

import step_timing as st
from inputs import synthetic_molecule
from make_ccn1d_golden import random_params
from make_theta_golden import model_blocks
from make_theta_golden import random_params as theta_params
from graphflow_amd.smp import CCN1D, SMPModel

kernels_only = "--kernels-only" in sys.argv
regions, steps, B, out_path = st.parse_args(sys.argv[1:])
maxV, cap, L, Cn, F, decay = 10, 6, 7, 16, 5, 0.5
g1, g2, tg = [], [], []
for i in range(B):
    a, fa, ta = synthetic_molecule(i, 3 + i % 8)
    b, fb, tb = synthetic_molecule(50000 + i, 3 + (i // 8) % 8)
    g1.append((a, fa))
    g2.append((b, fb))
    tg.append(ta - tb)
targets = torch.as_tensor(np.array(tg, dtype=np.float32)).cuda()
ccn = CCN1D(maxV, maxV, cap, L, Cn, F, F, decay)
ccn.prepare(g1, g2)
modes = {"ccn_1d": (ccn, random_params(Cn, L, [F, F], [maxV, maxV], decay, [np.ones(F), np.ones(F)], np.random.default_rng(1)))}
if not kernels_only:
    pair = SMPModel(L, Cn, cap, [F, F], first_order=True, max_nVertices=[maxV, maxV])
    pair.prepare(g1, g2)
    modes["theta_pairgraphs"] = (pair, theta_params(model_blocks(2, Cn, L, [F, F], [maxV, maxV]), np.random.default_rng(1)))
state = st.device_state(modes)
for k, (net, p) in modes.items():
    assert len(p) == net.n_params, k


def step(name):
    net = modes[name][0]
    p, g = state[name]
    net.forward(p, targets)
    net.backward(p, g)
    net.adam_step(p, g, 1e-6, B)


if kernels_only:
    for _ in range(3 + steps):   # (three of them the warm-up)
        step("ccn_1d")
    torch.cuda.synchronize()
    ccn.close()
    sys.exit(0)
times = st.time_handles(modes, step, regions, steps)
traced = {name: {"launches": sum(n for _, n in t.values()), "kernel_ms_sum": round(sum(ms for ms, _ in t.values()), 4), "kernels_ms_launches": t}
          for name, t in st.trace_one_step({k: net for k, (net, _) in modes.items()}, step).items()}
st.emit({"tool": "ccn1d_time", "batch": B, "L": L, "C": Cn, "F": F, "cap": cap, "max_nVertices": maxV, "decay": decay,
         "regions": regions, "steps": steps, "vertices": [int(sum(len(a) for a, _ in g)) for g in (g1, g2)],
         "n_params": {k: int(net.n_params) for k, (net, _) in modes.items()}, **st.summary(times),
         "slowest_kernel": {k: next(iter(t["kernels_ms_launches"])) for k, t in traced.items()}, "one_traced_step": traced}, out_path)
for net, _ in modes.values():
    net.close()
