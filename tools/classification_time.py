"""Step time of the ver6 classifier against the ver6 regression model on the same 1024 synthetic molecules (C = 10, three levels, cap 29,
nClass = 11), ver6 and ver7: hipEvents, 3 warm-ups, median of 30, the two models alternating in one process; then the gf_ctx_set_timing rows
of the classifier's read-out kernels (profiles/classification_step.txt).
usage: python tools/classification_time.py [output file]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import graphflow_amd as gf  # noqa: E402
from graphflow_amd.smp import SMPClassifier, SMPOmega  # noqa: E402
from inputs import f32exact, synthetic_molecule  # noqa: E402

L, C, F, D, cap, nClass, N = 3, 10, 5, 2, 29, 11, 1024
mols = [synthetic_molecule(s)[:2] for s in range(N)]
rng = np.random.default_rng(1)
ctx = gf.default_context()
out = []
for nK in (10, 50):
    reg = SMPOmega(L, C, F, D, cap, True, nContractions=nK, custom_matmul=True)
    cls = SMPClassifier(nClass, L, C, F, D, cap, True, nContractions=nK, custom_matmul=True)
    body = rng.uniform(-1, 1, reg.n_params - C) / np.sqrt(nK * C)
    pr = torch.as_tensor(f32exact(np.concatenate([body, rng.uniform(-1, 1, C) / np.sqrt(C)])).astype(np.float32)).cuda()
    pc = torch.as_tensor(f32exact(np.concatenate([body, rng.uniform(-1, 1, nClass * C) * 0.02])).astype(np.float32)).cuda()
    tr = torch.as_tensor(np.array([len(a) for a, _ in mols], dtype=np.float32)).cuda()
    tc = torch.as_tensor((np.array([len(a) for a, _ in mols]) % nClass).astype(np.float32)).cuda()
    reg.prepare(mols)
    cls.prepare(mols)
    gr, gc = torch.empty(reg.n_params, device="cuda"), torch.empty(cls.n_params, device="cuda")

    def one(net, p, t, g):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        net.forward(p, t)
        net.backward(p, g)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(3):
        one(reg, pr, tr, gr), one(cls, pc, tc, gc)
    tr_ms, tc_ms = [], []
    for _ in range(30):
        tr_ms.append(one(reg, pr, tr, gr))
        tc_ms.append(one(cls, pc, tc, gc))
    assert torch.isfinite(gc).all() and torch.isfinite(gr).all()
    q = lambda v: (np.median(v), np.percentile(v, 10), np.percentile(v, 90))  # noqa: E731
    out.append("ver%d (nContractions %d) forward+backward, %d molecules, C=%d, L=%d, cap=%d, median of 30 [p10 .. p90] ms" % (6 if nK == 10 else 7, nK, N, C, L, cap))
    out.append("  regression  %.3f [%.3f .. %.3f]" % q(tr_ms))
    out.append("  classifier  %.3f [%.3f .. %.3f]   (nClass %d)   ratio %.4f" % (q(tc_ms) + (nClass, np.median(tc_ms) / np.median(tr_ms))))
    ctx.set_timing(True)
    for _ in range(10):
        cls.forward(pc, tc)
        cls.backward(pc, gc)
    tm = ctx.timings()
    ctx.set_timing(False)
    total = sum(v[0] for v in tm.values())
    out.append("  gf_ctx_set_timing over 10 classifier steps (serialised launches): all kernels %.3f ms per step" % (total / 10))
    for name in sorted(tm):
        if "classes" in name or name in ("smp_readout_nodes",):
            out.append("    %-28s %8.4f ms per step, %d launches per step" % (name, tm[name][0] / 10, tm[name][1] // 10))
    reg.close()
    cls.close()
text = "\n".join(out) + "\n"
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write(text)
