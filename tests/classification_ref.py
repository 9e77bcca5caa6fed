"""fp64 checker of the classification models (SMP_2D_ver6_classification / SMP_2D_ver7_classification).  TEST-SIDE ONLY.

The head is restated from the reference: MatVecMul (GraphFlow/MatVecMul.h: z = W g; dW += dz g^T; dg += W^T dz) and LogLoss
(GraphFlow/LogLoss.h:37-76: softmax with the maximum subtracted, value = log p[label] or LOG_ZERO where p[label] <= 0,
dz = p - onehot(label)); Predict is the first arg-max (SMP_2D_ver6_classification.h:706-712).

Everything below graph_feature is the regression models', so the whole-model checker reuses oracle/smp_oracle.py unchanged:
run(...) gives graph_feature; the level gradients for an ARBITRARY read-out gradient dg are what run(...) returns with W := dg
and target := predict - 1 (then dy = 1 and the regression head sends dy * W = dg down); its dW is replaced by the head's own.
tests/test_classification_cpu.py pins this construction against the reference's recorded gradients.
"""
import numpy as np

from oracle import smp_oracle

LOG_ZERO = -256.0   # LogLoss.h:20


def head(g, W, label=None):
    """g [C], W [nClass, C] -> dict(scores, probability, predict[, loss, dz, dW, dg])."""
    g = np.asarray(g, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    z = W @ g
    p = np.exp(z - z.max())
    total = 0.0
    for v in p:          # (the reference's summation order)
        total += v
    p = p / total
    out = {"scores": z, "probability": p, "predict": int(np.argmax(z))}   # (argmax: the first maximum, as the strict > loop)
    if label is None:
        return out
    label = int(label)
    out["loss"] = LOG_ZERO if p[label] <= 0.0 else float(np.log(p[label]))
    dz = p.copy()
    dz[label] -= 1.0
    out["dz"], out["dW"], out["dg"] = dz, np.outer(dz, g), W.T @ dz
    return out


def run(adj, feature, label, params, nClass, nLevels, C, nDepth, cap, has_wl=True, nK=10, custom=True, coulomb=None):
    """One molecule through a classifier.  params: H, (K_l, b_l) x L, W[nClass, C] (registration order).
    Returns dict(graph_feature, scores, probability, predict, loss, grads)."""
    params = np.asarray(params, dtype=np.float64)
    nW = nClass * C
    body, W = params[:-nW], params[-nW:].reshape(nClass, C)
    kw = dict(has_wl=has_wl, coulomb=coulomb, nK=nK, custom=custom)
    fwd = smp_oracle.run(adj, feature, 0.0, np.concatenate([body, np.zeros(C)]), nLevels, C, nDepth, cap, want_grads=False, **kw)
    g = fwd["graph_feature"]
    out = head(g, W, label)
    out["graph_feature"] = g
    if label is None:
        return out
    dg = out["dg"]
    y = float(g @ dg)
    bwd = smp_oracle.run(adj, feature, y - 1.0, np.concatenate([body, dg]), nLevels, C, nDepth, cap, **kw)   # dy = y - (y - 1) = 1
    out["grads"] = np.concatenate([bwd["grads"][:-C], out["dW"].ravel()])
    return out


def run_case(c):
    """A record of tests/golden/smp_classification.npz (util.golden_cases) through run()."""
    nClass, L, C, D, wl, maxV, nK, _ = (int(x) for x in c["cfg"])
    return run(c["adj"], c["feature"], int(c["target"][0]), c["params"], nClass, L, C, D, maxV, bool(wl), nK=nK, custom=True)


def load_golden():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smp_classification.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_cases(g=None):
    """{tag: record} of the per-molecule cases in the generator's order, every record with its `params` (the toy molecules of a
    model share one vector, recorded once: `params_from`)."""
    g = g or load_golden()
    cs = {}
    for tag in g["tags"]:
        tag = str(tag)
        cs[tag] = {k[len(tag) + 2:]: v for k, v in g.items() if k.startswith(tag + "__")}
    for c in cs.values():
        if "params" not in c:
            c["params"] = cs[str(c["params_from"])]["params"]
    return cs
