"""numpy restatement of the reference's SGD, AdaMax and AdaDelta steps (GraphFlow/SGD.h:44-50, AdaMax.h:97-122, AdaDelta.h:90-112) and of
L1Regularization / L2Regularization (L1Regularization.h:39-67, L2Regularization.h:39-58) on one flat vector with a block table.

Every expression is the reference's, operation for operation in its order, in float64 (numpy fuses nothing; +, -, *, / and sqrt are
correctly rounded).  `storage` is the dtype parameters, gradients and per-element state are KEPT in: float64 is the reference itself
(checked against tests/golden/optimisers.npz at 1e-12), float32 is the reference plus the rounding model of graphflow_amd/csrc/
smp_optimisers.hip -- every load widens, every store rounds once, and a state the reference reads back after writing it is read back as
stored.  AdaMax's infinity_norm and beta1_t are doubles in both."""
import numpy as np

SGD, ADAMAX, ADADELTA = 2, 3, 4   # gf_optim_config.kind
DEFAULTS = {"beta1": 0.9, "beta2": 0.999, "rho": 0.95, "epsilon": 1e-6}


def new_state(n, nBlocks, storage):
    return {"s0": np.zeros(n, dtype=storage), "s1": np.zeros(n, dtype=storage), "norms": np.zeros(nBlocks), "beta1_t": 1.0}


def step(kind, p, grad, state, offsets, lr, nBatch, storage, beta1=0.9, beta2=0.999, rho=0.95, epsilon=1e-6):
    """one Learn(lr, nBatch): returns the new parameters (dtype storage) and updates `state` in place"""
    p64, g = p.astype(np.float64), grad.astype(np.float64)
    nb = float(nBatch)
    if kind == SGD:
        return (p64 - lr * g / nb).astype(storage)
    g = g / nb
    if kind == ADADELTA:
        eg = (rho * state["s0"].astype(np.float64) + (1.0 - rho) * g * g).astype(storage)
        state["s0"] = eg
        old = state["s1"].astype(np.float64)
        deltax = -np.sqrt(old + epsilon) / np.sqrt(eg.astype(np.float64) + epsilon) * g
        state["s1"] = (rho * old + (1.0 - rho) * deltax * deltax).astype(storage)
        return (p64 + deltax).astype(storage)
    assert kind == ADAMAX
    state["beta1_t"] *= beta1
    first = (beta1 * state["s0"].astype(np.float64) + (1.0 - beta1) * g).astype(storage)
    state["s0"] = first
    norm_of = np.empty(p.size)
    for b in range(len(offsets) - 1):
        lo, hi = offsets[b], offsets[b + 1]
        g_norm = max(0.0, float(np.abs(g[lo:hi]).max()))
        decayed = beta2 * state["norms"][b]
        state["norms"][b] = g_norm if decayed < g_norm else decayed   # std::max(a, b): b where a < b
        norm_of[lo:hi] = state["norms"][b]
    with np.errstate(invalid="ignore", divide="ignore"):   # (0 / 0 in a block that has seen no gradient: the reference's NaN)
        return (p64 - lr / (1.0 - state["beta1_t"]) * first.astype(np.float64) / norm_of).astype(storage)


def regularise(norm, p, grad, lam, times, storage):
    """(value, new gradient): forward()'s value in ascending order, and `times` backward() calls folded into grads += times * term"""
    x = p.astype(np.float64)
    if norm == 1:
        terms = np.abs(x)
        term = lam * np.where(np.abs(x) < 1e-8, 0.0, np.where(x > 0.0, 1.0, -1.0))
    else:
        terms = x * x
        term = 2.0 * lam * 1.0 * x
    value = (np.cumsum(terms)[-1] if x.size else 0.0) * lam
    return float(value), (grad.astype(np.float64) + float(times) * term).astype(storage)
