"""fp64 restatement of GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (GraphFlow/GCN_*D_Kernel.h) and GCA_1D (GraphFlow/GCA_1D.h, LinearGram.h),
for the suites of gf_smp_config.readout.  tests/test_smp_pair_gram.py pins it to the real classes' numbers (tests/golden/smp_pair_gram.npz)
at 1e-9; the GPU suites use it at shapes without a golden.

`form` is the neighbourhood form of the levels: 2 (sum), 3 (RisiLayer2D), 6 (KMax(RisiLayer3D, H)).  For every graph
  x[v] = the shell sums [F'];   h_0[v] = softmax(W1_0 x[v]);   h_l[v] = softmax(W1_l x[v] + W2_l n_l[v])
  n_l[v] = the aggregate of h_{l-1}[u] over N_l(v) = {u: dist(v, u) <= min(l, max_Radius)}      (all forms read max_Radius here)
pairs:  final = [sum_v h^X_L[v] | sum_v h^Y_L[v]];  predict = <W, final>, W [2 H];  loss = 0.5 (predict - target)^2; the weights are shared,
        their gradient is the sum over both graphs
GCA:    G = h_L h_L^T;  loss = 0.5 sum (G - adj)^2, adj by value;  dh_L = (E + E^T) h_L, E = G - adj;  no W
Softmax::backward is the classes' diagonal rule.  `dtype=np.float32` evaluates everything in fp32: the golden generator's rounding check."""
import numpy as np

from distance_ref import aggregate, aggregate_backward, neighbourhoods
from neighbourhood_ref import hop_distances, lists_flat, shell_features, softmax  # noqa: F401


def blocks(H, FD, L, readout):
    """[(block name, size)] in registration (= Momentum, uniform_init and save_model) order; readout 1: pairs (W [2 H]), 2: GCA (no W)"""
    out = [("W1_0", H * FD)]
    for l in range(1, L + 1):
        out += [("W1_%d" % l, H * FD), ("W2_%d" % l, H * H)]
    return out + ([("W", 2 * H)] if readout == 1 else [])


def n_params(H, FD, L, readout):
    return sum(n for _, n in blocks(H, FD, L, readout))


def split(params, H, FD, L):
    """(W1 [L + 1], W2 [None, ..], the rest: W [2 H] or empty) as views"""
    W1, W2, off = [], [None], 0
    for l in range(L + 1):
        W1.append(params[off:off + H * FD].reshape(H, FD))
        off += H * FD
        if l:
            W2.append(params[off:off + H * H].reshape(H, H))
            off += H * H
    return W1, W2, params[off:]


def levels_forward(form, adj, feat, W1, W2, L, H, D, max_Radius, dtype):
    """the levels of one graph: what the reverse sweep needs"""
    adj = np.asarray(adj)
    feat = np.asarray(feat, dtype=dtype)
    V = len(adj)
    sp = hop_distances(adj)
    x = shell_features(feat, sp, D)
    N = neighbourhoods(adj, L, max_Radius, sp)
    h, n, kept, gap = [softmax(x @ W1[0].T)], [None], [None], np.inf
    for l in range(1, L + 1):
        nl, kl = np.zeros((V, H), dtype=dtype), []
        for v in range(V):
            nl[v], k, g = aggregate(form, h[l - 1][N[l][v]])
            kl.append(k)
            gap = min(gap, g)
        n.append(nl), kept.append(kl)
        h.append(softmax(x @ W1[l].T + nl @ W2[l].T))
    return {"x": x, "N": N, "h": h, "n": n, "kept": kept, "gap": gap}


def levels_backward(form, st, dh, W2, gW1, gW2, L, H, dtype):
    """dh = dh_L [V, H]; adds the graph's share to gW1 / gW2"""
    one = dtype(1)
    V = dh.shape[0]
    for l in range(L, -1, -1):
        dz = dh * st["h"][l] * (one - st["h"][l])   # Softmax::backward: diagonal only
        gW1[l] += dz.T @ st["x"]
        if l == 0:
            break
        gW2[l] += dz.T @ st["n"][l]
        dn = dz @ W2[l]
        dh = np.zeros((V, H), dtype=dtype)
        for v in range(V):
            mem = st["N"][l][v]
            dh[mem] += aggregate_backward(form, st["h"][l - 1][mem], st["kept"][l][v], dn[v])


def run_pair(form, gx, gy, target, params, L, H, D, max_Radius=1, dtype=np.float64):
    """One pair (gx, gy = (adj, feature)): predict, loss, final_feature [2 H], grads (flat), h = (X's [h_0 .. h_L], Y's), N = (X's lists, Y's),
    gap = the smallest KMax gap met on either graph (form 6; inf otherwise)"""
    params = np.asarray(params, dtype=dtype)
    FD = np.asarray(gx[1]).shape[1] * (D + 1)
    W1, W2, W = split(params, H, FD, L)
    grads = np.zeros_like(params)
    gW1, gW2, gW = split(grads, H, FD, L)
    st = [levels_forward(form, a, f, W1, W2, L, H, D, max_Radius, dtype) for a, f in (gx, gy)]
    final = np.concatenate([s["h"][L].sum(axis=0) for s in st])
    predict = (W * final).sum()
    dy = predict - dtype(target)
    gW += dy * final
    for side, s in enumerate(st):
        dh = np.tile(dy * W[side * H:(side + 1) * H], (len(gx[0]) if side == 0 else len(gy[0]), 1))
        levels_backward(form, s, dh, W2, gW1, gW2, L, H, dtype)
    return {"predict": predict, "loss": 0.5 * dy * dy, "final_feature": final, "grads": grads, "h": (st[0]["h"], st[1]["h"]),
            "N": (st[0]["N"], st[1]["N"]), "gap": min(st[0]["gap"], st[1]["gap"])}


def run_gca(adj, feat, params, L, H, D, max_Radius=1, dtype=np.float64):
    """One molecule of GCA_1D: gram [V, V], loss, grads (flat), h, N"""
    params = np.asarray(params, dtype=dtype)
    FD = np.asarray(feat).shape[1] * (D + 1)
    W1, W2, rest = split(params, H, FD, L)
    assert rest.size == 0
    grads = np.zeros_like(params)
    gW1, gW2, _ = split(grads, H, FD, L)
    st = levels_forward(2, adj, feat, W1, W2, L, H, D, max_Radius, dtype)
    hL = st["h"][L]
    G = hL @ hL.T
    E = G - np.asarray(adj).astype(dtype)
    levels_backward(2, st, (E + E.T) @ hL, W2, gW1, gW2, L, H, dtype)   # LinearGram::backward
    return {"gram": G, "loss": dtype(0.5) * (E * E).sum(), "grads": grads, "h": st["h"], "N": st["N"]}


def run_pairs(form, pairs, targets, params, L, H, D, max_Radius=1, dtype=np.float64):
    """(per-pair results, the batch sum of the gradients); pairs = [((adjX, featX), (adjY, featY))]"""
    res = [run_pair(form, gx, gy, t, params, L, H, D, max_Radius, dtype=dtype) for (gx, gy), t in zip(pairs, targets)]
    return res, sum(r["grads"] for r in res)


def run_gca_batch(mols, params, L, H, D, max_Radius=1, dtype=np.float64):
    res = [run_gca(a, f, params, L, H, D, max_Radius, dtype=dtype) for a, f in mols]
    return res, sum(r["grads"] for r in res)


def activations(h):
    """every h_l[v] of one graph, levels then vertices, back to back"""
    return np.concatenate([hl.ravel() for hl in h])


def momentum_steps(batch_grads, params, n_iter, lr, gamma, n_batch):
    """BatchLearn n_iter times with batch_grads(p) -> (sum of the losses, batch gradient, smallest gap): (losses [n_iter, 2], final parameters,
    the smallest gap met)"""
    p = np.array(params, dtype=np.float64)
    mom = np.zeros_like(p)
    losses, gap = [], np.inf
    for _ in range(n_iter):
        before, g, g0 = batch_grads(p)
        mom = gamma * mom + lr * g / n_batch
        p = p - mom
        after, _, g1 = batch_grads(p)
        gap = min(gap, g0, g1)
        losses.append((before, after))
    return np.array(losses), p, gap


def pairs_batch_grads(form, pairs, targets, L, H, D, max_Radius):
    def f(p):
        res, g = run_pairs(form, pairs, targets, p, L, H, D, max_Radius)
        return sum(r["loss"] for r in res), g, min(r["gap"] for r in res)
    return f


def gca_batch_grads(mols, L, H, D, max_Radius):
    def f(p):
        res, g = run_gca_batch(mols, p, L, H, D, max_Radius)
        return sum(r["loss"] for r in res), g, np.inf
    return f
