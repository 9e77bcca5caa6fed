"""fp64 restatement of GCN_1D_Distance, GCN_2D_Distance and GCN_3D_Distance of GraphFlow/GCN_1D_Distance.h, GCN_2D_Distance.h,
GCN_3D_Distance.h, for the suites of gf_smp_config.distance_channel.  tests/test_smp_distance.py pins it to the real classes' numbers
(tests/golden/smp_distance.npz) at 1e-9; the GPU suites use it at shapes without a golden.

`form` is the neighbourhood form of the level: 2 (sum), 3 (RisiLayer2D), 6 (KMax(RisiLayer3D, H)).  With M = max_nVertices:
  x_v[v] = the shell sums [F'];   x_d[v] = sort(distance[u][v], u = 0..V-1, then M - V zeros)  [M]   -- COLUMN v, ascending
  per channel c in {v, d}:  h^c_0[v] = softmax(W1^c_0 x_c[v]);   h^c_l[v] = softmax(W1^c_l x_c[v] + W2^c_l n^c_l[v])
  n^c_l[v] = the aggregate of h^c_{l-1}[u] over N_l(v) = {u: dist(v, u) <= min(l, max_Radius)}   (all three forms read max_Radius)
  final = [sum_v h^v_L[v] | sum_v h^d_L[v]];   predict = <W, final>;   loss = 0.5 (predict - target)^2
The sorted values are data: nothing flows back through the sort.  Softmax::backward is the classes' diagonal rule.
A molecule is (adj, feature, distance).  `dtype=np.float32` evaluates everything in fp32: the golden generator's rounding check."""
import numpy as np

import third_order_ref as tref
from neighbourhood_ref import hop_distances, lists_flat, risi2d_closed, risi2d_closed_backward, shell_features, softmax  # noqa: F401

CHANNELS = ("v", "d")


def sorted_rows(distance, M, dtype=np.float64):
    """x_d [V, M]: row v = column v of the matrix, M - V zeros, sorted ascending"""
    d = np.asarray(distance, dtype=dtype)
    V = d.shape[0]
    rows = np.zeros((V, M), dtype=dtype)
    rows[:, :V] = d.T
    return np.sort(rows, axis=1)


def neighbourhoods(adj, L, max_Radius, sp=None):
    """[l][v] = N_l(v) ascending (entry 0: [v])"""
    V = len(adj)
    sp = hop_distances(adj) if sp is None else sp
    return [[[v] for v in range(V)]] + [[[u for u in range(V) if sp[v][u] <= min(l, max_Radius)] for v in range(V)] for l in range(1, L + 1)]


def blocks(H, FD, M, L):
    """[(block name, size)] in registration order (= Momentum's and uniform_init's)"""
    out = []
    for l in range(L + 1):
        out += [("W1v_%d" % l, H * FD), ("W1d_%d" % l, H * M)]
        if l:
            out += [("W2v_%d" % l, H * H), ("W2d_%d" % l, H * H)]
    return out + [("W", 2 * H)]


def checkpoint_blocks(H, FD, M, L):
    """the same blocks in save_model / load_model order: the vertex channel by level, the distance channel by level, W"""
    out = []
    for c, width in (("v", FD), ("d", M)):
        for l in range(L + 1):
            out.append(("W1%s_%d" % (c, l), H * width))
            if l:
                out.append(("W2%s_%d" % (c, l), H * H))
    return out + [("W", 2 * H)]


def n_params(H, FD, M, L):
    return sum(n for _, n in blocks(H, FD, M, L))


def offsets(H, FD, M, L):
    """{block name: (first, size)} in the flat registration-order buffer"""
    out, off = {}, 0
    for name, n in blocks(H, FD, M, L):
        out[name] = (off, n)
        off += n
    return out


def split(params, H, FD, M, L):
    """({'v': [W1_0..], 'd': [..]}, {'v': [None, W2_1..], 'd': [..]}, W) as views"""
    at = offsets(H, FD, M, L)
    width = {"v": FD, "d": M}
    W1 = {c: [params[at["W1%s_%d" % (c, l)][0]:][:H * width[c]].reshape(H, width[c]) for l in range(L + 1)] for c in CHANNELS}
    W2 = {c: [None] + [params[at["W2%s_%d" % (c, l)][0]:][:H * H].reshape(H, H) for l in range(1, L + 1)] for c in CHANNELS}
    return W1, W2, params[at["W"][0]:][:2 * H]


def to_checkpoint(params, H, FD, M, L):
    at = offsets(H, FD, M, L)
    return np.concatenate([params[at[name][0]:at[name][0] + n] for name, n in checkpoint_blocks(H, FD, M, L)])


def from_checkpoint(values, H, FD, M, L):
    at = offsets(H, FD, M, L)
    out, off = np.zeros(n_params(H, FD, M, L), dtype=np.asarray(values).dtype), 0
    for name, n in checkpoint_blocks(H, FD, M, L):
        out[at[name][0]:at[name][0] + n] = values[off:off + n]
        off += n
    return out


def aggregate(form, a):
    """(n [H], what the reverse needs, gap)"""
    if form == 2:
        return a.sum(axis=0), None, np.inf
    if form == 3:
        return risi2d_closed(a), None, np.inf
    n, sel, gap = tref.pool(a)
    return n, sel, gap


def aggregate_backward(form, a, kept, g):
    """the gradient of every member [m, H]"""
    if form == 2:
        return np.tile(g, (a.shape[0], 1))
    if form == 3:
        return risi2d_closed_backward(a, g)
    return tref.pool_backward(a, kept, g)


def run(form, adj, feat, dist, target, params, L, H, D, M, max_Radius=1, dtype=np.float64):
    """One molecule: predict, loss, final_feature [2 H], grads (flat, registration order), h = {'v': [h_0 .. h_L], 'd': [..]}, x_d, N,
    gap = the smallest KMax gap met (form 6; inf otherwise)"""
    adj = np.asarray(adj)
    feat = np.asarray(feat, dtype=dtype)
    params = np.asarray(params, dtype=dtype)
    V, F = feat.shape
    FD = F * (D + 1)
    one = dtype(1)
    sp = hop_distances(adj)
    x = {"v": shell_features(feat, sp, D), "d": sorted_rows(dist, M, dtype)}
    N = neighbourhoods(adj, L, max_Radius, sp)
    W1, W2, W = split(params, H, FD, M, L)
    grads = np.zeros_like(params)
    gW1, gW2, gW = split(grads, H, FD, M, L)
    h, n, kept, gap = {}, {}, {}, np.inf
    for c in CHANNELS:
        h[c], n[c], kept[c] = [softmax(x[c] @ W1[c][0].T)], [None], [None]
        for l in range(1, L + 1):
            nl, kl = np.zeros((V, H), dtype=dtype), []
            for v in range(V):
                nl[v], k, g = aggregate(form, h[c][l - 1][N[l][v]])
                kl.append(k)
                gap = min(gap, g)
            n[c].append(nl), kept[c].append(kl)
            h[c].append(softmax(x[c] @ W1[c][l].T + nl @ W2[c][l].T))
    final = np.concatenate([h["v"][L].sum(axis=0), h["d"][L].sum(axis=0)])
    predict = (W * final).sum()
    dy = predict - dtype(target)
    gW += dy * final
    for i, c in enumerate(CHANNELS):
        dh = np.tile(dy * W[i * H:(i + 1) * H], (V, 1))
        for l in range(L, -1, -1):
            dz = dh * h[c][l] * (one - h[c][l])   # Softmax::backward: diagonal only
            gW1[c][l] += dz.T @ x[c]
            if l == 0:
                break
            gW2[c][l] += dz.T @ n[c][l]
            dn = dz @ W2[c][l]
            dh = np.zeros((V, H), dtype=dtype)
            for v in range(V):
                mem = N[l][v]
                dh[mem] += aggregate_backward(form, h[c][l - 1][mem], kept[c][l][v], dn[v])
    return {"predict": predict, "loss": 0.5 * dy * dy, "final_feature": final, "grads": grads, "h": h, "x_d": x["d"], "N": N, "gap": gap}


def run_batch(form, mols, targets, params, L, H, D, M, max_Radius=1, dtype=np.float64):
    """(per-molecule results, the batch sum of the gradients); mols = [(adj, feature, distance)]"""
    res = [run(form, a, f, d, t, params, L, H, D, M, max_Radius, dtype=dtype) for (a, f, d), t in zip(mols, targets)]
    return res, sum(r["grads"] for r in res)


def activations(res):
    """every [h^v_l[v] | h^d_l[v]], levels then vertices, back to back"""
    return np.concatenate([np.concatenate([hv, hd], axis=1).ravel() for hv, hd in zip(res["h"]["v"], res["h"]["d"])])


def momentum_steps(form, mols, targets, params, L, H, D, M, max_Radius, n_iter, lr, gamma):
    """BatchLearn n_iter times: (losses [n_iter, 2], final parameters, the smallest gap met)"""
    p = np.array(params, dtype=np.float64)
    mom = np.zeros_like(p)
    losses, gap = [], np.inf
    for _ in range(n_iter):
        res, g = run_batch(form, mols, targets, p, L, H, D, M, max_Radius)
        before = sum(r["loss"] for r in res)
        mom = gamma * mom + lr * g / len(mols)
        p = p - mom
        after = run_batch(form, mols, targets, p, L, H, D, M, max_Radius)[0]
        gap = min([gap] + [r["gap"] for r in res + after])
        losses.append((before, sum(r["loss"] for r in after)))
    return np.array(losses), p, gap
