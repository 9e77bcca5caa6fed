"""fp64 restatement of GRU_GCN_1D (form 4) and GRU_GCN_2D (form 5) of GraphFlow/GRU_GCN_1D.h, GRU_GCN_2D.h, for the suites of
gf_smp_config.neighbourhood = 4, 5.  tests/test_smp_gru_gcn.py pins it to the real classes' numbers (tests/golden/smp_gru_gcn.npz) at 1e-9;
the GPU suite uses it at shapes without a golden.  Written from the definitions, consumer by consumer; nothing of the device's regrouping.

  h_0[v] = softmax(W x[v]);  l = 1..L, hp = h_{l-1}[v], n = aggregate of h_{l-1}[u] over N_l(v) = {u: dist(v, u) <= min(l, max_Radius)}:
    z = sigmoid(W_z n + U_z hp), r = sigmoid(W_r n + U_r hp), q = r hp, c = tanh(W_h n + U_h q), h_l[v] = (1 - z) hp + z c
  g_v = sigmoid(W_g h_L[v]) tanh(U_g h_L[v]), graph_feature = tanh(sum_v g_v), predict = <U, graph_feature>, loss = 0.5 (predict - target)^2

The aggregate is a sum (form 4) or RisiLayer2D (form 5: neighbourhood_ref's loops or closed form).  Every gradient is the plain derivative
except level 0's softmax, which is the classes' diagonal rule.  The parameters are shared by all levels.  `dtype=np.float32` evaluates
everything in fp32: the golden generator's rounding check."""
import numpy as np

from neighbourhood_ref import (hop_distances, lists_flat, risi2d_closed, risi2d_closed_backward, risi2d_loops,  # noqa: F401
                               risi2d_loops_backward, shell_features, softmax)

MATRICES = ("W_z", "U_z", "W_r", "U_r", "W_h", "U_h", "W_g", "U_g")


def neighbourhoods(adj, L, max_Radius, sp=None):
    """[l][v] = N_l(v), ascending (entry 0: [v]): sp[v][u] <= min(l, max_Radius), in both forms"""
    V = len(adj)
    sp = hop_distances(adj) if sp is None else sp
    return [[[v] for v in range(V)]] + [[[u for u in range(V) if sp[v][u] <= min(l, max_Radius)] for v in range(V)] for l in range(1, L + 1)]


def blocks(H, FD, L=None):
    """[(block name, size)] in registration (= save_model) order; the same whatever nLevels is"""
    return [("W", H * FD)] + [(m, H * H) for m in MATRICES] + [("U", H)]


def n_params(H, FD, L=None):
    return sum(n for _, n in blocks(H, FD))


def split(params, H, FD):
    out, off = {}, 0
    for name, n in blocks(H, FD):
        out[name] = params[off:off + n].reshape((H, FD) if name == "W" else (H,) if name == "U" else (H, H))
        off += n
    assert off == params.size
    return out


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def run(form, adj, feat, target, params, L, H, D, max_Radius=1, nbh=None, aggregate="closed", dtype=np.float64):
    """One molecule: predict, loss, graph_feature, grads (flat, registration order), h = [h_0 .. h_L], n = [None, n_1 ..], N = the lists"""
    adj = np.asarray(adj)
    feat = np.asarray(feat, dtype=dtype)
    params = np.asarray(params, dtype=dtype)
    V, F = feat.shape
    FD = F * (D + 1)
    sp = hop_distances(adj)
    x = shell_features(feat, sp, D)
    N = neighbourhoods(adj, L, max_Radius, sp) if nbh is None else nbh
    P = split(params, H, FD)
    fwd, bwd = (risi2d_loops, risi2d_loops_backward) if aggregate == "loops" else (risi2d_closed, risi2d_closed_backward)
    one = dtype(1)
    h, n, z, r, c = [softmax(x @ P["W"].T)], [None], [None], [None], [None]
    for l in range(1, L + 1):
        hp = h[l - 1]
        nl = np.zeros((V, H), dtype=dtype)
        for v in range(V):
            a = hp[N[l][v]]
            nl[v] = a.sum(axis=0) if form == 4 else fwd(a)
        zl = sigmoid(nl @ P["W_z"].T + hp @ P["U_z"].T)
        rl = sigmoid(nl @ P["W_r"].T + hp @ P["U_r"].T)
        cl = np.tanh(nl @ P["W_h"].T + (rl * hp) @ P["U_h"].T)
        n.append(nl), z.append(zl), r.append(rl), c.append(cl)
        h.append((one - zl) * hp + zl * cl)
    s, t = sigmoid(h[L] @ P["W_g"].T), np.tanh(h[L] @ P["U_g"].T)
    gf = np.tanh((s * t).sum(axis=0))
    predict = (P["U"] * gf).sum()
    dy = predict - dtype(target)
    grads = np.zeros_like(params)
    G = split(grads, H, FD)
    G["U"] += dy * gf
    dg = dy * P["U"] * (one - gf * gf)          # the same for every vertex: the sum hands it on
    ds, dt = dg * t * s * (one - s), dg * s * (one - t * t)
    G["W_g"] += ds.T @ h[L]
    G["U_g"] += dt.T @ h[L]
    dh = ds @ P["W_g"] + dt @ P["U_g"]
    for l in range(L, 0, -1):
        hp = h[l - 1]
        dz = dh * (c[l] - hp) * z[l] * (one - z[l])
        dc = dh * z[l] * (one - c[l] * c[l])
        dq = dc @ P["U_h"]
        dr = dq * hp * r[l] * (one - r[l])
        G["W_z"] += dz.T @ n[l]
        G["U_z"] += dz.T @ hp
        G["W_r"] += dr.T @ n[l]
        G["U_r"] += dr.T @ hp
        G["W_h"] += dc.T @ n[l]
        G["U_h"] += dc.T @ (r[l] * hp)
        dn = dz @ P["W_z"] + dr @ P["W_r"] + dc @ P["W_h"]
        prev = dh * (one - z[l]) + dq * r[l] + dz @ P["U_z"] + dr @ P["U_r"]
        for v in range(V):   # consumer by consumer
            mem = N[l][v]
            if form == 4:
                prev[mem] += dn[v]
            elif mem:
                prev[mem] += bwd(hp[mem], dn[v])
        dh = prev
    G["W"] += (dh * h[0] * (one - h[0])).T @ x   # Softmax::backward: diagonal only
    return {"predict": predict, "loss": 0.5 * dy * dy, "graph_feature": gf, "grads": grads, "h": h, "n": n, "N": N}


def run_batch(form, mols, targets, params, L, H, D, max_Radius=1, dtype=np.float64):
    """(per-molecule results, the batch sum of the gradients)"""
    res = [run(form, a, f, t, params, L, H, D, max_Radius, dtype=dtype) for (a, f), t in zip(mols, targets)]
    return res, sum(r["grads"] for r in res)


def activations(res):
    """every h_l[v], levels then vertices, back to back"""
    return np.concatenate([hl.ravel() for hl in res["h"]])


def momentum_steps(form, mols, targets, params, L, H, D, max_Radius, n_iter, lr, gamma):
    """BatchLearn n_iter times: (losses [n_iter, 2], final parameters)"""
    p = np.array(params, dtype=np.float64)
    mom = np.zeros_like(p)
    losses = []
    for _ in range(n_iter):
        res, g = run_batch(form, mols, targets, p, L, H, D, max_Radius)
        before = sum(r["loss"] for r in res)
        mom = gamma * mom + lr * g / len(mols)
        p = p - mom
        losses.append((before, sum(r["loss"] for r in run_batch(form, mols, targets, p, L, H, D, max_Radius)[0])))
    return np.array(losses), p
