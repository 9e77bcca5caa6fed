"""fp64 restatement of NeuralFingerprint (form 1), GCN_1D (2) and GCN_2D (3) of GraphFlow/NeuralFingerprint.h, GCN_1D.h, GCN_2D.h, for the
suites of gf_smp_config.neighbourhood.  tests/test_smp_neighbourhood.py pins it to the real classes' numbers (tests/golden/
smp_neighbourhood.npz) at 1e-9; the GPU suite uses it at shapes without a golden.

  h_0[v] = softmax(W1_0 x[v]);   h_l[v] = softmax(W1_l x[v] + W2_l n_l[v]),  n_l[v] = aggregate of h_{l-1}[u] over N_l(v)
  predict = <W, sum_v h_L[v]>,  loss = 0.5 (predict - target)^2

Softmax::backward is the class's DIAGONAL rule dz = dh h (1 - h) (`softmax_grad="full"` evaluates the true Jacobian instead, for the test
that shows the difference).  RisiLayer2D is carried twice: as the class's loops over pairs of members and in the closed form the device
evaluates (`aggregate="loops"` / "closed").  `dtype=np.float32` evaluates everything in fp32: the golden generator's rounding check."""
import numpy as np

INF = 10 ** 9


def hop_distances(adj):
    """the classes' Floyd-Warshall, literally: an edge writes both [i][j] and [j][i], a later visit of (j, i) resets [j][i]"""
    V = len(adj)
    sp = np.zeros((V, V), dtype=np.int64)
    for i in range(V):
        for j in range(V):
            sp[i, j] = 0 if i == j else INF
            if i != j and adj[i][j] > 0:
                sp[i, j] = sp[j, i] = 1
    for k in range(V):
        sp = np.minimum(sp, sp[:, k:k + 1] + sp[k:k + 1, :])
    return sp


def shell_features(feat, sp, D):
    """x[v] block d = sum of feature[u] over sp[u][v] == d"""
    return np.concatenate([(sp.T == d).astype(feat.dtype) @ feat for d in range(D + 1)], axis=1)


def radius(form, l, max_Radius):
    return l if form == 3 else min(l, max_Radius)


def neighbourhoods(form, adj, L, max_Radius, sp=None):
    """[l][v] = N_l(v) as an ascending list (entry 0: [v]): form 1 adj[v][u] > 0 as written; 2, 3: sp[v][u] <= the level's radius"""
    V = len(adj)
    sp = hop_distances(adj) if sp is None else sp
    out = [[[v] for v in range(V)]]
    for l in range(1, L + 1):
        if form == 1:
            out.append([[u for u in range(V) if adj[v][u] > 0] for v in range(V)])
        else:
            out.append([[u for u in range(V) if sp[v][u] <= radius(form, l, max_Radius)] for v in range(V)])
    return out


def blocks(H, FD, L):
    """[(block name, size)] in registration (= save_model) order"""
    out = [("W1_0", H * FD)]
    for l in range(1, L + 1):
        out += [("W1_%d" % l, H * FD), ("W2_%d" % l, H * H)]
    return out + [("W", H)]


def n_params(H, FD, L):
    return sum(n for _, n in blocks(H, FD, L))


def split(params, H, FD, L):
    W1, W2, off = [], [None], 0
    for l in range(L + 1):
        W1.append(params[off:off + H * FD].reshape(H, FD))
        off += H * FD
        if l:
            W2.append(params[off:off + H * H].reshape(H, H))
            off += H * H
    assert off + H == params.size
    return W1, W2, params[off:]


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def risi2d_loops(a):
    """RisiLayer2D::forward on the member vectors a [m, H], as the class loops"""
    m, H = a.shape
    n = np.zeros(H, dtype=a.dtype)
    for i in range(H):
        for k in range(H):
            for u in range(m):
                for v in range(u + 1, m):
                    n[i] += a[u, i] * a[v, k]
                    n[i] += a[u, k] * a[v, i]
    return n


def risi2d_loops_backward(a, g):
    """RisiLayer2D::backward: the gradient of every member"""
    m, H = a.shape
    da = np.zeros_like(a)
    for i in range(H):
        for k in range(H):
            for u in range(m):
                for v in range(u + 1, m):
                    da[u, i] += g[i] * a[v, k]
                    da[v, k] += g[i] * a[u, i]
                    da[u, k] += g[i] * a[v, i]
                    da[v, i] += g[i] * a[u, k]
    return da


def risi2d_closed(a):
    T = a.sum(axis=1)
    return a.sum(axis=0) * T.sum() - (a * T[:, None]).sum(axis=0)


def risi2d_closed_backward(a, g):
    T = a.sum(axis=1)
    A = a.sum(axis=0)
    return g[None, :] * (T.sum() - T)[:, None] + ((A[None, :] - a) * g[None, :]).sum(axis=1, keepdims=True)


def run(form, adj, feat, target, params, L, H, D, max_Radius=1, nbh=None, softmax_grad="diagonal", aggregate="closed", dtype=np.float64):
    """One molecule: predict, loss, final_feature, grads (flat, registration order), h = [h_0 .. h_L] ([V, H] each), N = the lists"""
    adj = np.asarray(adj)
    feat = np.asarray(feat, dtype=dtype)
    params = np.asarray(params, dtype=dtype)
    V, F = feat.shape
    FD = F * (D + 1)
    sp = hop_distances(adj)
    x = shell_features(feat, sp, D)
    N = neighbourhoods(form, adj, L, max_Radius, sp) if nbh is None else nbh
    W1, W2, W = split(params, H, FD, L)
    fwd, bwd = (risi2d_loops, risi2d_loops_backward) if aggregate == "loops" else (risi2d_closed, risi2d_closed_backward)
    h = [softmax(x @ W1[0].T)]
    n = [None]
    for l in range(1, L + 1):
        nl = np.zeros((V, H), dtype=dtype)
        for v in range(V):
            a = h[l - 1][N[l][v]]
            nl[v] = a.sum(axis=0) if form != 3 else fwd(a)
        n.append(nl)
        h.append(softmax(x @ W1[l].T + nl @ W2[l].T))
    g = h[L].sum(axis=0)
    predict = (W * g).sum()
    tgt = dtype(target)
    dy = predict - tgt
    grads = np.zeros_like(params)
    gW1, gW2, gW = split(grads, H, FD, L)
    gW += dy * g
    dh = np.tile(dy * W, (V, 1))
    for l in range(L, -1, -1):
        if softmax_grad == "diagonal":
            dz = dh * h[l] * (1 - h[l])
        else:
            dz = h[l] * (dh - (dh * h[l]).sum(axis=1, keepdims=True))
        gW1[l] += dz.T @ x
        if l == 0:
            break
        gW2[l] += dz.T @ n[l]
        dn = dz @ W2[l]
        dh = np.zeros((V, H), dtype=dtype)
        for v in range(V):
            mem = N[l][v]
            if form != 3:
                dh[mem] += dn[v]
            elif mem:
                dh[mem] += bwd(h[l - 1][mem], dn[v])
    return {"predict": predict, "loss": 0.5 * dy * dy, "final_feature": g, "grads": grads, "h": h, "N": N}


def run_batch(form, mols, targets, params, L, H, D, max_Radius=1):
    """(per-molecule results, the batch sum of the gradients)"""
    res = [run(form, a, f, t, params, L, H, D, max_Radius) for (a, f), t in zip(mols, targets)]
    return res, sum(r["grads"] for r in res)


def activations(res):
    """every h_l[v], levels then vertices, back to back"""
    return np.concatenate([hl.ravel() for hl in res["h"]])


def lists_flat(N, L):
    """the lists of levels 1..L as one int array: per (l, v) the count, then the members"""
    out = []
    for l in range(1, L + 1):
        for mem in N[l]:
            out += [len(mem)] + list(mem)
    return np.array(out, dtype=np.int32)


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
