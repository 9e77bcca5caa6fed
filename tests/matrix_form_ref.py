"""Numpy restatement of the two matrix-form baselines, forward and gradient: GCN_MW (GraphFlow/GCN_MW.h, DenseGraph.h:69-111) and LCNN
(GraphFlow/LCNN.h with Conv1D.h, ShuffleMatrix.h).  Evaluated in `dtype` (float64: the reference of the suites; float32: the generator's
check of what the device's number format can reach).  Parameters are one flat vector in registration order (`blocks_*`).

LeakyReLU has slope 0.01 (x > 0 keeps x), the loss is 0.5 (predict - target)^2, every gradient is the plain derivative, the optimiser is
Momentum (m = gamma m + lr g / nBatch, p -= m).  What is literal about LCNN: every molecule is padded to V vertices with zero-feature,
edge-less dummies; hop distances and shell sums are those of the padded graph; the order is the class's exchange sort (descending,
lexicographic on the shell-sum rows; ties stay where that loop leaves them); the sequence pads with the value molV; layer 2 indexes a1,
whose rows are rank positions, with the vertex ids of the sequence; the dense layer reads the pre-activation c2."""
import numpy as np

INF = 10 ** 9
SLOPE = 0.01


def hop_distances(adj):
    """Floyd-Warshall as the classes write it: an edge (i, j) sets both directions, a later visit of (j, i) overwrites [j][i] again"""
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


def shell_sums(feat, sp, D):
    """x[v][d F + f] = the sum of feature f over the vertices u with dist(u, v) == d"""
    feat = np.asarray(feat, dtype=np.float64)
    V, F = feat.shape
    x = np.zeros((V, F * (D + 1)))
    for v in range(V):
        for d in range(D + 1):
            for u in range(V):
                if sp[u, v] == d:
                    x[v, d * F:(d + 1) * F] += feat[u]
    return x


def norm_adj(adj):
    """DenseGraph::create_norm_adj: A-hat[i][j] = (d_i (A + I)[i][j]) d_j, d = 1 / sqrt(row sums of A + I) where the sum is positive"""
    A = np.asarray(adj, dtype=np.float64) + np.eye(len(adj))
    d = A.sum(axis=1)
    d = np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), d)
    return (d[:, None] * A) * d[None, :]


def lrelu(z):
    return np.where(z > 0, z, z.dtype.type(SLOPE) * z)


def dlrelu(z, g):
    return np.where(z > 0, g, g.dtype.type(SLOPE) * g)


def margin(zs):
    """the smallest |z| over the largest, over every pre-activation of a run"""
    return min((float(np.abs(z).min() / max(np.abs(z).max(), 1e-300)) for z in zs if z.size), default=np.inf)


# ---- GCN_MW ----
def blocks_gcn(H, FD, L):
    return [("W_0", FD * H)] + [("W_%d" % l, H * H) for l in range(1, L + 1)] + [("W", H)]


def n_params_gcn(H, FD, L):
    return sum(n for _, n in blocks_gcn(H, FD, L))


def run_gcn(adj, feat, target, params, L, H, D, dtype=np.float64):
    adj = np.asarray(adj)
    V, F = np.asarray(feat).shape
    FD = F * (D + 1)
    sp = hop_distances(adj)
    x = shell_sums(feat, sp, D).astype(dtype)
    Ah64 = norm_adj(adj)
    Ah = Ah64.astype(dtype)
    p = np.asarray(params, dtype=dtype)
    Ws, off = [], 0
    for _, n in blocks_gcn(H, FD, L)[:-1]:
        Ws.append(p[off:off + n].reshape(-1, H))
        off += n
    W = p[off:]
    hs, As, zs = [], [], []
    prev = x
    for l in range(L + 1):
        A = Ah @ prev
        z = A @ Ws[l]
        As.append(A), zs.append(z)
        prev = lrelu(z)
        hs.append(prev)
    g = hs[L].sum(axis=0)
    y = W @ g
    dy = y - dtype(target)
    grads = [None] * (L + 1)
    dh = np.tile(dy * W, (V, 1))
    for l in range(L, -1, -1):
        dz = dlrelu(zs[l], dh)
        grads[l] = (As[l].T @ dz).ravel()
        dh = Ah.T @ (dz @ Ws[l].T)
    return {"predict": float(y), "loss": float(0.5 * dy * dy), "graph_feature": g.astype(np.float64), "norm_adj": Ah64,
            "grads": np.concatenate(grads + [dy * g]).astype(np.float64), "activations": [h.astype(np.float64) for h in hs],
            "margin": margin(zs)}


# ---- LCNN ----
def blocks_lcnn(V, FD, k, C1, C2, nD):
    return [("F1", k * FD * C1), ("b1", C1), ("F2", k * C1 * C2), ("b2", C2), ("Dm", nD * V * C2), ("W", nD)]


def n_params_lcnn(V, FD, k, C1, C2, nD):
    return sum(n for _, n in blocks_lcnn(V, FD, k, C1, C2, nD))


def lcnn_prepare(adj, feat, V, k, D):
    """(x [V][F'], order [V], seq [V][k]) of one molecule padded to V vertices"""
    adj, feat = np.asarray(adj), np.asarray(feat, dtype=np.float64)
    molV, F = feat.shape
    padj = np.zeros((V, V), dtype=np.int64)
    padj[:molV, :molV] = adj
    pfeat = np.zeros((V, F))
    pfeat[:molV] = feat
    sp = hop_distances(padj)
    x = shell_sums(pfeat, sp, D)

    def compare(u, v):
        for a, b in zip(x[u], x[v]):
            if a < b:
                return -1
            if a > b:
                return 1
        return 0

    order = list(range(V))
    for i in range(V):
        for j in range(i + 1, V):
            if compare(order[i], order[j]) < 0:
                order[i], order[j] = order[j], order[i]
    seq = np.full((V, k), molV, dtype=np.int64)
    for i in range(V):
        j = 0
        for d in range(V):
            for v in range(V):
                if j < k and sp[order[i], order[v]] == d and order[v] < molV:
                    seq[i, j] = order[v]
                    j += 1
    return x, np.array(order, dtype=np.int64), seq


def run_lcnn(adj, feat, target, params, V, k, D, C1, C2, nD, dtype=np.float64):
    molV, F = np.asarray(feat).shape
    FD = F * (D + 1)
    x64, order, seq = lcnn_prepare(adj, feat, V, k, D)
    assert seq.max() < V, "a pad entry of a full-size molecule: the class reads past its matrix"
    x = x64.astype(dtype)
    p = np.asarray(params, dtype=dtype)
    parts, off = {}, 0
    for name, n in blocks_lcnn(V, FD, k, C1, C2, nD):
        parts[name] = p[off:off + n]
        off += n
    F1, F2, Dm = parts["F1"].reshape(k * FD, C1), parts["F2"].reshape(k * C1, C2), parts["Dm"].reshape(nD, V * C2)
    A1 = x[seq].reshape(V, k * FD)
    c1 = A1 @ F1 + parts["b1"]
    a1 = lrelu(c1)
    A2 = a1[seq].reshape(V, k * C1)
    c2 = A2 @ F2 + parts["b2"]
    dense = Dm @ c2.ravel()
    y = parts["W"] @ dense
    dy = y - dtype(target)
    ddense = dy * parts["W"]
    dDm = np.outer(ddense, c2.ravel())
    dc2 = (Dm.T @ ddense).reshape(V, C2)
    dF2 = A2.T @ dc2
    dA2 = (dc2 @ F2.T).reshape(V, k, C1)
    da1 = np.zeros_like(a1)
    for j in range(k):   # (slot-major, ascending row: the order of the device's transposed list)
        for i in range(V):
            da1[seq[i, j]] += dA2[i, j]
    dc1 = dlrelu(c1, da1)
    dF1 = A1.T @ dc1
    grads = np.concatenate([dF1.ravel(), dc1.sum(axis=0), dF2.ravel(), dc2.sum(axis=0), dDm.ravel(), dy * dense])
    return {"predict": float(y), "loss": float(0.5 * dy * dy), "graph_feature": dense.astype(np.float64), "order": order, "seq": seq,
            "grads": grads.astype(np.float64), "a1": a1.astype(np.float64), "c2": c2.astype(np.float64), "margin": margin([c1])}


def run(kind, cfg, adj, feat, target, params, dtype=np.float64):
    """kind "gcn_mw": cfg = (L, H, D); "lcnn": cfg = (V, k, D, C1, C2, nD)"""
    return run_gcn(adj, feat, target, params, *cfg, dtype=dtype) if kind == "gcn_mw" else run_lcnn(adj, feat, target, params, *cfg, dtype=dtype)


def blocks(kind, cfg, F):
    if kind == "gcn_mw":
        L, H, D = cfg
        return blocks_gcn(H, F * (D + 1), L)
    V, k, D, C1, C2, nD = cfg
    return blocks_lcnn(V, F * (D + 1), k, C1, C2, nD)


def momentum_steps(kind, cfg, mols, targets, p0, n_iter, lr, gamma):
    """BatchLearn n_iter times: (losses [n_iter][2] before / after each step, final parameters, the smallest margin met)"""
    p = np.array(p0, dtype=np.float64)
    m = np.zeros_like(p)
    losses, small = [], np.inf
    for _ in range(n_iter):
        rs = [run(kind, cfg, a, f, t, p) for (a, f), t in zip(mols, targets)]
        small = min([small] + [r["margin"] for r in rs])
        m = gamma * m + lr * sum(r["grads"] for r in rs) / len(mols)
        p = p - m
        after = sum(run(kind, cfg, a, f, t, p)["loss"] for (a, f), t in zip(mols, targets))
        losses.append([sum(r["loss"] for r in rs), after])
    return np.array(losses), p, small
