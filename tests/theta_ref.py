"""fp64 numpy restatement of the first-order models SMP_theta, SMP_theta_physics and SMP_theta_pairgraphs, written from the formulas
(not from the device code):

  f_0[v]  = LeakyReLU(H x_v) as [1, C]                     x_v = the WL histogram features (raw features in a tower)
  S       = sum over the children w (hops[v, w] <= 1) of X[v][w] f_{l-1}[w],   X[i, j] = [phi_l(v)[i] == phi_{l-1}(w)[j]]
  f_l[v]  = LeakyReLU([lambda1_s S | lambda2_s 1 1^T S] K_l + 1 b_s^T)          s = |phi_l(v)|
  g       = sum_v LeakyReLU(column sums of f_L[v]),  y = <g, W>,  loss = (y - t)^2 / 2
  towers  : channels halve per level, every level is read out into the feature row, a fully connected head on top.

The receptive fields are an INPUT (the goldens record the reference's; elsewhere gf_smp_prepare_molecule_host, which a CPU test holds
against the goldens, supplies them).  tests/test_smp_theta.py checks this file against the real classes' numbers."""
import numpy as np

ALPHA = 0.01


def lrelu(z):
    return np.where(z > 0, z, ALPHA * z)


def dlrelu(z):
    return np.where(z > 0, 1.0, ALPHA)


def hop_distances(adj):
    V = len(adj)
    sp = np.full((V, V), 10 ** 9, dtype=np.int64)
    sp[np.asarray(adj) > 0] = 1
    sp = np.minimum(sp, sp.T)
    np.fill_diagonal(sp, 0)
    for k in range(V):
        sp = np.minimum(sp, sp[:, k:k + 1] + sp[k:k + 1, :])
    return sp


def executor_multiplicity(depth, k):
    """The executor's semantics of a shared op's gradient: k vertices of one size, processed in descending order; `depth` shared ops
    between a vertex's op and the parameter, every one adding its running gradient to the next on each appearance (depth 0: the vertex's
    op adds into the parameter's gradient directly).  Returns how often each vertex is counted, ascending."""
    out = []
    for j in range(1, k + 1):           # unit gradient at the j-th vertex (ascending) only
        ops = [0] * (depth + 1)          # gradients of the shared ops, nearest the vertex first, then the parameter's
        for v in range(k, 0, -1):        # reverse execution order
            ops[0] += 1 if v == j else 0
            for d in range(1, depth + 1):
                ops[d] += ops[d - 1]
        out.append(ops[-1])
    return out


def wl_features(feat, hops, D):
    V, F = feat.shape
    out = np.zeros((V, F * (D + 1)))
    for d in range(D + 1):
        out[:, d * F:(d + 1) * F] = (hops == d).astype(np.float64) @ feat
    return out


def channels(C, L, tower):
    return [max(1, C >> l) if tower else C for l in range(L + 1)]


def body_size(C, FD, L, maxV, tower):
    c = channels(C, L, tower)
    return C * FD + sum(maxV * (2 + c[l]) + 2 * c[l - 1] * c[l] for l in range(1, L + 1)) + (0 if tower else C)


def split_body(p, C, FD, L, maxV, tower):
    """views into a flat body vector: H, per level (lam1[maxV], lam2[maxV], b[maxV, C_l], K[2 C_{l-1}, C_l]), W (None in a tower)"""
    c = channels(C, L, tower)
    k = C * FD
    H = p[:k].reshape(C, FD)
    lv = [None]
    for l in range(1, L + 1):
        blk = p[k:k + maxV * (2 + c[l])].reshape(maxV, 2 + c[l])
        k += maxV * (2 + c[l])
        K = p[k:k + 2 * c[l - 1] * c[l]].reshape(2 * c[l - 1], c[l])
        k += 2 * c[l - 1] * c[l]
        lv.append((blk[:, 0], blk[:, 1], blk[:, 2:], K))
    W = None if tower else p[k:k + C]
    return H, lv, W


def fields_of(phi_table):
    """the [L + 1, V, cap + 1] table of the goldens / gf_smp_prepare_molecule_host (slot 0 = size) as lists"""
    return [[list(int(u) for u in row[1:1 + row[0]]) for row in level] for level in phi_table]


class Body:
    """forward state of one body (SMP_theta itself, or one tower) on one molecule"""

    def __init__(self, adj, feat, p, L, C, D, maxV, phi, tower):
        feat = np.asarray(feat, dtype=np.float64)
        self.V, self.L, self.C, self.maxV, self.tower, self.phi = len(adj), L, C, maxV, tower, phi
        self.c = channels(C, L, tower)
        self.hops = hop_distances(adj)
        self.x = wl_features(feat, self.hops, 0 if tower else D)
        self.FD = self.x.shape[1]
        self.p = np.asarray(p, dtype=np.float64)
        self.H, self.lv, self.W = split_body(self.p, C, self.FD, L, maxV, tower)
        V = self.V
        self.z = [[(self.H @ self.x[v])[None, :] for v in range(V)]]
        self.S = [None]
        for l in range(1, L + 1):
            lam1, lam2, b, K = self.lv[l]
            cp = self.c[l - 1]
            zs, Ss = [], []
            for v in range(V):
                fv = phi[l][v]
                s = len(fv)
                S = np.zeros((s, cp))
                for w in range(V):
                    if self.hops[v, w] > 1:
                        continue
                    fw = phi[l - 1][w]
                    for i, u in enumerate(fv):
                        if u in fw:
                            S[i] += lrelu(self.z[l - 1][w][fw.index(u)])
                M = np.concatenate([lam1[s - 1] * S, lam2[s - 1] * np.ones((s, 1)) * S.sum(0)[None, :]], axis=1)
                zs.append(M @ K + b[s - 1][None, :])
                Ss.append(S)
            self.z.append(zs)
            self.S.append(Ss)
        self.sh = [[lrelu(self.z[l][v]).sum(0) for v in range(V)] for l in range(L + 1)]
        # level features: sum over the vertices of LeakyReLU(column sums)
        self.level_feature = [sum(lrelu(self.sh[l][v]) for v in range(V)) for l in range(L + 1)]

    def backward(self, dlevel):
        """dlevel[l] = gradient of level_feature[l] (None: the level is not read out) -> gradient of the flat body vector"""
        g = np.zeros_like(self.p)
        gH, glv, _ = split_body(g, self.C, self.FD, self.L, self.maxV, self.tower)
        V, L = self.V, self.L
        df = [[np.zeros_like(self.z[l][v]) for v in range(V)] for l in range(L + 1)]
        for l in range(L, -1, -1):
            for v in range(V):
                if dlevel[l] is not None:
                    df[l][v] += (dlevel[l] * dlrelu(self.sh[l][v]))[None, :]
            if l == 0:
                break
            lam1, lam2, b, K = self.lv[l]
            gl1, gl2, gb, gK = glv[l]
            cp = self.c[l - 1]
            for v in range(V):
                fv = self.phi[l][v]
                s = len(fv)
                dz = df[l][v] * dlrelu(self.z[l][v])
                S = self.S[l][v]
                tot = np.ones((s, 1)) * S.sum(0)[None, :]
                M = np.concatenate([lam1[s - 1] * S, lam2[s - 1] * tot], axis=1)
                gb[s - 1] += dz.sum(0)
                gK += M.T @ dz
                dM = dz @ K.T
                # The reference adds the shared ops W_eye[s] / W_one[s] (ScalarMatMul) to its graph once per vertex of size s
                # (SMP_theta.h:590-591) and GraphFlow::backward runs an op once per appearance, on a gradient that keeps accumulating:
                # the j-th vertex of size s (ascending v) hands its gradient to lambda_s j times.  The class is the parity target.
                kv = 1 + sum(len(self.phi[l][u]) == s for u in range(v))
                gl1[s - 1] += kv * (dM[:, :cp] * S).sum()
                gl2[s - 1] += kv * (dM[:, cp:] * tot).sum()
                dS = lam1[s - 1] * dM[:, :cp] + lam2[s - 1] * np.ones((s, 1)) * dM[:, cp:].sum(0)[None, :]
                for w in range(V):
                    if self.hops[v, w] > 1:
                        continue
                    fw = self.phi[l - 1][w]
                    for i, u in enumerate(fv):
                        if u in fw:
                            df[l - 1][w][fw.index(u)] += dS[i]
        for v in range(V):
            gH += np.outer((df[0][v] * dlrelu(self.z[0][v]))[0], self.x[v])
        return g


def run(adj, feat, target, params, L, C, D, maxV, phi):
    """SMP_theta on one molecule: graph_feature, predict, loss, grads (flat, registration order)"""
    b = Body(adj, feat, params, L, C, D, maxV, phi, tower=False)
    g = b.level_feature[L]
    y = float(g @ b.W)
    grads = b.backward([None] * L + [(y - target) * b.W])
    grads[-C:] = (y - target) * g
    return {"graph_feature": g, "predict": y, "loss": 0.5 * (y - target) ** 2, "grads": grads}


def run_batch(mols, targets, params, L, C, D, maxV, phis):
    pred, feat, g = [], [], 0.0
    for (adj, x), t, phi in zip(mols, targets, phis):
        r = run(adj, x, float(t), params, L, C, D, maxV, phi)
        pred.append(r["predict"])
        feat.append(r["graph_feature"])
        g = g + r["grads"]
    return np.array(pred), np.array(feat), g


def run_model(graphs, target, params, L, C, maxV, phis):
    """SMP_theta_physics (one graph) / SMP_theta_pairgraphs (two): parameters in the class's registration order -- H per tower, the
    levels with the towers interleaved, then the head (one hidden layer of nTotal / 2; two of max(nTotal / 2, 10), max(that / 2, 10))."""
    nT = len(graphs)
    params = np.asarray(params, dtype=np.float64)
    c = channels(C, L, True)
    FD = [np.asarray(g[1]).shape[1] for g in graphs]
    # model vector -> per-tower body vectors (and the index map back)
    idx = [[] for _ in range(nT)]
    k = 0
    for t in range(nT):
        idx[t].append(np.arange(k, k + C * FD[t]))
        k += C * FD[t]
    for l in range(1, L + 1):
        for t in range(nT):
            n = maxV[t] * (2 + c[l]) + 2 * c[l - 1] * c[l]
            idx[t].append(np.arange(k, k + n))
            k += n
    idx = [np.concatenate(i) for i in idx]
    bodies = [Body(graphs[t][0], graphs[t][1], params[idx[t]], L, C, 0, maxV[t], phis[t], tower=True) for t in range(nT)]
    x = np.concatenate([bodies[t].level_feature[l] for l in range(L + 1) for t in range(nT)])
    nTot = x.size
    widths = [nTot, nTot // 2] if nT == 1 else [nTot, max(nTot // 2, 10), max(max(nTot // 2, 10) // 2, 10)]
    Ws, hs, pre = [], [x], []
    for i in range(1, len(widths)):
        Ws.append(params[k:k + widths[i] * widths[i - 1]].reshape(widths[i], widths[i - 1]))
        k += widths[i] * widths[i - 1]
        pre.append(Ws[-1] @ hs[-1])
        hs.append(lrelu(pre[-1]))
    w = params[k:k + widths[-1]]
    assert k + widths[-1] == params.size, (k + widths[-1], params.size)
    y = float(hs[-1] @ w)
    grads = np.zeros_like(params)
    dy = y - target
    grads[k:] = dy * hs[-1]
    dh = dy * w
    kk = k
    for i in range(len(Ws) - 1, -1, -1):
        dpre = dh * dlrelu(pre[i])
        kk -= Ws[i].size
        grads[kk:kk + Ws[i].size] = np.outer(dpre, hs[i]).ravel()
        dh = Ws[i].T @ dpre
    off = 0
    dlev = [[None] * (L + 1) for _ in range(nT)]
    for l in range(L + 1):
        for t in range(nT):
            dlev[t][l] = dh[off:off + c[l]]
            off += c[l]
    for t in range(nT):
        grads[idx[t]] = bodies[t].backward(dlev[t])
    return {"graph_feature": x, "predict": y, "loss": 0.5 * dy * dy, "grads": grads}
