"""fp64 numpy restatement of CCN_1D (GraphFlow/CCN_1D.h), the first-order covariant compositional network on a pair of graphs, written
from the formulas (not from the device code).  It is SMP_theta_pairgraphs (tests/theta_ref.py) with

  x_v     = feature row / its L1 norm                                                  (CCN_1D.h:439-448)
  C_0     = nChanels,  C_l = max(int(ceil(C_{l-1} * decay)), 16), the product in double (:200, :217)
  head    : nTotal -> max(int(ceil(nTotal * decay)), 16) -> max(int(ceil(that * decay)), 16) -> 1, LeakyReLU after each hidden layer

and otherwise the same tower: f_0[v] = LeakyReLU(H x_v) as [1, C]; S = the children's (hops <= 1) activations summed on the positions of
phi_l(v); f_l[v] = LeakyReLU([lambda1_s S | lambda2_s 1 1^T S] K_l + 1 b_s^T); level feature l = sum_v LeakyReLU(column sums of f_l[v]);
the feature row interleaves the towers level by level.  The receptive fields are an INPUT.  tests/test_ccn_1d.py checks this file against
the real class's numbers.

multiplicity / halving exist for the tests that show a named golden case tells the right rule from the wrong one: multiplicity = "one"
gives dlambda its plain derivative instead of the class's j-fold count; halving = True gives the widths of
SMP_theta_pairgraphs."""
import math

import numpy as np

from theta_ref import dlrelu, hop_distances, lrelu

MIN_CHANELS = 16


def channels(C, L, decay, halving=False):
    if halving:
        return [max(1, C >> l) for l in range(L + 1)]
    c = [C]
    for _ in range(L):
        c.append(max(int(math.ceil(c[-1] * decay)), MIN_CHANELS))
    return c


def head_widths(nTotal, decay, halving=False):
    if halving:
        h1 = max(nTotal // 2, 10)
        return [nTotal, h1, max(h1 // 2, 10)]
    h1 = max(int(math.ceil(nTotal * decay)), MIN_CHANELS)
    return [nTotal, h1, max(int(math.ceil(h1 * decay)), MIN_CHANELS)]


def param_count(C, L, F, maxV, decay, halving=False):
    c = channels(C, L, decay, halving)
    n = sum(C * F[t] + sum(maxV[t] * (2 + c[l]) + 2 * c[l - 1] * c[l] for l in range(1, L + 1)) for t in range(2))
    w = head_widths(2 * sum(c), decay, halving)
    return n + w[1] * w[0] + w[2] * w[1] + w[2]


def normalised(feat):
    feat = np.asarray(feat, dtype=np.float64)
    return feat / np.abs(feat).sum(axis=1, keepdims=True)


def split_tower(p, c, F, maxV):
    """views into a tower's flat vector: H, per level (lam1[maxV], lam2[maxV], b[maxV, C_l], K[2 C_{l-1}, C_l])"""
    k = c[0] * F
    H = p[:k].reshape(c[0], F)
    lv = [None]
    for l in range(1, len(c)):
        blk = p[k:k + maxV * (2 + c[l])].reshape(maxV, 2 + c[l])
        k += maxV * (2 + c[l])
        K = p[k:k + 2 * c[l - 1] * c[l]].reshape(2 * c[l - 1], c[l])
        k += 2 * c[l - 1] * c[l]
        lv.append((blk[:, 0], blk[:, 1], blk[:, 2:], K))
    assert k == p.size
    return H, lv


class Tower:
    """forward state of one tower on one graph"""

    def __init__(self, adj, feat, p, c, maxV, phi):
        self.V, self.L, self.c, self.maxV, self.phi = len(adj), len(c) - 1, c, maxV, phi
        self.hops = hop_distances(adj)
        self.x = normalised(feat)
        self.p = np.asarray(p, dtype=np.float64)
        self.H, self.lv = split_tower(self.p, c, self.x.shape[1], maxV)
        V = self.V
        self.z = [[(self.H @ self.x[v])[None, :] for v in range(V)]]
        self.S = [None]
        for l in range(1, self.L + 1):
            lam1, lam2, b, K = self.lv[l]
            zs, Ss = [], []
            for v in range(V):
                S = self.gather(l, v)
                s = len(S)
                M = np.concatenate([lam1[s - 1] * S, lam2[s - 1] * np.ones((s, 1)) * S.sum(0)[None, :]], axis=1)
                zs.append(M @ K + b[s - 1][None, :])
                Ss.append(S)
            self.z.append(zs)
            self.S.append(Ss)
        self.sh = [[lrelu(self.z[l][v]).sum(0) for v in range(V)] for l in range(self.L + 1)]
        self.level_feature = [sum(lrelu(self.sh[l][v]) for v in range(V)) for l in range(self.L + 1)]

    def children(self, l, v):
        """(w, [(i, j)]): child w holds the i-th vertex of phi_l(v) at position j of phi_{l-1}(w)"""
        fv = self.phi[l][v]
        for w in range(self.V):
            if self.hops[v, w] <= 1:
                fw = self.phi[l - 1][w]
                yield w, [(i, fw.index(u)) for i, u in enumerate(fv) if u in fw]

    def gather(self, l, v):
        S = np.zeros((len(self.phi[l][v]), self.c[l - 1]))
        for w, pairs in self.children(l, v):
            for i, j in pairs:
                S[i] += lrelu(self.z[l - 1][w][j])
        return S

    def backward(self, dlevel, multiplicity="class"):
        """dlevel[l] = gradient of level_feature[l] -> gradient of the tower's flat vector"""
        g = np.zeros_like(self.p)
        gH, glv = split_tower(g, self.c, self.x.shape[1], self.maxV)
        V, L = self.V, self.L
        df = [[np.zeros_like(self.z[l][v]) for v in range(V)] for l in range(L + 1)]
        for l in range(L, 0, -1):
            lam1, lam2, b, K = self.lv[l]
            gl1, gl2, gb, gK = glv[l]
            cp = self.c[l - 1]
            for v in range(V):
                s = len(self.phi[l][v])
                dz = (df[l][v] + (dlevel[l] * dlrelu(self.sh[l][v]))[None, :]) * dlrelu(self.z[l][v])
                S = self.S[l][v]
                tot = np.ones((s, 1)) * S.sum(0)[None, :]
                gb[s - 1] += dz.sum(0)
                gK += np.concatenate([lam1[s - 1] * S, lam2[s - 1] * tot], axis=1).T @ dz
                dM = dz @ K.T
                # The class adds the SHARED ops W_eye[s] / W_one[s] to its graph once per vertex of size s (CCN_1D.h:613-614) and
                # GraphFlow::backward runs an op once per appearance on a gradient that keeps accumulating: the j-th vertex of size s
                # (ascending v) hands its gradient to lambda_s j times.
                j = 1 + sum(len(self.phi[l][u]) == s for u in range(v)) if multiplicity == "class" else 1
                gl1[s - 1] += j * (dM[:, :cp] * S).sum()
                gl2[s - 1] += j * (dM[:, cp:] * tot).sum()
                dS = lam1[s - 1] * dM[:, :cp] + lam2[s - 1] * np.ones((s, 1)) * dM[:, cp:].sum(0)[None, :]
                for w, pairs in self.children(l, v):
                    for i, k in pairs:
                        df[l - 1][w][k] += dS[i]
        for v in range(V):
            dz0 = (df[0][v] + (dlevel[0] * dlrelu(self.sh[0][v]))[None, :]) * dlrelu(self.z[0][v])
            gH += np.outer(dz0[0], self.x[v])
        return g


def run(graphs, target, params, L, C, maxV, decay, phis, multiplicity="class", halving=False):
    """CCN_1D on one pair: graph_feature (the head's input row), predict, loss, grads (flat, registration order: H_1, H_2; per level
    tower 1's size entries and K1_l, then tower 2's; W1, W2, W3)"""
    params = np.asarray(params, dtype=np.float64)
    c = channels(C, L, decay, halving)
    F = [np.asarray(g[1]).shape[1] for g in graphs]
    idx = [[], []]
    k = 0
    for t in range(2):
        idx[t].append(np.arange(k, k + C * F[t]))
        k += C * F[t]
    for l in range(1, L + 1):
        for t in range(2):
            n = maxV[t] * (2 + c[l]) + 2 * c[l - 1] * c[l]
            idx[t].append(np.arange(k, k + n))
            k += n
    idx = [np.concatenate(i) for i in idx]
    towers = [Tower(graphs[t][0], graphs[t][1], params[idx[t]], c, maxV[t], phis[t]) for t in range(2)]
    x = np.concatenate([towers[t].level_feature[l] for l in range(L + 1) for t in range(2)])
    widths = head_widths(x.size, decay, halving)
    Ws, hs, pre = [], [x], []
    for i in (1, 2):
        Ws.append(params[k:k + widths[i] * widths[i - 1]].reshape(widths[i], widths[i - 1]))
        k += Ws[-1].size
        pre.append(Ws[-1] @ hs[-1])
        hs.append(lrelu(pre[-1]))
    w3 = params[k:]
    assert w3.size == widths[2], (k + widths[2], params.size)
    y = float(hs[-1] @ w3)
    dy = y - target
    grads = np.zeros_like(params)
    grads[k:] = dy * hs[-1]
    dh = dy * w3
    for i in (1, 0):
        dpre = dh * dlrelu(pre[i])
        k -= Ws[i].size
        grads[k:k + Ws[i].size] = np.outer(dpre, hs[i]).ravel()
        dh = Ws[i].T @ dpre
    off = 0
    dlev = [[None] * (L + 1), [None] * (L + 1)]
    for l in range(L + 1):
        for t in range(2):
            dlev[t][l] = dh[off:off + c[l]]
            off += c[l]
    for t in range(2):
        grads[idx[t]] = towers[t].backward(dlev[t], multiplicity)
    return {"graph_feature": x, "predict": y, "loss": 0.5 * dy * dy, "grads": grads}


def run_batch(pairs, targets, params, L, C, maxV, decay, phis):
    """predictions and the batch SUM of the gradients over pairs = [(graph1, graph2)], phis = [(fields1, fields2)]"""
    pred, g = [], 0.0
    for (ga, gb), t, ph in zip(pairs, targets, phis):
        r = run([ga, gb], float(t), params, L, C, maxV, decay, ph)
        pred.append(r["predict"])
        g = g + r["grads"]
    return np.array(pred), g
