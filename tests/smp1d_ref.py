"""fp64 numpy restatement of SMP_1D (version 1), SMP_1D_ver2 (2), SMP_1D_ver3 (3) and of the classifier read-out on them, written from the
formulas (not from the device code):

  f_0[v]  = LeakyReLU2D(H x_v, a) as [1, C]                       x_v = the WL histogram features
  S       = sum over the children w (hops[v, w] <= 1) of X[v][w] f_{l-1}[w],   X[i, j] = [phi_l(v)[i] == phi_{l-1}(w)[j]],  sumS = 1 1^T S
  1:  z = lambda1_s S + lambda2_s sumS + 1 b_s^T                   C_l = C,         a = 0.01       s = |phi_l(v)|
  2:  z = [lambda1_s S | lambda2_s sumS] + 1 b_s^T                 C_l = 2 C_{l-1}, a = 0
  3:  z = [lambda1_s S K_eye | lambda2_s sumS K_one] + 1 b_s^T     C_l = 2 C_{l-1}, a = 0
  f_l[v]  = LeakyReLU2D(z, a);   g = sum_v LeakyReLU(column sums of f_L[v], 0.01)
  regression: y = <g, W>, loss = (y - t)^2 / 2;   classifier: z = W g, p = softmax(z), loss = log p[label], dz = p - onehot.

The gradients of lambda1_s / lambda2_s follow the reference's EXECUTOR, not the calculus.  GraphFlow::backward runs an op once per
appearance in the graph and an op's gradient is never cleared in between, so a shared op that appears once per vertex of size s hands
its whole running gradient on every time:
  versions 2, 3 (and SMP_theta): one shared op, W_eye[s] / W_one[s], between a vertex and lambda_s.  Vertices are processed in
      descending order; after the t-th the op holds g_1 + .. + g_t and adds that to lambda_s: a running sum of a running sum.  The j-th
      vertex of its size in ASCENDING order (processed first when j is largest) is counted j times.
  version 1: three shared ops in a row, W[s] (Reshape2D) <- W_flat[s] (Add) <- W_eye[s] / W_one[s] (SMP_1D.h:498-503), each
      accumulating what the one above hands down: lambda_s receives a running sum three levels deeper than the plain sum, and the j-th
      vertex is counted C(j + 2, 3) = j (j + 1) (j + 2) / 6 times.
`multiplicity` below states both; `executor_multiplicity` derives them by running the accumulation itself, and a CPU test holds the two
together.  Every other gradient is plain.

The receptive fields are an INPUT, as in theta_ref (whose graph helpers this file uses)."""
import numpy as np

from theta_ref import executor_multiplicity as shared_op_multiplicity
from theta_ref import fields_of, hop_distances, wl_features  # noqa: F401

READOUT_ALPHA = 0.01


def slope(version):
    return 0.01 if version == 1 else 0.0


def lrelu(z, a):
    return np.where(z > 0, z, a * z)


def dlrelu(z, a):
    return np.where(z > 0, 1.0, a)


def channels(version, C, L):
    return [C if version == 1 else C << l for l in range(L + 1)]


def multiplicity(version, j):
    """how often the j-th vertex (1-based, ascending) of a field size is counted in dlambda_s"""
    return j * (j + 1) * (j + 2) // 6 if version == 1 else j


def executor_multiplicity(version, k):
    """the same numbers from the executor's semantics (theta_ref.executor_multiplicity): three shared ops in a row for version 1, else one"""
    return shared_op_multiplicity(3 if version == 1 else 1, k)


def split(p, version, C, FD, L, maxV, nClass=0):
    """views into a flat parameter vector: H, per level (lam1[maxV], lam2[maxV], b[maxV, C_l], K_eye, K_one (None below version 3)), W"""
    c = channels(version, C, L)
    k = C * FD
    H = p[:k].reshape(C, FD)
    lv = [None]
    for l in range(1, L + 1):
        blk = p[k:k + maxV * (2 + c[l])].reshape(maxV, 2 + c[l])
        k += maxV * (2 + c[l])
        Ke = Ko = None
        if version == 3:
            n = c[l - 1] * c[l - 1]
            Ke, Ko = p[k:k + n].reshape(c[l - 1], c[l - 1]), p[k + n:k + 2 * n].reshape(c[l - 1], c[l - 1])
            k += 2 * n
        lv.append((blk[:, 0], blk[:, 1], blk[:, 2:], Ke, Ko))
    W = p[k:].reshape(max(nClass, 1), c[L])
    assert W.size == p.size - k
    return H, lv, W


def run(version, adj, feat, target, params, L, C, D, maxV, phi, nClass=0):
    """one molecule: graph_feature, predict / loss (regression) or scores / probability / loss / label (classifier), grads"""
    a = slope(version)
    feat = np.asarray(feat, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64)
    V = len(adj)
    c = channels(version, C, L)
    hops = hop_distances(adj)
    x = wl_features(feat, hops, D)
    FD = x.shape[1]
    H, lv, W = split(p, version, C, FD, L, maxV, nClass)
    z = [[(H @ x[v])[None, :] for v in range(V)]]
    Ss = [None]
    for l in range(1, L + 1):
        lam1, lam2, b, Ke, Ko = lv[l]
        cp = c[l - 1]
        zl, Sl = [], []
        for v in range(V):
            fv = phi[l][v]
            s = len(fv)
            S = np.zeros((s, cp))
            for w in range(V):
                if hops[v, w] > 1:
                    continue
                fw = phi[l - 1][w]
                for i, u in enumerate(fv):
                    if u in fw:
                        S[i] += lrelu(z[l - 1][w][fw.index(u)], a)
            tot = np.ones((s, 1)) * S.sum(0)[None, :]
            if version == 1:
                zz = lam1[s - 1] * S + lam2[s - 1] * tot
            elif version == 2:
                zz = np.concatenate([lam1[s - 1] * S, lam2[s - 1] * tot], axis=1)
            else:
                zz = np.concatenate([lam1[s - 1] * S @ Ke, lam2[s - 1] * tot @ Ko], axis=1)
            zl.append(zz + b[s - 1][None, :])
            Sl.append(S)
        z.append(zl)
        Ss.append(Sl)
    sh = [lrelu(z[L][v], a).sum(0) for v in range(V)]
    g = sum(lrelu(sh[v], READOUT_ALPHA) for v in range(V))
    grads = np.zeros_like(p)
    gH, glv, gW = split(grads, version, C, FD, L, maxV, nClass)
    out = {"graph_feature": g}
    if nClass:
        sc = W @ g
        e = np.exp(sc - sc.max())
        prob = e / e.sum()
        label = int(target)
        dz = prob.copy()
        dz[label] -= 1.0
        gW += np.outer(dz, g)
        dg = W.T @ dz
        out.update(scores=sc, probability=prob, loss=float(np.log(prob[label])), label=int(np.argmax(sc)))
    else:
        y = float(g @ W[0])
        gW[0] += (y - target) * g
        dg = (y - target) * W[0]
        out.update(predict=y, loss=0.5 * (y - target) ** 2)
    df = [[np.zeros_like(z[l][v]) for v in range(V)] for l in range(L + 1)]
    for v in range(V):
        df[L][v] += (dg * dlrelu(sh[v], READOUT_ALPHA))[None, :]
    for l in range(L, 0, -1):
        lam1, lam2, b, Ke, Ko = lv[l]
        gl1, gl2, gb, gKe, gKo = glv[l]
        cp = c[l - 1]
        for v in range(V):
            fv = phi[l][v]
            s = len(fv)
            dz = df[l][v] * dlrelu(z[l][v], a)
            S = Ss[l][v]
            tot = np.ones((s, 1)) * S.sum(0)[None, :]
            gb[s - 1] += dz.sum(0)
            if version == 1:
                dtop = dbot = dz
            elif version == 2:
                dtop, dbot = dz[:, :cp], dz[:, cp:]
            else:
                gKe += (lam1[s - 1] * S).T @ dz[:, :cp]
                gKo += (lam2[s - 1] * tot).T @ dz[:, cp:]
                dtop, dbot = dz[:, :cp] @ Ke.T, dz[:, cp:] @ Ko.T
            kv = multiplicity(version, 1 + sum(len(phi[l][u]) == s for u in range(v)))
            gl1[s - 1] += kv * (dtop * S).sum()
            gl2[s - 1] += kv * (dbot * tot).sum()
            dS = lam1[s - 1] * dtop + lam2[s - 1] * np.ones((s, 1)) * dbot.sum(0)[None, :]
            for w in range(V):
                if hops[v, w] > 1:
                    continue
                fw = phi[l - 1][w]
                for i, u in enumerate(fv):
                    if u in fw:
                        df[l - 1][w][fw.index(u)] += dS[i]
    for v in range(V):
        gH += np.outer((df[0][v] * dlrelu(z[0][v], a))[0], x[v])
    out["grads"] = grads
    return out


def run_batch(version, mols, targets, params, L, C, D, maxV, phis, nClass=0):
    """per-molecule results and the summed gradient"""
    res = [run(version, adj, x, float(t), params, L, C, D, maxV, phi, nClass) for (adj, x), t, phi in zip(mols, targets, phis)]
    return res, sum(r["grads"] for r in res)
