"""fp64 numpy restatement of SMP_2D (form 1), SMP_2D_ver4 (form 2) and of the classifier read-out on them, written from the formulas (not
from the device code):

  f_0[v]  = LeakyReLU3D(H x_v) as [1, 1, C]                          x_v = the WL histogram features
  S       = sum over the children w (hops[v, w] <= 1) of X f_{l-1}[w] X^T + scalar_l (x) adj_v,   X[i, j] = [phi_l(v)[i] == phi_{l-1}(w)[j]]
  adj_v   = the adjacency reduced to phi_l(v) (form 1); with a unit diagonal and every row divided by its sum (form 2)
  col[j]  = sum_k S[k, j]                                             (W[s] = lambda1_s I + lambda2_s 1 1^T applied along the first index)
  1:  z[i, j] = lambda1_s S[i, j] + lambda2_s col[j] + b_s            C_l = C          (lambda1_s, lambda2_s, b_s, scalar_l: per channel)
  2:  z[i, j] = [lambda1_s S[i, j] | lambda2_s col[j]] + b_s          C_l = 2 C_{l-1}
  f_l[v]  = LeakyReLU3D(z), slope 0.01 at every level;   g = sum_v LeakyReLU(sum_ij f_L[v][i, j])
  regression: y = <g, W>, loss = (y - t)^2 / 2;   classifier: z = W g, p = softmax(z), loss = log p[label], dz = p - onehot.

The gradients of lambda1_s / lambda2_s follow the reference's EXECUTOR, not the calculus (see smp1d_ref.py): a shared op that appears in
the graph once per vertex of size s runs backward once per appearance on a gradient that is never cleared in between.
  form 2: one shared op, W_eye[s] / W_one[s] (VectorBroadcastMat), between a vertex's TensorMul and lambda_s: the j-th vertex of its size
      (ascending) is counted j times.
  form 1: two in a row, W[s] (SumTensor3D) <- W_eye[s] / W_one[s]: a running sum of a running sum, j (j + 1) / 2 times.
`multiplicity` states both; `executor_multiplicity` derives them by running the accumulation itself.  scalar_l (its VectorBroadcastMat
is per vertex), b_s (VectorAddTensor per vertex), H and W are plain.

The receptive fields are an INPUT, as in theta_ref (whose graph helpers this file uses)."""
import numpy as np

from theta_ref import executor_multiplicity as shared_op_multiplicity
from theta_ref import fields_of, hop_distances, wl_features  # noqa: F401

ALPHA = 0.01


def lrelu(z):
    return np.where(z > 0, z, ALPHA * z)


def dlrelu(z):
    return np.where(z > 0, 1.0, ALPHA)


def channels(form, C, L):
    return [C if form == 1 else C << l for l in range(L + 1)]


def multiplicity(form, j):
    """how often the j-th vertex (1-based, ascending) of a field size is counted in dlambda_s"""
    return j * (j + 1) // 2 if form == 1 else j


def executor_multiplicity(form, k):
    """the same numbers from the executor's semantics (theta_ref.executor_multiplicity): two shared ops in a row for form 1, else one"""
    return shared_op_multiplicity(2 if form == 1 else 1, k)


def param_count(form, C, FD, L, maxV, nClass=0):
    c = channels(form, C, L)
    return C * FD + sum(maxV * (2 * c[l - 1] + c[l]) + c[l - 1] for l in range(1, L + 1)) + max(nClass, 1) * c[L]


def split(p, form, C, FD, L, maxV, nClass=0):
    """views into a flat parameter vector: H, per level (lam1[maxV, Cp], lam2[maxV, Cp], b[maxV, C_l], scalar[Cp]), W"""
    c = channels(form, C, L)
    k = C * FD
    H = p[:k].reshape(C, FD)
    lv = [None]
    for l in range(1, L + 1):
        cp, w = c[l - 1], 2 * c[l - 1] + c[l]
        blk = p[k:k + maxV * w].reshape(maxV, w)
        k += maxV * w
        lv.append((blk[:, :cp], blk[:, cp:2 * cp], blk[:, 2 * cp:], p[k:k + cp]))
        k += cp
    W = p[k:].reshape(max(nClass, 1), c[L])
    assert W.size == p.size - k
    return H, lv, W


def reduced_adjacency(form, adj, field):
    a = np.asarray(adj, dtype=np.float64)[np.ix_(field, field)]
    if form == 2:
        a = a.copy()
        np.fill_diagonal(a, 1.0)
        a = a / a.sum(1, keepdims=True)
    return a


def run(form, adj, feat, target, params, L, C, D, maxV, phi, nClass=0):
    """one molecule: graph_feature, predict / loss (regression) or scores / probability / loss / label (classifier), grads, and the
    activations f[l][v] ([s, s, C_l]) and reduced adjacencies radj[l][v]"""
    feat = np.asarray(feat, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64)
    V = len(adj)
    c = channels(form, C, L)
    hops = hop_distances(adj)
    x = wl_features(feat, hops, D)
    FD = x.shape[1]
    H, lv, W = split(p, form, C, FD, L, maxV, nClass)
    z = [[(H @ x[v])[None, None, :] for v in range(V)]]
    Ss, radj, maps = [None], [None], [None]
    for l in range(1, L + 1):
        lam1, lam2, b, scalar = lv[l]
        cp = c[l - 1]
        zl, Sl, al, ml = [], [], [], []
        for v in range(V):
            fv = list(phi[l][v])
            s = len(fv)
            a = reduced_adjacency(form, adj, fv)
            S = a[:, :, None] * scalar[None, None, :]
            mv = []
            for w in range(V):
                if hops[v, w] > 1:
                    continue
                fw = list(phi[l - 1][w])
                idx = [i for i, u in enumerate(fv) if u in fw]
                src = [fw.index(fv[i]) for i in idx]
                S[np.ix_(idx, idx)] += lrelu(z[l - 1][w])[np.ix_(src, src)]
                mv.append((w, idx, src))
            col = S.sum(0)[None, :, :] * np.ones((s, 1, 1))
            if form == 1:
                zz = lam1[s - 1] * S + lam2[s - 1] * col
            else:
                zz = np.concatenate([lam1[s - 1] * S, lam2[s - 1] * col], axis=2)
            zl.append(zz + b[s - 1][None, None, :])
            Sl.append(S)
            al.append(a)
            ml.append(mv)
        z.append(zl)
        Ss.append(Sl)
        radj.append(al)
        maps.append(ml)
    sh = [lrelu(z[L][v]).sum((0, 1)) for v in range(V)]
    g = sum(lrelu(sh[v]) for v in range(V))
    grads = np.zeros_like(p)
    gH, glv, gW = split(grads, form, C, FD, L, maxV, nClass)
    out = {"graph_feature": g, "f": [[lrelu(zv) for zv in zl] for zl in z], "radj": radj}
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
        df[L][v] += (dg * dlrelu(sh[v]))[None, None, :]
    for l in range(L, 0, -1):
        lam1, lam2, b, scalar = lv[l]
        gl1, gl2, gb, gscalar = glv[l]
        cp = c[l - 1]
        for v in range(V):
            s = len(phi[l][v])
            dz = df[l][v] * dlrelu(z[l][v])
            S = Ss[l][v]
            col = S.sum(0)
            gb[s - 1] += dz.sum((0, 1))
            dtop, dbot = (dz, dz) if form == 1 else (dz[:, :, :cp], dz[:, :, cp:])
            kv = multiplicity(form, 1 + sum(len(phi[l][u]) == s for u in range(v)))
            gl1[s - 1] += kv * (dtop * S).sum((0, 1))
            gl2[s - 1] += kv * (dbot.sum(0) * col).sum(0)
            dS = lam1[s - 1] * dtop + lam2[s - 1] * dbot.sum(0)[None, :, :] * np.ones((s, 1, 1))
            gscalar += (radj[l][v][:, :, None] * dS).sum((0, 1))
            for w, idx, src in maps[l][v]:
                df[l - 1][w][np.ix_(src, src)] += dS[np.ix_(idx, idx)]
    for v in range(V):
        gH += np.outer((df[0][v] * dlrelu(z[0][v]))[0, 0], x[v])
    out["grads"] = grads
    return out


def run_batch(form, mols, targets, params, L, C, D, maxV, phis, nClass=0):
    """per-molecule results and the summed gradient"""
    res = [run(form, adj, x, float(t), params, L, C, D, maxV, phi, nClass) for (adj, x), t, phi in zip(mols, targets, phis)]
    return res, sum(r["grads"] for r in res)
