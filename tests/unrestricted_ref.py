"""fp64 numpy restatement of Unrestricted_SMP_1D (form 1), Unrestricted_SMP_1D_ver2 (form 2) and Unrestricted_SMP_2D (form 3), written
from the formulas (not from the device code):

  f_0[v]  = LeakyReLU(H x_v) as [1, C] (forms 1, 2) or [1, 1, C] (form 3)          x_v = the WL histogram features
  S       = sum over the children w (hops[v, w] <= 1) of X f_{l-1}[w] (forms 1, 2),   X[i, j] = [phi_l(v)[i] == phi_{l-1}(w)[j]]
            or of X f_{l-1}[w] X^T + scalar_l (x) adj_v (form 3), adj_v = the adjacency on phi_l(v) as it stands
  1:  z[i, c]    = sum_k W_s[i, k] S[k, c] + b_s[c]                  C_l = C,          slope 0.01
  2:  z[i]       = [(W1_s S)[i] | (W2_s S)[i]] + b_s                 C_l = 2 C_{l-1},  slope 0 at every level, level 0 included
  3:  z[i, j, c] = sum_k W_s[i, k, c] S[k, j, c] + b_s[c]            C_l = C,          slope 0.01
  g = sum_v LeakyReLU_{0.01}(sum over the positions of f_L[v]);   y = <g, W>, loss = (y - t)^2 / 2.

The gradients are the plain derivatives.  The restricted classes hand a vertex's filter gradient through shared ops that sit in the
graph once per vertex (smp1d_ref.py, smp2d_ref.py), which counts the j-th vertex of a size j or j (j + 1) / 2 times.  The unrestricted
classes have no such op: W_s is a parameter, added to the graph once in the preamble (Unrestricted_SMP_1D.h:420), and a vertex's MatMul /
TensorMul adds into its gradient directly -- `depth` = 0 shared ops in `executor_multiplicity`, which runs the accumulation itself.
`multiplicity` is the hook the tests swap to show that the rival rules miss the real classes' numbers.

`momentum_step` is Momentum::Learn(learning_rate, nBatch).  The receptive fields are an INPUT, as in theta_ref."""
import numpy as np

from theta_ref import executor_multiplicity as shared_op_multiplicity
from theta_ref import fields_of, hop_distances, wl_features  # noqa: F401

READOUT_ALPHA = 0.01


def slope(form):
    return 0.0 if form == 2 else 0.01


def lrelu(z, a):
    return np.where(z > 0, z, a * z)


def dlrelu(z, a):
    return np.where(z > 0, 1.0, a)


def channels(form, C, L):
    return [C << l if form == 2 else C for l in range(L + 1)]


def multiplicity(j):
    """how often the j-th vertex (1-based, ascending) of a field size is counted in dW_s: once"""
    return 1


def executor_multiplicity(k, depth=0):
    """theta_ref.executor_multiplicity with the unrestricted classes' depth as the default: no shared op, every vertex counted once"""
    return shared_op_multiplicity(depth, k)


def param_count(form, C, FD, L, maxV):
    c = channels(form, C, L)
    sq = maxV * (maxV + 1) * (2 * maxV + 1) // 6
    n = C * FD + c[L]
    for l in range(1, L + 1):
        fl = c[l - 1] if form == 3 else form
        n += fl * sq + maxV * c[l] + (c[l - 1] if form == 3 else 0)
    return n


def split(p, form, C, FD, L, maxV):
    """views into a flat parameter vector: H, per level (filters[s] = [halves, s, s] or [s, s, Cp], b[s], scalar or None), W"""
    c = channels(form, C, L)
    k = C * FD
    H = p[:k].reshape(C, FD)
    lv = [None]
    for l in range(1, L + 1):
        cp = c[l - 1]
        Ws, bs = {}, {}
        for s in range(1, maxV + 1):
            n = s * s * (cp if form == 3 else form)
            Ws[s] = p[k:k + n].reshape((s, s, cp) if form == 3 else (form, s, s))
            k += n
            bs[s] = p[k:k + c[l]]
            k += c[l]
        scalar = None
        if form == 3:
            scalar = p[k:k + cp]
            k += cp
        lv.append((Ws, bs, scalar))
    W = p[k:]
    assert W.size == c[L]
    return H, lv, W


def run(form, adj, feat, target, params, L, C, D, maxV, phi):
    """one molecule: graph_feature, predict, loss, grads, the pre-activations z[l][v], the activations f[l][v] ([s, C_l] or [s, s, C]) and
    for form 3 the adjacencies radj[l][v]"""
    feat = np.asarray(feat, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64)
    A = np.asarray(adj, dtype=np.float64)
    V = len(adj)
    a = slope(form)
    hops = hop_distances(adj)
    x = wl_features(feat, hops, D)
    FD = x.shape[1]
    H, lv, W = split(p, form, C, FD, L, maxV)
    first = (None, slice(None)) if form != 3 else (None, None, slice(None))
    z = [[(H @ x[v])[first] for v in range(V)]]
    Ss, radj, maps = [None], [None], [None]
    for l in range(1, L + 1):
        Ws, bs, scalar = lv[l]
        zl, Sl, al, ml = [], [], [], []
        for v in range(V):
            fv = list(phi[l][v])
            s = len(fv)
            ra = A[np.ix_(fv, fv)]
            if form == 3:
                S = ra[:, :, None] * scalar[None, None, :]
            else:
                S = np.zeros((s, z[l - 1][0].shape[-1]))
            mv = []
            for w in range(V):
                if hops[v, w] > 1:
                    continue
                fw = list(phi[l - 1][w])
                idx = [i for i, u in enumerate(fv) if u in fw]
                src = [fw.index(fv[i]) for i in idx]
                act = lrelu(z[l - 1][w], a)
                if form == 3:
                    S[np.ix_(idx, idx)] += act[np.ix_(src, src)]
                else:
                    S[idx] += act[src]
                mv.append((w, idx, src))
            if form == 3:
                zz = np.einsum("ikc,kjc->ijc", Ws[s], S) + bs[s][None, None, :]
            else:
                zz = np.concatenate([Ws[s][h] @ S for h in range(form)], axis=1) + bs[s][None, :]
            zl.append(zz)
            Sl.append(S)
            al.append(ra)
            ml.append(mv)
        z.append(zl)
        Ss.append(Sl)
        radj.append(al)
        maps.append(ml)
    pos = (0, 1) if form == 3 else (0,)
    sh = [lrelu(z[L][v], a).sum(pos) for v in range(V)]
    g = sum(lrelu(sh[v], READOUT_ALPHA) for v in range(V))
    grads = np.zeros_like(p)
    gH, glv, gW = split(grads, form, C, FD, L, maxV)
    y = float(g @ W)
    gW += (y - target) * g
    dg = (y - target) * W
    out = {"graph_feature": g, "z": z, "f": [[lrelu(zv, a) for zv in zl] for zl in z], "radj": radj, "predict": y,
           "loss": 0.5 * (y - target) ** 2}
    df = [[np.zeros_like(z[l][v]) for v in range(V)] for l in range(L + 1)]
    for v in range(V):
        df[L][v] += (dg * dlrelu(sh[v], READOUT_ALPHA))[first]
    for l in range(L, 0, -1):
        Ws, bs, scalar = lv[l]
        gWs, gbs, gscalar = glv[l]
        for v in range(V):
            s = len(phi[l][v])
            dz = df[l][v] * dlrelu(z[l][v], a)
            S = Ss[l][v]
            kv = multiplicity(1 + sum(len(phi[l][u]) == s for u in range(v)))
            gbs[s] += dz.sum(pos)
            if form == 3:
                gWs[s] += kv * np.einsum("ijc,kjc->ikc", dz, S)
                dS = np.einsum("ikc,ijc->kjc", Ws[s], dz)
                gscalar += (radj[l][v][:, :, None] * dS).sum((0, 1))
            else:
                cp = S.shape[1]
                dS = np.zeros_like(S)
                for h in range(form):
                    dzh = dz[:, h * cp:(h + 1) * cp]
                    gWs[s][h] += kv * (dzh @ S.T)
                    dS += Ws[s][h].T @ dzh
            for w, idx, src in maps[l][v]:
                if form == 3:
                    df[l - 1][w][np.ix_(src, src)] += dS[np.ix_(idx, idx)]
                else:
                    df[l - 1][w][src] += dS[idx]
    for v in range(V):
        gH += np.outer((df[0][v] * dlrelu(z[0][v], a)).reshape(-1), x[v])
    out["grads"] = grads
    return out


def run_batch(form, mols, targets, params, L, C, D, maxV, phis):
    """per-molecule results and the summed gradient"""
    res = [run(form, adj, x, float(t), params, L, C, D, maxV, phi) for (adj, x), t, phi in zip(mols, targets, phis)]
    return res, sum(r["grads"] for r in res)


def margin(res):
    """smallest |z| / largest |z| over the pre-activations of a batch (level 0, the levels, the read-out's sums); exact zeros excepted"""
    zs = []
    for r in res:
        zs += [np.abs(zv).ravel() for zl in r["z"] for zv in zl]
        L = len(r["z"]) - 1
        pos = (0, 1) if r["z"][L][0].ndim == 3 else (0,)
        zs += [np.abs(fv.sum(pos)) for fv in r["f"][L]]
    a = np.concatenate(zs)
    a = a[a > 0]
    return float(a.min() / a.max())


def momentum_step(params, moments, grads, learning_rate, nBatch, gamma=0.9):
    """Momentum::Learn(learning_rate, nBatch): returns (params, moments)"""
    moments = gamma * np.asarray(moments, dtype=np.float64) + learning_rate * np.asarray(grads, dtype=np.float64) / nBatch
    return np.asarray(params, dtype=np.float64) - moments, moments
