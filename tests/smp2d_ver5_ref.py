"""fp64 numpy restatement of SMP_2D_ver5 (gf_smp_config.steerable_2d = 5), written from the formulas (not from the device code), on the
unchanged helpers of smp2d_ref.py:

  f_0[v]  = LeakyReLU3D(H x_v) as [1, 1, C]
  S       = sum over the children w (hops[v, w] <= 1) of X f_{l-1}[w] X^T + scalar_l (x) adj_v
  adj_v   = the adjacency reduced to phi_l(v) with a unit diagonal, every row divided by its sum (SMP_2D_ver4's)
  col[j]  = sum_k S[k, j]
  z[i, j] = K_l [lambda1_s S[i, j] | lambda2_s col[j]] + b_s        K_l [C, 2C], row = output channel; C channels at every level
  f_l[v]  = LeakyReLU3D(z), slope 0.01;   g = sum_v LeakyReLU(sum_ij f_L[v][i, j]);   y = <g, W>, loss = (y - t)^2 / 2.

Gradients as the reference's EXECUTOR leaves them (smp2d_ref.py): W_eye[s] / W_one[s] (VectorBroadcastMat) are shared by the vertices of
a size and sit between a vertex's TensorMul and lambda_s, so the j-th vertex of its size (ascending) counts `multiplicity(j)` = j times
in dlambda1_s / dlambda2_s.  K_l is added to the graph once, in the preamble, and every vertex's CustomMatMulTensor adds into
K_l->gradient directly: `k_multiplicity(j)` = 1, dK_l is the plain derivative -- as are db_s, dscalar_l, dH and dW.

The receptive fields are an INPUT, as in smp2d_ref."""
import numpy as np

from smp2d_ref import dlrelu, fields_of, hop_distances, lrelu, reduced_adjacency, wl_features  # noqa: F401


def multiplicity(j):
    """how often the j-th vertex (1-based, ascending) of a field size is counted in dlambda_s: SMP_2D_ver4's rule"""
    return j


def k_multiplicity(j):
    """... and in dK_l: K_l is not behind a shared op"""
    return 1


def param_count(C, FD, L, maxV):
    return C * FD + L * (maxV * 3 * C + 2 * C * C + C) + C


def split(p, C, FD, L, maxV):
    """views into a flat parameter vector: H, per level (lam1[maxV, C], lam2[maxV, C], b[maxV, C], K[C, 2C], scalar[C]), W"""
    k = C * FD
    H = p[:k].reshape(C, FD)
    lv = [None]
    for l in range(1, L + 1):
        blk = p[k:k + maxV * 3 * C].reshape(maxV, 3 * C)
        k += maxV * 3 * C
        K = p[k:k + 2 * C * C].reshape(C, 2 * C)
        k += 2 * C * C
        lv.append((blk[:, :C], blk[:, C:2 * C], blk[:, 2 * C:], K, p[k:k + C]))
        k += C
    W = p[k:]
    assert W.size == C
    return H, lv, W


def run(adj, feat, target, params, L, C, D, maxV, phi):
    """one molecule: graph_feature, predict, loss, grads, the activations f[l][v] ([s, s, C]) and reduced adjacencies radj[l][v]; also the
    level's operands S[l][v] and dz[l][v] ([s, s, C]; col = S.sum(0), cz = dz.sum(0)), for tests/smp2d_ver5_ops_ref.py"""
    feat = np.asarray(feat, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64)
    V = len(adj)
    hops = hop_distances(adj)
    x = wl_features(feat, hops, D)
    FD = x.shape[1]
    H, lv, W = split(p, C, FD, L, maxV)
    z = [[(H @ x[v])[None, None, :] for v in range(V)]]
    Ss, radj, maps = [None], [None], [None]
    for l in range(1, L + 1):
        lam1, lam2, b, K, scalar = lv[l]
        zl, Sl, al, ml = [], [], [], []
        for v in range(V):
            fv = list(phi[l][v])
            s = len(fv)
            a = reduced_adjacency(2, adj, fv)
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
            col = S.sum(0)
            zz = (lam1[s - 1] * S) @ K[:, :C].T + ((lam2[s - 1] * col) @ K[:, C:].T)[None, :, :] + b[s - 1][None, None, :]
            zl.append(zz)
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
    gH, glv, gW = split(grads, C, FD, L, maxV)
    y = float(g @ W)
    gW += (y - target) * g
    dg = (y - target) * W
    out = {"graph_feature": g, "f": [[lrelu(zv) for zv in zl] for zl in z], "radj": radj, "predict": y, "loss": 0.5 * (y - target) ** 2}
    df = [[np.zeros_like(z[l][v]) for v in range(V)] for l in range(L + 1)]
    out["S"], out["dz"] = Ss, [None] + [[None] * V for _ in range(L)]
    for v in range(V):
        df[L][v] += (dg * dlrelu(sh[v]))[None, None, :]
    for l in range(L, 0, -1):
        lam1, lam2, b, K, scalar = lv[l]
        gl1, gl2, gb, gK, gscalar = glv[l]
        for v in range(V):
            s = len(phi[l][v])
            dz = out["dz"][l][v] = df[l][v] * dlrelu(z[l][v])
            S = Ss[l][v]
            col = S.sum(0)
            cz = dz.sum(0)
            gb[s - 1] += dz.sum((0, 1))
            j = 1 + sum(len(phi[l][u]) == s for u in range(v))
            kk = k_multiplicity(j)
            gK[:, :C] += kk * np.einsum("ijc,ijd->cd", dz, lam1[s - 1] * S)
            gK[:, C:] += kk * np.einsum("jc,jd->cd", cz, lam2[s - 1] * col)
            dE = dz @ K[:, :C]          # gradient of the eye half of the concatenation, [s, s, C]
            dO = cz @ K[:, C:]          # ... of the one half, one vector per column
            kv = multiplicity(j)
            gl1[s - 1] += kv * (dE * S).sum((0, 1))
            gl2[s - 1] += kv * (dO * col).sum(0)
            dS = lam1[s - 1] * dE + (lam2[s - 1] * dO)[None, :, :]
            gscalar += (radj[l][v][:, :, None] * dS).sum((0, 1))
            for w, idx, src in maps[l][v]:
                df[l - 1][w][np.ix_(src, src)] += dS[np.ix_(idx, idx)]
    for v in range(V):
        gH += np.outer((df[0][v] * dlrelu(z[0][v]))[0, 0], x[v])
    out["grads"] = grads
    return out


def run_batch(mols, targets, params, L, C, D, maxV, phis):
    """per-molecule results and the summed gradient"""
    res = [run(adj, x, float(t), params, L, C, D, maxV, phi) for (adj, x), t, phi in zip(mols, targets, phis)]
    return res, sum(r["grads"] for r in res)
