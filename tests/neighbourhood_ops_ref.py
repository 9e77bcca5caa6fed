"""Plain numpy reference of the operations that gf_smp_neighbourhood_{fwd,node_bwd,gather_bwd,readout}_ex_f32 run on the device
(smp_level_neighbourhood.hip: nbh_level_fwd, nbh_node_bwd, nbh_gather_bwd, nbh_readout / nbh_readout_dW), written from the definitions
of tests/neighbourhood_ref.py, vectorised over the edges of a CSR list, and the error measures of tests/test_smp_neighbourhood_ops_gpu.py.

  aggregate     n[v] = sum_u a_u over N(v)                      (sum)     a_u = hprev[u], T_u = Tprev[u]
                n[v] = A Tt - sum_u a_u T_u,  A = sum_u a_u, Tt = sum_u T_u   (pairs: risi2d_closed with the stored T)
  forward       h[v] = softmax(W1 x[v] + W2 n[v]),  T[v] = sum_k h[v][k]
  node backward dz = d h (1 - h), d = dh or dy[vmol] Wout;  dn = dz W2;  gTt = dn Tt;  sA = <dn, A>
  gather        dhprev[w] = sum over consumers v of w of dn[v]                                  (sum)
                dhprev[w] = sum over consumers v of w of the row of w in risi2d_closed_backward(a of N(v), dn[v])   (pairs)
                -- per consumer, NOT the four regrouped sums of the kernel: the regrouping is part of what is tested
  readout       g[m] = sum_v h[v], yhat = <W, g>, dy = yhat - target, loss = 0.5 dy^2, dW += sum_m dy[m] g[m]

Every function takes `dt`: float64 is the reference, float32 the evaluation that shows what a correct fp32 kernel can reach.  With
magnitude=True the same expression is evaluated on absolute values: the MAGNITUDE SUM an output is measured against, per row
(row_err: max_i |x - ref| over the largest magnitude of the row).  For h the denominator is max(1, zmag) max_i href[i] with zmag the
largest magnitude sum of a pre-activation of the row: a relative error delta in z moves h[i] by at most 2 delta h[i].

tests/test_smp_neighbourhood_ops.py ties these formulas to tests/neighbourhood_ref.py (and so to the real classes) on golden molecules."""
import numpy as np


def csr(lists):
    """(ptr int64 [n + 1], idx int32) of a list of member lists"""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(m) for m in lists])
    idx = np.fromiter((u for m in lists for u in m), dtype=np.int32, count=int(ptr[-1]))
    return ptr, idx


def owners(ptr):
    """the list every entry of idx belongs to"""
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def transpose(ptr, idx, n):
    """the CSR list of the reversed edges, members ascending"""
    own = owners(ptr)
    order = np.lexsort((own, idx))
    tptr = np.zeros(n + 1, dtype=np.int64)
    tptr[1:] = np.cumsum(np.bincount(idx, minlength=n))
    return tptr, own[order].astype(np.int32)


def seg_sum(vals, ptr):
    """out[i] = sum of vals[ptr[i] : ptr[i + 1]] in vals' own type (an empty segment gives 0)"""
    out = np.zeros((len(ptr) - 1,) + vals.shape[1:], dtype=vals.dtype)
    full = np.diff(ptr) > 0
    if full.any():
        out[full] = np.add.reduceat(vals, ptr[:-1][full], axis=0)
    return out


def aggregate(hprev, Tprev, ptr, idx, pairs, dt=np.float64, magnitude=False):
    """{n, A, Tt}; the sum form has A = n and no Tt.  magnitude: n's magnitude sum alone"""
    a = np.asarray(hprev, dtype=dt)[idx]
    if magnitude:
        a = np.abs(a)
    A = seg_sum(a, ptr)
    if not pairs:
        return A if magnitude else {"n": A, "A": A, "Tt": None}
    t = np.asarray(Tprev, dtype=dt)[idx]
    if magnitude:
        t = np.abs(t)
    Tt = seg_sum(t, ptr)
    S = seg_sum(a * t[:, None], ptr)
    if magnitude:
        return A * Tt[:, None] + S
    return {"n": A * Tt[:, None] - S, "A": A, "Tt": Tt}


def pre_activation(W1, x, W2, n, dt=np.float64, magnitude=False):
    """z = W1 x + W2 n (n None: level 0); magnitude: n is then n's magnitude sum"""
    W1, x = np.asarray(W1, dtype=dt), np.asarray(x, dtype=dt)
    if magnitude:
        W1, x = np.abs(W1), np.abs(x)
    z = x @ W1.T
    if W2 is not None:
        W2, n = np.asarray(W2, dtype=dt), np.asarray(n, dtype=dt)
        z = z + n @ (np.abs(W2) if magnitude else W2).T
    return z


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def forward(W1, x, W2, hprev, Tprev, ptr, idx, pairs, dt=np.float64):
    """{h, T, n, A, Tt} of one level (W2 None: level 0, no aggregate)"""
    agg = aggregate(hprev, Tprev, ptr, idx, pairs, dt) if W2 is not None else {"n": None, "A": None, "Tt": None}
    h = softmax(pre_activation(W1, x, W2, agg["n"], dt))
    return dict(agg, h=h, T=h.sum(axis=1))


def forward_dens(W1, x, W2, hprev, Tprev, ptr, idx, pairs, ref):
    """the denominators of h, T, n, A, Tt (one per row) beside the fp64 result `ref` of forward()"""
    nmag = aggregate(hprev, Tprev, ptr, idx, pairs, magnitude=True) if W2 is not None else None
    zmag = np.maximum(1.0, pre_activation(W1, x, W2, nmag, magnitude=True).max(axis=1))
    den = {"h": zmag * ref["h"].max(axis=1), "T": zmag * ref["T"]}
    if W2 is not None:
        den["n"] = nmag.max(axis=1)
        if pairs:
            den["A"], den["Tt"] = ref["A"].max(axis=1), ref["Tt"]
    return den


def node_backward(W2, h, dh, dy, Wout, vmol, A, Tt, pairs, dt=np.float64, magnitude=False):
    """{dz, dn, gTt, sA} (W2 None: dz alone; dy None: d = dh, else d = dy[vmol] Wout)"""
    f = (lambda a: np.abs(np.asarray(a, dtype=dt))) if magnitude else (lambda a: np.asarray(a, dtype=dt))
    h = np.asarray(h, dtype=dt)
    d = f(dh) if dy is None else f(dy)[vmol][:, None] * f(Wout)[None, :]
    one_minus = dt(1) - h
    out = {"dz": d * h * (np.abs(one_minus) if magnitude else one_minus)}
    if W2 is not None:
        out["dn"] = out["dz"] @ f(W2)
        if pairs:
            out["gTt"] = out["dn"] * f(Tt)[:, None]
            out["sA"] = (out["dn"] * f(A)).sum(axis=1)
    return out


def gather_backward(tptr, tidx, dn, hprev, Tprev, pairs, dt=np.float64, magnitude=False):
    """dhprev [nV][H] over the transposed list.  pairs: the consumers' lists are the transpose of (tptr, tidx); per consumer v and member
    w the row of risi2d_closed_backward is dn[v] (Tt_v - T_w) + <dn[v], A_v - a_w>, summed over the consumers of w"""
    nV = len(tptr) - 1
    g = np.asarray(dn, dtype=dt)
    if magnitude:
        g = np.abs(g)
    if not pairs:
        return seg_sum(g[tidx], tptr)
    a, T = np.asarray(hprev, dtype=dt), np.asarray(Tprev, dtype=dt)
    ptr, idx = transpose(tptr, tidx, nV)
    A, Tt = seg_sum(a[idx], ptr), seg_sum(T[idx], ptr)
    w = owners(tptr)
    gv = g[tidx]
    if magnitude:
        da = gv * (Tt[tidx] + T[w])[:, None] + (gv * (A[tidx] + a[w])).sum(axis=1, keepdims=True)
    else:
        da = gv * (Tt[tidx] - T[w])[:, None] + (gv * (A[tidx] - a[w])).sum(axis=1, keepdims=True)
    return seg_sum(da, tptr)


def readout(hL, mol_ptr, W, target, dW0, dt=np.float64, magnitude=False):
    """{g, yhat, dy, loss, dW}: dW = dW0 + sum_m dy[m] g[m]; target None: 0"""
    f = (lambda a: np.abs(np.asarray(a, dtype=dt))) if magnitude else (lambda a: np.asarray(a, dtype=dt))
    g = seg_sum(f(hL), np.asarray(mol_ptr, dtype=np.int64))
    yhat = (g * f(W)[None, :]).sum(axis=1)
    t = f(target) if target is not None else np.zeros(len(g), dtype=dt)
    dy = yhat + t if magnitude else yhat - t
    return {"g": g, "yhat": yhat, "dy": dy, "loss": dt(0.5) * dy * dy, "dW": f(dW0) + (dy[:, None] * g).sum(axis=0)}


def row_err(x, ref, den):
    """the largest per-row error: max_i |x - ref| over the row's denominator (vectors: one element per row).  A row whose magnitude sum
    is 0 has to be met exactly."""
    x, ref, den = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(den, dtype=np.float64)
    assert x.shape == ref.shape and den.shape == ref.shape[:1], (x.shape, ref.shape, den.shape)
    assert np.all(np.isfinite(ref)) and np.all(den >= 0)
    d = np.abs(x - ref)
    d = d.reshape(len(d), -1).max(axis=1)
    d = np.where(np.isfinite(d), d, np.inf)   # (a NaN is an infinite error, not an ignored one)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(den > 0, d / den, np.where(d == 0, 0.0, np.inf))
    return float(e.max())


def row_den(mag):
    """the largest magnitude of each row"""
    return mag.reshape(len(mag), -1).max(axis=1)
