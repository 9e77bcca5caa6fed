"""Plain numpy reference of the operations that gf_smp_gru_{cell_fwd,cell_bwd,readout_fwd,readout_bwd}_ex_f32 run on the device
(smp_level_gru.hip: gru_cell_fwd, gru_cell_bwd, gru_readout_fwd / gru_readout_mol, gru_readout_dU / gru_readout_bwd), one function per
operator, written from the formulas in the header of tests/gru_gcn_ref.py; the lists, the aggregate and the error measure are those of
tests/neighbourhood_ops_ref.py.  M6 = W_z, U_z, W_r, U_r, W_h, U_h [6][H][H], M2 = W_g, U_g [2][H][H].

  cell forward   n = the aggregate of hprev over N(v) (sum; pairs: A Tt - sum_u a_u T_u; given: an operand), hp = hprev[v]
                 z = sigmoid(W_z n + U_z hp), r = sigmoid(W_r n + U_r hp), q = r hp, c = tanh(W_h n + U_h q), h = (1 - z) hp + z c, T = sum_k h_k
  cell backward  from dh and the STORED z, r, c the kernel is given (not recomputed ones):
                 dz' = dh (c - hp) z (1 - z), dc' = dh z (1 - c^2), dq = U_h^T dc', dr' = dq hp r (1 - r), q = r hp,
                 dn = W_z^T dz' + W_r^T dr' + W_h^T dc', gTt = dn Tt, sA = <dn, A>, direct = dh (1 - z) + dq r + U_z^T dz' + U_r^T dr'
  read-out       s = sigmoid(W_g hL), t = tanh(U_g hL), g[m] = tanh(sum_v s t), yhat = <U, g>, dy = yhat - target, loss = 0.5 dy^2
  its reverse    dg = dy[vmol] U (1 - g^2), ds = dg t s (1 - s), dt = dg s (1 - t^2), dh = W_g^T ds + U_g^T dt, dU = dU0 + sum_m dy[m] g[m]

Every function takes `dt` (float64 is the reference, float32 the yardstick: what a correct fp32 evaluation reaches) and `magnitude`:
with magnitude=True the same expression is evaluated on absolute values -- the MAGNITUDE SUM an output row is measured against
(row_err: max_i |x - ref| over the row's largest magnitude; a row of magnitude 0 is met exactly).

In a magnitude sum the difference 1 - c^2 counts as 1 + c^2 and c - hp as |c| + |hp|.  The reason is cancellation at |c| near 1: c is an
fp32 operand there, 1 - c^2 is formed from it in fp32 and loses every bit that c^2 shares with 1, so against |1 - c^2| the quotient is
unbounded on correct arithmetic.  A numpy float32 cell against float64 (H = 5 .. 64, both aggregates, lists up to 300 members) measures
up to 7.8e-5 on dc' and dr' with |1 - c^2| as the magnitude, and below 2.2e-7 on every output with 1 + c^2.  1 - z and 1 - r (z, r in
[0, 1]) stay as they are: the subtraction is exact above 0.5 and rounds once below.

The non-linear outputs are measured as the softmax level's h is, amag being the largest magnitude sum of the row's pre-activation:
  z, r, s   max(1, amag) max_i ref_i        sigmoid' = z (1 - z) <= z: a relative error delta of the argument moves z by at most delta amag z
  c, t, g   max(1, amag) min(1, amag)       tanh is 1-Lipschitz and |tanh a| <= |a|
  h         max(1, the largest amag of the three gates) max_i (|hp_i| + |c_i|)

tests/test_smp_gru_ops.py ties these formulas to tests/gru_gcn_ref.py (and so to the real classes) on golden molecules."""
import numpy as np

from neighbourhood_ops_ref import aggregate, csr, gather_backward, owners, row_den, row_err, seg_sum, transpose  # noqa: F401

SUM, PAIRS, GIVEN = 0, 1, 2


def sigmoid(x):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-x))


def _f(dt, magnitude):
    return (lambda a: np.abs(np.asarray(a, dtype=dt))) if magnitude else (lambda a: np.asarray(a, dtype=dt))


def cell_forward(M6, hprev, Tprev, ptr, idx, agg, n=None, dt=np.float64, magnitude=False):
    """{h, n, z, r, c, A, T, Tt} (A, Tt: the pair form alone; T = sum_k h_k in every form, stored by the pair form).
    magnitude: {n, az, ar, ac, A, Tt} -- the magnitude sums of n, of the three pre-activations, of A and of Tt; the gates inside are the
    true ones of the same dt (r <= 1 scales |hp| in q's magnitude)"""
    f = _f(dt, magnitude)
    M, hp = f(M6).reshape(6, hprev.shape[1], hprev.shape[1]), f(hprev)
    if agg == GIVEN:
        a = {"n": f(n), "A": None, "Tt": None}
    elif magnitude:
        a = {"n": aggregate(hprev, Tprev, ptr, idx, agg == PAIRS, dt, True), "A": None, "Tt": None}
        if agg == PAIRS:
            a["A"], a["Tt"] = seg_sum(hp[idx], ptr), seg_sum(f(Tprev)[idx], ptr)
    else:
        a = aggregate(hprev, Tprev, ptr, idx, agg == PAIRS, dt)
    az = a["n"] @ M[0].T + hp @ M[1].T
    ar = a["n"] @ M[2].T + hp @ M[3].T
    if magnitude:
        r = cell_forward(M6, hprev, Tprev, ptr, idx, agg, n, dt)["r"]
        return {"n": a["n"], "az": az, "ar": ar, "ac": a["n"] @ M[4].T + (r * hp) @ M[5].T, "A": a["A"], "Tt": a["Tt"]}
    z, r = sigmoid(az), sigmoid(ar)
    c = np.tanh(a["n"] @ M[4].T + (r * hp) @ M[5].T)
    h = (dt(1) - z) * hp + z * c
    return {"h": h, "n": a["n"], "z": z, "r": r, "c": c, "A": a["A"] if agg == PAIRS else None, "T": h.sum(axis=1),
            "Tt": a["Tt"] if agg == PAIRS else None}


def cell_forward_dens(M6, hprev, Tprev, ptr, idx, agg, n, ref):
    """the denominators (one per row) of h, n, z, r, c (, A, T, Tt) beside the fp64 result `ref` of cell_forward()"""
    mag = cell_forward(M6, hprev, Tprev, ptr, idx, agg, n, magnitude=True)
    amag = {k: row_den(mag["a" + k]) for k in "zrc"}
    one = {k: np.maximum(1.0, v) for k, v in amag.items()}
    den = {"z": one["z"] * ref["z"].max(axis=1), "r": one["r"] * ref["r"].max(axis=1), "c": one["c"] * np.minimum(1.0, amag["c"]),
           "h": np.maximum(one["z"], np.maximum(one["r"], one["c"])) * (np.abs(hprev) + np.abs(ref["c"])).max(axis=1)}
    if agg != GIVEN:
        den["n"] = row_den(mag["n"])
    if agg == PAIRS:
        den["A"], den["Tt"], den["T"] = row_den(mag["A"]), mag["Tt"], np.abs(ref["h"]).sum(axis=1)
    return den


def cell_backward(M6, hprev, dh, z, r, c, A, Tt, pairs, dt=np.float64, magnitude=False):
    """{dzp, drp, dcp, q, dn, direct} and with pairs {gTt, sA}; z, r, c are the stored gates"""
    f = _f(dt, magnitude)
    H = hprev.shape[1]
    M, hp, d, z, r, c = f(M6).reshape(6, H, H), f(hprev), f(dh), f(z), f(r), f(c)
    one = dt(1)
    diff, omc = (c + hp, one + c * c) if magnitude else (c - hp, one - c * c)
    dz = d * diff * z * (one - z)
    dc = d * z * omc
    dq = dc @ M[5]
    dr = dq * hp * r * (one - r)
    out = {"dzp": dz, "drp": dr, "dcp": dc, "q": r * hp, "dn": dz @ M[0] + dr @ M[2] + dc @ M[4],
           "direct": d * (one - z) + dq * r + dz @ M[1] + dr @ M[3]}
    if pairs:
        out["gTt"] = out["dn"] * f(Tt)[:, None]
        out["sA"] = (out["dn"] * f(A)).sum(axis=1)
    return out


def readout_forward(M2, U, hL, mol_ptr, target, dt=np.float64, magnitude=False):
    """{s, t, g, yhat, dy, loss}; target None: 0.  magnitude: {as, at, ag, yhat, dy, loss} -- the magnitude sums of the three arguments
    (g's with the true s, t of the same dt) and of the linear outputs: yhat is computed from the operator's own g, whose sum of s t may
    cancel, so g counts as min(1, its argument's magnitude sum) there, not as |g|"""
    f = _f(dt, magnitude)
    H = hL.shape[1]
    M, h = f(M2).reshape(2, H, H), f(hL)
    a_s, a_t = h @ M[0].T, h @ M[1].T
    ptr = np.asarray(mol_ptr, dtype=np.int64)
    tg = f(target) if target is not None else np.zeros(len(ptr) - 1, dtype=dt)
    if magnitude:
        true = readout_forward(M2, U, hL, mol_ptr, target, dt)
        ag = seg_sum(true["s"] * np.abs(true["t"]), ptr)
        yhat = (np.minimum(dt(1), ag) * f(U)[None, :]).sum(axis=1)
        dy = yhat + tg
        return {"as": a_s, "at": a_t, "ag": ag, "yhat": yhat, "dy": dy, "loss": dt(0.5) * dy * dy}
    s, t = sigmoid(a_s), np.tanh(a_t)
    g = np.tanh(seg_sum(s * t, ptr))
    yhat = (g * f(U)[None, :]).sum(axis=1)
    dy = yhat - tg
    return {"s": s, "t": t, "g": g, "yhat": yhat, "dy": dy, "loss": dt(0.5) * dy * dy}


def readout_forward_dens(M2, U, hL, mol_ptr, target, ref):
    mag = readout_forward(M2, U, hL, mol_ptr, target, magnitude=True)
    a = {k: row_den(mag["a" + k]) for k in "stg"}
    return {"s": np.maximum(1.0, a["s"]) * ref["s"].max(axis=1), "t": np.maximum(1.0, a["t"]) * np.minimum(1.0, a["t"]),
            "g": np.maximum(1.0, a["g"]) * np.minimum(1.0, a["g"]), "yhat": mag["yhat"], "dy": mag["dy"], "loss": mag["loss"]}


def readout_backward(M2, U, s, t, g, dy, vmol, dU0, dt=np.float64, magnitude=False):
    """{ds, dt, dh, dU} from the stored s, t, g, dy"""
    f = _f(dt, magnitude)
    H = s.shape[1]
    M, U, s, t, g, dy = f(M2).reshape(2, H, H), f(U), f(s), f(t), f(g), f(dy)
    one = dt(1)
    omg, omt = (one + g * g, one + t * t) if magnitude else (one - g * g, one - t * t)
    dg = (dy[:, None] * U[None, :] * omg)[np.asarray(vmol)]
    ds, dtt = dg * t * s * (one - s), dg * s * omt
    return {"ds": ds, "dt": dtt, "dh": ds @ M[0] + dtt @ M[1], "dU": f(dU0) + (dy[:, None] * g).sum(axis=0)}


def unsaturated(z, r, c):
    """the shares of z, r in [0.05, 0.95] and of |c| < 0.95"""
    return tuple(float(np.mean(m)) for m in ((z >= 0.05) & (z <= 0.95), (r >= 0.05) & (r <= 0.95), np.abs(c) < 0.95))
