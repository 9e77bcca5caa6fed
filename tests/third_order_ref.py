"""fp64 restatement of GCN_3D (form 6) and GRU_GCN_3D (form 7) of GraphFlow/GCN_3D.h, GRU_GCN_3D.h, RisiLayer3D.h and KMax.h, for the
suites of gf_smp_config.neighbourhood = 6, 7.  tests/test_smp_third_order.py pins it to the real classes' numbers (tests/golden/
smp_third_order.npz) at 1e-9; the GPU suites use it at shapes without a golden.

The two models are GCN_1D / GRU_GCN_1D (neighbourhood_ref.py, gru_gcn_ref.py: x, N_l(v) = {u: dist(v, u) <= min(l, max_Radius)}, level 0,
the update, the read-out, the parameter blocks) with another aggregate:  n_l[v] = KMax(RisiLayer3D(members), K = H), the H largest of
  T[x, y, z] = sum over ordered triples (i, j, k) of distinct members of a_i[x] a_j[y] a_k[z]
in ascending order.  T is symmetric, so it is carried by canonical classes x <= y <= z of 6, 3 or 1 equal entries, in the closed form
  T = A_x A_y A_z - B_yz A_x - B_xz A_y - B_xy A_z + 2 sum_u a_u[x] a_u[y] a_u[z],   A = sum_u a_u,  B_pq = sum_u a_u[p] a_u[q];
which members of a class KMax keeps changes nothing.  Under three members T = 0 exactly: n = 0, nothing flows back.  Classes of equal
value are ordered by their largest flat index z H^2 + y H + x (the class's sort by (value, index), applied to classes).
`dtype=np.float32` evaluates everything in fp32, the selection included: the golden generator's rounding check."""
import itertools

import numpy as np

import gru_gcn_ref as gref
import neighbourhood_ref as nref
from neighbourhood_ref import hop_distances, lists_flat, shell_features, softmax  # noqa: F401

GAP = 1e-5   # the gap condition: adjacent classes around the cut differ by at least GAP * max|T| in fp64
_CLASSES = {}


def neighbourhoods(adj, L, max_Radius, sp=None):
    return gref.neighbourhoods(adj, L, max_Radius, sp)


def blocks(form, H, FD, L):
    return nref.blocks(H, FD, L) if form == 6 else gref.blocks(H, FD)


def n_params(form, H, FD, L):
    return sum(n for _, n in blocks(form, H, FD, L))


def classes(H):
    """(X, Y, Z, multiplicity, largest flat index) of the canonical classes x <= y <= z"""
    if H not in _CLASSES:
        t = np.array([(x, y, z) for x in range(H) for y in range(x, H) for z in range(y, H)], dtype=np.int64)
        X, Y, Z = t[:, 0], t[:, 1], t[:, 2]
        mult = np.where((X == Y) & (Y == Z), 1, np.where((X == Y) | (Y == Z), 3, 6))
        _CLASSES[H] = (X, Y, Z, mult, (Z * H + Y) * H + X)
    return _CLASSES[H]


def class_values(a):
    """T of every canonical class, in a's dtype, by the closed form"""
    X, Y, Z, _, _ = classes(a.shape[1])
    A = a.sum(axis=0)
    B = a.T @ a
    two = a.dtype.type(2)
    return A[X] * A[Y] * A[Z] - B[Y, Z] * A[X] - B[X, Z] * A[Y] - B[X, Y] * A[Z] + two * (a[:, X] * a[:, Y] * a[:, Z]).sum(axis=0)


def risi3d_loops(a):
    """RisiLayer3D::forward as the class loops: the full [H, H, H] tensor, T[x, y, z] at flat index z H^2 + y H + x"""
    m, H = a.shape
    T = np.zeros((H, H, H), dtype=a.dtype)
    for i, j, k in itertools.permutations(range(m), 3):
        T += np.einsum("x,y,z->xyz", a[i], a[j], a[k])
    return T


def kmax_loops(a):
    """the literal class: sort every entry by (value, flat index), keep the last H.  (n [H] ascending, kept flat indices)"""
    H = a.shape[1]
    flat = risi3d_loops(a).transpose(2, 1, 0).ravel()   # index z H^2 + y H + x
    order = np.lexsort((np.arange(flat.size), flat))[-H:]
    return flat[order], order


def kmax_loops_backward(a, kept, dn):
    """KMax::backward then RisiLayer3D::backward, literally"""
    m, H = a.shape
    da = np.zeros_like(a)
    for g, f in zip(dn, kept):
        x, y, z = f % H, (f // H) % H, f // (H * H)
        for i, j, k in itertools.permutations(range(m), 3):
            da[i, x] += g * a[j, y] * a[k, z]
            da[j, y] += g * a[i, x] * a[k, z]
            da[k, z] += g * a[i, x] * a[j, y]
    return da


def pool(a):
    """(n [H] ascending, sel [H, 3] the canonical triple per rank or -1, gap): the top H entries counted with multiplicity.  gap = the
    smallest difference of adjacent classes among those that hold the top H entries and the first below, over max|T| (inf under three
    members and where no class lies below)"""
    m, H = a.shape
    n, sel = np.zeros(H, dtype=a.dtype), np.full((H, 3), -1, dtype=np.int64)
    if m < 3:
        return n, sel, np.inf
    X, Y, Z, mult, flat = classes(H)
    T = class_values(a)
    order = np.lexsort((flat, T))[::-1]
    filled = used = 0
    while filled < H:
        c = order[used]
        take = min(int(mult[c]), H - filled)
        n[H - filled - take:H - filled] = T[c]
        sel[H - filled - take:H - filled] = (X[c], Y[c], Z[c])
        filled += take
        used += 1
    around = T[order[:used + 1]].astype(np.float64)   # (used + 1 runs past the end only at H = 1: one class)
    scale = np.abs(T).max()
    gap = np.inf if around.size < 2 or scale == 0 else float(np.abs(np.diff(around)).min() / scale)
    return n, sel, gap


def pool_backward(a, sel, dn):
    """the gradient of every member: per kept entry with gradient g, da_u[x] += g D_u(y, z) and its two rotations"""
    m, H = a.shape
    da = np.zeros_like(a)
    if m < 3:
        return da
    A = a.sum(axis=0)
    B = a.T @ a

    def D(p, q):   # [m]
        return (A[p] - a[:, p]) * (A[q] - a[:, q]) - (B[p, q] - a[:, p] * a[:, q])

    for (x, y, z), g in zip(sel, dn):
        da[:, x] += g * D(y, z)
        da[:, y] += g * D(x, z)
        da[:, z] += g * D(x, y)
    return da


def run(form, adj, feat, target, params, L, H, D, max_Radius=1, nbh=None, dtype=np.float64):
    """One molecule: predict, loss, graph_feature, grads (flat, registration order), h = [h_0 .. h_L], n = [None, n_1 ..], sel likewise,
    N = the lists, gap = the smallest gap over the vertex-levels with three members or more"""
    adj = np.asarray(adj)
    feat = np.asarray(feat, dtype=dtype)
    params = np.asarray(params, dtype=dtype)
    V, F = feat.shape
    FD = F * (D + 1)
    sp = hop_distances(adj)
    x = shell_features(feat, sp, D)
    N = neighbourhoods(adj, L, max_Radius, sp) if nbh is None else nbh
    one = dtype(1)
    grads = np.zeros_like(params)
    if form == 6:
        W1, W2, W = nref.split(params, H, FD, L)
        gW1, gW2, gW = nref.split(grads, H, FD, L)
        h = [softmax(x @ W1[0].T)]
    else:
        P, G = gref.split(params, H, FD), gref.split(grads, H, FD)
        h = [softmax(x @ P["W"].T)]
    n, sel, z, r, c, gap = [None], [None], [None], [None], [None], np.inf
    for l in range(1, L + 1):
        hp = h[l - 1]
        nl, sl = np.zeros((V, H), dtype=dtype), []
        for v in range(V):
            nl[v], s, g = pool(hp[N[l][v]])
            sl.append(s)
            gap = min(gap, g)
        n.append(nl), sel.append(sl)
        if form == 6:
            h.append(softmax(x @ W1[l].T + nl @ W2[l].T))
        else:
            zl = gref.sigmoid(nl @ P["W_z"].T + hp @ P["U_z"].T)
            rl = gref.sigmoid(nl @ P["W_r"].T + hp @ P["U_r"].T)
            cl = np.tanh(nl @ P["W_h"].T + (rl * hp) @ P["U_h"].T)
            z.append(zl), r.append(rl), c.append(cl)
            h.append((one - zl) * hp + zl * cl)
    if form == 6:
        gf = h[L].sum(axis=0)
        predict = (W * gf).sum()
        dy = predict - dtype(target)
        gW += dy * gf
        dh = np.tile(dy * W, (V, 1))
    else:
        s, t = gref.sigmoid(h[L] @ P["W_g"].T), np.tanh(h[L] @ P["U_g"].T)
        gf = np.tanh((s * t).sum(axis=0))
        predict = (P["U"] * gf).sum()
        dy = predict - dtype(target)
        G["U"] += dy * gf
        dg = dy * P["U"] * (one - gf * gf)
        ds, dt = dg * t * s * (one - s), dg * s * (one - t * t)
        G["W_g"] += ds.T @ h[L]
        G["U_g"] += dt.T @ h[L]
        dh = ds @ P["W_g"] + dt @ P["U_g"]
    for l in range(L, 0, -1):
        hp = h[l - 1]
        if form == 6:
            dz = dh * h[l] * (one - h[l])   # Softmax::backward: diagonal only
            gW1[l] += dz.T @ x
            gW2[l] += dz.T @ n[l]
            dn = dz @ W2[l]
            prev = np.zeros((V, H), dtype=dtype)
        else:
            dz = dh * (c[l] - hp) * z[l] * (one - z[l])
            dc = dh * z[l] * (one - c[l] * c[l])
            dq = dc @ P["U_h"]
            dr = dq * hp * r[l] * (one - r[l])
            G["W_z"] += dz.T @ n[l]
            G["U_z"] += dz.T @ hp
            G["W_r"] += dr.T @ n[l]
            G["U_r"] += dr.T @ hp
            G["W_h"] += dc.T @ n[l]
            G["U_h"] += dc.T @ (r[l] * hp)
            dn = dz @ P["W_z"] + dr @ P["W_r"] + dc @ P["W_h"]
            prev = dh * (one - z[l]) + dq * r[l] + dz @ P["U_z"] + dr @ P["U_r"]
        for v in range(V):   # consumer by consumer
            mem = N[l][v]
            if len(mem) >= 3:
                prev[mem] += pool_backward(hp[mem], sel[l][v], dn[v])
        dh = prev
    first = gW1[0] if form == 6 else G["W"]
    first += (dh * h[0] * (one - h[0])).T @ x
    return {"predict": predict, "loss": 0.5 * dy * dy, "graph_feature": gf, "grads": grads, "h": h, "n": n, "sel": sel, "N": N, "gap": gap}


def run_batch(form, mols, targets, params, L, H, D, max_Radius=1, dtype=np.float64):
    """(per-molecule results, the batch sum of the gradients)"""
    res = [run(form, a, f, t, params, L, H, D, max_Radius, dtype=dtype) for (a, f), t in zip(mols, targets)]
    return res, sum(r["grads"] for r in res)


def activations(res):
    return np.concatenate([hl.ravel() for hl in res["h"]])


def momentum_steps(form, mols, targets, params, L, H, D, max_Radius, n_iter, lr, gamma):
    """BatchLearn n_iter times: (losses [n_iter, 2], final parameters, the smallest gap met)"""
    p = np.array(params, dtype=np.float64)
    mom = np.zeros_like(p)
    losses, gap = [], np.inf
    for _ in range(n_iter):
        res, g = run_batch(form, mols, targets, p, L, H, D, max_Radius)
        before = sum(r["loss"] for r in res)
        mom = gamma * mom + lr * g / len(mols)
        p = p - mom
        after = run_batch(form, mols, targets, p, L, H, D, max_Radius)[0]
        gap = min([gap] + [r["gap"] for r in res + after])
        losses.append((before, sum(r["loss"] for r in after)))
    return np.array(losses), p, gap
