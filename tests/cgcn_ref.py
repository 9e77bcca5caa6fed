"""numpy restatement of CGCN_1D and CGCN_2D (GraphFlow/CGCN_1D.h, CGCN_2D.h; gf_smp_config.covariant = 1, 2), in fp64 or fp32: forward,
backward and the Momentum step.  A vertex carries one vector h_l[v] of length M = max_nVertices indexed by the molecule's vertex ids:
  h_0[v] = e_v <x[v], H>;  n_l[v] = the aggregate of h_{l-1} over N(v) = {u : adj[u][v] > 0} (ascending);
  h_l[v] = LeakyReLU(mask_l(v) * (F_l n_l[v])), mask_l(v)[i] = sp[i][v] <= l, slope 0.01;
  graph feature = sum_v h_L[v], predict = the sum of its components, loss = 0.5 (predict - target)^2.
The 2D aggregate (RisiLayer2D) is written twice: as the class's loops over pairs u < w of members, and in the closed form with the
exclusive sums evaluated directly.  Parameters in registration order: H [F'], F_1 .. F_L [M][M] each."""
import numpy as np

from neighbourhood_ref import hop_distances, shell_features

SLOPE = 0.01


def blocks(FD, L, M):
    """[(block name, size)] in registration (= Momentum = save_model) order"""
    return [("H", FD)] + [("F_%d" % l, M * M) for l in range(1, L + 1)]


def n_params(FD, L, M):
    return FD + L * M * M


def neighbours(adj):
    """N(v) = {u : adj[u][v] > 0}: column v, ascending; a set diagonal entry makes v its own neighbour"""
    V = len(adj)
    return [[u for u in range(V) if adj[u][v] > 0] for v in range(V)]


def masks(adj, L, M, sp=None):
    """[L + 1][V][M] 0/1: position i of vertex v where sp[i][v] <= l (zero beyond the molecule)"""
    sp = hop_distances(adj) if sp is None else sp
    V = len(adj)
    out = np.zeros((L + 1, V, M))
    for l in range(L + 1):
        out[l, :, :V] = (sp.T <= l)
    return out


def aggregate_pairs(hs, M):
    """RisiLayer2D as the class writes it: over pairs u < w of members and all (i, k), value[i] += h_u[i] h_w[k] + h_u[k] h_w[i]"""
    out = np.zeros(M, dtype=hs[0].dtype if hs else np.float64)
    for a in range(len(hs)):
        for b in range(a + 1, len(hs)):
            out += hs[a] * hs[b].sum() + hs[a].sum() * hs[b]
    return out


def aggregate_closed(hs, M):
    """the same in closed form: sum_u h_u[i] * (sum over the OTHER members w of s_w), the exclusive sums added directly"""
    dt = hs[0].dtype if hs else np.float64
    s = [h.sum(dtype=dt) for h in hs]
    out = np.zeros(M, dtype=dt)
    for a, h in enumerate(hs):
        ex = dt.type(0)
        for b in range(len(hs)):
            if b != a:
                ex = ex + s[b]
        out = out + h * ex
    return out


def network(form, N, mk, s0, Fs, target, M, dtype=np.float64, pair_loops=False):
    """The network of one molecule on prepared operands: N [V] the lists, mk [L + 1][V][M] the 0/1 masks, s0 [V] the level-0 scalars,
    Fs [L] the matrices [M][M].  Returns h [L + 1][V][M], n [L][V][M], the graph feature, predict, loss, dy, dF [L][M][M], ds0 [V]."""
    V, L = len(N), len(Fs)
    slope = dtype(SLOPE)
    mk = np.asarray(mk, dtype=dtype)
    h = np.zeros((L + 1, V, M), dtype=dtype)
    n = np.zeros((L, V, M), dtype=dtype)
    for v in range(V):
        h[0, v, v] = s0[v]
    for l in range(1, L + 1):
        for v in range(V):
            hs = [h[l - 1, u] for u in N[v]]
            if form == 1:
                n[l - 1, v] = sum(hs, np.zeros(M, dtype=dtype))
            else:
                n[l - 1, v] = aggregate_pairs(hs, M) if pair_loops else aggregate_closed(hs, M)
            z = (Fs[l - 1] @ n[l - 1, v]) * mk[l, v]
            h[l, v] = np.where(z > 0, z, slope * z)
    g = h[L].sum(axis=0)
    predict = g.sum()
    dy = predict - dtype(target)
    loss = dtype(0.5) * dy * dy
    dF = np.zeros((L, M, M), dtype=dtype)
    dh = np.full((V, M), dy, dtype=dtype)   # SumComponents, SumVectors (positions >= V too, as the class)
    for l in range(L, 0, -1):
        dprev = np.zeros((V, M), dtype=dtype)
        for v in range(V):
            dz = dh[v] * np.where(h[l, v] > 0, dtype(1), slope) * mk[l, v]
            dF[l - 1] += np.outer(dz, n[l - 1, v])
            dn = Fs[l - 1].T @ dz
            if form == 1:
                for u in N[v]:
                    dprev[u] += dn
            else:
                s = {u: h[l - 1, u].sum() for u in N[v]}
                q = {u: dn @ h[l - 1, u] for u in N[v]}
                for u in N[v]:
                    ex = sum((s[w] for w in N[v] if w != u), dtype(0))
                    c = sum((q[w] for w in N[v] if w != u), dtype(0))
                    dprev[u] += dn * ex + c
        dh = dprev
    return {"h": h, "n": n, "feature": g, "predict": predict, "loss": loss, "dy": dy, "dF": dF,
            "ds0": np.array([dh[v, v] for v in range(V)], dtype=dtype)}


def run(form, adj, feat, target, params, L, M, D, dtype=np.float64, pair_loops=False):
    """One molecule, forward and backward.  Returns network()'s entries and the masks, lists, x and the gradient in registration order."""
    adj = np.asarray(adj)
    V, FD = len(adj), feat.shape[1] * (D + 1)
    sp = hop_distances(adj)
    x = shell_features(np.asarray(feat, dtype=np.float64), sp, D).astype(dtype)
    p = np.asarray(params, dtype=dtype)
    Hw, Fs = p[:FD], [p[FD + l * M * M:FD + (l + 1) * M * M].reshape(M, M) for l in range(L)]
    N, mk = neighbours(adj), masks(adj, L, M, sp).astype(dtype)
    r = network(form, N, mk, [x[v] @ Hw for v in range(V)], Fs, target, M, dtype, pair_loops)
    dH = np.zeros(FD, dtype=dtype)
    for v in range(V):
        dH += r["ds0"][v] * x[v]
    r.update(masks=mk, lists=N, x=x, grads=np.concatenate([dH, r["dF"].ravel()]))
    return r


def lists_flat(N):
    """the lists as one int array: per vertex the count, then the members"""
    out = []
    for mem in N:
        out += [len(mem)] + list(mem)
    return np.array(out, dtype=np.int32)


def min_preactivation_gap(form, adj, feat, params, L, M, D):
    """the smallest |z| of an in-mask pre-activation over max |z| (levels 1 .. L); inf without levels.  A vertex whose aggregate is
    identically zero (no neighbour; in the 2D class fewer than two) has z = 0 exactly in every precision: not a rounding hazard, left out."""
    r = run(form, adj, feat, 0.0, params, L, M, D)
    FD, worst = feat.shape[1] * (D + 1), np.inf
    p = np.asarray(params, dtype=np.float64)
    for l in range(1, L + 1):
        F = p[FD + (l - 1) * M * M:FD + l * M * M].reshape(M, M)
        z = r["n"][l - 1] @ F.T
        inm = (r["masks"][l] > 0) & (np.abs(r["n"][l - 1]).max(axis=1, keepdims=True) > 0)
        if inm.any() and np.abs(z).max() > 0:
            worst = min(worst, np.abs(z[inm]).min() / np.abs(z[inm]).max())
    return worst


def batch_grads(form, mols, targets, params, L, M, D, dtype=np.float64):
    """(sum of the losses, batch gradient) of a batch, as BatchLearn accumulates them"""
    loss, g = 0.0, 0.0
    for (adj, feat), t in zip(mols, targets):
        r = run(form, adj, feat, t, params, L, M, D, dtype)
        loss, g = loss + r["loss"], g + r["grads"]
    return loss, g


def momentum_steps(form, mols, targets, params, L, M, D, n_iter, lr, gamma, dtype=np.float64):
    """BatchLearn n_iter times (Momentum::Learn(lr, nBatch)): (losses [n_iter, 2], final parameters)"""
    p = np.array(params, dtype=dtype)
    mom = np.zeros_like(p)
    losses = []
    for _ in range(n_iter):
        before, g = batch_grads(form, mols, targets, p, L, M, D, dtype)
        mom = dtype(gamma) * mom + dtype(lr) * g / dtype(len(mols))
        p = p - mom
        losses.append((before, batch_grads(form, mols, targets, p, L, M, D, dtype)[0]))
    return np.array(losses), p
