"""The two network kernels of the covariant level (smp_level_covariant.hip), one by one on caller-supplied operands:
  gf_smp_covariant_forward_ex_f32    cov_network_fwd: every h_l[v] and n_l[v], the graph feature, prediction, loss and dy
  gf_smp_covariant_backward_ex_f32   cov_network_bwd and cov_fold: dF [L][M][M] and the gradient of the level-0 scalars
against tests/cgcn_ref.py in fp64 on synthetic packed batches, at the smallest shapes where they can go wrong: V = 1, 2, 31, 32, 33, 64
(the half-wave and wave boundaries) with M = V and M = 64; a vertex with no neighbour and one with a single neighbour (the 2D aggregate is
zero), a self-neighbour, an asymmetric list; V = 1 and V = M in one launch; L = 0, 1, 4; 300 molecules of at most 6 vertices (several
chunks of the gradient's partition and a ragged last one).  Tolerance: field_suite.TOL per output block; the same call twice gives the
same bits.  Every output lies in a buffer with sentinel rows behind its last row.

The inputs: s0 and F are multiples of 1/64, mostly positive, F_l times the power of two that brings max |h_l| into [0.5, 1).  LeakyReLU's
derivative jumps at zero, so a pre-activation that fp32 rounding can carry across zero would be a property of the inputs, not of the kernels.
The rounding of z[i] = sum_j F[i][j] n[j] is bounded by about (V + L) 2^-24 sum_j |F[i][j]| |n[j]| (4e-6 of that sum at V = 64, the error n
brings along included), so a batch whose fp64 reference has an in-mask pre-activation below 1e-4 sum_j |F[i][j]| |n[j]| -- other than the
exact zeros of an empty aggregate -- is drawn again with the next seed, before the device is asked."""
import numpy as np
import pytest

import cgcn_ref as cref
from field_suite import TOL, dev
from neighbourhood_ref import hop_distances
from test_smp_neighbourhood_ops_gpu import context, guarded, ptr, same_bits, taken
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INVALID = 1
_BATCHES = {}


def molecule(V, rng, special):
    """adjacency: a random tree plus a few extra bonds; special (V >= 4): vertex V - 1 has no neighbour, V - 2 a single one, written on
    one side only, and vertex 0 is its own neighbour"""
    adj = np.zeros((V, V), dtype=np.int32)
    body = V - 2 if special and V >= 4 else V
    for v in range(1, body):
        u = int(rng.integers(0, v))
        adj[u, v] = adj[v, u] = 1
    for _ in range(body // 3):
        a, b = (int(t) for t in rng.integers(0, body, 2))
        if a != b:
            adj[a, b] = adj[b, a] = 1
    if special and V >= 4:
        adj[V - 3, V - 2] = 1   # (column V - 2: N(V - 2) = {V - 3}; row V - 2 is empty, so V - 3 does not list it)
        adj[0, 0] = 1
    return adj


def build(form, sizes, M, L, seed, special=True):
    """the packed operands and the fp64 reference of a batch, drawn until no in-mask pre-activation lies at the kink (the module docstring)"""
    key = (form, tuple(sizes), M, L, seed, special)
    if key in _BATCHES:
        return _BATCHES[key]
    for attempt in range(50):
        rng = np.random.default_rng(1000 * seed + attempt)
        adjs = [molecule(V, rng, special) for V in sizes]
        Ns = [cref.neighbours(a) for a in adjs]
        sps = [hop_distances(a) for a in adjs]
        mks = [cref.masks(a, L, M, sp) for a, sp in zip(adjs, sps)]
        s0s = [rng.integers(16, 65, V) / 64.0 for V in sizes]
        tg = rng.integers(-64, 65, len(sizes)) / 32.0
        Fs = []
        for l in range(1, L + 1):
            F = (rng.integers(16, 65, (M, M)) / 64.0) * np.where(rng.random((M, M)) < 0.15, -1.0, 1.0)
            top = max(np.abs(cref.network(form, N, mk[:l + 1], s0, Fs + [F], 0.0, M)["h"][l]).max(initial=0.0) for N, mk, s0 in zip(Ns, mks, s0s))
            Fs.append(F * 2.0 ** (-np.floor(np.log2(top)) - 1) if top > 0 else F)
        ref = [cref.network(form, N, mk, s0, Fs, t, M) for N, mk, s0, t in zip(Ns, mks, s0s, tg)]
        gap = np.inf
        for r, mk in zip(ref, mks):
            for l in range(1, L + 1):
                z = r["n"][l - 1] @ Fs[l - 1].T
                inm = (mk[l] > 0) & (np.abs(r["n"][l - 1]).max(axis=1, keepdims=True) > 0)
                if inm.any():
                    gap = min(gap, (np.abs(z[inm]) / (np.abs(r["n"][l - 1]) @ np.abs(Fs[l - 1]).T)[inm]).min())
        if gap >= 1e-4:
            break
    else:
        raise AssertionError("no batch without a pre-activation at the kink in 50 draws")
    nV = int(sum(sizes))
    mp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    lists, tlists, hop = [], [], np.full((max(nV, 1), M), 255, dtype=np.uint8)
    for m, (N, sp) in enumerate(zip(Ns, sps)):
        V, v0 = sizes[m], int(mp[m])
        lists += [[v0 + u for u in N[v]] for v in range(V)]
        tlists += [[v0 + v for v in range(V) if u in N[v]] for u in range(V)]
        hop[v0:v0 + V, :V] = np.minimum(sp.T, 255)
    out = {"sizes": list(sizes), "M": M, "L": L, "form": form, "nV": nV, "mol_ptr": mp, "hop": hop,
           "ptr": np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64),
           "idx": np.array([u for x in lists for u in x] + [0], dtype=np.int32),
           "tptr": np.concatenate([[0], np.cumsum([len(x) for x in tlists])]).astype(np.int64),
           "tidx": np.array([u for x in tlists for u in x] + [0], dtype=np.int32),
           "s0": np.concatenate(s0s), "F": np.array(Fs).reshape(L, M, M), "target": tg, "ref": ref, "lists": Ns}
    _BATCHES[key] = out
    return out


def call(b, want_loss=True):
    """both operators once: (status fwd, status bwd, h, n, g, yhat, loss, dy, dF, ds0) as numpy"""
    L, M, nV, nMol = b["L"], b["M"], b["nV"], len(b["sizes"])
    ctx = context()
    d = {k: dev(b[k], t) for k, t in (("mol_ptr", np.int32), ("ptr", np.int64), ("idx", np.int32), ("tptr", np.int64), ("tidx", np.int32),
                                      ("hop", np.uint8), ("s0", np.float32), ("F", np.float32), ("target", np.float32))}
    h, n, g = guarded((L + 1) * nV, M), guarded(L * nV, M), guarded(nMol, M)
    yhat, loss, dy = guarded(nMol, 1), guarded(nMol, 1), guarded(nMol, 1)
    dF, ds0 = guarded(L * M, M, fill=np.zeros((L * M, M))), guarded(nV, 1)
    st = ctx.lib.gf_smp_covariant_forward_ex_f32(ctx.handle, b["form"], L, M, nV, nMol, ptr(d["mol_ptr"]), ptr(d["ptr"]), ptr(d["idx"]), ptr(d["hop"]),
                                                 ptr(d["s0"]), ptr(d["F"]), ptr(d["target"]), ptr(h), ptr(n), ptr(g), ptr(yhat),
                                                 ptr(loss) if want_loss else None, ptr(dy))
    torch.cuda.synchronize()
    assert st == 0, ctx.lib.gf_last_error(ctx.handle)
    st2 = ctx.lib.gf_smp_covariant_backward_ex_f32(ctx.handle, b["form"], L, M, nV, nMol, ptr(d["mol_ptr"]), ptr(d["ptr"]), ptr(d["idx"]),
                                                   ptr(d["tptr"]), ptr(d["tidx"]), ptr(d["hop"]), ptr(d["F"]), ptr(h), ptr(n), ptr(dy), ptr(dF), ptr(ds0))
    torch.cuda.synchronize()
    assert st2 == 0, ctx.lib.gf_last_error(ctx.handle)
    return [taken(h, (L + 1) * nV, M), taken(n, L * nV, M) if L else np.zeros((0, M)), taken(g, nMol, M), taken(yhat, nMol, 1),
            taken(loss, nMol, 1, written=want_loss), taken(dy, nMol, 1), taken(dF, L * M, M, prefilled=True) if L else np.zeros((0, M)),
            taken(ds0, nV, 1)]


def check(form, sizes, M, L, seed, special=True):
    b = build(form, sizes, M, L, seed, special)
    nV, ref, mp = b["nV"], b["ref"], b["mol_ptr"]
    h, n, g, yhat, loss, dy, dF, ds0 = call(b)
    h, n, g = h.reshape(L + 1, nV, M), n.reshape(L, nV, M), g.reshape(len(sizes), M)   # (a width of 1 comes back flat)
    worst = {}

    def hold(name, x, r):
        worst[name] = max(worst.get(name, 0.0), rel_err(x, r))

    for m, r in enumerate(ref):
        v0, v1 = int(mp[m]), int(mp[m + 1])
        for l in range(L + 1):
            hold("h_%d" % l, h[l, v0:v1], r["h"][l])
        for l in range(L):
            hold("n_%d" % (l + 1), n[l, v0:v1], r["n"][l])
        hold("g", g[m], r["feature"])
        hold("ds0", ds0[v0:v1], r["ds0"])
    hold("yhat", yhat, [r["predict"] for r in ref])
    hold("loss", loss, [r["loss"] for r in ref])
    hold("dy", dy, [r["dy"] for r in ref])
    for l in range(L):
        hold("dF_%d" % (l + 1), dF.reshape(L, M, M)[l], sum(r["dF"][l] for r in ref))
    print(form, sizes if len(sizes) < 8 else len(sizes), M, L, worst)
    assert all(e <= TOL for e in worst.values()), worst
    same_bits([x for x in (h, n, g, yhat, loss, dy, dF, ds0)], [y.reshape(x.shape) for x, y in zip((h, n, g, yhat, loss, dy, dF, ds0), call(b))])
    return b, (h, n, g, yhat, loss, dy, dF, ds0)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("V,M", [(1, 1), (1, 64), (2, 2), (2, 64), (31, 31), (31, 64), (32, 32), (32, 64), (33, 33), (33, 64), (64, 64)])
def test_at_the_vertex_counts(gf, form, V, M):
    """three molecules of V vertices at L = 4: around the half-wave (32) and the wave (64), the vector as long as the molecule and longer"""
    b, out = check(form, [V, V, V], M, 4, 10 * V + M + form)
    if V >= 4:   # the special vertices are there, and do what they are there for
        N = b["lists"][0]
        assert N[V - 1] == [] and N[V - 2] == [V - 3] and 0 in N[0] and V - 2 not in N[V - 3]
        n1 = out[1].reshape(4, b["nV"], M)[0]
        assert not n1[V - 1].any() and (form == 1) == bool(n1[V - 2].any())
        assert np.abs(out[6]).max() > 0 and np.abs(out[7]).max() > 0


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("L", [0, 1])
def test_at_the_level_counts(gf, form, L):
    """no level (the graph feature is the level-0 scalars, ds0 = dy) and one"""
    b, out = check(form, [5, 33, 2], 64, L, 77 + L)
    if L == 0:
        assert rel_err(out[7], np.repeat(out[5], b["sizes"])) == 0


@pytest.mark.parametrize("form", [1, 2])
def test_batch_mixing_the_extremes(gf, form):
    """V = 1 and V = M = 64 in one launch (the dynamic LDS is sized for the largest), and an empty molecule between them"""
    check(form, [1, 64, 1, 0, 29, 64, 1], 64, 2, 5)


@pytest.mark.parametrize("form", [1, 2])
def test_gradient_partition_with_a_ragged_last_chunk(gf, form):
    """300 molecules of at most 6 vertices: 150 chunks of two molecules (256 chunks at most, ceil(300 / 256) = 2 per chunk); then 257
    molecules: 129 chunks, the last with one molecule"""
    rng = np.random.default_rng(3)
    check(form, [int(v) for v in rng.integers(1, 7, 300)], 6, 2, 31, special=False)
    check(form, [int(v) for v in rng.integers(1, 7, 257)], 7, 1, 32, special=False)


def test_refusals_leave_the_context_usable(gf):
    """GF_ERR_INVALID with its message before anything is launched; the next call on the same context works"""
    ctx = context()
    b = build(2, [3, 4], 5, 1, 9, special=False)

    def forward(**over):
        c = dict(b, **over)
        d = {k: dev(c[k], t) for k, t in (("mol_ptr", np.int32), ("ptr", np.int64), ("idx", np.int32), ("hop", np.uint8), ("s0", np.float32),
                                          ("F", np.float32))}
        nV, nMol, M, L = c["nV"], len(c["sizes"]), c["M"], c["L"]
        outs = [guarded((L + 1) * max(nV, 1), M), guarded(max(L * nV, 1), M), guarded(nMol, M), guarded(nMol, 1)]
        st = ctx.lib.gf_smp_covariant_forward_ex_f32(ctx.handle, c["form"], L, M, nV, nMol, ptr(d["mol_ptr"]), ptr(d["ptr"]), ptr(d["idx"]),
                                                     ptr(d["hop"]), ptr(d["s0"]), ptr(d["F"]), None, *[ptr(t) for t in outs], None, None)
        torch.cuda.synchronize()
        return st, ctx.lib.gf_last_error(ctx.handle)

    assert forward()[0] == 0
    for over, text in (({"form": 3}, b"form = 3"), ({"L": 65}, b"65 levels"), ({"M": 76}, b"M = 76"), ({"M": 3}, b"molecule 1 has 4 vertices, M = 3"),
                       ({"mol_ptr": np.array([0, 4, 3], dtype=np.int32)}, b"mol_ptr decreases"),
                       ({"mol_ptr": np.array([0, 3, 6], dtype=np.int32)}, b"mol_ptr ends at 6"),
                       ({"idx": np.where(np.arange(b["idx"].size) == 0, 5, b["idx"]).astype(np.int32)}, b"outside its molecule 0"),
                       ({"ptr": b["ptr"][::-1].copy()}, b"starts at")):
        st, msg = forward(**over)
        assert st == INVALID and text in msg, (over, msg)
        assert forward()[0] == 0
