"""The two read-outs of gf_smp_config.readout, one by one on caller-supplied operands (smp_level_readouts.hip):
  gf_smp_gram_readout_ex_f32   gram_readout: G = h h^T, loss = 0.5 sum (G - adj)^2, dh = (E + E^T) h per molecule, against fp64 per molecule
  gf_smp_pair_readout_ex_f32   pair_readout, pair_readout_dW, pair_dh: the two segment sums, prediction, loss, dy, dW [2 H], dh_L
at the shapes where they can go wrong: one vertex, an asymmetric adjacency, V around the wave width, V at the LDS bound, widths below, at
and above 64 channels, a batch that mixes the extremes.  Tolerance: field_suite.TOL on every quantity; two runs give the same bits.
Every output lies in a buffer with sentinel rows behind its last row."""
import numpy as np
import pytest

from field_suite import TOL, dev
from test_smp_neighbourhood_ops_gpu import SENTINEL, context, guarded, ptr, same_bits, taken
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INVALID = 1


def exact(x, steps=256):
    """float32-exact values: multiples of 1 / steps"""
    return np.round(np.asarray(x) * steps) / steps


# ---- the Gram read-out ---------------------------------------------------------------------------------------------------------------
def gram_batch(sizes, H, seed):
    """(hL [nV, H], [adj]): signed entries scaled so that a row's squared norm is about 1.3, hence G on both sides of the adjacency values 0,
    1 and 2; every adjacency asymmetric where it has room, with an entry of 2"""
    rng = np.random.default_rng(seed)
    hL = exact(rng.uniform(-0.6, 1.0, (sum(sizes), H)) * np.sqrt(3.0 / H), 4096)
    adjs = []
    for V in sizes:
        a = (rng.random((V, V)) < 0.35).astype(np.float64)
        if V > 1:
            a[0, 1], a[1, 0] = 2.0, 0.0
        adjs.append(a)
    return hL, adjs


def gram_reference(hL, adjs):
    out, v0 = [], 0
    for a in adjs:
        V = len(a)
        h = hL[v0:v0 + V]
        G = h @ h.T
        E = G - a
        out.append((G, 0.5 * (E * E).sum(), (E + E.T) @ h))
        v0 += V
    return out


def gram_call(hL, adjs, H, want_dh=True, want_loss=True, mol_ptr=None, nV=None):
    sizes = [len(a) for a in adjs]
    mp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32) if mol_ptr is None else np.asarray(mol_ptr, dtype=np.int32)
    rows = int(sum(sizes)) if nV is None else nV
    flat = np.concatenate([a.ravel() for a in adjs])
    gram, loss, dh = guarded(flat.size, 1), guarded(len(adjs), 1), guarded(rows, H)
    ctx = context()
    d_h, d_mp, d_adj = dev(hL), dev(mp, np.int32), dev(flat)   # (named: an operand lives until the call has returned)
    st = ctx.lib.gf_smp_gram_readout_ex_f32(ctx.handle, H, rows, len(adjs), ptr(d_h), ptr(d_mp), ptr(d_adj), ptr(gram),
                                            ptr(loss) if want_loss else None, ptr(dh) if want_dh else None)
    torch.cuda.synchronize()
    return st, gram, loss, dh


def check_gram(sizes, H, seed):
    hL, adjs = gram_batch(sizes, H, seed)
    st, gram, loss, dh = gram_call(hL, adjs, H)
    assert st == 0, context().lib.gf_last_error(context().handle)
    nV, nG = sum(sizes), sum(V * V for V in sizes)
    g, lo, d = taken(gram, nG, 1), taken(loss, len(sizes), 1), taken(dh, nV, H)
    ref = gram_reference(hL, adjs)
    worst, v0, g0, above, below = {}, 0, 0, False, False
    for m, (G, l, dhr) in enumerate(ref):
        V = sizes[m]
        for k, e in (("G", rel_err(g[g0:g0 + V * V].reshape(V, V), G)), ("loss", rel_err(lo[m:m + 1], [l])), ("dh", rel_err(d[v0:v0 + V].reshape(V, H), dhr))):
            worst[k] = max(worst.get(k, 0.0), e)
        above, below = above or (G > adjs[m]).any(), below or (G < adjs[m]).any()
        v0, g0 = v0 + V, g0 + V * V
    print(sizes if len(sizes) < 8 else len(sizes), H, worst)
    assert above and (below or max(sizes) == 1)
    assert all(v <= TOL for v in worst.values()), worst
    again = gram_call(hL, adjs, H)
    same_bits([g, lo, d], [taken(again[1], nG, 1), taken(again[2], len(sizes), 1), taken(again[3], nV, H)])


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 199])
def test_gram_at_the_vertex_counts(gf, V):
    """one vertex, two (asymmetric), around a wave's 64 lanes, and the configuration's bound at H = 5 (199: 159,996 of 163,840 bytes)"""
    check_gram([V, V, V] if V < 199 else [V], 5, 100 + V)


@pytest.mark.parametrize("H", [1, 33, 65, 128])
def test_gram_at_the_widths(gf, H):
    """V = 7: the row stride H | 1 below, at and above a wave; 70 molecules, more than the device has workgroups in flight per CU"""
    check_gram([7] * 70, H, 200 + H)


def test_gram_batch_mixing_the_extremes(gf):
    """V = 1 and V = 65 in one launch (the dynamic LDS is sized for the largest), an empty molecule between them"""
    check_gram([1, 65, 1, 1, 65, 29, 9], 64, 7)
    hL, adjs = gram_batch([3, 65], 17, 8)
    st, gram, loss, dh = gram_call(hL, [adjs[0], np.zeros((0, 0)), adjs[1]], 17)
    assert st == 0
    ref = gram_reference(hL, adjs)
    lo = taken(loss, 3, 1)
    assert lo[1] == 0.0 and rel_err(lo[[0, 2]], [ref[0][1], ref[1][1]]) <= TOL
    assert rel_err(taken(dh, 68, 17), np.concatenate([ref[0][2], ref[1][2]])) <= TOL


def test_gram_optional_outputs_and_refusals(gf):
    """loss and dhL may be NULL (and are then not written); a bad list, a width outside 1 .. 128 and a molecule beyond the LDS bound are
    GF_ERR_INVALID before anything is launched, and the context stays usable"""
    hL, adjs = gram_batch([4, 6], 9, 3)
    st, gram, loss, dh = gram_call(hL, adjs, 9, want_dh=False, want_loss=False)
    assert st == 0
    taken(loss, 2, 1, written=False), taken(dh, 10, 9, written=False)
    ref = gram_reference(hL, adjs)
    assert rel_err(taken(gram, 52, 1), np.concatenate([r[0].ravel() for r in ref])) <= TOL
    lib, ctx = context().lib, context()
    for bad_ptr, text in (([1, 4, 10], b"starts at 1"), ([0, 6, 4], b"decreases"), ([0, 4, 11], b"beyond the 10 rows")):
        st, gram, loss, dh = gram_call(hL, adjs, 9, mol_ptr=bad_ptr)
        assert st == INVALID and text in lib.gf_last_error(ctx.handle), lib.gf_last_error(ctx.handle)
        assert np.all(gram.cpu().numpy() == SENTINEL) and np.all(dh.cpu().numpy() == SENTINEL)
        check_gram([2, 3], 4, 1)
    d_h, d_mp, d_adj, out = dev(hL), dev([0, 4, 10], np.int32), dev(np.zeros(52)), guarded(52, 1)
    for H in (0, 129):
        assert lib.gf_smp_gram_readout_ex_f32(ctx.handle, H, 10, 2, ptr(d_h), ptr(d_mp), ptr(d_adj), ptr(out), None, None) == INVALID
        assert b"channels (1 .. 128)" in lib.gf_last_error(ctx.handle)
    d_h, d_mp, d_adj, out = dev(np.zeros((200, 5))), dev([0, 200], np.int32), dev(np.zeros(40000)), guarded(40000, 1)
    st = lib.gf_smp_gram_readout_ex_f32(ctx.handle, 5, 200, 1, ptr(d_h), ptr(d_mp), ptr(d_adj), ptr(out), None, None)
    assert st == INVALID and b"molecule 0 has 200 vertices" in lib.gf_last_error(ctx.handle)
    check_gram([2, 3], 4, 1)


# ---- the pair read-out ---------------------------------------------------------------------------------------------------------------
def pair_call(hL, sizes, W, target, H, want_dh=True):
    """sizes = [V of X_0, Y_0, X_1, ..]"""
    nPairs, nV = len(sizes) // 2, int(sum(sizes))
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    g, yhat, loss, dy, dh = guarded(nPairs, 2 * H), guarded(nPairs, 1), guarded(nPairs, 1), guarded(nPairs, 1), guarded(nV, H)
    dW0 = exact(np.random.default_rng(5).uniform(-1, 1, 2 * H))
    dW = guarded(1, 2 * H, fill=dW0)   # (`+=`: onto what is there)
    ctx = context()
    d_h, d_gp, d_W, d_t = dev(hL), dev(gp, np.int32), dev(W), dev(target) if target is not None else None   # (named: alive until the call is over)
    st = ctx.lib.gf_smp_pair_readout_ex_f32(ctx.handle, H, nV, nPairs, ptr(d_h), ptr(d_gp), ptr(d_W), ptr(d_t), ptr(g), ptr(yhat), ptr(loss), ptr(dy),
                                            ptr(dW), ptr(dh) if want_dh else None)
    torch.cuda.synchronize()
    assert st == 0, ctx.lib.gf_last_error(ctx.handle)
    return [taken(g, nPairs, 2 * H), taken(yhat, nPairs, 1), taken(loss, nPairs, 1), taken(dy, nPairs, 1),
            taken(dW, 1, 2 * H, prefilled=True) - dW0, taken(dh, nV, H, written=want_dh)]


def check_pairs(sizes, H, seed):
    rng = np.random.default_rng(seed)
    nPairs, nV = len(sizes) // 2, int(sum(sizes))
    hL, W, target = exact(rng.uniform(0, 1, (nV, H)), 4096), exact(rng.uniform(-1, 1, 2 * H)), exact(rng.uniform(-2, 2, nPairs))
    out = pair_call(hL, sizes, W, target, H)
    gp = np.concatenate([[0], np.cumsum(sizes)])
    g = np.array([np.concatenate([hL[gp[2 * p]:gp[2 * p + 1]].sum(axis=0), hL[gp[2 * p + 1]:gp[2 * p + 2]].sum(axis=0)]) for p in range(nPairs)])
    yhat = g @ W
    dy = yhat - target
    dh = np.concatenate([np.tile(dy[k // 2] * W[(k % 2) * H:(k % 2 + 1) * H], (sizes[k], 1)) for k in range(2 * nPairs)])
    ref = [g, yhat, 0.5 * dy * dy, dy, (dy[:, None] * g).sum(axis=0)[None, :], dh]
    errs = [rel_err(np.asarray(x).reshape(np.shape(r)), r) for x, r in zip(out, ref)]
    print(nPairs, H, errs)
    assert max(errs) <= TOL, errs
    same_bits([np.ravel(x) for x in out], [np.ravel(x) for x in pair_call(hL, sizes, W, target, H)])
    return hL, W


@pytest.mark.parametrize("H", [1, 17, 65, 128])
def test_pair_readout_at_the_widths(gf, H):
    """33 pairs of unequal graphs (1 to 12 vertices, several of one vertex): more pairs than the 16 rows of the dW fold, both channel
    strides of a wave, dW [2 H] against fp64"""
    rng = np.random.default_rng(H)
    sizes = [int(v) for v in rng.integers(1, 13, 66)]
    sizes[1] = sizes[4] = sizes[65] = 1
    check_pairs(sizes, H, 300 + H)


def test_one_pair_with_a_one_vertex_graph(gf):
    hL, W = check_pairs([5, 1], 8, 11)
    out = pair_call(hL, [5, 1], W, None, 8, want_dh=False)   # no target: dy = predict; no dhL: not written
    assert np.array_equal(out[1], out[3]) and out[5] is None
    check_pairs([1, 1], 64, 12)


def test_pair_refusals_leave_the_context_usable(gf):
    ctx = context()
    lib = ctx.lib
    hL, W = dev(np.zeros((6, 4))), dev(np.zeros(8))
    bufs = [guarded(1, 8), guarded(1, 1), guarded(1, 1), guarded(1, 1), guarded(1, 8), guarded(6, 4)]
    for gp, text in (([1, 5, 6], b"starts at 1"), ([0, 5, 3], b"decreases"), ([0, 5, 7], b"beyond the 6 rows")):
        d_gp = dev(gp, np.int32)
        st = lib.gf_smp_pair_readout_ex_f32(ctx.handle, 4, 6, 1, ptr(hL), ptr(d_gp), ptr(W), None, *[ptr(b) for b in bufs])
        assert st == INVALID and text in lib.gf_last_error(ctx.handle)
        assert all(np.all(b.cpu().numpy() == SENTINEL) for b in bufs)
        check_pairs([2, 3], 4, 1)
    d_gp = dev([0, 5, 6], np.int32)
    for H, nP in ((0, 1), (129, 1), (4, 0)):
        assert lib.gf_smp_pair_readout_ex_f32(ctx.handle, H, 6, nP, ptr(hL), ptr(d_gp), ptr(W), None, *[ptr(b) for b in bufs]) == INVALID
    assert lib.gf_smp_pair_readout_ex_f32(ctx.handle, 4, 6, 1, ptr(hL), ptr(d_gp), None, None, *[ptr(b) for b in bufs]) == INVALID
    assert b"bad argument" in lib.gf_last_error(ctx.handle)
    check_pairs([2, 3], 4, 1)
