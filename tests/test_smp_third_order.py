"""CPU suite for GCN_3D and GRU_GCN_3D (gf_smp_config.neighbourhood = 6, 7): tests/third_order_ref.py, the fp64 restatement the GPU suites
lean on, against the real classes' numbers (tests/golden/smp_third_order.npz, written by tests/golden/make_third_order_golden.py) and
against the literal loops of RisiLayer3D / KMax; what the library answers without a device (parameter counts, refusals, initial weights,
the agreement of the resolver with the block enumeration); and the gap condition on every input the GPU suites use
(tests/test_smp_third_order_ops_gpu.py, tests/test_smp_third_order_gpu.py), whose inputs are built here, once per process.

The gap condition (third_order_ref.GAP): at every (vertex, level) with three members or more, the classes that hold the top H entries and
the first class below are pairwise-adjacently at least 1e-5 max|T| apart in fp64 -- ten times the fp32 evaluation error of the closed
form -- so that fp32 and fp64 select the same classes.  Inputs that fail are drawn again; nothing is excused afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

import third_order_ref as tref
from field_suite import TOL, blockwise, load_golden
from inputs import synthetic_molecule, toy_molecules
from util import rel_err

FORMS = {6: "gcn_3d", 7: "gru_gcn_3d"}
WIDTHS = (1, 5, 8, 9, 16, 17, 32, 33, 64)
OPS_WIDTHS = (1, 2, 5, 8, 9, 16, 17, 32, 33, 64)
OPS_KINDS = ("softmax", "tanh")
INVALID, UNSUPPORTED = 1, 4   # gf_status (include/gf_hip.h)


def golden():
    return load_golden("smp_third_order.npz")


def case(gz, tag):
    form, L, H, D, R, V = (int(x) for x in gz[tag + "__cfg"])
    return form, L, H, D, R, gz[tag + "__adj"], gz[tag + "__feature"], gz[tag + "__result"], gz[tag + "__params"].astype(np.float64)


# ---- the inputs of the GPU suites ----
def random_params(form, H, FD, L, rng, scale):
    """float32-exact parameters in registration order: multiples of 1/64 in [-1, 1] times `scale`"""
    p = np.concatenate([rng.integers(-64, 65, n) / 64.0 * scale for _, n in tref.blocks(form, H, FD, L)])
    return p.astype(np.float32).astype(np.float64)


def small_batch():
    """a one-vertex molecule first and last, the four toy molecules (four feature columns) and a nine-vertex one between them: 32 vertices"""
    one = (np.zeros((1, 1), dtype=np.int32), np.array([[0.5, 0.0, 1.0, 0.25]]))
    adj9, x9, _ = synthetic_molecule(3, 9)
    mols = [one] + [(a, f) for _, a, f, _ in toy_molecules()] + [(adj9, x9[:, :4] + 0.5 * x9[:, 4:5])] + [(one[0], one[1][:, ::-1].copy())]
    return mols, np.array([0.5, 5.0, 4.0, 3.0, 6.0, 9.0, -1.0])


@functools.lru_cache(maxsize=None)
def model_case(form, H, L, R, D=1):
    """(mols, targets, params, per-molecule fp64 results, summed gradient, smallest gap) of the small batch: the parameters are drawn until
    every vertex-level satisfies the gap condition; the scale is halved until a numpy float32 evaluation of the restatement, selection
    included, meets the fp64 one within half the tolerance, block by block.  Decided on the CPU, before any device runs."""
    mols, tg = small_batch()
    FD = 4 * (D + 1)
    rng, scale = np.random.default_rng(1000 * form + 100 * H + 10 * L + R), 0.5
    for _ in range(400):
        params = random_params(form, H, FD, L, rng, scale)
        res, rg = tref.run_batch(form, mols, tg, params, L, H, D, R)
        gap = min(r["gap"] for r in res)
        if gap < tref.GAP:
            continue
        rg32 = tref.run_batch(form, mols, tg, params, L, H, D, R, dtype=np.float32)[1]
        if blockwise(rg32.astype(np.float64), rg, tref.blocks(form, H, FD, L))[0] <= 0.5 * TOL:
            return mols, tg, params, res, rg, gap
        scale *= 0.5
    raise AssertionError(("no admissible draw", form, H, L, R))


MODEL_CASES = [(form, H, L, R) for form in (6, 7) for H in WIDTHS for L in (0, 1, 3) for R in (0, 5)]
OTHER_MODEL_CASES = [(6, 33, 3, 2), (7, 17, 3, 2), (6, 9, 3, 2), (7, 64, 3, 2)]   # accumulate; two runs


class OpsCase:
    pass


@functools.lru_cache(maxsize=None)
def ops_case(H, kind):
    """One batch of 40 vertices for the two operators: list lengths 1, 2, 3, 4, 7, 29 mixed, members drawn without the vertex itself unless
    chance has it (vertex 2 holds itself, vertex 3 does not), vertex 39 in nobody's list (a source without a consumer), vertex 5 with the
    three members 10, 11, 12 whose vectors are equal; softmax-valued or tanh-valued members, float32-exact.  Drawn again until every list
    of three or more satisfies the gap condition.  The fp64 reference per vertex: n, sel, dhprev."""
    nV, lengths = 40, (1, 2, 3, 4, 7, 29)
    rng = np.random.default_rng(17 * H + len(kind))
    for _ in range(400):
        z = rng.normal(size=(nV, H))
        h = tref.softmax(2.0 * z) if kind == "softmax" else np.tanh(z)
        h[11] = h[12] = h[10]
        h = h.astype(np.float32).astype(np.float64)
        lists = []
        for v in range(nV):
            m = lengths[(v + v // 6) % 6]
            lists.append(sorted(int(u) for u in rng.choice(nV - 1, size=m, replace=False)))
        if 2 not in lists[2]:
            lists[2] = sorted(lists[2][:-1] + [2])
        if 3 in lists[3]:
            lists[3] = sorted([u for u in lists[3] if u != 3] + [min(u for u in range(4, nV - 1) if u not in lists[3])])
        lists[5] = [10, 11, 12]
        pooled = [tref.pool(h[mem]) for mem in lists]
        gap = min(g for _, _, g in pooled)
        if gap >= tref.GAP:
            break
    else:
        raise AssertionError(("no admissible draw", H, kind))
    c = OpsCase()
    c.H, c.nV, c.kind, c.lists, c.gap, c.hprev = H, nV, kind, lists, gap, h
    c.ptr = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int64)
    c.idx = np.concatenate(lists).astype(np.int32)
    consumers = [[v for v in range(nV) if w in lists[v]] for w in range(nV)]
    c.tptr = np.concatenate([[0], np.cumsum([len(m) for m in consumers])]).astype(np.int64)
    c.tidx = np.array([v for m in consumers for v in m], dtype=np.int32)
    c.consumers = consumers
    c.n = np.stack([p[0] for p in pooled])
    c.sel = np.stack([p[1] for p in pooled])   # [nV, H, 3], -1 under three members
    c.dn = (rng.integers(-64, 65, (nV, H)) / 64.0).astype(np.float64)
    c.dh = np.zeros((nV, H))
    for v, mem in enumerate(lists):
        if len(mem) >= 3:
            c.dh[mem] += tref.pool_backward(h[mem], c.sel[v], c.dn[v])
    return c


# ---- the restatement ----
def test_golden_holds_the_cases_the_issue_lists():
    gz = golden()
    tags = list(gz["tags"])
    cfgs = np.array([gz[t + "__cfg"] for t in tags])
    for form in (6, 7):
        mine = cfgs[cfgs[:, 0] == form]
        assert len(mine) == 16
        assert set(mine[:, 1]) == {0, 1, 3} and set(mine[:, 4]) == {0, 1, 2, 5} and set(mine[:, 3]) == {0, 2}
        assert {1, 9, 12, 29} <= set(mine[:, 5])
        assert all(H <= 16 for H, V in zip(mine[:, 2], mine[:, 5]) if V == 29) and all(V <= 9 for H, V in zip(mine[:, 2], mine[:, 5]) if H == 64)
        for name in ("CH4", "NH3", "H2O", "C2H4", "single", "isolated", "disconnected", "cycle6", "star8_r0", "star8_far", "syn9", "syn12", "syn29"):
            assert "n%d_%s" % (form, name) in tags
    assert set(cfgs[:, 2]) == set(WIDTHS)
    for k in gz:   # every input is float32-representable
        if k.endswith(("__feature", "__params")) and k.split("__")[0] in tags:
            assert np.array_equal(gz[k], gz[k].astype(np.float32).astype(gz[k].dtype)), k
    assert sum(1 for t in tags if t + "__activations" in gz) >= 20


@pytest.mark.parametrize("form", [6, 7])
def test_restatement_meets_the_real_classes(form):
    """every golden case at 1e-9: the neighbourhoods, graph feature, prediction, loss, each parameter block, the recorded h_l[v]; and every
    case satisfies the gap condition"""
    gz = golden()
    smallest = np.inf
    for tag in [t for t in gz["tags"] if t.startswith("n%d_" % form)]:
        form, L, H, D, R, adj, feat, result, params = case(gz, tag)
        r = tref.run(form, adj, feat, result[2], params, L, H, D, R)
        assert np.array_equal(tref.lists_flat(r["N"], L), gz[tag + "__lists"]), tag
        blocks = tref.blocks(form, H, feat.shape[1] * (D + 1), L)
        assert len(blocks) == (2 * L + 2 if form == 6 else 10)
        e = blockwise(r["grads"], gz[tag + "__grads"], blocks)
        assert rel_err(r["graph_feature"], gz[tag + "__graph_feature"]) <= 1e-9, tag
        assert rel_err([r["predict"], r["loss"]], result[:2]) <= 1e-9, tag
        assert e[0] <= 1e-9, (tag, e)
        assert np.abs(gz[tag + "__grads"]).max() > 0
        if tag + "__activations" in gz:
            assert rel_err(tref.activations(r), gz[tag + "__activations"]) <= 1e-9, tag
        assert r["gap"] >= tref.GAP, (tag, r["gap"])
        smallest = min(smallest, r["gap"])
    print("form %d: smallest gap over the golden cases %.3g of max|T|" % (form, smallest))


def test_class_form_equals_the_literal_loops():
    """RisiLayer3D's loops, a sort of all H^3 entries by (value, index) and the literal backward against the class-based closed form: pooled
    values and member gradients at 1e-12, softmax-valued and signed members, H = 2 and 5 among them (the cut falls inside a class)"""
    rng = np.random.default_rng(3)
    cut_inside = 0
    for H, m in ((2, 3), (2, 5), (3, 4), (4, 3), (5, 3), (5, 4), (6, 4)):
        for kind in OPS_KINDS:
            z = rng.normal(size=(m, H))
            a = tref.softmax(z) if kind == "softmax" else np.tanh(z)
            n, sel, gap = tref.pool(a)
            n_loops, kept = tref.kmax_loops(a)
            dn = rng.normal(size=H)
            assert rel_err(n, n_loops) <= 1e-12 and np.all(np.diff(n) >= 0), (H, m, kind)
            assert rel_err(tref.pool_backward(a, sel, dn), tref.kmax_loops_backward(a, kept, dn)) <= 1e-12, (H, m, kind)
            triples = sorted(tuple(sorted((f % H, (f // H) % H, f // (H * H)))) for f in kept)
            if gap >= tref.GAP:   # (the same classes, each as often)
                assert triples == sorted(tuple(int(x) for x in t) for t in sel), (H, m, kind)
            X, Y, Z, mult, _ = tref.classes(H)
            count = {t: triples.count(t) for t in set(triples)}
            cut_inside += any(count[t] < mult[(X == t[0]) & (Y == t[1]) & (Z == t[2])][0] for t in count)
    assert cut_inside >= 3


def test_fewer_than_three_members_give_exact_zeros():
    gz = golden()
    for form in (6, 7):
        form, L, H, D, R, adj, feat, result, params = case(gz, "n%d_star8_r0" % form)
        r = tref.run(form, adj, feat, result[2], params, L, H, D, R)
        assert all(not n.any() for n in r["n"][1:]) and r["gap"] == np.inf
        assert all((s == -1).all() for lv in r["sel"][1:] for s in lv)
    n, sel, gap = tref.pool(np.ones((2, 4)))
    assert not n.any() and (sel == -1).all() and not tref.pool_backward(np.ones((2, 4)), sel, np.ones(4)).any()


def test_neighbourhoods_read_max_radius_in_both_forms():
    gz = golden()
    for form in (6, 7):
        star = gz["n%d_star8_far__adj" % form]
        assert tref.hop_distances(star).max() == 2 and int(gz["n%d_star8_far__cfg" % form][4]) == 5
        N = tref.neighbourhoods(gz["n%d_disconnected__adj" % form], 3, 5)
        assert N[3][0] == [0, 1, 2] and N[3][4] == [3, 4, 5]
        N = tref.neighbourhoods(gz["n%d_cycle6__adj" % form], 3, 2)
        assert len(N[3][0]) == 5 and len(N[1][0]) == 3   # min(l, max_Radius), unlike GCN_2D


@pytest.mark.parametrize("form", [6, 7])
def test_momentum_trajectory_of_the_restatement(form):
    """three BatchLearn steps of the real class: the restatement follows them at 1e-9 (losses) and 1e-12 (weights), and every step satisfies
    the gap condition"""
    gz = golden()
    p_ = "train_n%d__" % form
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in gz[p_ + "cfg"])
    mols = [(a, f) for _, a, f, _ in toy_molecules()]
    losses, p, gap = tref.momentum_steps(form, mols, gz[p_ + "targets"], gz[p_ + "params0"], L, H, D, R, nIter, float(gz[p_ + "lr"][0]),
                                         float(gz[p_ + "momentum"][0]))
    assert rel_err(losses, gz[p_ + "losses"]) <= 1e-9
    assert np.abs(p - gz[p_ + "params"]).max() <= 1e-12
    assert (gz[p_ + "losses"][:, 1] <= gz[p_ + "losses"][:, 0]).all()
    assert gap >= tref.GAP, gap


def test_checkpoint_is_the_parameters_in_registration_order():
    gz = golden()
    text = bytes(gz["checkpoint__text"]).decode().split()
    params = gz[str(gz["checkpoint__tag"]) + "__params"]
    assert text == ["%g" % x for x in params]


# ---- the gap condition on the inputs of the GPU suites ----
@pytest.mark.parametrize("H", OPS_WIDTHS)
def test_operator_inputs_satisfy_the_gap_condition(H):
    for kind in OPS_KINDS:
        c = ops_case(H, kind)
        lens = {len(m) for m in c.lists}
        assert lens == {1, 2, 3, 4, 7, 29} and c.nV == 40
        assert c.gap >= tref.GAP, (H, kind, c.gap)
        assert 2 in c.lists[2] and 3 not in c.lists[3] and not c.consumers[39] and c.lists[5] == [10, 11, 12]
        assert np.array_equal(c.hprev[10], c.hprev[11]) and np.array_equal(c.hprev[10], c.hprev[12])
        assert np.array_equal(c.hprev, c.hprev.astype(np.float32).astype(np.float64))
        assert (c.sel[[len(m) < 3 for m in c.lists]] == -1).all() and (c.sel[[len(m) >= 3 for m in c.lists]] >= 0).all()
        assert (kind == "tanh") == bool((c.hprev < 0).any())
    if H in (2, 5):   # the cut falls inside a class of 3 or 6 at some vertex
        X, Y, Z, mult, _ = tref.classes(H)
        inside = 0
        for kind in OPS_KINDS:
            c = ops_case(H, kind)
            for v in range(c.nV):
                t = [tuple(s) for s in c.sel[v] if s[0] >= 0]
                inside += any(t.count(k) < mult[(X == k[0]) & (Y == k[1]) & (Z == k[2])][0] for k in set(t))
        assert inside > 0


@pytest.mark.parametrize("form,H", [(f, H) for f in (6, 7) for H in WIDTHS])
def test_model_inputs_satisfy_the_gap_condition(form, H):
    smallest = np.inf
    for f, h, L, R in MODEL_CASES + OTHER_MODEL_CASES:
        if (f, h) == (form, H):
            mols, tg, params, res, rg, gap = model_case(f, h, L, R)
            assert gap >= tref.GAP and all(r["gap"] >= tref.GAP for r in res), (f, h, L, R, gap)
            assert np.array_equal(params, params.astype(np.float32).astype(np.float64)) and np.abs(rg).max() > 0
            if R == 0:
                assert gap == np.inf and all(not r["n"][l].any() for r in res for l in range(1, L + 1))
            smallest = min(smallest, gap)
    print("form %d, H = %d: smallest gap %.3g" % (form, H, smallest))


# ---- the library without a device ----
def config(form, L, H, F, D, maxV, R=1, **over):
    from graphflow_amd.smp import SMPGatedNeighbourhood, SMPNeighbourhood
    cfg = (SMPNeighbourhood if form == 6 else SMPGatedNeighbourhood).config(FORMS[form], L, H, F, D, maxV, R)
    assert cfg.neighbourhood == form
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def refused_configs(form):
    """the configurations gf_smp_create answers GF_ERR_INVALID to, with a piece of the message"""
    needs = b"gf_smp_create: neighbourhood = %d (6: GCN_3D, 7: GRU_GCN_3D) needs" % form
    bad = [(config(form, 2, 8, 5, 1, 9, **{k: 1}), needs) for k in ("first_order", "steerable_2d", "unrestricted", "physics", "custom_matmul")]
    bad.append((config(form, 2, 8, 5, 1, 9, nContractions=18), needs))
    bad.append((config(form, 2, 8, 5, 1, 9, max_receptive_field=6), needs))
    bad.append((config(form, 2, 8, 5, 1, 9, R=-1), needs))   # (GCN_3D reads max_Radius, unlike GCN_2D)
    bad.append((config(form, 2, 65, 5, 1, 9), b"at most 64 channels"))
    bad.append((config(form, 2, 128, 5, 1, 9), b"packs a triple of channels into 18 bits"))
    bad.append((config(form, 2, 64, 5, 1, 475), b"at most 474 vertices"))
    bad.append((config(form, 2, 32, 5, 1, 1200), b"stages a neighbourhood's members in LDS"))
    return bad


def test_parameter_counts(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    for form in (6, 7):
        for L, H, F, D in ((0, 5, 4, 0), (1, 6, 4, 0), (3, 20, 5, 0), (3, 64, 5, 0), (3, 20, 5, 2), (0, 6, 4, 2), (7, 1, 1, 0)):
            cfg = config(form, L, H, F, D, 12, 2)
            FD = F * (D + 1)
            expect = H * FD + L * (H * FD + H * H) + H if form == 6 else H * FD + 8 * H * H + H
            assert lib.gf_smp_config_param_count(C.byref(cfg)) == tref.n_params(form, H, FD, L) == expect, (form, L, H)
            assert lib.gf_smp_classifier_config_param_count(C.byref(cfg), 3) == 0
        assert lib.gf_smp_config_param_count(C.byref(config(form, 2, 8, 5, 1, 9, R=0))) > 0
        assert lib.gf_smp_config_param_count(C.byref(config(form, 2, 64, 5, 1, 474))) > 0
        for bad, _ in refused_configs(form):
            assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
            assert lib.gf_smp_classifier_config_param_count(C.byref(bad), 3) == 0


def test_python_forms_and_their_refusal():
    from graphflow_amd.smp import SMPGatedNeighbourhood, SMPNeighbourhood
    assert SMPNeighbourhood.FORMS["gcn_3d"] == 6 and SMPGatedNeighbourhood.FORMS["gru_gcn_3d"] == 7
    with pytest.raises(ValueError, match="GCN_3D"):
        SMPNeighbourhood.config("gru_gcn_3d", 1, 4, 4, 0, 6)
    with pytest.raises(ValueError, match="GRU_GCN_3D"):
        SMPGatedNeighbourhood.config("gcn_3d", 1, 4, 4, 0, 6)
    assert "GCN_3D" in SMPNeighbourhood.__doc__ and "GRU_GCN_3D" in SMPGatedNeighbourhood.__doc__


def test_uniform_init_draws_the_classes_weights(gf):
    """after srand(seed): GCN_3D draws W1_l / W2_l as Matrices (divisor 10 H) and W as a Vector, GRU_GCN_3D every block as a Vector (10 x
    its own size), in registration order -- the recorded weights of the real classes bit for bit"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    for form in (6, 7):
        p_ = "train_n%d__" % form
        _, L, H, D, R, maxV, seed, _ = (int(x) for x in gz[p_ + "cfg"])
        cfg = config(form, L, H, 4, D, maxV, R)
        out = np.zeros(tref.n_params(form, H, 4 * (D + 1), L), dtype=np.float32)
        C.CDLL(None).srand(seed)
        assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
        assert np.array_equal(out, gz[p_ + "params0"].astype(np.float32))
        assert np.abs(out).max() > 0
        second = gz[p_ + "params0"][4 * (D + 1) * H:][:H * H]   # form 6: W1_1's first rows (10 H); form 7: W_z (10 H^2)
        assert np.abs(second).max() <= 0.9 / (H if form == 6 else H * H) * (1 + 1e-12)


# ---- the resolver and the enumeration for the new forms, as tests/test_smp_config_agreement.py does it for the others ----
ACCEPTED = [("gcn_3d", 6, dict(L=2, R=1)), ("gru_gcn_3d", 7, dict(L=2, R=1)), ("gcn_3d_no_levels", 6, dict(L=0, R=1)),
            ("gru_gcn_3d_no_levels", 7, dict(L=0, R=2)), ("gcn_3d_radius_0", 6, dict(L=3, R=0)), ("gru_gcn_3d_radius_0", 7, dict(L=3, R=0)),
            ("gcn_3d_64", 6, dict(L=1, R=5, H=64)), ("gru_gcn_3d_64", 7, dict(L=1, R=5, H=64))]


@pytest.mark.parametrize("name,form,kw", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_what_create_accepts_is_counted_as_the_restatement_lists_it(gf, name, form, kw):
    from graphflow_amd import _lib
    lib = _lib.load()
    H, L = kw.get("H", 4), kw["L"]
    c = config(form, L, H, 4, 1, 6, kw["R"])
    count = tref.n_params(form, H, 8, L)
    assert lib.gf_smp_config_param_count(C.byref(c)) == count
    out = np.full(count + 1, 7.0, dtype=np.float32)
    C.CDLL(None).srand(5)
    assert lib.gf_smp_uniform_init_host(C.byref(c), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
    assert out[count] == 7.0 and 0 < np.abs(out[:count]).max() < 1
    off = 0
    for bname, n in tref.blocks(form, H, 8, L):   # every draw is (rand() % 10) / (10 d): d = H for a Matrix of form 6, else the block's size
        d = H if form == 6 and bname != "W" else n
        assert np.abs(out[off:off + n]).max() <= 0.9 / d * (1 + 1e-6), bname
        off += n
    assert lib.gf_smp_classifier_config_param_count(C.byref(c), 3) == 0
    assert lib.gf_smp_classifier_uniform_init_host(C.byref(c), 3, out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID


@pytest.mark.parametrize("form", [6, 7])
def test_what_create_refuses_has_no_host_only_answer(gf, form):
    from graphflow_amd import _lib
    lib = _lib.load()
    out = np.full(1 << 16, 7.0, dtype=np.float32)
    p = out.ctypes.data_as(C.POINTER(C.c_float))
    for bad, _ in refused_configs(form):
        assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
        assert lib.gf_smp_uniform_init_host(C.byref(bad), p) == _lib.GF_ERR_INVALID
        assert lib.gf_smp_classifier_config_param_count(C.byref(bad), 3) == 0
        assert lib.gf_smp_classifier_uniform_init_host(C.byref(bad), 3, p) == _lib.GF_ERR_INVALID
        assert (out == 7.0).all()
