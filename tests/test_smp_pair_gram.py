"""CPU suite for GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel (gf_smp_config.readout = 1 with neighbourhood = 2, 3, 6) and GCA_1D (readout = 2
with neighbourhood = 2): tests/pair_gram_ref.py, the fp64 restatement the GPU suites lean on, against the real classes' numbers
(tests/golden/smp_pair_gram.npz, written by tests/golden/make_pair_gram_golden.py), and what the library answers without a device:
parameter counts, block layouts, refusals with a piece of their message, initial weights, and a zero tail that changes nothing."""
import ctypes as C

import numpy as np
import pytest

import neighbourhood_ref as nref
import pair_gram_ref as pref
from field_suite import blockwise, load_golden
from util import rel_err

FORMS = {2: "gcn_1d_kernel", 3: "gcn_2d_kernel", 6: "gcn_3d_kernel"}
PAIR_CASES = ("CH4_one", "same", "isolated", "cycle6_syn12_L0", "cycle6_syn12", "radius0")
GCA_CASES = ("one", "CH4", "isolated", "asymmetric", "entry2", "syn12_L0", "syn12")
INVALID, UNSUPPORTED = 1, 4   # gf_status (include/gf_hip.h)
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)


def golden():
    return load_golden("smp_pair_gram.npz")


def pair_case(gz, tag):
    """(form, L, H, D, R, M, X, Y, result, params), X and Y = (adj, feature)"""
    form, L, H, D, R, M = (int(x) for x in gz[tag + "__cfg"])
    return (form, L, H, D, R, M, (gz[tag + "__adj_x"], gz[tag + "__feature_x"]), (gz[tag + "__adj_y"], gz[tag + "__feature_y"]),
            gz[tag + "__result"], gz[tag + "__params"].astype(np.float64))


def gca_case(gz, tag):
    """(L, H, D, R, M, (adj, feature), loss, params)"""
    _, L, H, D, R, M = (int(x) for x in gz[tag + "__cfg"])
    return L, H, D, R, M, (gz[tag + "__adj"], gz[tag + "__feature"]), float(gz[tag + "__result"][0]), gz[tag + "__params"].astype(np.float64)


def pair_tags(gz, form):
    return [t for t in gz["tags"] if t.startswith("p%d_" % form)]


def gca_tags(gz):
    return [t for t in gz["tags"] if t.startswith("g_")]


def test_golden_holds_the_cases_of_every_class():
    gz = golden()
    for form in FORMS:
        want = ["p%d_%s" % (form, c) for c in PAIR_CASES] + (["p3_radius1_L3"] if form == 3 else [])
        assert pair_tags(gz, form) == want
        cfgs = np.array([gz[t + "__cfg"] for t in want])
        assert {0, 3} <= set(cfgs[:, 1]) and 0 in set(cfgs[:, 4])                       # L = 0 and 3, max_Radius = 0
        assert len(gz["p%d_CH4_one__adj_y" % form]) == 1                                # a one-vertex graph
        assert np.array_equal(gz["p%d_same__adj_x" % form], gz["p%d_same__adj_y" % form])
        assert (len(gz["p%d_cycle6_syn12__adj_x" % form]), len(gz["p%d_cycle6_syn12__adj_y" % form])) == (6, 12)
        assert not gz["p%d_isolated__adj_y" % form][3].any()                            # an isolated vertex on one side
        assert "p%d_CH4_one__activations_x" % form in gz and "p%d_CH4_one__activations_y" % form in gz
    assert tuple(gz["p3_radius1_L3__cfg"][[1, 4]]) == (3, 1)   # the case that tells min(l, max_Radius) from l
    assert gca_tags(gz) == ["g_" + c for c in GCA_CASES]
    cfgs = np.array([gz["g_%s__cfg" % c] for c in GCA_CASES])
    sizes = np.array([len(gz["g_%s__adj" % c]) for c in GCA_CASES])
    assert {0, 3} <= set(cfgs[:, 1]) and 1 in sizes and (sizes == cfgs[:, 5]).any() and (sizes < cfgs[:, 5]).any()
    a = gz["g_asymmetric__adj"]
    assert not np.array_equal(a, a.T) and (gz["g_entry2__adj"] == 2).any() and not gz["g_isolated__adj"][3].any()
    for k in gz:   # every input is float32-representable
        if k.endswith(("__feature", "__feature_x", "__feature_y", "__params")) and k.split("__")[0] in gz["tags"]:
            assert np.array_equal(gz[k], gz[k].astype(np.float32).astype(gz[k].dtype)), k


@pytest.mark.parametrize("form", list(FORMS))
def test_pair_restatement_meets_the_real_classes(form):
    """every golden pair at 1e-9: the neighbourhoods of both graphs, final feature, prediction, loss, every parameter block in registration
    order, and for the small case every h_l[v] of both graphs"""
    gz = golden()
    for tag in pair_tags(gz, form):
        _, L, H, D, R, M, gx, gy, result, params = pair_case(gz, tag)
        r = pref.run_pair(form, gx, gy, result[2], params, L, H, D, R)
        assert np.array_equal(pref.lists_flat(r["N"][0], L), gz[tag + "__lists_x"]), tag
        assert np.array_equal(pref.lists_flat(r["N"][1], L), gz[tag + "__lists_y"]), tag
        e = blockwise(r["grads"], gz[tag + "__grads"], pref.blocks(H, gx[1].shape[1] * (D + 1), L, 1))
        assert rel_err(r["final_feature"], gz[tag + "__final_feature"]) <= 1e-9, tag
        assert rel_err([r["predict"], r["loss"]], result[:2]) <= 1e-9, tag
        assert e[0] <= 1e-9, (tag, e)
        assert np.abs(gz[tag + "__grads"]).max() > 0
        if tag + "__activations_x" in gz:
            assert rel_err(pref.activations(r["h"][0]), gz[tag + "__activations_x"]) <= 1e-9, tag
            assert rel_err(pref.activations(r["h"][1]), gz[tag + "__activations_y"]) <= 1e-9, tag


def test_the_2d_pair_class_reads_max_radius():
    """GCN_2D_Kernel's lists at levels 2 and 3 stay at radius 1 where max_Radius = 1: not GCN_2D's N_l = {dist <= l}"""
    gz = golden()
    _, L, H, D, R, M, gx, gy, result, params = pair_case(gz, "p3_radius1_L3")
    plain = nref.neighbourhoods(3, gy[0], L, R)
    assert not np.array_equal(nref.lists_flat(plain, L), gz["p3_radius1_L3__lists_y"])
    assert np.array_equal(nref.lists_flat(nref.neighbourhoods(2, gy[0], L, R), L), gz["p3_radius1_L3__lists_y"])


def test_gca_restatement_meets_the_real_class():
    """every golden molecule at 1e-9: the lists, G, the loss (the adjacency by value, an asymmetric matrix as written), every block"""
    gz = golden()
    for tag in gca_tags(gz):
        L, H, D, R, M, (adj, feat), loss, params = gca_case(gz, tag)
        r = pref.run_gca(adj, feat, params, L, H, D, R)
        assert np.array_equal(pref.lists_flat(r["N"], L), gz[tag + "__lists"]), tag
        e = blockwise(r["grads"], gz[tag + "__grads"], pref.blocks(H, feat.shape[1] * (D + 1), L, 2))
        assert rel_err(r["gram"], gz[tag + "__gram"]) <= 1e-9 and rel_err([r["loss"]], [loss]) <= 1e-9, tag
        assert e[0] <= 1e-9, (tag, e)
        assert np.abs(gz[tag + "__grads"]).max() > 0
        if tag + "__activations" in gz:
            assert rel_err(pref.activations(r["h"]), gz[tag + "__activations"]) <= 1e-9, tag
    # an entry of 2 counts as 2: with it clipped to 1 the loss is another
    L, H, D, R, M, (adj, feat), loss, params = gca_case(gz, "g_entry2")
    hL = pref.run_gca(adj, feat, params, L, H, D, R)["h"][L]
    assert abs(0.5 * ((hL @ hL.T - np.minimum(adj, 1)) ** 2).sum() - loss) > 1e-3


def train_batch(gz, form):
    """the trajectory's batch: the four toy molecules, as pairs (toy p, toy p + 1) for a pair class"""
    from inputs import f32exact, toy_molecules
    mols = [(a, f32exact(f)) for _, a, f, _ in toy_molecules()]
    return [(mols[p], mols[(p + 1) % 4]) for p in range(4)] if form else mols


@pytest.mark.parametrize("form", [2, 3, 6, 0])
def test_momentum_trajectory_of_the_restatement(form):
    """three BatchLearn steps of the real class: the restatement follows them at 1e-9 (losses) and 1e-12 (weights)"""
    gz = golden()
    p_ = "train_%s__" % ("p%d" % form if form else "g")
    _, L, H, D, R, maxV, seed, nIter = (int(x) for x in gz[p_ + "cfg"])
    batch = train_batch(gz, form)
    grads = pref.pairs_batch_grads(form, batch, gz[p_ + "targets"], L, H, D, R) if form else pref.gca_batch_grads(batch, L, H, D, R)
    losses, p, _ = pref.momentum_steps(grads, gz[p_ + "params0"], nIter, float(gz[p_ + "lr"][0]), float(gz[p_ + "momentum"][0]), len(batch))
    assert rel_err(losses, gz[p_ + "losses"]) <= 1e-9
    assert np.abs(p - gz[p_ + "params"]).max() <= 1e-12


CHECKPOINTS = ("p2", "p3", "p6", "g")   # one save_model file per class: GCN_1D_Kernel, GCN_2D_Kernel, GCN_3D_Kernel, GCA_1D


@pytest.mark.parametrize("kind", CHECKPOINTS)
def test_checkpoints_are_in_registration_order(kind):
    """every class's save_model writes W1_0; W1_l, W2_l; then W [2 H] (pairs) or nothing more (GCA_1D has no W)"""
    gz = golden()
    tag = str(gz["checkpoint_%s__tag" % kind])
    assert tag == ("g_CH4" if kind == "g" else kind + "_CH4_one")
    params = gz[tag + "__params"]
    assert bytes(gz["checkpoint_%s__text" % kind]).decode().split() == ["%g" % x for x in params]
    _, L, H, D, R, M = (int(x) for x in gz[tag + "__cfg"])
    assert params.size == nref.n_params(H, 4 * (D + 1), L) + (-H if kind == "g" else H)


# ---- what the library answers without a device ----
def pair_config(form, L, H, F, D, maxV, R=1, **over):
    from graphflow_amd.smp import SMPKernelPairs
    cfg = SMPKernelPairs.config(FORMS[form], L, H, F, D, maxV, R)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def gca_config(L, H, F, D, maxV, R=1, **over):
    from graphflow_amd.smp import GCA1D
    cfg = GCA1D.config("gca_1d", L, H, F, D, maxV, R)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def refused_configs():
    """[(configuration gf_smp_create answers GF_ERR_INVALID to, a piece of its message)]"""
    named = b"the read-outs are readout = 1 (pairs)"
    rules = b"needs first_order = steerable_2d"
    bad = []
    for form in FORMS:
        bad += [(pair_config(form, 2, 8, 5, 1, 9, **{k: 1}), rules) for k in ("first_order", "steerable_2d", "unrestricted", "physics", "custom_matmul")]
        bad.append((pair_config(form, 2, 8, 5, 1, 9, matrix_form=1), named))
        bad.append((pair_config(form, 2, 8, 5, 1, 9, distance_channel=1), named))
        bad.append((pair_config(form, 2, 8, 5, 1, 9, nContractions=18), rules))
        bad.append((pair_config(form, 2, 8, 5, 1, 9, max_receptive_field=6), rules))
        bad.append((pair_config(form, 2, 8, 5, 1, 9, R=-1), b"max_Radius (-1) >= 0"))   # max_Radius >= 0 in all three, the 2D class included
        bad.append((pair_config(form, 2, 129, 5, 1, 9), b"third-order pool takes at most 64" if form == 6 else b"nChanels (129) <= 128"))
        bad.append((pair_config(form, 2, 64, 600, 0, 9), b"within 160 KiB"))           # F' beyond the LDS bound at 64 channels
        bad += [(pair_config(form, 2, 8, 5, 1, 9, readout=r), named) for r in (3, -1, 7)]
        bad += [(pair_config(form, 2, 8, 5, 1, 9, neighbourhood=n), named) for n in (0, 1, 4, 5, 7)]   # any other form
    bad.append((pair_config(6, 2, 65, 5, 1, 9), b"third-order pool takes at most 64"))
    bad.append((pair_config(6, 2, 64, 5, 0, 475), b"at most 474 vertices"))           # form 6's max_nVertices bound
    bad += [(gca_config(2, 8, 5, 1, 9, neighbourhood=n), named) for n in (0, 1, 3, 4, 5, 6, 7)]   # the Gram read-out sits on form 2 alone
    bad.append((gca_config(2, 8, 5, 1, 9, distance_channel=1), named))
    bad.append((gca_config(2, 8, 5, 1, 9, matrix_form=2), named))
    bad.append((gca_config(2, 8, 5, 1, 9, R=-1), b"max_Radius (-1) >= 0"))
    bad.append((gca_config(2, 64, 5, 0, 173), b"against 160 KiB"))                    # the Gram kernel's LDS bound: 172 vertices at 64 channels
    bad.append((gca_config(2, 128, 5, 0, 148), b"4 (V (H | 1) + V (V | 1) + 4)"))     # ... 147 at 128
    bad.append((gca_config(2, 5, 5, 0, 200), b"against 160 KiB"))                     # ... 199 at 5
    return bad


def last_refusal(lib, cfg):
    """the resolver's verdict and message for cfg, through a host-only entry point that asks it first"""
    one, x = np.zeros(1, dtype=np.int32), np.zeros(64, dtype=np.float64)
    st = lib.gf_smp_matrix_form_molecule_host(C.byref(cfg), 1, one.ctypes.data_as(IP), x.ctypes.data_as(DP), one.ctypes.data_as(IP),
                                              one.ctypes.data_as(IP), x.ctypes.data_as(DP))
    return st, lib.gf_last_error(None)


def test_parameter_counts_and_block_layouts(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    for L, H, F, D, M in ((0, 5, 4, 0, 3), (1, 6, 4, 0, 29), (3, 20, 5, 2, 12), (3, 64, 5, 0, 64), (2, 33, 4, 1, 100)):
        FD = F * (D + 1)
        for form in FORMS:
            cfg = pair_config(form, L, H, F, D, M, 2)
            assert lib.gf_smp_config_param_count(C.byref(cfg)) == pref.n_params(H, FD, L, 1) == nref.n_params(H, FD, L) + H, (form, L, H)
            assert lib.gf_smp_classifier_config_param_count(C.byref(cfg), 3) == 0
        cfg = gca_config(L, H, F, D, M, 2)
        assert lib.gf_smp_config_param_count(C.byref(cfg)) == pref.n_params(H, FD, L, 2) == nref.n_params(H, FD, L) - H
        assert lib.gf_smp_classifier_config_param_count(C.byref(cfg), 3) == 0
    # the Gram kernel's LDS bound, at its edges
    for H, M in ((64, 172), (128, 147), (5, 199)):
        assert lib.gf_smp_config_param_count(C.byref(gca_config(2, H, 5, 0, M))) == pref.n_params(H, 5, 2, 2)
        assert lib.gf_smp_config_param_count(C.byref(gca_config(2, H, 5, 0, M + 1))) == 0
        assert 4 * (M * (H | 1) + M * (M | 1) + 4) <= 160 * 1024 < 4 * ((M + 1) * (H | 1) + (M + 1) * ((M + 1) | 1) + 4)


def test_every_refusal_names_its_reason(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    out = np.full(1 << 16, 7.0, dtype=np.float32)
    for bad, text in refused_configs():
        assert lib.gf_smp_config_param_count(C.byref(bad)) == 0
        assert lib.gf_smp_uniform_init_host(C.byref(bad), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_ERR_INVALID
        st, why = last_refusal(lib, bad)
        assert st == INVALID and text in why, (text, why)
    assert (out == 7.0).all()
    # an accepted configuration reaches the entry point's own refusal: the resolver had no objection
    for cfg in (pair_config(3, 2, 8, 5, 1, 9), gca_config(2, 8, 5, 1, 9)):
        st, why = last_refusal(lib, cfg)
        assert st == INVALID and b"matrix_form = 0" in why
        phi = np.zeros(4096, dtype=np.int32)
        one, x = np.zeros(1, dtype=np.int32), np.zeros(64, dtype=np.float64)
        assert lib.gf_smp_prepare_molecule_host(C.byref(cfg), 1, one.ctypes.data_as(IP), x.ctypes.data_as(DP), phi.ctypes.data_as(IP), None) == INVALID
        assert b"has no receptive fields" in lib.gf_last_error(None)


def test_zero_tail_reproduces_every_existing_form(gf):
    """readout = 0 is everything as before: a structure without the new field (the library reads a zero there) and one with it set to 0
    count the same parameters, for every family of configurations the resolver takes"""
    from graphflow_amd import _lib
    from graphflow_amd.smp import GCNMW, LCNN, SMP1D, SMP2D, SMPConfig, SMPDistance, SMPGatedNeighbourhood, SMPNeighbourhood, SMPTheta, SMPUnrestricted
    lib = _lib.load()
    cfgs = [SMPConfig(2, 8, 5, 1, 12, 1), SMPConfig(2, 8, 5, 1, 12, 1, 10, 1), SMPConfig(2, 8, 5, 1, 12, 1, 50, 1), SMPConfig(2, 8, 5, 1, 12, 1, 4),
            SMPTheta.config(12, 9, 2, 8, 5, 1)]
    cfgs += [SMP1D.config(v, 9, 2, 6, 5, 1) for v in (1, 2, 3)] + [SMP2D.config(f, 9, 2, 6, 5, 1) for f in SMP2D.FORMS]
    cfgs += [SMPUnrestricted.config(f, 9, 2, 6, 5, 1) for f in SMPUnrestricted.FORMS]
    cfgs += [SMPNeighbourhood.config(f, 2, 8, 5, 0 if f == "fingerprint" else 1, 9, 1) for f in SMPNeighbourhood.FORMS]
    cfgs += [SMPGatedNeighbourhood.config(f, 2, 8, 5, 1, 9, 1) for f in SMPGatedNeighbourhood.FORMS]
    cfgs += [SMPDistance.config(f, 2, 8, 5, 1, 9, 1) for f in SMPDistance.FORMS]
    cfgs += [GCNMW.config(2, 9, 5, 8, 1), LCNN.config(9, 5, 3, 1, 8, 6, 4)]
    old_fields = [f for f in SMPConfig._fields_ if f[0] != "readout"]
    assert len(old_fields) == len(SMPConfig._fields_) - 1 and SMPConfig._fields_[-1][0] == "readout"

    class Padded(C.Structure):   # the parent's structure, followed by the zero the library reads as `readout`
        _fields_ = old_fields + [("tail", C.c_int)]

    for cfg in cfgs:
        assert cfg.readout == 0
        n = lib.gf_smp_config_param_count(C.byref(cfg))
        assert n > 0, [getattr(cfg, f[0]) for f in SMPConfig._fields_]
        old = Padded(*[getattr(cfg, f[0]) for f in old_fields])
        assert lib.gf_smp_config_param_count(C.cast(C.byref(old), C.POINTER(SMPConfig))) == n
    # ... and the plain forms under the new classes' constructors count their own parameters
    for form in FORMS:
        assert lib.gf_smp_config_param_count(C.byref(pair_config(form, 2, 8, 5, 1, 9, readout=0))) == nref.n_params(8, 10, 2)


def test_uniform_init_draws_the_classes_weights(gf):
    """after srand(seed): every matrix by uniform_init(Matrix*) (10 x nRows = 10 H), W by uniform_init(Vector*) (10 x 2 H), in
    registration order -- bit for bit the weights the classes drew; GCA_1D draws no W"""
    from graphflow_amd import _lib
    lib = _lib.load()
    gz = golden()
    for form in (2, 3, 6, 0):
        p_ = "train_%s__" % ("p%d" % form if form else "g")
        _, L, H, D, R, maxV, seed, _ = (int(x) for x in gz[p_ + "cfg"])
        cfg = pair_config(form, L, H, 4, D, maxV, R) if form else gca_config(L, H, 4, D, maxV, R)
        count = pref.n_params(H, 4 * (D + 1), L, 1 if form else 2)
        out = np.full(count + 1, 7.0, dtype=np.float32)
        C.CDLL(None).srand(seed)
        assert lib.gf_smp_uniform_init_host(C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_float))) == _lib.GF_OK
        assert np.array_equal(out[:count], gz[p_ + "params0"].astype(np.float32)) and out[count] == 7.0
        assert np.abs(out[:count]).max() > 0
        off = 0
        for name, n in pref.blocks(H, 4 * (D + 1), L, 1 if form else 2):   # the divisor the block list implies
            steps = np.abs(out[off:off + n].astype(np.float64)) * 10.0 * (2 * H if name == "W" else H)
            assert np.abs(steps - np.round(steps)).max() < 1e-4 and steps.max() <= 9.0 + 1e-4, name
            off += n


def test_python_classes_describe_themselves():
    from graphflow_amd import GCA1D, SMPKernelPairs, SMPNeighbourhood
    assert issubclass(SMPKernelPairs, SMPNeighbourhood) and issubclass(GCA1D, SMPNeighbourhood)
    for cls, words in ((SMPKernelPairs, ("GCN_1D_Kernel", "GCN_2D_Kernel", "GCN_3D_Kernel", "W[2 H]", "prepare(graphs_x, graphs_y)")),
                       (GCA1D, ("GCA_1D", "LinearGram", "gram()", "E[y, x]"))):
        for w in words:
            assert w in cls.__doc__, (cls.__name__, w)
    with pytest.raises(ValueError, match="gcn_1d_kernel"):
        SMPKernelPairs.config("gcn_1d", 2, 8, 5, 1, 9)
    cfg = SMPKernelPairs.config("gcn_2d_kernel", 2, 8, 5, 1, 9, 3)
    assert (cfg.neighbourhood, cfg.max_Radius, cfg.readout, cfg.distance_channel) == (3, 3, 1, 0)
    cfg = GCA1D.config("gca_1d", 2, 8, 5, 1, 9, 3)
    assert (cfg.neighbourhood, cfg.max_Radius, cfg.readout) == (2, 3, 2)
