"""The fused SMP level at 128 channels: every 128 x 128 block product as four 64 x 64 sub-block passes (reduction half i, output half j)
of the split-operand row-panel kernels, the weight gradients as four independent 64 x 64 jobs per product (smp_level_c64_split.hip, smp_level_wgrad_split.hip: W = 2).

1. The stand-alone operators gf_smp_level_products_ex_f32 / gf_smp_level_wgrad_ex_f32 at C = 128 against the fp64 product of the same
   operands (tests/level_ref.py), per (row, block of 128 columns) and per (weight-gradient block, row), TOL = 1e-5: level-shaped rows
   (nodes of 1 .. 12 positions up and down: 650 rows) plain, packed and with skip_zero_grads; ragged row counts; operands and weights
   that live in ONE (i, j) sub-block; a loud channel in the other 64-column half; the same bits twice; the refusals.
2. A 128-channel model (L = 2, 3; molecules of 3 .. 12 atoms) with GF_SMP_C128=1 against the fp64 port per parameter block, against the
   same batch under GF_SMP_C128=0, and twice for the same bits; and the operator and model tests once more in a child process that has
   GF_POISON=1 in its environment from the start (the library reads it once per process).  The port takes the device's LeakyReLU slope only inside KINK_TOL
   of the kink; the tests require that it never had to (n_override == 0), so the allowance hides nothing.
3. The timing table: the dedicated launches are there and the level-sized GEMMs are gone; a 64-channel handle's table is the one
   pinned below whatever the switch says.

Every test prints its figures (pytest -s).  Worst measured on an MI355X: operators forward 3.0e-7, backward 2.9e-7 (with skip_zero_grads the
same), weight gradients 6.7e-7, loud channel 2.8e-7; model against the fp64 port 5.1e-7 (dK3) and 4.9e-7 (prediction); against the generic
path 3.5e-7 forward, 3.6e-7 gradients, no slope taken differently."""
import numpy as np
import pytest

import level_ref as lr
import test_level_ops_ex_gpu as ex
import test_smp_gpu as sg
from inputs import smp_params, synthetic_molecule
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C128 = 128
TOL = 1e-5
SENTINEL = ex.SENTINEL
RAGGED = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 80]


# ---- 1. the operators ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [False, True], ids=["plain", "packed"])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_level_shaped_rows(gf, order, packed):
    """650 rows: 21 panels of 32 rows (the last one partial), 41 slices of 16, node boundaries inside panels and slices.  Packed: absent
    blocks of T hold garbage; with skip_zero_grads dO of uncovered rows does too and the skipped blocks keep the sentinel (check_case)."""
    sizes = list(range(1, 13)) if order == "ascending" else list(range(12, 0, -1))
    c = ex.Case(sizes, C128, 2, 0, packed, seed=128 + 2 * packed + (order == "descending"))
    assert c.rows == 650
    if packed:
        own, trp, bc = c.bits
        assert (~own & bc).any() and (~bc).any() and (~own & trp).any() and (own & ~trp).any()
    ex.report("C=128 level 1..12 %s %s" % (order, "packed" if packed else "plain"), ex.check_case(c))


def test_ragged_row_counts(gf):
    worst = {}
    for rows in RAGGED:
        for ones in (True, False):
            for packed in (False, True):
                sizes = ex.small_sizes(rows, ones)
                assert sum(s * s for s in sizes) == rows
                c = ex.Case(sizes, C128, 2, 0, packed, seed=rows + 1000 * ones)
                for k, v in ex.check_case(c).items():
                    worst[k] = max(worst.get(k, 0.0), v)
                    assert v <= TOL, (rows, ones, packed, k, v)
    ex.report("C=128 ragged rows", worst)


@pytest.mark.parametrize("i,j", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_one_sub_block_at_a_time(gf, i, j):
    """Weights that are nonzero in sub-block (i, j) only -- rows [64 i, +64), columns [64 j, +64) of every W_p -- on dense operands, and
    dense weights on operands that are nonzero in one half only: a wrong offset, a swapped half or a missed accumulation is a zero or
    misplaced block of the result, and the blocks that must be zero are checked to be exactly zero."""
    sizes = [5, 4, 7, 1, 6]   # 127 rows
    c = ex.Case(sizes, C128, 2, 0, False, seed=40 + 2 * i + j)
    ki, kj = slice(64 * i, 64 * i + 64), slice(64 * j, 64 * j + 64)
    W = np.zeros_like(c.W)
    W[:, ki, kj] = c.W[:, ki, kj]
    err = {}
    got = ex.run_products(False, C128, 2, 0, c.T, c.rf, W, None, c.trow)
    err["fwd_w"] = lr.row_block_err(got, lr.forward_ref(c.T, c.rf, W, c.trow, C128), C128)
    assert np.all(got.reshape(c.rows, 2, 2, 64)[:, :, 1 - j] == 0.0)       # the other output half
    got = ex.run_products(True, C128, 2, 0, c.dO, c.rf, W, None, c.trow)    # dT[:, i-half] = dO[:, j-half] (W[i, j])^T
    err["bwd_w"] = lr.row_block_err(got, lr.backward_ref(c.dO, c.rf, W, c.trow, C128), C128)
    assert np.all(got.reshape(c.rows, 4, 2, 64)[:, :, 1 - i] == 0.0)
    # operands in one half: T in columns [64 i, +64) of every block, dO in [64 j, +64)
    T = np.zeros_like(c.T).reshape(c.rows, 4, 128)
    T[:, :, ki] = c.T.reshape(c.rows, 4, 128)[:, :, ki]
    T = T.reshape(c.rows, 512)
    dO = np.zeros_like(c.dO).reshape(c.rows, 2, 128)
    dO[:, :, kj] = c.dO.reshape(c.rows, 2, 128)[:, :, kj]
    dO = dO.reshape(c.rows, 256)
    got = ex.run_products(False, C128, 2, 0, T, c.rf, c.W, None, c.trow)
    err["fwd_a"] = lr.row_block_err(got, lr.forward_ref(T, c.rf, c.W, c.trow, C128), C128)
    got = ex.run_products(True, C128, 2, 0, dO, c.rf, c.W, None, c.trow)
    err["bwd_a"] = lr.row_block_err(got, lr.backward_ref(dO, c.rf, c.W, c.trow, C128), C128)
    dW, _ = ex.run_wgrad(C128, 2, 0, T, dO, c.rf, c.trow)
    rW, _ = lr.wgrad_ref(T, dO, c.rf, c.trow, C128)
    err["wgrad_a"] = lr.wgrad_row_err(dW[:, ki, kj], rW[:, ki, kj])
    keep = np.zeros((128, 128), dtype=bool)
    keep[ki, kj] = True
    assert np.all(dW[:, ~keep] == 0.0)                                      # the other three sub-blocks of every product
    ex.report("C=128 sub-block (%d, %d) alone" % (i, j), err)


@pytest.mark.parametrize("half", [0, 1])
def test_loud_channel_in_the_other_half(gf, half):
    """One channel of every block 1e6 : 1 above the rest, in the 64-column half `1 - half`; the weights ignore it in the output columns
    of half `half`, which are made of the small entries alone and held to the fp64 product per (row, 64-column half block)."""
    big = 1e6
    sizes = [7] * 13   # 637 rows
    rng = np.random.default_rng(70 + half)
    trow, _ = lr.level_rows(sizes)
    rows = trow.size
    rf = lr.row_factors(sizes, rng, 2)
    loud = 64 * (1 - half) + int(rng.integers(64))
    cols = slice(64 * half, 64 * half + 64)

    def operand(width):
        A = rng.standard_normal((rows, width)) * np.exp(rng.uniform(-9, 9, (rows, 1)))
        A[:, loud::128] *= big
        return A.astype(np.float32)

    def half_err(got, ref, nblk):
        g, r = got.reshape(rows, nblk, 128)[:, :, cols], ref.reshape(rows, nblk, 128)[:, :, cols]
        return lr.row_block_err(g.reshape(rows, -1), r.reshape(rows, -1), 64)

    T = operand(512)
    W = rng.uniform(-1, 1, (8, 128, 128)).astype(np.float32)
    W[:, loud, cols] = 0.0
    e_f = half_err(ex.run_products(False, C128, 2, 0, T, rf, W, None, trow), lr.forward_ref(T, rf, W, trow, C128), 2)
    dO = operand(256)
    W = rng.uniform(-1, 1, (8, 128, 128)).astype(np.float32)
    W[:, cols, loud] = 0.0
    e_b = half_err(ex.run_products(True, C128, 2, 0, dO, rf, W, None, trow), lr.backward_ref(dO, rf, W, trow, C128), 4)
    ex.report("C=128 loud channel %d, columns of half %d" % (loud, half), {"fwd": e_f, "bwd": e_b})


def test_same_bits_twice_operators(gf):
    c = ex.Case(list(range(1, 13)), C128, 2, 0, True, seed=77)
    runs = []
    for _ in range(2):
        a = [ex.run_products(False, C128, 2, 0, c.T, c.rf, c.W, None, c.trow, c.trowf),
             ex.run_products(True, C128, 2, 0, c.dO, c.rf, c.W, None, c.trow, c.trowf),
             ex.run_wgrad(C128, 2, 0, c.T, c.dO, c.rf, c.trow, c.trowf)[0]]
        runs.append(a)
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_refusals_at_128(gf, monkeypatch):
    from graphflow_amd import _lib
    good = ex.Case([3, 2, 1], C128, 2, 0, False, seed=5)
    c8 = ex.Case([3, 2, 1], C128, 8, 0, False, seed=6)
    c3 = ex.Case([3, 2, 1], C128, 2, 3, False, seed=7)
    for c in (c8, c3):
        st, out = ex.products_status(False, C128, c.nf, c.nx, c.T, c.rf, c.W, c.X, c.trow)
        assert st == _lib.GF_ERR_UNSUPPORTED and np.all(out == SENTINEL), (c.nf, c.nx, st)
        st, dW, _ = ex.wgrad_status(C128, c.nf, c.nx, c.T, c.dO, c.rf, c.trow)
        assert st == _lib.GF_ERR_UNSUPPORTED and np.all(dW == SENTINEL), (c.nf, c.nx, st)
        ex.report("after a refusal", ex.check_case(good))
    for Cc in (48, 256):
        c = ex.Case([3, 2, 1], Cc, 2, 0, False, seed=8)
        assert ex.products_status(False, Cc, 2, 0, c.T, c.rf, c.W, None, c.trow)[0] == _lib.GF_ERR_UNSUPPORTED
        assert ex.wgrad_status(Cc, 2, 0, c.T, c.dO, c.rf, c.trow)[0] == _lib.GF_ERR_UNSUPPORTED
    c = ex.Case([3, 2, 1], 64, 2, 0, False, seed=9)
    assert ex.wgrad_status(64, 2, 0, c.T, c.dO, c.rf, c.trow)[0] == _lib.GF_ERR_UNSUPPORTED
    monkeypatch.setenv("GF_SMP_SPLIT", "0")   # 128 channels on the fp32 pipe
    st, out = ex.products_status(False, C128, 2, 0, good.T, good.rf, good.W, None, good.trow)
    assert st == _lib.GF_ERR_UNSUPPORTED and np.all(out == SENTINEL)
    st, dW, _ = ex.wgrad_status(C128, 2, 0, good.T, good.dO, good.rf, good.trow)
    assert st == _lib.GF_ERR_UNSUPPORTED and np.all(dW == SENTINEL)
    monkeypatch.delenv("GF_SMP_SPLIT")
    ex.report("after a refusal", ex.check_case(good))


# ---- 2. the model --------------------------------------------------------------------------------------------------------------

F, D, CAP = 5, 2, 12


def model_batch(L):
    mols, tg = [], []
    # 3 .. 12 atoms: every field is at most 12 positions.  Seeds chosen on the CPU (fp64 port, 1.5e6 pre-activations per batch): the
    # one closest to the LeakyReLU kink lies 2.9e-7 (L = 2) and 6.7e-7 (L = 3) of its level's largest from it, outside KINK_TOL = 1e-7
    for k in range(10):
        adj, feat, t = synthetic_molecule(3400 + 16 * L + k, nV=3 + k)
        mols.append((adj, feat))
        tg.append(t)
    return mols, np.array(tg), smp_params(C128, F, D, L, 9)


def param_blocks(n, L):
    """(name, slice) of H, K_l, b_l, W in the parameter vector of a 128-channel model"""
    per = 18 * C128 * C128 + C128
    nH = n - L * per - C128
    out, o = [("H", slice(0, nH))], nH
    for l in range(1, L + 1):
        out.append(("K%d" % l, slice(o, o + 18 * C128 * C128)))
        out.append(("b%d" % l, slice(o + 18 * C128 * C128, o + per)))
        o += per
    out.append(("W", slice(o, n)))
    return out


def port_reference(mols, tg, params, L, net):
    """the fp64 port of every molecule, with the device's LeakyReLU slopes offered inside KINK_TOL (sg.kink_aware_reference): sums"""
    pred, feat, grads, n_over = [], [], 0.0, 0
    for m, ((adj, fe), t) in enumerate(zip(mols, tg)):
        o = sg.kink_aware_reference({"adj": adj, "feature": fe, "target": np.array([t])}, params, (L, C128, D, CAP), net, m)
        pred.append(o["predict"])
        feat.append(o["graph_feature"])
        grads = grads + o["grads"]
        n_over += o["n_override"]
    return np.array(pred), np.stack(feat), grads, n_over


@pytest.mark.parametrize("L", [2, 3])
def test_model_against_the_port_and_the_generic_path(gf, L, monkeypatch):
    mols, tg, params = model_batch(L)
    monkeypatch.setenv("GF_SMP_C128", "1")
    p1, _, f1, g1, n1 = sg.run_batch(gf, mols, tg, params, L, C128, F, D, CAP)
    rp, rf_, rg, n_over = port_reference(mols, tg, params.astype(np.float64), L, n1)
    assert n_over == 0, "%d activations inside the kink tolerance: choose other seeds" % n_over
    errs = {"pred": rel_err(p1, rp), "feat": rel_err(f1, rf_)}
    for name, sl in param_blocks(g1.size, L):
        errs["d" + name] = rel_err(g1[sl], rg[sl])
    print("C=128 L=%d vs the fp64 port: %s" % (L, ", ".join("%s %.2e" % kv for kv in errs.items())))
    bad = {k: v for k, v in errs.items() if not v <= sg.TOL_GRAD}
    assert not bad, bad
    # the same batch on the path GF_SMP_C128=0 selects
    monkeypatch.setenv("GF_SMP_C128", "0")
    p0, _, f0, g0, n0 = sg.run_batch(gf, mols, tg, params, L, C128, F, D, CAP)
    monkeypatch.setenv("GF_SMP_C128", "1")
    assert not np.array_equal(f1, f0)   # (the switch switches something)
    print("C=128 L=%d vs GF_SMP_C128=0: pred %.2e feat %.2e" % (L, rel_err(p1, p0), rel_err(f1, f0)))
    assert rel_err(p1, p0) <= 2e-6 and rel_err(f1, f0) <= 2e-6
    sg.assert_grads_agree_kink_aware("c128_kernels_vs_tiled_gemms", g1, g0, n1, n0, mols, L)
    # two sweeps, the same bits
    p2, _, f2, g2, _ = sg.run_batch(gf, mols, tg, params, L, C128, F, D, CAP)
    assert np.array_equal(p1, p2) and np.array_equal(f1, f2) and np.array_equal(g1, g2)


def test_no_kernel_reads_what_nobody_wrote_at_128():
    """GF_POISON=1 NaN-fills every buffer the library hands out, and is read ONCE per process: the operator tests and the model test above
    in a child process that starts with it.  The 128-channel path leans on unwritten memory in three places, and none may be read into
    a result: the accumulating passes load dT blocks that skip_zero_grads never stores (their sums go to the scratch rows), the weight
    gradients take column maxima over all of T and dO (T is written densely at 128), and the partial images are filled by four jobs."""
    from field_suite import run_under_poison
    run_under_poison(__file__, "level_shaped_rows or ragged_row_counts or one_sub_block or model_against_the_port")


# ---- 3. the plan ---------------------------------------------------------------------------------------------------------------

def launch_counts(gf, C, L, monkeypatch, switch):
    from graphflow_amd.smp import SMPOmega
    if switch is None:
        monkeypatch.delenv("GF_SMP_C128", raising=False)
    else:
        monkeypatch.setenv("GF_SMP_C128", switch)
    mols, tg, _ = model_batch(L)
    params = smp_params(C, F, D, L, 9)
    net = SMPOmega(L, C, F, D, CAP, True)
    net.prepare(mols)
    p = sg.dev(params)
    grads = torch.empty(net.n_params, device="cuda")
    net.ctx.set_timing(True)
    net.forward(p, sg.dev(tg))
    net.backward(p, grads)
    counts = {k: n for k, (_, n) in net.ctx.timings().items()}
    net.ctx.set_timing(False)
    monkeypatch.delenv("GF_SMP_C128", raising=False)
    return counts


# one forward + backward of the 64-channel model on model_batch(2): kernel names and launch counts, as the library gave them before the
# 128-channel path existed
C64_PLAN = {'gemm_nt': 1, 'gemm_tn': 1, 'smp_bias_lrelu': 1, 'smp_lrelu_bwd': 1, 'smp_readout_bwd': 1, 'smp_readout_dW': 1, 'smp_readout_mol': 1,
            'smp_readout_nodes': 1, 'smp_zero': 1, 'smpf_bwd_gather': 2, 'smpf_colmax': 2, 'smpf_combine_bwd': 2, 'smpf_combine_fwd': 2,
            'smpf_diag_gather': 2, 'smpf_diag_gather_bwd': 2, 'smpf_fold': 2, 'smpf_products_bwd': 2, 'smpf_products_fwd': 2, 'smpf_small_nn': 2,
            'smpf_small_nt': 2, 'smpf_small_tn': 2, 'smpf_stack_w': 2, 'smpf_tables_fwd_ni1': 2, 'smpf_tables_fwd_ni2': 2, 'smpf_tables_fwd_ni4': 1,
            'smpf_wgrad': 2}


def test_the_plan_runs_the_dedicated_kernels(gf, monkeypatch):
    L = 2
    new, old = launch_counts(gf, C128, L, monkeypatch, "1"), launch_counts(gf, C128, L, monkeypatch, "0")
    print("C=128 launches: %s\nGF_SMP_C128=0: %s" % (sorted(new.items()), sorted(old.items())))
    # four sub-block passes per level and direction, four jobs of weight gradients
    assert new.get("smpf_products_fwd") == 4 * L and new.get("smpf_products_bwd") == 4 * L and new.get("smpf_wgrad") == 4 * L
    for k in ("smpf_products_fwd", "smpf_products_bwd", "smpf_wgrad"):
        assert k not in old, k
    # the level-rows GEMMs: forward products (nn), table gradients (nt), weight gradients (tn) -- at least one launch each per level on the
    # generic path (one grouped launch, or one per product where the grouped form does not apply), none on the new one: what remains
    # under these names are the small products and the level-0 / read-out GEMMs
    for k in ("gemm_nn", "gemm_nt", "gemm_tn"):
        assert old.get(k, 0) - new.get(k, 0) >= L, (k, old.get(k, 0), new.get(k, 0))
    assert launch_counts(gf, C128, L, monkeypatch, None) == new   # (unset: the dedicated kernels)


@pytest.mark.parametrize("switch", [None, "0", "1"])
def test_a_64_channel_plan_is_what_it_was(gf, monkeypatch, switch):
    got = launch_counts(gf, 64, 2, monkeypatch, switch)
    print("C=64 launches (GF_SMP_C128=%s): %r" % (switch, dict(sorted(got.items()))))
    assert got == C64_PLAN
