"""CPU suite: the fp64 reference and the operand generators of tests/level_ref.py, which every per-row GPU test of the fused level's
block products stands on (tests/test_level_ops_ex_gpu.py), checked against the three C = 64 functions of tests/test_level_ops_gpu.py and
against their own definitions."""
import numpy as np
import pytest

import level_ref as lr

SIZES = [1, 2, 5, 31, 32, 33, 36, 64]


def operands(rng, rows, C, nx=0):
    T = rng.standard_normal((rows, 4 * C)).astype(np.float32)
    dO = rng.standard_normal((rows, 2 * C)).astype(np.float32)
    W = rng.uniform(-1, 1, (8, C, C)).astype(np.float32)
    X = rng.uniform(-1, 1, (3, C, C)).astype(np.float32) if nx else None
    return T, dO, W, X


def test_equal_to_the_c64_functions_of_the_existing_suite():
    old = pytest.importorskip("test_level_ops_gpu")
    rng = np.random.default_rng(0)
    sizes = [3, 1, 7, 2]
    trow, _ = lr.level_rows(sizes)
    rows = trow.size
    T, dO, W, _ = operands(rng, rows, 64)
    rs = lr.row_factors(sizes, rng, 2)
    for bits in (None, lr.all_present(rows)):
        # (fp64 sums in another order: 1e-12 of the largest entry)
        close = dict(rtol=0, atol=1e-12 * 29 * 64 * 8)
        np.testing.assert_allclose(lr.forward_ref(T, rs, W, trow, 64, bits=bits), old.forward_ref(T, rs, W, trow), **close)
        np.testing.assert_allclose(lr.backward_ref(dO, rs, W, trow, 64, bits=bits, skip_zero_grads=bits is not None),
                                   old.backward_ref(dO, rs, W, trow), **close)
        dW, dX = lr.wgrad_ref(T, dO, rs, trow, 64, bits=bits)
        assert dX is None
        np.testing.assert_allclose(dW, old.wgrad_ref(T, dO, rs, trow), **close)


def test_generated_trow_is_an_involution_inside_each_node():
    trow, node = lr.level_rows(SIZES)
    rows = sum(s * s for s in SIZES)
    assert rows == 8496 and trow.size == rows and trow.dtype == np.int32
    assert np.array_equal(trow[trow], np.arange(rows))
    assert np.array_equal(node[trow], node)
    dist = np.abs(trow.astype(np.int64) - np.arange(rows))
    for n, s in enumerate(SIZES):
        assert dist[node == n].max() == (s - 1) ** 2
    assert dist.max() == 63 ** 2 == 3969


def test_presence_bits_obey_the_structure_of_a_level():
    rng = np.random.default_rng(1)
    trow, _ = lr.level_rows(SIZES)
    own, trp, bc = bits = lr.presence_bits(SIZES, rng)
    assert np.array_equal(trp, own[trow])            # bit 30 of a row = bit 31 of its transposed row
    assert not np.any(own & ~bc)                     # a row with data in S_ab has a source that holds both its positions
    assert np.array_equal(bc, bc[trow])
    assert 0.1 < own.mean() < 0.9 and 0.01 < (~bc).mean() < 0.9    # (rows of every kind occur)
    t, o, r, b = lr.unpack(lr.pack(trow, bits))
    assert np.array_equal(t, trow) and np.array_equal(o, own) and np.array_equal(r, trp) and np.array_equal(b, bc)
    w = lr.pack(trow, bits).view(np.uint32)
    assert np.array_equal(w >> 31 == 1, own) and np.array_equal((w >> 30) & 1 == 1, trp) and np.array_equal((w >> 29) & 1 == 1, bc)


def test_row_factors_are_per_node_and_dropout_only_zeroes():
    rng = np.random.default_rng(2)
    sizes = [2, 3, 1, 4] * 8
    trow, node = lr.level_rows(sizes)
    f2, f8 = lr.row_factors(sizes, rng, 2), lr.row_factors(sizes, rng, 8)
    assert f2.shape == (trow.size, 2) and f8.shape == (trow.size, 8)
    assert np.array_equal(f8[trow], f8) and np.array_equal(f2[trow], f2)
    assert (f8 == 0).any() and (f8[:, 3:][f8[:, 3:] != 0] == 1).all()
    kept = f8[:, 0] != 0
    assert np.all((f8[kept, 0] >= 1) & (f8[kept, 0] <= 29))
    assert np.array_equal(lr.factors8(f2)[:, [0, 2]], f2.astype(np.float64))


@pytest.mark.parametrize("C,nf,nx", [(64, 2, 0), (32, 2, 0), (32, 8, 0), (32, 2, 3), (16, 2, 0), (16, 8, 0), (16, 2, 3)])
def test_full_mask_is_no_mask_and_an_absent_block_is_a_zero_block(C, nf, nx):
    rng = np.random.default_rng(C + nf + nx)
    sizes = [1, 2, 5, 3]
    trow, _ = lr.level_rows(sizes)
    rows = trow.size
    T, dO, W, X = operands(rng, rows, C, nx)
    rf = lr.row_factors(sizes, rng, nf)
    full = lr.all_present(rows)
    assert np.array_equal(lr.forward_ref(T, rf, W, trow, C, X, full), lr.forward_ref(T, rf, W, trow, C, X))
    assert np.array_equal(lr.backward_ref(dO, rf, W, trow, C, X, full, True), lr.backward_ref(dO, rf, W, trow, C, X))
    assert lr.stored_blocks(rows, full, True).all()
    a, b = lr.wgrad_ref(T, dO, rf, trow, C, nx, full), lr.wgrad_ref(T, dO, rf, trow, C, nx)
    assert np.array_equal(a[0], b[0]) and (nx == 0 or np.array_equal(a[1], b[1]))
    # garbage in the absent blocks changes nothing; zeroing them by hand gives the same as the bits
    bits = lr.presence_bits(sizes, rng)
    G = lr.fill_absent(T, C, bits, rng)
    Z = np.array(T)
    for blk, have in ((0, bits[0]), (1, bits[2]), (2, bits[0]), (3, bits[2])):
        assert np.all(G[have, blk * C:(blk + 1) * C] == T[have, blk * C:(blk + 1) * C])
        assert np.all(G[~have, blk * C:(blk + 1) * C] != T[~have, blk * C:(blk + 1) * C])
        Z[~have, blk * C:(blk + 1) * C] = 0
    assert np.array_equal(lr.forward_ref(G, rf, W, trow, C, X, bits), lr.forward_ref(Z, rf, W, trow, C, X))
    a, b = lr.wgrad_ref(G, dO, rf, trow, C, nx, bits), lr.wgrad_ref(Z, dO, rf, trow, C, nx)
    assert np.array_equal(a[0], b[0]) and (nx == 0 or np.array_equal(a[1], b[1]))


@pytest.mark.parametrize("nf,nx", [(2, 0), (8, 0), (2, 3)])
def test_backward_and_wgrad_are_the_derivatives_of_forward(nf, nx):
    """<forward(T), dO> is linear in T and in W: its gradients are backward(dO) and wgrad(T, dO), masked or not."""
    C = 16
    rng = np.random.default_rng(10 * nf + nx)
    sizes = [3, 1, 4]
    trow, _ = lr.level_rows(sizes)
    rows = trow.size
    T, dO, W, X = operands(rng, rows, C, nx)
    rf = lr.row_factors(sizes, rng, nf)
    for bits in (None, lr.presence_bits(sizes, rng)):
        Tz = np.concatenate(lr.t_blocks(T, C, bits), axis=1)
        val = np.sum(lr.forward_ref(T, rf, W, trow, C, X, bits) * dO)
        dT = lr.backward_ref(dO, rf, W, trow, C, X)
        np.testing.assert_allclose(np.sum(Tz * dT), val, rtol=1e-10)
        dW, dX = lr.wgrad_ref(T, dO, rf, trow, C, nx, bits)
        np.testing.assert_allclose(np.sum(dW * W) + (np.sum(dX * X) if nx else 0.0), val, rtol=1e-10)
        # with skip_zero_grads the blocks that ARE stored are the same numbers wherever dO of an uncovered row is zero anyway
        if bits is not None:
            dOz = dO * bits[2][:, None]
            st = np.repeat(lr.stored_blocks(rows, bits, True), C, axis=1)
            a, b = lr.backward_ref(dO, rf, W, trow, C, X, bits, True), lr.backward_ref(dOz, rf, W, trow, C, X)
            assert np.array_equal(a[st], b[st]) and not st.all()


def test_error_measures_see_a_small_block_beside_a_large_one():
    ref = np.ones((3, 8))
    ref[:, 4:] = 1e6
    x = ref.copy()
    x[1, 2] += 1e-3
    assert abs(lr.row_block_err(x, ref, 4) - 1e-3) < 1e-12 and lr.row_block_err(x, ref, 8) < 1e-8
    keep = np.ones((3, 2), dtype=bool)
    keep[1, 0] = False
    assert lr.row_block_err(x, ref, 4, keep) == 0.0
    ref[2, :4] = 0
    x = ref.copy()
    x[2, 0] = 0.25
    assert lr.row_block_err(x, ref, 4) == 0.25
    w = np.ones((2, 4, 4))
    w[1, 3] = 1e-6
    y = w.copy()
    y[1, 3, 0] += 1e-9
    assert abs(lr.wgrad_row_err(y, w) - 1e-3) < 1e-9
