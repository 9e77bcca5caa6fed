"""splitk_reduce (mixers.hip), the ordered fold of a split-K product's partial images, bit for bit against the same sums in numpy, through
the product that level 0's weight gradient is: dH [64][30] (+)= dZ^T X over nV rows (gf.matmul_backward's dB).  The operands are built so
that every partial image is EXACT in float32 -- one non-zero row per split, integer mantissas of 11 bits -- and of magnitudes 2^-10 .. 2^10
apart, so the only rounding is the fold's and any other order, chunking or tail gives other bits.  Then the product itself against fp64 at
the row-magnitude measure, at the row counts that take gemm()'s unsplit, threshold and two-pass routes."""
import numpy as np
import pytest

from field_suite import dev

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

C, FD = 64, 30      # level 0 of cfg3: M = C, N = F (D + 1), one 128 x 64 output tile
BK = 32             # gemm_lds.h
TOL_GRAD = 1e-5     # the golden / parity suites' bound on a gradient block (tests/test_smp_gpu.py)


def split_plan(K):
    """(splits, kchunk) of gemm() for one output tile and K rows: no split below 8 BK rows, at least eight k-steps per split"""
    splits = 1
    if K >= 8 * BK:
        splits = max(1, min(2048, K // (8 * BK)))
    kchunk = -(-(-(-K // splits)) // BK) * BK
    return -(-K // kchunk), kchunk


def ordered_sum(parts):
    s = np.zeros_like(parts[0])
    for p in parts:
        s = s + p
    return s


def fold(parts, old):
    """splitk_reduce as gemm() launches it: up to 64 images in one pass, more in chunks of 32 and then the chunks, all in order"""
    if len(parts) > 64:
        parts = [ordered_sum(parts[c:c + 32]) for c in range(0, len(parts), 32)]
    s = ordered_sum(parts)
    return s if old is None else old + s


# rows -> split count: 256 is the unsplit product (no fold launch), 16,793 the cfg3 batch (59 splits, a short last one)
CASES = {256: 1, 512: 2, 1280: 5, 4096: 16, 4352: 17, 15104: 59, 16793: 59, 16384: 64, 16640: 65, 25600: 100}


def test_cases_take_the_split_counts_they_name():
    assert {K: split_plan(K)[0] for K in CASES} == CASES
    assert split_plan(255)[0] == 1 and split_plan(16793) == (59, 288)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("K", sorted(CASES))
def test_split_k_fold_is_the_ordered_sum_of_its_images(gf, K, accumulate):
    splits, kchunk = split_plan(K)
    rng = np.random.default_rng(K + accumulate)
    A, X, parts = np.zeros((K, C), dtype=np.float32), np.zeros((K, FD), dtype=np.float32), []
    for s in range(splits):
        r = int(rng.integers(s * kchunk, min((s + 1) * kchunk, K)))
        A[r] = rng.integers(-2047, 2048, C) * 2.0 ** int(rng.integers(-10, 11))
        X[r] = rng.integers(-2047, 2048, FD)
        p = np.outer(A[r], X[r])
        assert np.array_equal(p.astype(np.float64), np.outer(A[r].astype(np.float64), X[r].astype(np.float64)))   # exact in float32
        parts.append(p)
    old = rng.normal(0, 2.0 ** 8, (C, FD)).astype(np.float32) if accumulate else None
    dB = dev(old) if accumulate else torch.full((C, FD), float("nan"), device="cuda")
    gf.matmul_backward(dev(X), dev(A), torch.empty((C, FD), device="cuda"), dB=dB, accumulate=bool(accumulate))
    got, expect = dB.cpu().numpy(), fold(parts, old)
    assert expect.dtype == np.float32 and np.abs(expect).max() > 0
    if splits > 2:   # (the order matters for these operands: summed the other way round, some element differs)
        assert not np.array_equal(fold(parts[::-1], old), expect)
    assert np.array_equal(got, expect), (splits, np.abs(got.astype(np.float64) - expect).max())


@pytest.mark.parametrize("nV", [3, 257, 20000])
def test_level0_weight_gradient_against_fp64(gf, nV):
    """dH = dZ^T X at 3 rows (one k-step), 257 (past the split threshold of 8 BK rows, still one image) and 20,000 (70 images: the
    two-pass fold), each output row's largest error over the row's largest magnitude sum |dZ|^T |X|"""
    rng = np.random.default_rng(nV)
    dZ = rng.normal(0, 1, (nV, C)).astype(np.float32)
    X = rng.integers(0, 5, (nV, FD)).astype(np.float32)   # shell sums of one-hot features
    dH = torch.zeros((C, FD), device="cuda")
    gf.matmul_backward(dev(X), dev(dZ), torch.empty((C, FD), device="cuda"), dB=dH, accumulate=True)
    ref = dZ.astype(np.float64).T @ X.astype(np.float64)
    mag = np.abs(dZ.astype(np.float64)).T @ np.abs(X.astype(np.float64))
    err = (np.abs(dH.cpu().numpy() - ref).max(axis=1) / np.maximum(mag.max(axis=1), 1e-300)).max()
    print("dH nV=%d: row-magnitude error %.3e" % (nV, err))
    assert split_plan(nV)[0] == {3: 1, 257: 1, 20000: 70}[nV]
    assert err <= TOL_GRAD
