"""Plain numpy reference of the operations of SMP_2D_ver5's level that gf_smp_2d_ver5_{rows,cols,wgrad}_ex_f32 run on the device
(smp_level_2d_ver5.hip: v5_row_proj, v5_col_proj, v5_wgrad / v5_wgrad_fold), the error measures of tests/test_smp_2d_ver5_ops_gpu.py
and its operands.  With K [C][2 C] = [K1 | K2] and the size entries (lambda1_s | lambda2_s | b_s) of 3 C values:

  rows forward    f  = lrelu((lambda1_s(row) . S[row]) K1^T + u[col(row)])        cols forward    u  = (lambda2_s . col) K2^T + b_s
  rows backward   dE = dz K1                                                      cols backward   dO = cz K2
  dK1 = sum_rows dz^T (lambda1_s . S)                                             dK2 = sum_cols cz^T (lambda2_s . col)

Every function takes `dt`: float64 is the reference, float32 the evaluation that shows what a correct fp32 kernel can reach.

The measure is per output row (per row c' of a half of dK): max_o |x - ref| over the row's MAGNITUDE SUM, the same product evaluated
on absolute values (forward: times the slope of the reference's branch, maximum over the row).  Not over max |ref| of the row: with five
outputs per row some row has every output cancelling, and a correct fp32 evaluation then reaches 1.2e-5 .. 1.4e-5 of max |ref| (C = 5 ..
8, 22,000 rows, eight seeds) where it is 1.9e-7 (C = 5) .. 3.2e-7 (C = 128) of the magnitude sum.  A misplaced element is wrong by the
order of the magnitude itself.

tests/test_smp_2d_ver5.py ties these formulas to the real class: composed on a golden molecule's S, col and dz they reproduce the
level's f_l and the dK_l block of the golden gradient at 1e-9."""
import numpy as np

ALPHA = 0.01


def level_tables(node_sizes):
    """row_cs [sum s^2][2] = (column, s) and col_s [sum s] of a level of nodes with these sizes: node n owns s^2 consecutive rows (i, j)
    and s consecutive columns j, as v5_store_S writes them"""
    row_cs, col_s, c0 = [], [], 0
    for s in node_sizes:
        j = np.arange(s * s) % s
        row_cs.append(np.stack([c0 + j, np.full(s * s, s)], axis=1))
        col_s.append(np.full(s, s))
        c0 += s
    return np.concatenate(row_cs).astype(np.int32), np.concatenate(col_s).astype(np.int32)


def _halves(K, dt):
    Cn = K.shape[0]
    assert K.shape == (Cn, 2 * Cn)
    K = np.asarray(K, dtype=dt)
    return K[:, :Cn], K[:, Cn:]


def _entry(sizes, s, part, dt):
    """lambda1 (part 0), lambda2 (1) or b (2) of the sizes s, one row each"""
    Cn = np.shape(sizes)[1] // 3
    return np.asarray(sizes, dtype=dt)[:, part * Cn:(part + 1) * Cn][np.asarray(s) - 1]


def rows_forward(K, X, sizes, u, row_cs, alpha=ALPHA, dt=np.float64, magnitude=False):
    """(f, z); magnitude: (mag, None) with mag = |lambda1 X| |K1|^T + |u|"""
    K1, _ = _halves(K, dt)
    x = _entry(sizes, row_cs[:, 1], 0, dt) * np.asarray(X, dtype=dt)
    ub = np.asarray(u, dtype=dt)[row_cs[:, 0]]
    if magnitude:
        return np.abs(x) @ np.abs(K1).T + np.abs(ub), None
    z = x @ K1.T + ub
    return np.where(z > 0, z, dt(alpha) * z), z


def rows_backward(K, dz, dt=np.float64, magnitude=False):
    K1, _ = _halves(K, dt)
    dz = np.asarray(dz, dtype=dt)
    return np.abs(dz) @ np.abs(K1) if magnitude else dz @ K1


def cols_forward(K, col, sizes, col_s, dt=np.float64, magnitude=False):
    _, K2 = _halves(K, dt)
    l2, b = _entry(sizes, col_s, 1, dt), _entry(sizes, col_s, 2, dt)
    x = l2 * np.asarray(col, dtype=dt)
    return np.abs(x) @ np.abs(K2).T + np.abs(b) if magnitude else x @ K2.T + b


def cols_backward(K, cz, dt=np.float64, magnitude=False):
    _, K2 = _halves(K, dt)
    cz = np.asarray(cz, dtype=dt)
    return np.abs(cz) @ np.abs(K2) if magnitude else cz @ K2


def wgrad(dz, S, row_cs, cz, col, col_s, sizes, dt=np.float64, magnitude=False):
    """dK [C][2 C] = (dK1 | dK2) (what the operator ADDS to its dK)"""
    a = _entry(sizes, row_cs[:, 1], 0, dt) * np.asarray(S, dtype=dt)
    b = _entry(sizes, col_s, 1, dt) * np.asarray(col, dtype=dt)
    dz, cz = np.asarray(dz, dtype=dt), np.asarray(cz, dtype=dt)
    if magnitude:
        return np.concatenate([np.abs(dz).T @ np.abs(a), np.abs(cz).T @ np.abs(b)], axis=1)
    return np.concatenate([dz.T @ a, cz.T @ b], axis=1)


def row_err(x, ref, den):
    """the largest per-row error: max_o |x - ref| over the row's denominator (one value per row)"""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape and den.shape == ref.shape[:1] and np.all(den > 0), (x.shape, ref.shape, den.shape)
    return float((np.abs(x - ref).max(axis=1) / den).max())


def forward_den(mag, z, alpha=ALPHA):
    """max_o (slope_o mag_o) per row, slope by the reference's branch"""
    return (np.where(z > 0, 1.0, alpha) * mag).max(axis=1)


def half_err(dK, ref, mag):
    """(error of the dK1 half, of the dK2 half), per row c' of the half"""
    Cn = ref.shape[0]
    return tuple(row_err(dK[:, h], ref[:, h], mag[:, h].max(axis=1)) for h in (slice(0, Cn), slice(Cn, 2 * Cn)))


class Level:
    """The operands of one level of nodes `node_sizes` at C channels, as float32 arrays: S, dz [rows][C] and col, cz [cols][C] of O(1)
    entries whose scale wanders over two decades from row to row (exp(uniform(-2.3, 2.3))), K and the size entries uniform(-1, 1), cz
    inside rows of `ldcz` floats, u = the fp64 column projection of col rounded to fp32 and then nudged: an element that leaves a
    pre-activation within 1e-3 of its magnitude sum of zero moves by 4e-3 of it in the direction of its own sign, until none is left
    (fp32 and fp64 then take the same LeakyReLU branch).  loud: the index of a node whose rows and columns are 1e4 times the rest."""

    MARGIN, NUDGE = 1e-3, 4e-3

    def __init__(self, node_sizes, Cn, seed, ldcz=None, loud=None):
        rng = np.random.default_rng(seed)
        self.C, self.node_sizes = Cn, list(node_sizes)
        self.nsizes = max(node_sizes)
        self.row_cs, self.col_s = level_tables(node_sizes)
        self.rows, self.cols = rows, cols = len(self.row_cs), len(self.col_s)
        self.ldcz = ldcz or Cn

        def operand(n):
            return rng.standard_normal((n, Cn), dtype=np.float32) * np.exp(rng.uniform(-2.3, 2.3, (n, 1))).astype(np.float32)

        S, dz, col, cz = operand(rows), operand(rows), operand(cols), operand(cols)
        if loud is not None:
            r0 = sum(s * s for s in node_sizes[:loud])
            c0 = sum(node_sizes[:loud])
            s = node_sizes[loud]
            self.loud_rows = np.zeros(rows, dtype=bool)
            self.loud_rows[r0:r0 + s * s] = True
            for a in (S, dz):
                a[r0:r0 + s * s] *= np.float32(1e4)
            for a in (col, cz):
                a[c0:c0 + s] *= np.float32(1e4)
        self.S, self.dz, self.col = S, dz, col
        self.cz_wide = rng.standard_normal((cols, self.ldcz)).astype(np.float32)   # (what lies between the rows of cz is never read)
        self.cz_wide[:, :Cn] = cz
        self.cz = self.cz_wide[:, :Cn]
        self.K = rng.uniform(-1, 1, (Cn, 2 * Cn)).astype(np.float32)
        self.sizes = rng.uniform(-1, 1, (self.nsizes, 3 * Cn)).astype(np.float32)
        self.dK0 = rng.uniform(-1, 1, (Cn, 2 * Cn)).astype(np.float32)   # what dK holds before the weight gradients are added
        u = cols_forward(self.K, self.col, self.sizes, self.col_s).astype(np.float32)
        _, zx = rows_forward(self.K, self.S, self.sizes, np.zeros_like(u), self.row_cs)   # (the product without u: computed once)
        magx, _ = rows_forward(self.K, self.S, self.sizes, np.zeros_like(u), self.row_cs, magnitude=True)
        for _ in range(10):
            ub = u.astype(np.float64)[self.row_cs[:, 0]]
            self.z, self.mag = zx + ub, magx + np.abs(ub)
            r, o = np.nonzero(np.abs(self.z) < self.MARGIN * self.mag)
            if r.size == 0:
                break
            step = np.zeros(u.shape)
            np.maximum.at(step, (self.row_cs[r, 0], o), self.NUDGE * self.mag[r, o])
            u = (u + np.where(u >= 0, step, -step)).astype(np.float32)
        self.u = u

    # -- the fp64 references (computed once each) with their denominators, and the conditions on the inputs ---------------------------
    OPS = ("rows_fwd", "rows_bwd", "cols_fwd", "cols_bwd", "wgrad")

    def _eval(self, op, **kw):
        if op == "rows_fwd":
            return rows_forward(self.K, self.S, self.sizes, self.u, self.row_cs, **kw)
        if op == "rows_bwd":
            return rows_backward(self.K, self.dz, **kw)
        if op == "cols_fwd":
            return cols_forward(self.K, self.col, self.sizes, self.col_s, **kw)
        if op == "cols_bwd":
            return cols_backward(self.K, self.cz, **kw)
        assert op == "wgrad"
        return wgrad(self.dz, self.S, self.row_cs, self.cz, self.col, self.col_s, self.sizes, **kw)

    def ref(self, op):
        """(fp64 result, denominators): one per row; for "wgrad" the result is dK0 + dK and the second entry the magnitude image"""
        cache = self.__dict__.setdefault("_ref", {})
        if op not in cache:
            if op == "rows_fwd":
                cache[op] = (np.where(self.z > 0, self.z, ALPHA * self.z), forward_den(self.mag, self.z))
            elif op == "wgrad":
                cache[op] = (self.dK0.astype(np.float64) + self._eval(op), np.abs(self.dK0).astype(np.float64) + self._eval(op, magnitude=True))
            else:
                cache[op] = (self._eval(op), self._eval(op, magnitude=True).max(axis=1))
        return cache[op]

    def err(self, op, got):
        """the measure of `got` (dK: the worse half)"""
        return max(half_err(got, *self.ref(op))) if op == "wgrad" else row_err(got, *self.ref(op))

    def check_conditions(self, tol, ops=OPS):
        """asserted on the reference alone: a numpy float32 evaluation of each operation holds tol / 2 by the same measure; no forward
        pre-activation within MARGIN of zero; both LeakyReLU branches occur (a tenth of the elements at least on each side)"""
        e = {}
        for op in ops:
            x = self._eval(op, dt=np.float32)
            e[op] = self.err(op, self.dK0 + x if op == "wgrad" else x[0] if op == "rows_fwd" else x)
        assert all(v <= tol / 2 for v in e.values()), e
        if "rows_fwd" in ops:
            assert not (np.abs(self.z) < self.MARGIN * self.mag).any()
            pos = float((self.z > 0).mean())
            assert 0.1 <= pos <= 0.9, pos
        return e
