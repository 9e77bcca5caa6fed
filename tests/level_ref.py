"""fp64 reference of the fused level's block products in every variant the kernels of smp_level_c64_split.hip have, and generators
of level-shaped operands for them (tests/test_level_ops_ex_gpu.py; checked on the CPU by tests/test_level_ref_cpu.py).

Blocks are C columns wide:  T = [S_ab | S_bc | T6 | T10] (4 C),  O / dO = [O_loc | U] = [L | dU] (2 C),  W [8][C][C],  X [3][C][C].
Row factors f[row][p] of the stacked products p = 0..7: nf = 2 rows (tot, tr) stand for (tot, tot, tr, 1, 1, 1, 1, 1), nf = 8 rows are
the eight factors themselves (the plain ones times the node's slice-dropout factors, in the order written above smp_rowpanel_split).

    forward    O_loc = f0 S_ab W0 + f1 S_bc W1 + f2 S_ab W2 + f3 T6 W3 + f4 T10 W4  [+ S_ab X_a + S_bc X_b + f2 S_bc X_c]
               U     = f5 S_ab W5 + f6 S_bc W6 + f7 S_ab[trow] W7
    backward   dS_ab = f0 L W0^T + f2 L W2^T + f5 dU W5^T + (f7 dU)[trow] W7^T       [+ L X_a^T]
               dS_bc = f1 L W1^T + f6 dU W6^T                                         [+ L X_b^T + f2 L X_c^T]
               dT6   = f3 L W3^T,   dT10 = f4 L W4^T
    wgrad      dW_p  = (T block of p)^T (f_p x (L | dU | dU[trow]))                   [dX = S_ab^T L, S_bc^T L, S_bc^T (f2 L)]

Presence bits (the packed table, include/gf_hip.h): bit 31 = the row's S_ab / T6 blocks hold data, bit 30 = the transposed row's do,
bit 29 = the row's S_bc / T10 blocks do.  A block whose bit is clear counts as zero whatever the matrix holds there."""
import numpy as np

ROW_MASK = 0x1FFFFFFF
# the eight products' operand blocks: block of T, block of dO (0 = L, 1 = dU, 2 = dU at the transposed rows)
A_BLOCK = (0, 1, 0, 2, 3, 0, 1, 0)
B_BLOCK = (0, 0, 0, 0, 0, 1, 1, 2)


# ---- tables ------------------------------------------------------------------------------------------------------------------

def level_rows(sizes):
    """A level whose nodes have sizes[i] positions and sizes[i]^2 rows each, back to back: (trow, node of every row).  trow is the
    transposition (x, e) <-> (e, x) inside each node."""
    trow, node, r0 = [], [], 0
    for n, s in enumerate(sizes):
        i = np.arange(s * s)
        trow.append(r0 + (i % s) * s + i // s)
        node.append(np.full(s * s, n))
        r0 += s * s
    return np.concatenate(trow).astype(np.int32), np.concatenate(node)


def presence_bits(sizes, rng):
    """(own, trp, bc) per row, drawn the way the level's table builder derives them: P[x][e] = position e lies in the field of x's
    source (drawn per row, at a density drawn per node so that sparse and dense fields both occur; P[x][x] always), own(x, e) =
    P[x][e], trp = own of the transposed row, bc(b, c) = some source holds both b and c.  Hence bit 30 of a row is bit 31 of its transposed row, bit 31 implies bit 29, and bit 29 is symmetric."""
    own, trp, bc = [], [], []
    for s in sizes:
        P = rng.random((s, s)) < rng.uniform(0.1, 0.7)
        P[np.arange(s), np.arange(s)] = True
        Pi = P.astype(np.int64)
        own.append(P.reshape(-1))
        trp.append(P.T.reshape(-1))
        bc.append(((Pi.T @ Pi) > 0).reshape(-1))
    return np.concatenate(own), np.concatenate(trp), np.concatenate(bc)


def all_present(rows):
    one = np.ones(rows, dtype=bool)
    return one, one, one


def pack(trow, bits):
    own, trp, bc = bits
    w = trow.astype(np.uint32) | (own.astype(np.uint32) << 31) | (trp.astype(np.uint32) << 30) | (bc.astype(np.uint32) << 29)
    return w.view(np.int32)


def unpack(trowf):
    w = np.asarray(trowf).view(np.uint32)
    return (w & ROW_MASK).astype(np.int32), ((w >> 31) & 1).astype(bool), ((w >> 30) & 1).astype(bool), ((w >> 29) & 1).astype(bool)


def row_factors(sizes, rng, nf):
    """(tot, tr) of every row's node; nf = 8: (tot, tot, tr, 1, 1, 1, 1, 1) times a random 0 / 1 mask per node (what slice dropout gives)"""
    n = len(sizes)
    tot, tr = rng.uniform(1, 29, n), rng.uniform(1, 6, n)
    if nf == 2:
        per = np.stack([tot, tr], axis=1)
    else:
        one = np.ones(n)
        per = np.stack([tot, tot, tr, one, one, one, one, one], axis=1) * rng.integers(0, 2, (n, 8))
    return np.repeat(per, [s * s for s in sizes], axis=0).astype(np.float32)


def fill_absent(T, C, bits, rng):
    """a copy of T whose absent blocks hold finite garbage of the operand's own magnitude (a kernel that reads one fails)"""
    own, _, bc = bits
    T = np.array(T, dtype=np.float32)
    scale = float(np.sqrt(np.mean(np.square(T, dtype=np.float64)))) or 1.0
    for blk, have in ((0, own), (1, bc), (2, own), (3, bc)):
        gone = np.flatnonzero(~have)
        T[gone, blk * C:(blk + 1) * C] = (3.0 * scale * rng.standard_normal((gone.size, C))).astype(np.float32)
    return T


# ---- the reference -----------------------------------------------------------------------------------------------------------

def factors8(rf):
    rf = np.asarray(rf, dtype=np.float64)
    if rf.shape[1] == 8:
        return rf
    one = np.ones(rf.shape[0])
    return np.stack([rf[:, 0], rf[:, 0], rf[:, 1], one, one, one, one, one], axis=1)


def t_blocks(T, C, bits):
    """the four blocks of T in fp64, absent ones zeroed"""
    T = np.asarray(T, dtype=np.float64)
    blk = [T[:, C * i:C * i + C] for i in range(4)]
    if bits is not None:
        own, _, bc = bits
        blk = [b * (own if i in (0, 2) else bc)[:, None] for i, b in enumerate(blk)]
    return blk


def forward_ref(T, rf, W, trow, C=64, X=None, bits=None):
    W = np.asarray(W, dtype=np.float64)
    f = factors8(rf)[:, :, None]
    Sab, Sbc, T6, T10 = t_blocks(T, C, bits)
    oloc = f[:, 0] * (Sab @ W[0]) + f[:, 1] * (Sbc @ W[1]) + f[:, 2] * (Sab @ W[2]) + f[:, 3] * (T6 @ W[3]) + f[:, 4] * (T10 @ W[4])
    if X is not None:
        X = np.asarray(X, dtype=np.float64)
        oloc = oloc + Sab @ X[0] + Sbc @ X[1] + f[:, 2] * (Sbc @ X[2])
    u = f[:, 5] * (Sab @ W[5]) + f[:, 6] * (Sbc @ W[6]) + f[:, 7] * (Sab[trow] @ W[7])
    return np.concatenate([oloc, u], axis=1)


def backward_ref(dO, rf, W, trow, C=64, X=None, bits=None, skip_zero_grads=False):
    """dT [rows][4 C].  With the packed table and skip_zero_grads, dO of a row no source covers (bit 29 clear) counts as zero; which
    blocks the kernel then leaves unwritten: stored_blocks()."""
    dO = np.array(dO, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    f = factors8(rf)[:, :, None]
    if bits is not None and skip_zero_grads:
        dO = dO * bits[2][:, None]
    L, dU = dO[:, :C], dO[:, C:]
    dSab = f[:, 0] * (L @ W[0].T) + f[:, 2] * (L @ W[2].T) + f[:, 5] * (dU @ W[5].T) + (f[:, 7] * dU)[trow] @ W[7].T
    dSbc = f[:, 1] * (L @ W[1].T) + f[:, 6] * (dU @ W[6].T)
    if X is not None:
        X = np.asarray(X, dtype=np.float64)
        dSab = dSab + L @ X[0].T
        dSbc = dSbc + L @ X[1].T + f[:, 2] * (L @ X[2].T)
    return np.concatenate([dSab, dSbc, f[:, 3] * (L @ W[3].T), f[:, 4] * (L @ W[4].T)], axis=1)


def stored_blocks(rows, bits=None, skip_zero_grads=False):
    """[rows][4]: the blocks of dT the backward kernel writes (dS_ab and dT6 of a row without bit 31 are skipped on request)"""
    st = np.ones((rows, 4), dtype=bool)
    if bits is not None and skip_zero_grads:
        st[:, 0] = st[:, 2] = bits[0]
    return st


def wgrad_ref(T, dO, rf, trow, C=64, nx=0, bits=None):
    """(dW [8][C][C], dX [3][C][C] or None)"""
    dO = np.asarray(dO, dtype=np.float64)
    f = factors8(rf)
    A = t_blocks(T, C, bits)
    L, dU = dO[:, :C], dO[:, C:]
    dW = []
    for p in range(8):
        fp = f[:, p:p + 1]
        B = fp * L if B_BLOCK[p] == 0 else fp * dU if B_BLOCK[p] == 1 else (fp * dU)[trow]
        dW.append(A[A_BLOCK[p]].T @ B)
    dX = np.stack([A[0].T @ L, A[1].T @ L, A[1].T @ (f[:, 2:3] * L)]) if nx == 3 else None
    return np.stack(dW), dX


# ---- error measures ----------------------------------------------------------------------------------------------------------

def row_block_err(x, ref, width, keep=None):
    """max over (row, block of `width` columns) of max|x - ref| / max|ref| inside that block of the row (a block whose reference is
    all zero: absolute).  keep [rows][blocks]: the blocks that count."""
    rows = ref.shape[0]
    d = np.abs(np.asarray(x, dtype=np.float64) - ref).reshape(rows, -1, width).max(axis=2)
    m = np.abs(ref).reshape(rows, -1, width).max(axis=2)
    e = d / np.where(m > 0, m, 1.0)
    if keep is not None:
        e = np.where(keep, e, 0.0)
    return float(e.max()) if e.size else 0.0


def wgrad_row_err(x, ref):
    """max over (block, row of dW) of max|x - ref| / max|ref| along that row (all-zero rows: absolute)"""
    d = np.abs(np.asarray(x, dtype=np.float64) - ref).max(axis=-1)
    m = np.abs(ref).max(axis=-1)
    return float((d / np.where(m > 0, m, 1.0)).max())
