"""The two products of the row-list GEMM level (smp_level_rowlist.hip) as stand-alone operators -- gf_smp_rowlist_product_ex_f32 and
gf_smp_rowlist_wgrad_ex_f32 -- on synthetic lists against an fp64 numpy product per output row.  The operand is
A[r][slot Cin + c] = sum over the entries e of row r with that slot of coef[e] X[src[e]][c].  List kinds: "sequence" (k slots, one entry
each, coefficient 1: LCNN forward), "scattered" (k slots, any number of entries per slot including none, rows without entries, one
source row shared by many output rows: LCNN backward-data) and "weighted" (one slot, random coefficients: GCN_MW).  130 rows: more than
one 128-row tile and no multiple of it.  Inputs are float32-exact multiples of 1/64, so the fp64 reference sees what the device sees;
tolerance: the suite's 1e-5 (tests/util.py: rel_err), every output row checked on its own."""
import ctypes as C
import functools

import numpy as np
import pytest

from field_suite import TOL, dev
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

R, NX = 130, 57
KINDS = {"sequence": 3, "scattered": 4, "weighted": 1}   # slots
CINS, COUTS = (5, 16, 64), (8, 10, 64, 80)


@functools.lru_cache(maxsize=None)
def rowlist(kind):
    """(ptr, src, slot, coef or None) of R rows over NX source rows"""
    rng = np.random.default_rng(len(kind))
    slots = KINDS[kind]
    ptr, src, slot, coef = [0], [], [], []
    for r in range(R):
        if kind == "sequence":
            ent = [(s, int(rng.integers(0, NX))) for s in range(slots)]
        elif kind == "scattered":   # rows 0, 7, 14, .. are empty; slot 2 is empty in every odd row; up to four entries in a slot
            ent = [] if r % 7 == 0 else [(s, int(u)) for s in range(slots) if not (s == 2 and r % 2)
                                         for u in rng.integers(0, NX, int(rng.integers(1, 5)))]
            if r % 3 == 1:
                ent.append((0, 11))   # (source row 11 is shared by a third of the output rows)
            ent.sort(key=lambda e: e[0])
        else:
            ent = [(0, int(u)) for u in rng.choice(NX, size=int(rng.integers(0, 6)), replace=False)] + [(0, 11)] * (r % 2)
        src += [u for _, u in ent]
        slot += [s for s, _ in ent]
        coef += list(rng.integers(-64, 65, len(ent)) / 64.0) if kind == "weighted" else [1.0] * len(ent)
        ptr.append(len(src))
    lens = np.diff(ptr)
    assert kind == "sequence" or (lens == 0).any()
    assert src.count(11) > R // 4 or kind == "sequence"
    return (np.array(ptr, dtype=np.int64), np.array(src, dtype=np.int32), np.array(slot, dtype=np.int32),
            np.array(coef, dtype=np.float32) if kind == "weighted" else None)


def operand(kind, X):
    """A [R][slots Cin] in fp64"""
    ptr, src, slot, coef = rowlist(kind)
    Cin = X.shape[1]
    A = np.zeros((R, KINDS[kind] * Cin))
    for r in range(R):
        for e in range(ptr[r], ptr[r + 1]):
            A[r, slot[e] * Cin:(slot[e] + 1) * Cin] += (1.0 if coef is None else float(coef[e])) * X[src[e]]
    return A


def draw(rng, *shape):
    return (rng.integers(-64, 65, shape) / 64.0).astype(np.float32).astype(np.float64)


def device_list(kind):
    ptr, src, slot, coef = rowlist(kind)
    d = [dev(ptr, np.int64), dev(src, np.int32), dev(slot, np.int32), dev(coef) if coef is not None else None]
    return d, [C.c_void_p(t.data_ptr()) if t is not None else None for t in d]


def per_row(x, ref):
    """the largest rel_err over the rows, each against its own scale"""
    assert x.shape == ref.shape
    return max(rel_err(x[r], ref[r]) for r in range(len(ref)))


@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_product_per_row(gf, kind, Cin, Cout):
    """out = act(A B + bias): plain and LeakyReLU, with and without bias, B as [slots Cin][N] and read transposed slot by slot"""
    from graphflow_amd.ops import default_context
    ctx = default_context()
    slots, rng = KINDS[kind], np.random.default_rng(1000 * Cin + Cout)
    X, B, bias = draw(rng, NX, Cin), draw(rng, slots * Cin, Cout), draw(rng, Cout)
    A = operand(kind, X)
    keep, ptrs = device_list(kind)
    Xd, Bd, bd = dev(X), dev(B), dev(bias)
    Bt = dev(B.reshape(slots, Cin, Cout).transpose(0, 2, 1))   # [slots][N][Cin]
    for tb, act, with_bias in ((0, 0, True), (0, 1, True), (0, 1, False), (1, 0, False), (1, 1, True)):
        out = torch.full((R, Cout), float("nan"), device="cuda")
        ctx.check(ctx.lib.gf_smp_rowlist_product_ex_f32(ctx.handle, tb, R, slots, Cin, Cout, NX, *ptrs, C.c_void_p(Xd.data_ptr()),
                                                        C.c_void_p((Bt if tb else Bd).data_ptr()), C.c_void_p(bd.data_ptr()) if with_bias else None,
                                                        act, C.c_void_p(out.data_ptr())))
        z = A @ B + (bias if with_bias else 0.0)
        ref = np.where(z > 0, z, 0.01 * z) if act else z
        e = per_row(out.cpu().numpy().astype(np.float64), ref)
        print(kind, Cin, Cout, tb, act, with_bias, e)
        assert e <= TOL, (tb, act, with_bias)
        empty = np.flatnonzero(np.diff(rowlist(kind)[0]) == 0)
        if empty.size and not act:   # a row without entries is the bias alone, exactly
            assert np.array_equal(out.cpu().numpy()[empty], np.tile((bias if with_bias else np.zeros(Cout)).astype(np.float32), (empty.size, 1)))
    del keep


@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_weight_gradient_per_row(gf, kind, Cin, Cout):
    """dB += A^T dOut and db += the column sums of dOut, onto values the caller left there; two calls give the same bits"""
    from graphflow_amd.ops import default_context
    ctx = default_context()
    slots, rng = KINDS[kind], np.random.default_rng(2000 * Cin + Cout)
    X, dOut, dB0, db0 = draw(rng, NX, Cin), draw(rng, R, Cout), draw(rng, slots * Cin, Cout), draw(rng, Cout)
    A = operand(kind, X)
    keep, ptrs = device_list(kind)
    Xd, dOd = dev(X), dev(dOut)
    results = []
    for _ in range(2):
        dB, db = dev(dB0), dev(db0)
        ctx.check(ctx.lib.gf_smp_rowlist_wgrad_ex_f32(ctx.handle, R, slots, Cin, Cout, NX, *ptrs, C.c_void_p(Xd.data_ptr()),
                                                      C.c_void_p(dOd.data_ptr()), C.c_void_p(dB.data_ptr()), C.c_void_p(db.data_ptr())))
        results.append((dB.cpu().numpy(), db.cpu().numpy()))
    e = per_row(results[0][0].astype(np.float64), dB0 + A.T @ dOut)
    eb = rel_err(results[0][1].astype(np.float64), db0 + dOut.sum(axis=0))
    print(kind, Cin, Cout, e, eb)
    assert e <= TOL and eb <= TOL
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    dB = dev(dB0)   # (db is optional)
    ctx.check(ctx.lib.gf_smp_rowlist_wgrad_ex_f32(ctx.handle, R, slots, Cin, Cout, NX, *ptrs, C.c_void_p(Xd.data_ptr()), C.c_void_p(dOd.data_ptr()),
                                                  C.c_void_p(dB.data_ptr()), None))
    assert np.array_equal(dB.cpu().numpy(), results[0][0])
    del keep


def test_refusals_leave_the_context_usable(gf):
    """GF_ERR_INVALID before anything is launched: shapes, missing operands, and lists that would read out of bounds"""
    from graphflow_amd import _lib
    from graphflow_amd.ops import default_context
    ctx = default_context()
    lib = ctx.lib
    Cin, Cout, slots = 5, 8, KINDS["scattered"]
    rng = np.random.default_rng(3)
    X, B = draw(rng, NX, Cin), draw(rng, slots * Cin, Cout)
    ptr, src, slot, _ = rowlist("scattered")
    Xd, Bd, out = dev(X), dev(B), torch.zeros((R, Cout), device="cuda")

    def call(ptr_, src_, slot_, R_=R, slots_=slots, Cin_=Cin, N_=Cout, nX_=NX, X_=Xd):
        t = [dev(ptr_, np.int64), dev(src_, np.int32), dev(slot_, np.int32)]
        st = lib.gf_smp_rowlist_product_ex_f32(ctx.handle, 0, R_, slots_, Cin_, N_, nX_, *[C.c_void_p(x.data_ptr()) for x in t], None,
                                               C.c_void_p(X_.data_ptr()) if X_ is not None else None, C.c_void_p(Bd.data_ptr()), None, 0,
                                               C.c_void_p(out.data_ptr()))
        return st, lib.gf_last_error(ctx.handle)

    bad_src, bad_slot, unsorted, bad_ptr, late = src.copy(), slot.copy(), slot.copy(), ptr.copy(), ptr.copy()
    bad_src[5] = NX
    bad_slot[9] = slots
    e0 = int(ptr[1])
    unsorted[e0], unsorted[e0 + 1] = 3, 0   # (row 1 has entries in several slots)
    bad_ptr[4] = bad_ptr[3] - 1
    late[0] = 1
    for args, text in (((ptr, bad_src, slot), b"outside [0, 57)"), ((ptr, src, bad_slot), b"outside [0, 4)"),
                       ((ptr, src, unsorted), b"decrease"), ((bad_ptr, src, slot), b"ptr decreases"), ((late, src, slot), b"starts at 1"),
                       ((ptr, src, slot, 0), b"bad shape"), ((ptr, src, slot, R, slots, 65536), b"at most 65536"),
                       ((ptr, src, slot, R, slots, Cin, 65537), b"at most 65536"), ((ptr, src, slot, R, slots, Cin, Cout, NX, None), b"bad argument")):
        st, msg = call(*args)
        assert st == _lib.GF_ERR_INVALID and text in msg, (text, msg)
        st, msg = call(ptr, src, slot)
        assert st == _lib.GF_OK
    ref = operand("scattered", X) @ B
    assert per_row(out.cpu().numpy().astype(np.float64), ref) <= TOL
