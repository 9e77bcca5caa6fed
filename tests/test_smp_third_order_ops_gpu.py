"""The two kernels of the third-order pool one by one (gf_smp_third_order_pool_fwd_ex_f32 / _bwd_ex_f32: third_pool_fwd and third_pool_bwd
of smp_level_third.hip, through the level's own launchers) against the fp64 restatement of the same operands
(tests/third_order_ref.py: pool, pool_backward), per vertex.  The operands are built and checked for the gap condition on the CPU
(tests/test_smp_third_order.py: ops_case).  n and dhprev meet the restatement at field_suite.TOL = 1e-5 (tests/util.py: rel_err) per
vertex; sel is exactly the restatement's multiset of canonical triples per vertex, in rank order; a list under three members gives n = 0,
sel = -1 and no contribution.  Every output lies in a buffer with sentinel rows behind its last row."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import field_suite as kit
from field_suite import TOL, dev
from test_smp_third_order import OPS_KINDS, OPS_WIDTHS, ops_case
from util import rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 12345.0
TAIL_ROWS = 3
INVALID = 1


def ptr(t):
    return C.c_void_p(t.data_ptr())


def context():
    from graphflow_amd.ops import default_context
    return default_context(0)


def guarded(rows, width, dtype=torch.float32):
    return torch.full(((rows + TAIL_ROWS) * width,), SENTINEL, device="cuda").to(dtype)


def taken(t, rows, width):
    a = t.cpu().numpy()
    assert np.all(a[rows * width:] == a.dtype.type(SENTINEL)), "wrote behind the last row"
    return a[:rows * width].reshape(rows, width)


def forward(c, status=False, **over):
    """(n [nV, H] float32, sel [nV, H] int32) of the device, or the status with `status`"""
    ctx = context()
    n, sel = guarded(c.nV, c.H), guarded(c.nV, c.H, torch.int32)
    a = dict(H=c.H, nV=c.nV, ptr=dev(c.ptr, np.int64), idx=dev(c.idx, np.int32), hprev=dev(c.hprev))
    a.update({k: (v if isinstance(v, int) else dev(v, v.dtype)) for k, v in over.items()})
    st = ctx.lib.gf_smp_third_order_pool_fwd_ex_f32(ctx.handle, a["H"], a["nV"], ptr(a["ptr"]), ptr(a["idx"]), ptr(a["hprev"]), ptr(n), ptr(sel))
    torch.cuda.synchronize()
    if status:
        return st, taken(n, c.nV, c.H), taken(sel, c.nV, c.H)
    ctx.check(st)
    return taken(n, c.nV, c.H), taken(sel, c.nV, c.H)


def backward(c, sel, status=False, **over):
    """dhprev [nV, H] float32 of the device from the restatement's dn and the given selection record"""
    ctx = context()
    out = guarded(c.nV, c.H)
    a = dict(H=c.H, nV=c.nV, ptr=dev(c.ptr, np.int64), idx=dev(c.idx, np.int32), tptr=dev(c.tptr, np.int64), tidx=dev(c.tidx, np.int32),
             hprev=dev(c.hprev), sel=dev(sel, np.int32), dn=dev(c.dn))
    a.update({k: (v if isinstance(v, int) else dev(v, v.dtype)) for k, v in over.items()})
    st = ctx.lib.gf_smp_third_order_pool_bwd_ex_f32(ctx.handle, a["H"], a["nV"], ptr(a["ptr"]), ptr(a["idx"]), ptr(a["tptr"]), ptr(a["tidx"]),
                                                    ptr(a["hprev"]), ptr(a["sel"]), ptr(a["dn"]), ptr(out))
    torch.cuda.synchronize()
    if status:
        return st, taken(out, c.nV, c.H)
    ctx.check(st)
    return taken(out, c.nV, c.H)


def unpack(sel):
    """[nV, H, 3]: the triple per rank, -1 where the record is -1"""
    s = sel.astype(np.int64)
    t = np.stack([s & 255, (s >> 8) & 255, (s >> 16) & 255], axis=-1)
    t[s < 0] = -1
    return t


@pytest.mark.parametrize("kind", OPS_KINDS)
@pytest.mark.parametrize("H", OPS_WIDTHS)
def test_operators_meet_the_restatement(gf, H, kind):
    """H = 1, 2, 5, 8, 9, 16, 17, 32, 33, 64; lists of 1, 2, 3, 4, 7 and 29 members in one batch of 40 vertices, with and without the
    vertex itself, a source without a consumer, three equal members; softmax- and tanh-valued.  At H = 2 and 5 the cut falls inside a
    class of 3 or 6."""
    c = ops_case(H, kind)
    n, sel = forward(c)
    triples = unpack(sel)
    worst_n = worst_d = 0.0
    for v, mem in enumerate(c.lists):
        if len(mem) < 3:
            assert not n[v].any() and (sel[v] == -1).all(), v
            continue
        worst_n = max(worst_n, rel_err(n[v], c.n[v]))
        assert np.all(np.diff(n[v]) >= 0), v                         # ascending: n[H - 1] the largest
        assert np.all(triples[v][:, 0] <= triples[v][:, 1]) and np.all(triples[v][:, 1] <= triples[v][:, 2]) and triples[v].max() < H, v
        assert sorted(map(tuple, triples[v])) == sorted(map(tuple, c.sel[v])), v   # the same classes, each as often
        assert np.array_equal(triples[v], c.sel[v]), v                # ... and rank by rank (no two classes tie: the gap condition)
    d = backward(c, sel)
    for w in range(c.nV):
        worst_d = max(worst_d, rel_err(d[w], c.dh[w]))
    print("H = %d, %s: n within %.3g, dhprev within %.3g per vertex (smallest gap %.3g)" % (H, kind, worst_n, worst_d, c.gap))
    assert worst_n <= TOL and worst_d <= TOL
    assert not d[39].any() and np.abs(c.dh).max() > 0 and np.abs(c.n).max() > 0   # the source without a consumer
    # a consumer under three members hands nothing back: with every other dn at zero the result is zero
    small = np.array([len(m) < 3 for m in c.lists])
    only_small = OpsCaseView(c, dn=np.where(small[:, None], c.dn, 0.0))
    assert not backward(only_small, sel).any()


class OpsCaseView:
    """a case with some operands replaced"""

    def __init__(self, c, **over):
        self.__dict__.update(c.__dict__)
        self.__dict__.update(over)


def digest(H, kind):
    c = ops_case(H, kind)
    n, sel = forward(c)
    d = backward(c, sel)
    return hashlib.sha256(n.tobytes() + sel.tobytes() + d.tobytes()).hexdigest()


BITS = [(5, "softmax"), (33, "tanh"), (64, "softmax")]


def test_two_runs_give_the_same_bits(gf):
    """n, sel and dhprev of two runs, bit for bit; in the child process of test_parity_under_poison also the bits of the parent's run"""
    first = [digest(H, kind) for H, kind in BITS]
    assert first == [digest(H, kind) for H, kind in BITS]
    if os.environ.get("GF_THIRD_ORDER_OPS_BITS"):
        assert ",".join(first) == os.environ["GF_THIRD_ORDER_OPS_BITS"]


def test_parity_under_poison(gf, monkeypatch):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns): neither kernel reads memory nobody wrote,
    and the outputs are the bits of this process's run"""
    monkeypatch.setenv("GF_THIRD_ORDER_OPS_BITS", ",".join(digest(H, kind) for H, kind in BITS))
    kit.run_under_poison(__file__, "same_bits or (meets_the_restatement and (5- or 64-))")


def test_refusals_leave_the_context_usable(gf):
    """H = 65, a list index out of range, a list that decreases, a selection record that is no triple: GF_ERR_INVALID before anything is
    launched, the outputs untouched, and the next call works"""
    c = ops_case(8, "tanh")
    ctx = context()

    def refused(result, text):
        st, *outs = result
        assert st == INVALID and text in ctx.lib.gf_last_error(ctx.handle), ctx.lib.gf_last_error(ctx.handle)
        for o in outs:
            assert np.all(o == o.dtype.type(SENTINEL))
        n, sel = forward(c)
        assert rel_err(n, c.n) <= TOL

    bad_idx = c.idx.copy()
    bad_idx[7] = c.nV
    refused(forward(c, status=True, H=65), b"65 channels (1 .. 64)")
    refused(forward(c, status=True, idx=bad_idx), b"outside [0, 40)")
    bad_idx[7] = -1
    refused(forward(c, status=True, idx=bad_idx), b"outside [0, 40)")
    bad_ptr = c.ptr.copy()
    bad_ptr[3] = bad_ptr[2] - 1
    refused(forward(c, status=True, ptr=bad_ptr), b"decreases")
    sel = np.where(c.sel[..., 0] < 0, -1, c.sel[..., 0] | (c.sel[..., 1] << 8) | (c.sel[..., 2] << 16)).astype(np.int32)
    refused(backward(c, sel, status=True, H=65), b"65 channels (1 .. 64)")
    refused(backward(c, sel, status=True, idx=bad_idx), b"outside [0, 40)")
    bad_t = c.tidx.copy()
    bad_t[0] = c.nV
    refused(backward(c, sel, status=True, tidx=bad_t), b"outside [0, 40)")
    bad_sel = sel.copy()
    bad_sel[np.argmax(sel[:, 0] >= 0), 1] = 8 | (8 << 8) | (8 << 16)   # channel 8 of 8
    refused(backward(c, bad_sel, status=True), b"is no triple")
    assert rel_err(backward(c, sel), c.dh) <= TOL
