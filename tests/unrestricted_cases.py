"""The batches the GPU suite of the unrestricted models (tests/test_smp_unrestricted_gpu.py) compares against tests/unrestricted_ref.py,
and their fp64 expectations -- computed once, on the host, so that the CPU suite can check the seeds the GPU suite will use.

Parameters come from the golden generator's random_params with fixed seeds; the 1e-3 margin on the restatement's pre-activations is
checked before anything is compared, and the next seed is taken where it fails (at most 8)."""
import ctypes as C

import numpy as np

import unrestricted_ref as uref
from inputs import synthetic_molecule, toy_molecules
from make_unrestricted_golden import random_params, unrestricted_blocks

FORM = {1: "1d", 2: "1d_ver2", 3: "2d"}
MARGIN = 1e-3
MAX_SEEDS = 8
LDS_FLOATS = 2048   # floats of S a workgroup of the first-order forward keeps in LDS (smp_level_unrestricted.hip: kUnLds)


def host_fields(mols, form, L, Cn, D, maxV):
    """phi[mol][l][v] from gf_smp_prepare_molecule_host"""
    from graphflow_amd import _lib
    from graphflow_amd.smp import SMPUnrestricted
    lib = _lib.load()
    out = []
    for adj, feat in mols:
        cfg = SMPUnrestricted.config(FORM[form], maxV, L, Cn, feat.shape[1], D, True)
        a, f = np.ascontiguousarray(adj, dtype=np.int32), np.ascontiguousarray(feat, dtype=np.float64)
        phi = np.zeros((L + 1, len(a), maxV + 1), dtype=np.int32)
        st = lib.gf_smp_prepare_molecule_host(C.byref(cfg), len(a), a.ctypes.data_as(C.POINTER(C.c_int)), f.ctypes.data_as(C.POINTER(C.c_double)),
                                              phi.ctypes.data_as(C.POINTER(C.c_int)), None)
        assert st == 0
        out.append(uref.fields_of(phi))
    return out


def packing_batch():
    """70 molecules: the four toy molecules 17 times (their features in five columns), the 12-vertex synthetic molecule and a 7-vertex one
    -- more nodes than one workgroup packs (64), packed runs that break inside and between molecules, a ragged last workgroup, 68 nodes
    of size 2 at level 1 (CH4's hydrogens: more than one node per reduction chunk) and sizes that only one node has"""
    mols, tg = [], []
    for rep in range(17):
        for _, adj, feat, t in toy_molecules():
            mols.append((adj, np.concatenate([feat, np.zeros((len(adj), 1))], axis=1)))
            tg.append(0.05 * t + 0.01 * rep)
    for seed, V in ((5, 12), (7, 7)):
        adj, x, _ = synthetic_molecule(seed, V)
        mols.append((adj, x))
        tg.append(0.05 * V)
    return mols, np.array(tg)


def expectation(form, mols, tg, L, Cn, D, maxV, seed0):
    """(params, blocks, phis, per-molecule results, summed gradient, margin) at the first of MAX_SEEDS seeds whose margin holds"""
    FD = mols[0][1].shape[1] * (D + 1)
    phis = host_fields(mols, form, L, Cn, D, maxV)
    for seed in range(seed0, seed0 + MAX_SEEDS):
        params = random_params(form, Cn, FD, L, maxV, np.random.default_rng(seed))
        res, rg = uref.run_batch(form, mols, tg, params, L, Cn, D, maxV, phis)
        m = uref.margin(res)
        if m >= MARGIN:
            return params, unrestricted_blocks(form, Cn, FD, L, maxV), phis, res, rg, m
    raise AssertionError("no seed in [%d, %d) keeps the margin" % (seed0, seed0 + MAX_SEEDS))


PACK_L, PACK_D, PACK_MAXV = 2, 1, 13
# channels 3, 4, 6, 8 for the first-order forms (lane vectors 1, 4, 2 and the doubled widths), 3, 5, 8 for form 3
PACKED_SHAPES = [(1, 3), (1, 4), (1, 6), (1, 8), (2, 3), (2, 4), (2, 6), (2, 8), (3, 3), (3, 5), (3, 8)]
_PACKED = {}


def packed_reference(form, Cn):
    if (form, Cn) not in _PACKED:
        mols, tg = packing_batch()
        _PACKED[(form, Cn)] = (mols, tg) + expectation(form, mols, tg, PACK_L, Cn, PACK_D, PACK_MAXV, 100 * form + Cn)
    return _PACKED[(form, Cn)]


# Form 2 at C = 16, three levels: C_2 = 64, so a level-3 node keeps s * 64 floats of S and the LDS variant takes fields up to 32 positions
# (one node per workgroup there: 16 lane vectors per position).  One molecule whose largest level-3 field has 31 positions, one with fields of 33 and 34.
LDS_FORM, LDS_C, LDS_L, LDS_D = 2, 16, 3, 0
LDS_MOLECULES = {"below": (3, 40), "above": (3, 44)}   # (seed, vertices) of synthetic_molecule
_LDS = {}


def lds_reference(which):
    if which not in _LDS:
        seed, V = LDS_MOLECULES[which]
        adj, x, _ = synthetic_molecule(seed, V)
        mols, tg = [(adj, x)], np.array([0.05 * V])
        _LDS[which] = (mols, tg) + expectation(LDS_FORM, mols, tg, LDS_L, LDS_C, LDS_D, V, 500)
    return _LDS[which]
