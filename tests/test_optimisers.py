"""CPU suite for the SGD / AdaMax / AdaDelta steps and the L1 / L2 regularisers: everything that needs no device.

  - tests/optim_ref.py with storage = float64 IS the reference: it reproduces Part A of tests/golden/optimisers.npz (recorded from the real
    classes by tests/golden/make_optimiser_golden.py) to 1e-12 relative, the bound test_oracle_golden.py puts on restatements;
  - gf_smp_config_param_blocks and its classifier / model siblings give the sizes of sgd->params[i] of the real classes (Part B) exactly,
    end at the *_param_count calls, and follow the count / capacity protocol;
  - every refusal of the new entries that is decided before a device is touched;
  - tests/cpp/optim_blocks_sanitize.cpp, the block-table functions over the Part B configurations under AddressSanitizer + UBSan."""
import ctypes as C
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

import optim_ref
from make_optimiser_golden import (A_KIND, A_LR, BLOCK_CASES, BLOCKS, N_BATCH, N_STEPS, REG_LAMBDA, REG_TIMES, a_index, case_grads, offsets_of,
                                   part_a_inputs)
from test_prep_neighbourhood_sanitizers import runtime_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphflow_amd", "csrc")
REL = 1e-12


def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "optimisers.npz")) as z:
        return {k: z[k] for k in z.files}


def close(a, b, rel=REL):
    """|a - b| <= rel max(|b|, tiny) element by element, NaN where and only where the record has one"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    return bool(np.all(np.abs(a[ok] - b[ok]) <= rel * np.maximum(np.abs(b[ok]), 1e-300)))


def run_case(case, storage):
    """the six steps of one Part A case through optim_ref: per step (p, s0, s1, norms, beta1_t)"""
    params, grads, _ = part_a_inputs()
    g = case_grads(case, grads)
    off = offsets_of(BLOCKS)
    p = params.astype(storage)
    state = optim_ref.new_state(p.size, len(BLOCKS), storage)
    steps = []
    for s in range(N_STEPS):
        p = optim_ref.step(A_KIND[case], p, g[s].astype(storage), state, off, A_LR[case], N_BATCH, storage)
        steps.append((p.copy(), state["s0"].copy(), state["s1"].copy(), state["norms"].copy(), state["beta1_t"]))
    return steps


def test_inputs_are_the_generators():
    z = golden()
    params, grads, reg = part_a_inputs()
    assert np.array_equal(z["a_checksum"], [params.sum(), grads.sum(), reg.sum()])
    assert np.array_equal(z["a_blocks"], BLOCKS) and np.array_equal(z["a_index"], a_index())
    assert np.array_equal(params, params.astype(np.float32)) and np.array_equal(grads, grads.astype(np.float32))


@pytest.mark.parametrize("case", list(A_KIND))
def test_restatement_in_float64_is_the_reference(case):
    z, idx = golden(), a_index()
    steps = run_case(case, np.float64)
    for s, (p, s0, s1, norms, beta1_t) in enumerate(steps):
        assert close(p[idx], z["a_%s__p" % case][s]), (case, s)
        if A_KIND[case] != optim_ref.SGD:
            assert close(s0[idx], z["a_%s__s0" % case][s]), (case, s)
        if A_KIND[case] == optim_ref.ADADELTA:
            assert close(s1[idx], z["a_%s__s1" % case][s]), (case, s)
        if A_KIND[case] == optim_ref.ADAMAX:
            assert np.array_equal(norms, z["a_%s__norms" % case][s]) and beta1_t == z["a_%s__beta1_t" % case][s][0], (case, s)


def test_zero_blocks_behave_as_recorded():
    """what the two zero-block cases are for: NaN in exactly the zero block, from the step the record says, and nowhere else"""
    z, idx = golden(), a_index()
    off = offsets_of(BLOCKS)
    inside = (idx >= off[4]) & (idx < off[5])
    for case in ("adamax_zero", "adamax_zero1"):
        p = z["a_%s__p" % case]
        assert np.isnan(p[:, inside]).all() and np.isfinite(p[:, ~inside]).all()
        assert np.array_equal(p[:, ~inside], z["a_adamax__p"][:, ~inside])   # no other block is touched
    assert (z["a_adamax_zero__norms"][:, 4] == 0.0).all() and (z["a_adamax_zero1__norms"][1:, 4] > 0.0).all()
    assert np.isfinite(z["a_adamax__p"]).all()


@pytest.mark.parametrize("norm", [1, 2])
def test_regularisers_in_float64_are_the_reference(norm):
    z, idx = golden(), a_index()
    _, grads, reg = part_a_inputs()
    for s in range(N_STEPS):
        value, g = optim_ref.regularise(norm, reg[s], grads[s], REG_LAMBDA, REG_TIMES, np.float64)
        assert close(value, z["a_l%d__value" % norm][s]), (norm, s)
        # (the class adds the term REG_TIMES times, the restatement once times REG_TIMES: 1e-12 of the operands, which may cancel)
        assert np.all(np.abs(g[idx] - z["a_l%d__g" % norm][s]) <= REL * np.maximum(np.abs(grads[s][idx]), 1.0)), (norm, s)


def smp_config(fields):
    from graphflow_amd import smp as gfa
    cfg = gfa.SMPConfigCovariant()
    for k, v in fields.items():
        setattr(cfg, k, v)
    return cfg


def blocks_and_count(gf, name):
    """(offsets, parameter count) the library gives the Part B configuration of class `name`"""
    from graphflow_amd import _lib, smp as gfa
    lib = _lib.load()
    how = BLOCK_CASES[name][1]
    if how[0] == "model":
        cfg = gfa.SMPModel.config(**how[1])
        return _lib.param_blocks("gf_smp_model_config_param_blocks", C.byref(cfg)), lib.gf_smp_model_config_param_count(C.byref(cfg))
    cfg = smp_config(how[1])
    if how[0] == "classifier":
        return (_lib.param_blocks("gf_smp_classifier_config_param_blocks", C.byref(cfg), how[2]),
                lib.gf_smp_classifier_config_param_count(C.byref(cfg), how[2]))
    return _lib.param_blocks("gf_smp_config_param_blocks", C.byref(cfg)), lib.gf_smp_config_param_count(C.byref(cfg))


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_block_table_is_the_classes_registration(gf, name):
    z = golden()
    sizes = z["b_%s__sizes" % name]
    offsets, count = blocks_and_count(gf, name)
    assert count == sizes.sum() and count > 0
    assert offsets == list(offsets_of(sizes)), (name, np.diff(offsets), sizes)
    assert offsets[-1] == count


def test_capacity_protocol_and_refusals(gf):
    from graphflow_amd import _lib, smp as gfa
    lib = _lib.load()
    cfg = smp_config(BLOCK_CASES["SMP_omega"][1][1])
    n = lib.gf_smp_config_param_blocks(C.byref(cfg), None, 0)
    assert n == 6
    buf = (C.c_size_t * (n + 2))(*([77] * (n + 2)))
    assert lib.gf_smp_config_param_blocks(C.byref(cfg), buf, n) == n and list(buf) == [77] * (n + 2)        # too small: the count, nothing written
    assert lib.gf_smp_config_param_blocks(C.byref(cfg), buf, n + 1) == n and buf[n + 1] == 77 and buf[0] == 0   # exactly count + 1 entries
    assert buf[n] == lib.gf_smp_config_param_count(C.byref(cfg))
    assert lib.gf_smp_classifier_config_param_blocks(C.byref(cfg), 3, buf, n + 2) == n and buf[n] == lib.gf_smp_classifier_config_param_count(C.byref(cfg), 3)
    # what create refuses has no blocks
    bad = smp_config(dict(BLOCK_CASES["SMP_omega"][1][1], nContractions=7))
    assert lib.gf_smp_config_param_blocks(C.byref(bad), buf, n + 2) == 0 and lib.gf_smp_config_param_blocks(None, buf, n + 2) == 0
    assert lib.gf_smp_classifier_config_param_blocks(C.byref(cfg), 1, buf, n + 2) == 0
    gcn = smp_config(BLOCK_CASES["GCN_1D"][1][1])
    assert lib.gf_smp_classifier_config_param_blocks(C.byref(gcn), 3, buf, n + 2) == 0   # (no classifier of that family)
    model = gfa.SMPModel.config(2, 4, 6, [4, 3, ][:2])
    model.nTowers = 3
    assert lib.gf_smp_model_config_param_blocks(C.byref(model), None, 0) == 0 and lib.gf_smp_model_config_param_blocks(None, None, 0) == 0


def test_entries_refuse_bad_arguments_without_a_device(gf):
    from graphflow_amd import _lib
    lib = _lib.load()
    INV = _lib.GF_ERR_INVALID
    cfg = _lib.OptimConfig(2, 4, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0)
    v = C.c_double(0.0)
    assert lib.gf_smp_optimiser_step(None, None, None, C.byref(cfg)) == INV
    assert lib.gf_smp_model_optimiser_step(None, None, None, C.byref(cfg)) == INV
    assert lib.gf_smp_regularise(None, None, None, 1, 0.1, 1, C.byref(v)) == INV
    assert lib.gf_smp_model_regularise(None, None, None, 2, 0.1, 1, C.byref(v)) == INV
    assert lib.gf_optimiser_step_f32(None, C.byref(cfg), None, None, 0, None, 0, None, None, None, None) == INV
    assert lib.gf_regularise_f32(None, None, None, 0, 1, 0.1, 1, C.byref(v)) == INV
    assert sorted(_lib.OPTIMISERS.items(), key=lambda kv: kv[1]) == [("adam", 0), ("momentum", 1), ("sgd", 2), ("adamax", 3), ("adadelta", 4)]
    assert C.sizeof(_lib.OptimConfig) == 56


def build_sanitize(tmp_path, flags=()):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "optim_blocks")
    srcs = [os.path.join(ROOT, "tests", "cpp", "optim_blocks_sanitize.cpp"), os.path.join(CSRC, "smp_config.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *flags, "-I" + CSRC, "-o", exe, *srcs], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "warning" not in r.stderr, r.stderr[-2000:]
    return exe


def expected_tables():
    z = golden()
    return "".join("%s %s\n" % (name, " ".join(str(int(x)) for x in z["b_%s__sizes" % name])) for name in BLOCK_CASES)


def test_block_tables_stand_alone(tmp_path):
    """the host-only functions without the library: the program's tables are Part B's"""
    exe = build_sanitize(tmp_path)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-1500:]
    assert run.stdout.replace("PASSED\n", "") == expected_tables()


def test_block_tables_are_clean_under_sanitizers(tmp_path):
    flags = "-fsanitize=address,undefined"
    if not runtime_present(tmp_path, flags):
        pytest.skip("no runtime for %s on this machine" % flags)
    exe = build_sanitize(tmp_path, (flags, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    cmd = ["setarch", platform.machine(), "-R", exe] if shutil.which("setarch") else [exe]   # (randomisation off: see tests/test_prep_sanitizers.py)
    run = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-3000:]
    assert "PASSED" in run.stdout and "runtime error" not in run.stderr
    assert run.stdout.replace("PASSED\n", "") == expected_tables()
