"""The decision rule of the iterative training calls (graphflow_amd/csrc/smp_fit_policy.h: no HIP, no handle) on the CPU: every loss
sequence the reference's classes produced (tests/golden/smp_iterative.npz, written by tests/golden/make_iterative_golden.py) goes through
tests/cpp/fit_policy_sanitize.cpp, and decisions, rates, counts and the returned pair must be the record's exactly -- doubles throughout,
passed as hexadecimal floats.  The same program, with its built-in branch sequences, runs under AddressSanitizer + UBSan."""
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

from test_prep_neighbourhood_sanitizers import runtime_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphflow_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "fit_policy_sanitize.cpp")
RUNS = ("batch_mixed", "batch_leave", "learn_epsilon", "learn_immediate", "learn_exhaust")
ACCEPT, REJECT, REJECT_LEAVE, LEAVE = 1, 2, 3, 4


def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "smp_iterative.npz")) as z:
        return {k: z[k] for k in z.files}


def recorded_runs(z):
    return [(str(c), r) for c in z["classes"] for r in RUNS if "%s__%s__pair" % (c, r) in z]


def build(tmp_path, flags=()):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "fit_policy")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", *flags, "-I" + CSRC, "-o", exe, SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "warning" not in r.stderr, r.stderr[-2000:]
    return exe


def test_fixture_covers_every_branch_with_room():
    """what the generator asserts, asked of the file: every run exists for some class, every class has a kept and a restored step, and
    every comparison a recorded loop made has a gap of 1e-3"""
    z = golden()
    runs = recorded_runs(z)
    assert {r for _, r in runs} == set(RUNS)
    # five runs of six classes; exactly two may be missing (make_iterative_golden.MAY_BE_MISSING: Adam cannot leave through lr < 1e-6 with a gap)
    assert len(z["classes"]) == 6 and len(runs) == 6 * len(RUNS) - 2
    assert sorted(z["missing"]) == ["SMP_omega/batch_leave", "SMP_omega_physics/batch_leave"]
    for c in z["classes"]:
        d = np.concatenate([z["%s__%s__decisions" % (c, r)] for cc, r in runs if cc == c])
        assert ACCEPT in d and REJECT in d, c
    gap = lambda a, b: abs(a - b) / max(abs(b), 1.0)  # noqa: E731
    for c, r in runs:
        p = "%s__%s__" % (c, r)
        kind, eps, best = int(z[p + "cfg"][0]), float(z[p + "eps"][0]), float(z[p + "pair"][0])
        if kind == 1:
            assert gap(best, eps) >= 1e-3, p
        for loss, dec in zip(z[p + "losses"], z[p + "decisions"]):
            if kind == 1:
                assert gap(loss, eps) >= 1e-3, p
            if dec != LEAVE:
                assert gap(loss, best) >= 1e-3, p
            if dec == ACCEPT:
                best = loss
        assert best == z[p + "pair"][1], p


def test_policy_reproduces_the_recorded_loops(tmp_path):
    z = golden()
    runs = recorded_runs(z)
    exe = build(tmp_path)
    lines = []
    for c, r in runs:
        p = "%s__%s__" % (c, r)
        v = [float(z[p + "cfg"][0]), float(z[p + "cfg"][1]), float(z[p + "lr"][0]), float(z[p + "eps"][0]), float(z[p + "pair"][0])]
        lines.append(" ".join(float(x).hex() for x in v + list(z[p + "losses"])))
    path = tmp_path / "loops.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
    assert len(out) == len(runs)
    for (c, r), line in zip(runs, out):
        p, tok = "%s__%s__" % (c, r), line.split()
        dec = z[p + "decisions"]
        assert [float.fromhex(t) for t in tok[:3]] == [z[p + "pair"][0], z[p + "pair"][1], z[p + "final_lr"][0]], p
        left = int(len(dec) > 0 and dec[-1] in (REJECT_LEAVE, LEAVE)) or int(r == "learn_immediate")
        assert [int(t) for t in tok[3:7]] == [len(dec), int((dec == ACCEPT).sum()), int((dec == REJECT).sum() + (dec == REJECT_LEAVE).sum()), left], p
        assert [int(t) for t in tok[7:]] == list(dec), p


def test_policy_is_clean_under_sanitizers(tmp_path):
    flags = "-fsanitize=address,undefined"
    if not runtime_present(tmp_path, flags):
        pytest.skip("no runtime for %s on this machine" % flags)
    exe = build(tmp_path, (flags, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    # (randomisation off for the program's own process: see tests/test_prep_sanitizers.py)
    cmd = ["setarch", platform.machine(), "-R", exe] if shutil.which("setarch") else [exe]
    run = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-3000:]
    assert "PASSED" in run.stdout and "runtime error" not in run.stderr
