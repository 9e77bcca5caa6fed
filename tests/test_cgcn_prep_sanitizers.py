"""What CGCN_1D and CGCN_2D (gf_smp_config.covariant = 1, 2) add to the host side -- the resolver's branch
(graphflow_amd/csrc/smp_config.cpp), the block enumeration of the Config they become and the batch (smp_prep.cpp: build_batch_covariant)
-- as a stand-alone program under AddressSanitizer + UBSan, on the CPU: accepted configurations, every refusal with a piece of its
message, hostile structs, and batches with V = 1, V = max_nVertices, an isolated vertex, an asymmetric adjacency and a set diagonal entry,
checked entry by entry against a direct evaluation."""
import os
import platform
import shutil
import subprocess

import pytest

from test_prep_neighbourhood_sanitizers import runtime_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphflow_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "cgcn_prep_sanitize.cpp"), os.path.join(CSRC, "smp_config.cpp"), os.path.join(CSRC, "smp_prep.cpp")]
FLAGS = "-fsanitize=address,undefined"


def test_cgcn_host_side_is_clean_under_sanitizers(tmp_path):
    if not runtime_present(tmp_path, FLAGS):
        pytest.skip("no runtime for %s on this machine" % FLAGS)
    exe = str(tmp_path / "cgcn_prep_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", FLAGS, "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread", "-I" + CSRC, "-o", exe] + SRC
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    # (randomisation off for the program's own process: see tests/test_prep_sanitizers.py)
    cmd = ["setarch", platform.machine(), "-R", exe] if shutil.which("setarch") else [exe]
    run = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-3000:]
    assert "PASSED" in run.stdout and "runtime error" not in run.stderr
