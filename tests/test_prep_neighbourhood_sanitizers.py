"""The host preparation of the neighbourhood models (gfsmp::build_batch_neighbourhood in graphflow_amd/csrc/smp_prep.cpp: threads, reused
vectors, the neighbour lists and their transposes) as a stand-alone program under AddressSanitizer + UBSan and under ThreadSanitizer,
on the CPU."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "cpp", "prep_neighbourhood_sanitize.cpp"), os.path.join(ROOT, "graphflow_amd", "csrc", "smp_prep.cpp")]


def runtime_present(tmp_path, flags):
    """does a trivial program link against the sanitizer's runtime here?  Asked before the code under test is built."""
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", flags, "-o", str(tmp_path / "probe"), str(src)], capture_output=True).returncode == 0


@pytest.mark.parametrize("flags", ["-fsanitize=address,undefined", "-fsanitize=thread"])
def test_neighbour_lists_are_clean_under_sanitizers(tmp_path, flags):
    if not runtime_present(tmp_path, flags):
        pytest.skip("no runtime for %s on this machine" % flags)
    exe = str(tmp_path / "prep_neighbourhood_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", flags, "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "graphflow_amd", "csrc"), "-o", exe] + SRC
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", TSAN_OPTIONS="halt_on_error=1")
    env.pop("GF_PREP_THREADS", None)
    # (randomisation off for the program's own process: see tests/test_prep_sanitizers.py)
    cmd = ["setarch", platform.machine(), "-R", exe] if shutil.which("setarch") else [exe]
    run = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, run.stdout[-1500:] + run.stderr[-3000:]
    assert "PASSED" in run.stdout
