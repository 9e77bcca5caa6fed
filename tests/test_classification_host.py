"""Host drop-ins of the classification models (graphflow_amd/host/SMP_classification_hip.h), driven by
tests/cpp/test_SMP_classification_hip.cpp like the reference's tests/test_SMP_2D_ver6_classification.cpp.  The program is compiled here,
into tmp_path, with the flags of tests/cpp/Makefile (the precedent: tests/test_prep_sanitizers.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_program(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine: the host C++ test program cannot be compiled")
    exe = str(tmp_path / "test_SMP_classification_hip")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "graphflow_amd", "host"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_SMP_classification_hip.cpp"),
           "-L" + os.path.join(ROOT, "graphflow_amd", "csrc"), "-lgf_hip", "-L" + os.path.join(ROOT, "oracle"), "-lgf_oracle",
           "-Wl,-rpath," + os.path.join(ROOT, "graphflow_amd", "csrc"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"),
           "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def test_dropin_program_compiles_and_refuses_to_run_without_a_gpu(gf, oracle, tmp_path):
    import torch
    exe = compile_program(tmp_path)
    if torch.cuda.is_available():
        return
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_classification_dropins_reproduce_reference_training(gf, oracle, tmp_path):
    """Same srand -> same initial weights -> the real classes' BatchLearn loss pairs; after the demo's 1000 epochs Predict returns
    5, 4, 3, 6; save_model -> load_model into a second network -> the same labels."""
    exe = compile_program(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
