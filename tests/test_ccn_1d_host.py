"""Host drop-ins of the first-order models (graphflow_amd/host/SMP_physics_hip.h: CCN_1D_hip, SMP_theta_pairgraphs_hip,
SMP_theta_physics_hip), driven by tests/cpp/test_CCN_1D_hip.cpp like the reference's tests/test_CCN_1D.cpp.  The program is compiled
here, into tmp_path, with the flags of tests/cpp/Makefile (the precedent: tests/test_classification_host.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_program(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine: the host C++ test program cannot be compiled")
    exe = str(tmp_path / "test_CCN_1D_hip")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "graphflow_amd", "host"),
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_CCN_1D_hip.cpp"),
           "-L" + os.path.join(ROOT, "graphflow_amd", "csrc"), "-lgf_hip", "-Wl,-rpath," + os.path.join(ROOT, "graphflow_amd", "csrc"),
           "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def write_theta_cases(tmp_path):
    """what the `_theta` drop-ins are held to, from the real classes' numbers in tests/golden/smp_theta_physics.npz: the first loss pair
    of SMP_theta_physics' BatchLearn trajectory, and the pair_c16 case of SMP_theta_pairgraphs with its parameters as a checkpoint"""
    with np.load(os.path.join(ROOT, "tests", "golden", "smp_theta_physics.npz")) as pz:
        assert tuple(pz["train__cfg"][:6]) == (1, 2, 16, 4, 10, 7)   # towers, L, C, cap, max_nVertices, seed: what the program constructs
        p = "tphys_pair_c16__"
        towers, L, Cn, cap, maxV1, maxV2 = (int(x) for x in pz[p + "cfg"])
        assert towers == 2
        graphs = [(pz[p + "adj"], pz[p + "feature"]), (pz[p + "adj2"], pz[p + "feature2"])]
        text = "%.17g %.17g\n" % tuple(pz["train__losses"][0])
        text += "%d %d %d %d %d %d %d %.17g %.17g %.17g\n" % (maxV1, maxV2, cap, L, Cn, graphs[0][1].shape[1], graphs[1][1].shape[1],
                                                              pz[p + "target"][0], pz[p + "predict"][0], pz[p + "loss"][0])
        for adj, feat in graphs:
            text += "%d\n%s\n%s\n" % (len(adj), " ".join(str(int(x)) for x in adj.ravel()), " ".join("%.17g" % x for x in feat.ravel()))
        (tmp_path / "theta_cases.txt").write_text(text)
        (tmp_path / "theta_pair_params.dat").write_text("".join("%.9g " % x for x in pz[p + "params"]))


def test_dropin_program_compiles_and_refuses_to_run_without_a_gpu(gf, tmp_path):
    import torch
    exe = compile_program(tmp_path)
    if torch.cuda.is_available():
        return
    write_theta_cases(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_first_order_dropins_reproduce_reference_training(gf, tmp_path):
    """Same srand -> same initial weights -> the real CCN_1D's three BatchLearn loss pairs at the demo's settings; save_model -> load_model
    into a second network -> the same Predict; one step each of SMP_theta_physics_hip and SMP_theta_pairgraphs_hip."""
    exe = compile_program(tmp_path)
    write_theta_cases(tmp_path)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
