"""The host drop-in classes of graphflow_amd/host/SMP_families_hip.h (one per reference class, on the skeleton of SMP_handle_hip.h) and
the two iterative methods the older classes gained, driven by tests/cpp/test_family_dropins_hip.cpp.  The program is compiled here, into
tmp_path, with the flags of tests/cpp/Makefile (the precedent: tests/test_classification_host.py); the cases reach it as a text file.

Against the family goldens (recorded(): every BatchLearn trajectory of a real class that they hold -- 24 of the 32 classes; the goldens
record one class per level form and no classifier of these families, UNRECORDED names the other eight): at the record's constructor
arguments, seed, molecules, targets and rate, the constructor's weights are the record's params0 bit for bit, and the recorded steps give
its loss pairs and final weights within field_suite.check_momentum_trajectory's bounds, as the family's own *_gpu.py test asks.
The other eight meet their real constructors through the goldens' initial-weight records (initial_weight_records(): params0 bit for bit at the
record's arguments and seed), so every class has a real-class yardstick for its weights.  Where a golden holds a real class's own save_model
file (checkpoint_records(): eleven classes), the drop-in at the file's weights writes that file token for token, and a second object loads it.
Beside that, for every class, on the four toy molecules as one batch, against its Python wrapper (whose own suite pins it to the real class):
  - after srand(seed) the constructor's weights are, bit for bit, what the wrapper draws after the same srand;
  - three BatchLearn steps give the loss pairs and final weights of the same three steps through the wrapper, bit for bit (the same
    library calls in the same order);
  - save_model writes the weights as "%g " in registration order (the classes' checkpoint text; the distance models channel by channel),
    the file the wrapper's save_model writes;
  - load_model into a second object, built after another srand, gives the Predict of the wrapper's load_model of the same file.
For the six classes of tests/golden/smp_iterative.npz the two iterative methods return the recorded pair (field_suite's bounds), the
recorded decisions exactly, and the final weights within the trajectory bounds.
Without a GPU the program must stop with "no CPU fallback"."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import field_suite as kit
from field_suite import TOL, dev, f64
from inputs import toy_molecules
from make_iterative_golden import CLASSES as FIT_CLASSES, batch_of
from test_fit_policy import recorded_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "graphflow_amd", "host")
SEED, LR, GAMMA, STEPS = 23, 0.05, 0.9, 3

# class -> (constructor integers, Python wrapper: lambda smp module -> net, kind of batch, golden record or None)
FIELD = (6, 2, 4, 4, 1)          # max_nVertices, nLevels, nChanels, nFeatures, nDepth
CLS = (3,) + FIELD               # nClass in front
VERTEX = (2, 6, 4, 5, 1, 1)      # nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius
DROPINS = {
    "SMP_theta": ((6, 4, 2, 4, 4, 1), lambda m: m.SMPTheta(6, 4, 2, 4, 4, 1), "single"),
    "SMP_1D": (FIELD, lambda m: m.SMP1D(1, *FIELD), "single"),
    "SMP_1D_ver2": (FIELD, lambda m: m.SMP1D(2, *FIELD), "single"),
    "SMP_1D_ver3": (FIELD, lambda m: m.SMP1D(3, *FIELD), "single"),
    "SMP_1D_classification": (CLS, lambda m: m.SMP1D(1, *FIELD, nClass=3), "labels"),
    "SMP_1D_ver3_classification": (CLS, lambda m: m.SMP1D(3, *FIELD, nClass=3), "labels"),
    "SMP_2D": (FIELD, lambda m: m.SMP2D("2d", *FIELD), "single"),
    "SMP_2D_ver4": (FIELD, lambda m: m.SMP2D("ver4", *FIELD), "single"),
    "SMP_2D_ver5": (FIELD, lambda m: m.SMP2D("ver5", *FIELD), "single"),
    "SMP_2D_classification": (CLS, lambda m: m.SMP2D("2d", *FIELD, n_class=3), "labels"),
    "SMP_2D_ver4_classification": (CLS, lambda m: m.SMP2D("ver4", *FIELD, n_class=3), "labels"),
    "Unrestricted_SMP_1D": (FIELD, lambda m: m.SMPUnrestricted("1d", *FIELD), "single"),
    "Unrestricted_SMP_1D_ver2": (FIELD, lambda m: m.SMPUnrestricted("1d_ver2", *FIELD), "single"),
    "Unrestricted_SMP_2D": (FIELD, lambda m: m.SMPUnrestricted("2d", *FIELD), "single"),
    "NeuralFingerprint": ((2, 6, 4, 5), lambda m: m.SMPNeighbourhood("fingerprint", 2, 5, 4, 0, 6, 0), "single"),
    "GCN_1D": (VERTEX, lambda m: m.SMPNeighbourhood("gcn_1d", 2, 5, 4, 1, 6, 1), "single"),
    "GCN_2D": (VERTEX, lambda m: m.SMPNeighbourhood("gcn_2d", 2, 5, 4, 1, 6, 1), "single"),
    "GCN_3D": (VERTEX, lambda m: m.SMPNeighbourhood("gcn_3d", 2, 5, 4, 1, 6, 1), "single"),
    "GRU_GCN_1D": (VERTEX, lambda m: m.SMPGatedNeighbourhood("gru_gcn_1d", 2, 5, 4, 1, 6, 1), "single"),
    "GRU_GCN_2D": (VERTEX, lambda m: m.SMPGatedNeighbourhood("gru_gcn_2d", 2, 5, 4, 1, 6, 1), "single"),
    "GRU_GCN_3D": (VERTEX, lambda m: m.SMPGatedNeighbourhood("gru_gcn_3d", 2, 5, 4, 1, 6, 1), "single"),
    "GCN_1D_Distance": (VERTEX, lambda m: m.SMPDistance("gcn_1d_distance", 2, 5, 4, 1, 6, 1), "distance"),
    "GCN_2D_Distance": (VERTEX, lambda m: m.SMPDistance("gcn_2d_distance", 2, 5, 4, 1, 6, 1), "distance"),
    "GCN_3D_Distance": (VERTEX, lambda m: m.SMPDistance("gcn_3d_distance", 2, 5, 4, 1, 6, 1), "distance"),
    "GCN_1D_Kernel": (VERTEX, lambda m: m.SMPKernelPairs("gcn_1d_kernel", *VERTEX), "pairs"),
    "GCN_2D_Kernel": (VERTEX, lambda m: m.SMPKernelPairs("gcn_2d_kernel", *VERTEX), "pairs"),
    "GCN_3D_Kernel": (VERTEX, lambda m: m.SMPKernelPairs("gcn_3d_kernel", *VERTEX), "pairs"),
    "GCA_1D": (VERTEX, lambda m: m.GCA1D(*VERTEX), "gram"),
    "LCNN": ((6, 4, 3, 1, 4, 4, 8), lambda m: m.LCNN(6, 4, 3, 1, 4, 4, 8), "single"),
    "GCN_MW": ((2, 6, 4, 5, 1), lambda m: m.GCNMW(2, 6, 4, 5, 1), "single"),
    "CGCN_1D": ((2, 6, 4, 1), lambda m: m.CGCN1D(2, 6, 4, 1), "single"),
    "CGCN_2D": ((2, 6, 4, 1), lambda m: m.CGCN2D(2, 6, 4, 1), "single"),
}
def recorded():
    """Every BatchLearn trajectory of a real class that the family goldens hold, as the family's own *_gpu.py test reads it:
    class -> (golden arrays, prefix, constructor integers, momentum_param, seed, steps, rate, (x, y or None, has a target))"""
    from make_theta_golden import small_molecules
    toys = [(a, f) for _, a, f, _ in toy_molecules()]
    out = {}

    def add(name, fname, pre, ctor, seed, steps, x=toys, y=None, target=True):
        z = kit.load_golden(fname)
        gamma = float(z[pre + "momentum"][0]) if pre + "momentum" in z else 0.0
        out[name] = (z, pre, tuple(int(c) for c in ctor), gamma, int(seed), int(steps), float(z[pre + "lr"][0]), (x, y, target))

    def cfg(fname, pre):
        return [int(v) for v in kit.load_golden(fname)[pre + "cfg"]]

    # the vertex-level families: cfg = form, L, H, D, R, maxV, seed, steps
    for name, fname, pre in (("NeuralFingerprint", "smp_neighbourhood.npz", "train_n1__"), ("GCN_1D", "smp_neighbourhood.npz", "train_n2__"),
                             ("GCN_2D", "smp_neighbourhood.npz", "train_n3__"), ("GCN_3D", "smp_third_order.npz", "train_n6__"),
                             ("GRU_GCN_1D", "smp_gru_gcn.npz", "train_n4__"), ("GRU_GCN_2D", "smp_gru_gcn.npz", "train_n5__"),
                             ("GRU_GCN_3D", "smp_third_order.npz", "train_n7__"), ("GCN_1D_Distance", "smp_distance.npz", "train_n2__"),
                             ("GCN_2D_Distance", "smp_distance.npz", "train_n3__"), ("GCN_3D_Distance", "smp_distance.npz", "train_n6__"),
                             ("GCN_1D_Kernel", "smp_pair_gram.npz", "train_p2__"), ("GCN_2D_Kernel", "smp_pair_gram.npz", "train_p3__"),
                             ("GCN_3D_Kernel", "smp_pair_gram.npz", "train_p6__"), ("GCA_1D", "smp_pair_gram.npz", "train_g__")):
        _, L, H, D, R, maxV, seed, steps = cfg(fname, pre)
        ctor = (L, maxV, 4, H) if name == "NeuralFingerprint" else (L, maxV, 4, H, D, R)
        if name.endswith("_Distance"):   # (tests/test_smp_distance.py: train_molecules)
            dz = kit.load_golden(fname)
            add(name, fname, pre, ctor, seed, steps, x=[(a, f, dz["train__distance_%d" % i]) for i, (a, f) in enumerate(toys)])
        elif name.endswith("_Kernel"):   # (tests/test_smp_pair_gram.py: train_batch -- toy p with toy p + 1)
            add(name, fname, pre, ctor, seed, steps, y=toys[1:] + toys[:1])
        else:
            add(name, fname, pre, ctor, seed, steps, target=name != "GCA_1D")
    for form in (1, 2):   # cfg = form, L, M, D, seed, steps
        _, L, M, D, seed, steps = cfg("smp_cgcn.npz", "train_c%d__" % form)
        add("CGCN_%dD" % form, "smp_cgcn.npz", "train_c%d__" % form, (L, M, 4, D), seed, steps)
    mz = kit.load_golden("smp_matrix_form.npz")   # cfg = the class's own integers; seed = seed, steps, maxV
    V, k, D, C1, C2, nD = cfg("smp_matrix_form.npz", "train_lcnn__")
    add("LCNN", "smp_matrix_form.npz", "train_lcnn__", (V, 4, k, D, C1, C2, nD), *mz["train_lcnn__seed"][:2])
    L, H, D = cfg("smp_matrix_form.npz", "train_gcn_mw__")
    add("GCN_MW", "smp_matrix_form.npz", "train_gcn_mw__", (L, int(mz["train_gcn_mw__seed"][2]), 4, H, D), *mz["train_gcn_mw__seed"][:2])
    # the field-level families: cfg = form, L, C, D, has_WL_ordering, maxV (, nClass), seed, steps; which class, by the form
    for fname, pre, names in (("smp_unrestricted.npz", "train_u3__", {3: "Unrestricted_SMP_2D"}), ("smp_unrestricted.npz", "train_u2__", {2: "Unrestricted_SMP_1D_ver2"}),
                              ("smp_1d.npz", "train__", {1: "SMP_1D", 2: "SMP_1D_ver2", 3: "SMP_1D_ver3"}),
                              ("smp_2d.npz", "train__", {1: "SMP_2D", 2: "SMP_2D_ver4"}), ("smp_2d_ver5.npz", "train__", {5: "SMP_2D_ver5"})):
        c = cfg(fname, pre)
        form, L, Cn, D, wl, maxV = c[:6]
        assert wl == 1 and (len(c) == 8 or c[6] == 0)   # (the constructors' default ordering; a regression class)
        add(names[form], fname, pre, (maxV, L, Cn, 4, D), c[-2], c[-1])
    L, Cn, D, cap, maxV, seed, steps = cfg("smp_theta.npz", "train__")   # (Adam; tests/test_smp_theta_gpu.py: its own four small molecules)
    add("SMP_theta", "smp_theta.npz", "train__", (maxV, cap, L, Cn, 4, D), seed, steps, x=[(a, f) for _, a, f, _ in small_molecules()])
    return out


# the classes of DROPINS whose family golden holds no BatchLearn trajectory: the goldens record one class per level form (SMP_1D_ver3 for
# the SMP_1D forms, SMP_2D_ver4 for SMP_2D's, Unrestricted_SMP_2D and _1D_ver2), and none of a classifier of these families
UNRECORDED = ("SMP_1D", "SMP_1D_ver2", "SMP_1D_classification", "SMP_1D_ver3_classification", "SMP_2D", "SMP_2D_classification",
              "SMP_2D_ver4_classification", "Unrestricted_SMP_1D")


def compile_program(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++ on this machine: the host C++ test program cannot be compiled")
    exe = str(tmp_path / "test_family_dropins_hip")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_family_dropins_hip.cpp"), "-L" + os.path.join(ROOT, "graphflow_amd", "csrc"), "-lgf_hip",
           "-Wl,-rpath," + os.path.join(ROOT, "graphflow_amd", "csrc"), "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def hop_distance(adj):
    V = len(adj)
    d = np.where(np.asarray(adj) > 0, 1.0, np.inf)
    np.fill_diagonal(d, 0.0)
    for k in range(V):
        d = np.minimum(d, d[:, k:k + 1] + d[k:k + 1, :])
    return d


def toy_batch(kind):
    """(x, y or None, targets or None) of a class's kind of batch; x holds (adj, feature) or (adj, feature, distance)"""
    tm = toy_molecules()
    x = [(a, f) for _, a, f, _ in tm]
    t = [tg for *_, tg in tm]
    if kind == "labels":
        t = [float(i % 3) for i in range(len(x))]
    if kind == "distance":
        x = [(a, f, hop_distance(a)) for a, f in x]
    if kind == "pairs":
        return x, x[1:] + x[:1], [a + b for a, b in zip(t, t[1:] + t[:1])]
    return x, None, (None if kind == "gram" else t)


def graph_text(g):
    out = "%d\n%s\n%s\n" % (len(g[0]), " ".join(str(int(v)) for v in np.asarray(g[0]).ravel()), " ".join("%.17g" % v for v in np.asarray(g[1]).ravel()))
    if len(g) == 3:
        out += " ".join("%.17g" % v for v in g[2].ravel()) + "\n"
    return out


def case_text(cid, cls, ctor, momentum, seed, batch, verb):
    x, y, t = batch
    s = "case %s %s %d %s %.17g %d\n" % (cid, cls, len(ctor), " ".join(str(c) for c in ctor), momentum, seed)
    s += "batch %d %d %d %d\n" % (len(x), x[0][1].shape[1], 1 if y else 0, 1 if len(x[0]) == 3 else 0)
    s += "".join(graph_text(g) for g in x) + ("".join(graph_text(g) for g in y) if y else "")
    s += "targets %d %s\n" % (len(t) if t else 0, " ".join("%.17g" % v for v in t) if t else "")
    return s + verb + "\n"


def run_program(exe, tmp_path, text):
    path = tmp_path / "cases.txt"
    path.write_text(text)
    r = subprocess.run([exe, str(path), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("DONE"), r.stdout[-1500:] + r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stdout.split("\n"):
        tok = line.split()
        if not tok or tok[0] == "DONE":
            continue
        if tok[0] == "case":
            cur = out.setdefault(tok[1], {"pair": []})
        elif tok[0] == "pair":
            cur["pair"].append([float.fromhex(v) for v in tok[1:]])
        elif tok[0] in ("decisions", "rate"):
            cur[tok[0]] = [float.fromhex(v) if "x" in v else int(v) for v in tok[1:]]
        else:
            cur[tok[0]] = np.array([float.fromhex(v) for v in tok[1:]])
    return out


def test_dropin_program_compiles_without_a_warning(gf, tmp_path):
    """every new header under -Wall without a warning (the program includes them all)"""
    compile_program(tmp_path)


def test_dropin_program_refuses_to_run_without_a_gpu(gf, tmp_path):
    """no CPU fallback: on a machine without a GPU the first constructor stops the program with the library's message"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible; the refusal path is exercised on CPU-only machines")
    exe = compile_program(tmp_path)
    (tmp_path / "cases.txt").write_text(case_text("a", "GCN_1D", VERTEX, GAMMA, SEED, toy_batch("single"), "steps 1 0.1"))
    r = subprocess.run([exe, str(tmp_path / "cases.txt"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_headers_compile_against_the_real_densegraph(tmp_path):
    """where the reference tree is present (GF_REFERENCE): the classes' templates instantiated on the real DenseGraph, -Wall, no warning"""
    ref = os.environ.get("GF_REFERENCE", "")
    if not os.path.exists(os.path.join(ref, "GraphFlow", "DenseGraph.h")) or not shutil.which("g++"):
        pytest.skip("no reference tree (GF_REFERENCE) or no g++ on this machine")
    src = tmp_path / "real_densegraph.cpp"
    src.write_text('#include "DenseGraph.h"\n#include "SMP_families_hip.h"\n#include "SMP_omega_hip.h"\n#include "SMP_classification_hip.h"\n'
                   '#include "SMP_physics_hip.h"\n'
                   "double a(GCN_1D_Distance_hip &n, DenseGraph **m, double *t) { return n.BatchLearn(4, m, t, 3, 0.1, 0.0).second + n.Learn(m[0], t[0], 3, 0.1, 0.0).first + n.Predict(m[0]) + n.Feature(m[0])[0]; }\n"
                   "double b(GCN_1D_Kernel_hip &n, DenseGraph **m, double *t) { return n.BatchLearn(4, m, m, t, 3, 0.1, 0.0).second + n.Learn(m[0], m[1], t[0], 3, 0.1, 0.0).first + n.getLoss(4, m, m, t); }\n"
                   "double c(GCA_1D_hip &n, DenseGraph **m, double **mat) { n.Predict(m[0], mat); return n.BatchLearn(4, m, 3, 0.1, 0.0).second + n.Learn(m[0], 3, 0.1, 0.0).first + n.BatchLearn(4, m, 0.1).first; }\n"
                   "double d(SMP_omega_hip &n, SMP_2D_ver6_classification_hip &k, SMP_omega_physics_hip &p, DenseGraph **m, double *t) {\n"
                   "    return n.Learn(m[0], t[0], 3, 0.1, 0.0).first + k.BatchLearn(4, m, t, 3, 0.1, 0.0).first + p.Learn(m[0], t[0], 3, 0.1, 0.0).second; }\n")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-c", "-I" + os.path.join(ref, "GraphFlow"), "-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                        "-o", str(tmp_path / "real_densegraph.o"), str(src)], capture_output=True, text=True)
    ours = "\n".join(ln for ln in r.stderr.split("\n") if "_hip.h" in ln)   # (the reference's own headers warn; ours must not)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in ours, ours[-3000:]


def wrapper_steps(smp, make, kind):
    """the same three BatchLearn steps through the Python wrapper: (params0, pairs, params, predictions, net, p)"""
    torch = pytest.importorskip("torch")
    net = make(smp)
    adam = isinstance(net, smp.SMPTheta) and type(net) is smp.SMPTheta
    C.CDLL(None).srand(SEED)
    p0 = net.uniform_init()
    p = dev(p0)
    x, y, t = toy_batch(kind)
    net.prepare(x, y) if y else net.prepare(x)
    tg = dev(np.array(t)) if t else None
    g = torch.empty_like(p)

    def loss():
        out = net.forward(p) if kind == "gram" else net.forward(p, tg)[1]
        return sum(float(v) for v in out.cpu().numpy())   # (doubles, ascending: the classes' loop)

    pairs = []
    for _ in range(STEPS):
        before = loss()
        net.backward(p, g)
        net.adam_step(p, g, LR, len(x)) if adam else net.momentum_step(p, g, LR, len(x), GAMMA)
        pairs.append([before, loss()])
    return p0, pairs, p, net, tg


def predictions(net, p, kind, n):
    """Predict of every sample alone, as the classes do it: one sample per forward"""
    x, y, _ = toy_batch(kind)
    out = []
    for i in range(n):
        net.prepare(x[i:i + 1], y[i:i + 1]) if y else net.prepare(x[i:i + 1])
        if kind == "gram":
            net.forward(p)
            out += [gm.astype(np.float64).ravel() for gm in net.gram()]
        else:
            out.append(f64(net.forward(p)[0]))
    return np.concatenate(out)


@pytest.mark.gpu
def test_every_dropin_is_its_python_wrapper_and_its_real_class(gf, tmp_path):
    torch = pytest.importorskip("torch")
    from graphflow_amd import smp
    exe = compile_program(tmp_path)
    text = "".join(case_text(name, name, ctor, GAMMA, SEED, toy_batch(kind), "steps %d %.17g" % (STEPS, LR)) for name, (ctor, _, kind) in DROPINS.items())
    out = run_program(exe, tmp_path, text)
    assert sorted(out) == sorted(DROPINS)
    for name, (ctor, make, kind) in DROPINS.items():
        got = out[name]
        p0, pairs, p, net, tg = wrapper_steps(smp, make, kind)
        print(name, got["pair"], pairs)
        assert np.array_equal(got["params0"].astype(np.float32), p0), name
        assert got["pair"] == pairs, name
        assert np.array_equal(got["params"].astype(np.float32), p.cpu().numpy()), name
        # the checkpoint: "%g " per weight, in the wrapper's save_model order
        mine = tmp_path / (name + "_py.txt")
        net.save_model(p, mine)
        text_cpp = (tmp_path / (name + ".txt")).read_text()
        assert text_cpp == mine.read_text() and len(text_cpp.split()) == net.n_params, name
        q = net.load_model(torch.zeros_like(p), mine)
        n = len(toy_batch(kind)[0])
        assert np.array_equal(got["predict"], predictions(net, p, kind, n)), name
        assert np.array_equal(got["reloaded"], predictions(net, q, kind, n)), name
        net.close()


def initial_weight_records():
    """The real constructors' params0 the goldens hold beside the trajectories: id -> (class, constructor integers, seed, params0).  With
    recorded() every class of DROPINS meets its real class's initial weights."""
    out = {}
    z = kit.load_golden("smp_1d.npz")   # cfg = version, L, C, D, has_WL_ordering, maxV, nClass, seed
    names = {(1, 0): "SMP_1D", (2, 0): "SMP_1D_ver2", (3, 0): "SMP_1D_ver3", (1, 1): "SMP_1D_classification", (3, 1): "SMP_1D_ver3_classification"}
    for k in range(1, 6):
        version, L, Cn, D, wl, maxV, nClass, seed = (int(v) for v in z["init_k%d__cfg" % k])
        assert wl == 1
        out["1d_k%d" % k] = (names[version, int(nClass > 0)], ((nClass,) if nClass else ()) + (maxV, L, Cn, 4, D), seed, z["init_k%d__params0" % k])
    z = kit.load_golden("smp_2d.npz")   # cfg = form, ...
    names = {(1, 0): "SMP_2D", (2, 0): "SMP_2D_ver4", (1, 1): "SMP_2D_classification", (2, 1): "SMP_2D_ver4_classification"}
    for k in range(1, 5):
        form, L, Cn, D, wl, maxV, nClass, seed = (int(v) for v in z["init_k%d__cfg" % k])
        assert wl == 1
        out["2d_k%d" % k] = (names[form, int(nClass > 0)], ((nClass,) if nClass else ()) + (maxV, L, Cn, 4, D), seed, z["init_k%d__params0" % k])
    z = kit.load_golden("smp_unrestricted.npz")   # cfg = form, L, C, D, has_WL_ordering, maxV, seed
    names = {1: "Unrestricted_SMP_1D", 2: "Unrestricted_SMP_1D_ver2", 3: "Unrestricted_SMP_2D"}
    for form in (1, 2, 3):
        _, L, Cn, D, wl, maxV, seed = (int(v) for v in z["init_u%d__cfg" % form])
        assert wl == 1
        out["u%d" % form] = (names[form], (maxV, L, Cn, 4, D), seed, z["init_u%d__params0" % form])
    return out


def checkpoint_records():
    """The real classes' own save_model files in the goldens, with the weights they were written from:
    id -> (class, constructor integers, params, the file's bytes)"""
    out = {}

    def add(fname, key, cls_of, ctor_of):
        z = kit.load_golden(fname)
        tag = str(z[key + "tag"])
        cfg = [int(v) for v in z[tag + "__cfg"]]
        V = len(z[tag + "__adj"]) if tag + "__adj" in z else 0
        out[fname[4:-4] + "_" + tag] = (cls_of(cfg), ctor_of(cfg, V), z[tag + "__params"], bytes(z[key + "text"]))

    vertex = {1: "NeuralFingerprint", 2: "GCN_1D", 3: "GCN_2D", 6: "GCN_3D", 4: "GRU_GCN_1D", 5: "GRU_GCN_2D", 7: "GRU_GCN_3D"}
    for fname in ("smp_neighbourhood.npz", "smp_gru_gcn.npz", "smp_third_order.npz"):   # cfg = form, L, H, D, R, V
        add(fname, "checkpoint__", lambda c: vertex[c[0]], lambda c, V: (c[1], c[5], 4, c[2], c[3], c[4]))
    add("smp_distance.npz", "checkpoint__", lambda c: "GCN_%dD_Distance" % {2: 1, 3: 2, 6: 3}[c[0]],   # cfg = form, L, H, D, R, V, M
        lambda c, V: (c[1], c[6], 4, c[2], c[3], c[4]))
    add("smp_matrix_form.npz", "checkpoint__", lambda c: "GCN_MW", lambda c, V: (c[0], V, 4, c[1], c[2]))   # cfg = L, H, D
    for form, d in ((2, 1), (3, 2), (6, 3)):   # cfg = form, L, H, D, R, M
        add("smp_pair_gram.npz", "checkpoint_p%d__" % form, lambda c, d=d: "GCN_%dD_Kernel" % d, lambda c, V: (c[1], c[5], 4, c[2], c[3], c[4]))
    add("smp_pair_gram.npz", "checkpoint_g__", lambda c: "GCA_1D", lambda c, V: (c[1], c[5], 4, c[2], c[3], c[4]))
    for form in (1, 2):   # cfg = form, L, M, D
        add("smp_cgcn.npz", "checkpoint_c%d__" % form, lambda c: "CGCN_%dD" % c[0], lambda c, V: (c[1], c[2], 4, c[3]))
    return out


def test_every_class_meets_its_real_constructor():
    """a trajectory record (its params0) or an initial-weight record of the real class exists for every one of the 32 classes"""
    assert sorted(set(recorded()) | {v[0] for v in initial_weight_records().values()}) == sorted(DROPINS)
    assert {v[0] for v in initial_weight_records().values()} >= set(UNRECORDED)
    assert len(checkpoint_records()) == 11


@pytest.mark.gpu
def test_constructors_draw_the_real_classes_weights(gf, tmp_path):
    """after srand(seed) the drop-in's weights are the real constructor's params0, bit for bit: the twelve records beside the
    trajectories -- every class without a recorded trajectory among them"""
    exe = compile_program(tmp_path)
    recs = initial_weight_records()
    out = run_program(exe, tmp_path, "".join("case %s %s %d %s %.17g %d\ninit\n" % (cid, cls, len(ctor), " ".join(str(c) for c in ctor), GAMMA, seed)
                                              for cid, (cls, ctor, seed, _) in recs.items()))
    for cid, (cls, ctor, seed, params0) in recs.items():
        assert np.array_equal(out[cid]["params0"].astype(np.float32), params0.astype(np.float32)), (cid, cls)


@pytest.mark.gpu
def test_checkpoints_are_the_real_classes_files(gf, tmp_path):
    """at the weights a real class saved, the drop-in's save_model writes that class's file, token for token (the distance models channel
    by channel); a second object that load_model's the class's own file holds the float32 of its values, each at its registration-order place"""
    exe = compile_program(tmp_path)
    recs, text = checkpoint_records(), ""
    for cid, (cls, ctor, params, ref) in recs.items():
        (tmp_path / (cid + "_reference.txt")).write_bytes(ref)
        text += "case %s %s %d %s %.17g %d\ncheckpoint %d %s\n" % (cid, cls, len(ctor), " ".join(str(c) for c in ctor), GAMMA, SEED, len(params),
                                                                  " ".join("%.17g" % v for v in params))
    out = run_program(exe, tmp_path, text)
    for cid, (cls, ctor, params, ref) in recs.items():
        assert (tmp_path / (cid + ".txt")).read_text().split() == ref.decode().split(), (cid, cls)
        want = np.array([float("%g" % v) for v in params.astype(np.float32)], dtype=np.float32)
        assert np.array_equal(out[cid]["loaded"].astype(np.float32), want), (cid, cls)


def test_which_classes_have_a_recorded_trajectory():
    rec = recorded()
    assert sorted(set(rec) | set(UNRECORDED)) == sorted(DROPINS) and not set(rec) & set(UNRECORDED)
    assert len(rec) == 24


@pytest.mark.gpu
def test_recorded_trajectories_through_the_dropins(gf, tmp_path):
    """every class whose family golden holds a BatchLearn trajectory, at the golden's own constructor arguments, seed, molecules, targets
    and rate: params0 bit for bit, the loss pairs and final weights within field_suite.check_momentum_trajectory's bounds -- what the
    family's own *_gpu.py test asks of the Python wrapper on the same record"""
    exe = compile_program(tmp_path)
    rec, text = recorded(), ""
    for name, (z, pre, ctor, gamma, seed, steps, lr, (x, y, target)) in rec.items():
        text += case_text(name, name, ctor, gamma, seed, (x, y, list(z[pre + "targets"]) if target else None), "steps %d %.17g" % (steps, lr))
    out = run_program(exe, tmp_path, text)
    for name, (z, pre, ctor, gamma, seed, steps, lr, _) in rec.items():
        got = out[name]
        assert np.array_equal(got["params0"].astype(np.float32), z[pre + "params0"].astype(np.float32)), name
        for it in range(steps):
            before, after = got["pair"][it]
            assert abs(before - z[pre + "losses"][it, 0]) <= TOL * max(1.0, before), (name, it)
            assert abs(after - z[pre + "losses"][it, 1]) <= 5 * TOL * max(1.0, after), (name, it)
        err = np.abs(got["params"] - z[pre + "params"])
        print(name, got["pair"], "max %.3g median %.3g" % (err.max(), np.median(err)))
        assert err.max() <= 0.005 * lr and np.median(err) <= 1e-6, name


@pytest.mark.gpu
def test_iterative_methods_return_the_recorded_pairs_and_decisions(gf, tmp_path):
    exe = compile_program(tmp_path)
    z = kit.load_golden("smp_iterative.npz")
    runs, text = recorded_runs(z), ""
    for name, run in runs:
        pre = "%s__%s__" % (name, run)
        kind, nIter = (int(v) for v in z[pre + "cfg"])
        ctor = FIT_CLASSES[name][1][:5] if name == "SMP_omega_physics" else FIT_CLASSES[name][1]
        x, y, t = batch_of(name, kind)
        text += case_text(name + "." + run, name, ctor, float(z[pre + "momentum"][0]), int(z[pre + "seed"][0]), (x, y, t),
                          "fit %d %d %.17g %.17g" % (kind, nIter, float(z[pre + "lr"][0]), float(z[pre + "eps"][0])))
    out = run_program(exe, tmp_path, text)
    for name, run in runs:
        pre, got = "%s__%s__" % (name, run), out[name + "." + run]
        want, pair, lr = list(z[pre + "decisions"]), z[pre + "pair"], float(z[pre + "lr"][0])
        err = np.abs(got["params"] - z[pre + "params"])
        print(pre, got["pair"], got["decisions"], got["rate"], "max %.3g median %.3g" % (err.max(), np.median(err)))
        assert np.array_equal(got["params0"].astype(np.float32), z[pre + "params0"].astype(np.float32)), pre
        assert got["decisions"] == want and got["rate"][0] == z[pre + "final_lr"][0] and got["rate"][1] == len(want), pre
        first, second = got["pair"][0]
        assert abs(first - pair[0]) <= TOL * max(1.0, abs(pair[0])), pre
        assert abs(second - pair[1]) <= 5 * TOL * max(1.0, abs(pair[1])), pre
        assert err.max() <= 0.005 * lr and np.median(err) <= 1e-6, pre
