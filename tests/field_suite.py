"""What the GPU suites of the field-level families share (test_smp_theta_gpu.py, test_smp_1d_gpu.py, test_smp_2d_gpu.py,
test_smp_2d_ver5_gpu.py, test_smp_unrestricted_gpu.py, test_ccn_1d_gpu.py): the device helpers, the tolerance, and the flows every suite
runs on its own constructor, batch and fp64 restatement.  A plain module: no fixtures, no pytest settings.  A batch is a list of
(adjacency, features), or a tuple (graphs 1, graphs 2) of two such lists for a model on pairs of graphs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from util import rel_err

try:
    import torch
except ImportError:   # (the suites skip themselves; blockwise needs no device)
    torch = None

TOL = 1e-5   # the suite's end-to-end tolerance (tests/util.py: rel_err): graph feature, prediction, loss and every parameter block
HERE = os.path.dirname(os.path.abspath(__file__))
_GOLDEN, _PACKED = {}, {}


def dev(x, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=dtype)).cuda()


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def load_golden(name):
    """the arrays of tests/golden/<name>, read once"""
    if name not in _GOLDEN:
        with np.load(os.path.join(HERE, "golden", name)) as z:
            _GOLDEN[name] = {k: z[k] for k in z.files}
    return _GOLDEN[name]


def blockwise(x, ref, blocks):
    """the largest rel_err over the parameter blocks: one norm over the whole vector cannot see an error confined to a small block"""
    off, worst = 0, (0.0, "")
    for name, n in blocks:
        worst = max(worst, (rel_err(x[off:off + n], ref[off:off + n]), name))
        off += n
    assert off == ref.size
    return worst


def prepare(net, mols):
    net.prepare(*mols) if isinstance(mols, tuple) else net.prepare(mols)


def fields_of(net, m, nV):
    """phi_l(v) of molecule m, every level and vertex, from the handle"""
    return [[net.receptive_field(m, l, v) for v in range(nV)] for l in range(net.cfg.nLevels + 1)]


def run_net(make_net, mols, targets, params, *, n_class=0, want_fields=False, inspect=None):
    """One forward and backward of make_net() on the batch: [everything forward returns (predict, loss(, feature)), grads (, scores,
    probability) (, fields) (, inspect(net))], the arrays as float64"""
    net = make_net()
    assert net.n_params == np.asarray(params).size
    prepare(net, mols)
    p = dev(params)
    out = [f64(t) for t in net.forward(p, dev(targets))]
    grads = torch.empty(net.n_params, device="cuda")
    net.backward(p, grads)
    out.append(f64(grads))
    if n_class:
        out += [f64(t) for t in net.scores()]
    if want_fields:
        out.append([fields_of(net, m, len(mols[m][0])) for m in range(len(mols))])
    if inspect:
        out.append(inspect(net))
    net.close()
    return out


def packed_case(key, batch, params, run, reference, **run_kw):
    """(mols, targets, params, out, ref) of a suite's packing batch, on the device and in fp64, computed once per key (the suite's name in
    front): batch() -> (mols, targets); params() -> the flat vector; run(mols, targets, params, **run_kw) -> run_net's list;
    reference(mols, targets, params, out) -> whatever the suite compares with"""
    if key not in _PACKED:
        mols, tg = batch()
        p = params()
        out = run(mols, tg, p, **run_kw)
        _PACKED[key] = (mols, tg, p, out, reference(mols, tg, p, out))
    return _PACKED[key]


def check_isolated(case, k, run, blocks, outputs=False):
    """With every other target equal to its prediction only sample k has a loss gradient: the batch gradient is then that sample's own;
    with `outputs`, its prediction (and graph feature, where forward returns one) are those it has alone."""
    mols, tg, params, out = case[:4]
    t2 = out[0].astype(np.float32).astype(np.float64).copy()   # (the device's own fp32 predictions: y - t is exactly 0)
    t2[k] = tg[k]
    batch = run(mols, t2, params)
    alone = run(tuple(g[k:k + 1] for g in mols) if isinstance(mols, tuple) else mols[k:k + 1], tg[k:k + 1], params)
    e = blockwise(batch[-1], alone[-1], blocks)
    assert np.abs(alone[-1]).max() > 0
    assert e[0] <= TOL, e
    if outputs:
        assert rel_err(batch[0][k:k + 1], alone[0]) <= TOL
        assert len(batch) == 3 or rel_err(batch[2][k], alone[2][0]) <= TOL


def check_same_bits(case, run):
    """a second run of the packed case gives the bits of the first"""
    mols, tg, params, out = case[:4]
    again = run(mols, tg, params)
    for x, y in zip(out[:len(again)], again):
        assert np.array_equal(x, y)


def run_under_poison(test_file, selector, timeout=600):
    """GF_POISON=1 (every buffer the library hands out without contents starts as NaN patterns; read once per process): the selected
    tests of test_file (a path or a list of paths) once more in a fresh child process"""
    env = dict(os.environ, GF_POISON="1")
    files = [os.path.abspath(f) for f in ([test_file] if isinstance(test_file, str) else test_file)]
    r = subprocess.run([sys.executable, "-m", "pytest", *files, "-q", "-x", "-m", "gpu", "-k", selector, "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=timeout)
    tail = (r.stdout + r.stderr)[-2000:]
    assert r.returncode == 0, tail
    assert " passed" in tail and "failed" not in tail, tail


def check_momentum_trajectory(net, step, z, prefix, mols, seed, n_iter, lr, init=None, show="trajectory: max %s median %s"):
    """BatchLearn steps of the real class, recorded in z[prefix + ...]: initial weights from init() (net.uniform_init) after the same
    srand, then n_iter times forward, backward, step(p, grads), forward; the loss before and after every step and the final weights
    against the record.  `show`: the format of the last printed line, None to print nothing.  Returns the final weights."""
    C.CDLL(None).srand(seed)
    p = dev((init or net.uniform_init)())
    assert np.array_equal(p.cpu().numpy(), z[prefix + "params0"].astype(np.float32))
    prepare(net, mols)
    tg = dev(z[prefix + "targets"])
    grads = torch.empty(net.n_params, device="cuda")
    for it in range(n_iter):
        before = float(net.forward(p, tg)[1].sum())
        net.backward(p, grads)
        step(p, grads)
        after = float(net.forward(p, tg)[1].sum())
        if show:
            print(it, before, z[prefix + "losses"][it, 0], after, z[prefix + "losses"][it, 1])
        assert abs(before - z[prefix + "losses"][it, 0]) <= TOL * max(1.0, before), it
        assert abs(after - z[prefix + "losses"][it, 1]) <= 5 * TOL * max(1.0, after), it
    err = np.abs(f64(p) - z[prefix + "params"])
    if show:
        print(show % (err.max(), np.median(err)))
    assert err.max() <= 0.005 * lr
    assert np.median(err) <= 1e-6
    return p


def check_checkpoint_round_trip(net, tag, mol, params, target, golden_predict, reference, tmp_path):
    """save -> load in the reference's text format (six significant digits per value, registration order), then the loaded model's
    prediction against the golden's and against reference(loaded values, fields), the restatement's prediction.  Closes net."""
    p = dev(params)
    path = tmp_path / (tag + ".txt")
    net.save_model(p, path)
    text = path.read_text().split()
    assert len(text) == net.n_params and text == ["%g" % x for x in params]
    q = net.load_model(torch.zeros_like(p), path)
    loaded = q.cpu().numpy()
    assert np.array_equal(loaded, np.array([float(t) for t in text], dtype=np.float32))
    net.prepare([mol])
    pred = f64(net.forward(q, dev(target))[0])
    fields = fields_of(net, 0, len(mol[0]))
    net.close()
    r = reference(loaded, fields)
    print(tag, pred, r, golden_predict)
    assert rel_err(pred, [r]) <= TOL, tag
    assert rel_err(pred, np.atleast_1d(golden_predict)) <= TOL, tag


def check_permutation_invariance(adj, x, run, reference):
    """Feature of one molecule under a random vertex permutation.  The fp64 restatement's own difference under the same permutation is at
    rounding level first, so the property holds for the inputs chosen.  run(mols, targets) -> run_net's list with the fields;
    reference(adj, x, fields) -> the restatement's graph feature."""
    perm = np.random.default_rng(0).permutation(len(adj))
    padj, px = adj[np.ix_(perm, perm)], x[perm]
    a = run([(adj, x)], np.array([1.0]))
    b = run([(padj, px)], np.array([1.0]))
    ra = reference(adj, x, a[4][0])
    rb = reference(padj, px, b[4][0])
    assert rel_err(rb, ra) <= 1e-12
    assert rel_err(b[2], a[2]) <= TOL
    assert rel_err(a[2][0], ra) <= TOL


def traced_counts(net, step):
    """{kernel: launches} of step() under gf_ctx_set_timing"""
    net.ctx.set_timing(True)
    step()
    counts = {k: n for k, (_, n) in net.ctx.timings().items()}
    net.ctx.set_timing(False)
    return counts
