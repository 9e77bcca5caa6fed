"""Python handle on the batched SMP_omega driver of the C ABI (gf_smp_*).  Plumbing only: torch owns the parameter,
gradient and output buffers; everything else lives in libgf_hip.so."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .ops import default_context


class SMPConfig(C.Structure):
    _fields_ = [("nLevels", C.c_int), ("nChanels", C.c_int), ("nFeatures", C.c_int), ("nDepth", C.c_int),
                ("max_receptive_field", C.c_int), ("has_WL_ordering", C.c_int), ("nContractions", C.c_int),
                ("custom_matmul", C.c_int), ("physics", C.c_int), ("first_order", C.c_int), ("max_nVertices", C.c_int),
                ("steerable_2d", C.c_int), ("unrestricted", C.c_int), ("neighbourhood", C.c_int), ("max_Radius", C.c_int),
                ("matrix_form", C.c_int), ("nNeighbors", C.c_int), ("nChanels2", C.c_int), ("nDense", C.c_int),
                ("distance_channel", C.c_int), ("readout", C.c_int)]


class SMPConfigCovariant(SMPConfig):
    """gf_smp_config in full: SMPConfig's fields, then the trailing `covariant` (1: CGCN_1D, 2: CGCN_2D).  SMPConfig itself stays the
    structure up to `readout`: the library's prototypes take a configuration through _lib.ConfigPointer, which hands a structure of an
    earlier, shorter layout on with a zero tail -- what the C ABI defines as "everything as before"."""
    _fields_ = [("covariant", C.c_int)]


assert C.sizeof(SMPConfigCovariant) == _lib.SMP_CONFIG_BYTES


class SMPOmega:
    """Batched SMP_omega (GraphFlow/SMP_omega.h).  Parameters/gradients are one flat fp32 tensor in the reference's
    registration order: H[C, F(D+1)], (K_l[18C, C], b_l[C]) for l = 1..L, W[C]."""

    def __init__(self, nLevels, nChanels, nFeatures, nDepth, max_receptive_field, has_WL_ordering=True, ctx=None,
                 nContractions=18, custom_matmul=False, physics=False):
        """nContractions / custom_matmul select the SMP_2D_ver6 (10, True) / ver7 (50, True) / ver8 (18, True) wirings;
        physics=True makes the handle one tower of the _physics / _pairgraphs models (see gf_smp_config.physics)."""
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.cfg = SMPConfig(nLevels, nChanels, nFeatures, nDepth, max_receptive_field, 1 if has_WL_ordering else 0,
                             nContractions, 1 if custom_matmul else 0, 1 if physics else 0)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def pack(molecules, coulomb=None):
        """The flat host arrays gf_smp_prepare takes (vertex counts, adjacency and feature matrices back to back): a data
        loader builds these once per batch; prepare() accepts the result in place of the molecule list."""
        nV = np.array([len(m[0]) for m in molecules], dtype=np.int32)
        adj = np.concatenate([np.ascontiguousarray(m[0], dtype=np.int32).ravel() for m in molecules])
        feat = np.concatenate([np.ascontiguousarray(m[1], dtype=np.float64).ravel() for m in molecules])
        cm = None
        if coulomb is not None:
            cm = np.concatenate([np.ascontiguousarray(c, dtype=np.float64).ravel() for c in coulomb])
            assert cm.size == adj.size
        return {"nV": nV, "adj": adj, "feature": feat, "coulomb": cm}

    def prepare(self, molecules, coulomb=None):
        """molecules: list of (adj int[V,V], feature float[V,F]) or the dict pack() returns; coulomb: optional list of
        float[V,V] Coulomb matrices (the use_coulomb variant of SMP_omega).  Host graph preparation + upload (blocking)."""
        pk = molecules if isinstance(molecules, dict) else self.pack(molecules, coulomb)
        nV, adj, feat, cm = pk["nV"], pk["adj"], pk["feature"], pk["coulomb"]
        molecules = nV
        self.ctx.check(self.lib.gf_smp_prepare_coulomb(self.handle, len(nV), nV.ctypes.data_as(C.POINTER(C.c_int)),
                                                       adj.ctypes.data_as(C.POINTER(C.c_int)),
                                                       feat.ctypes.data_as(C.POINTER(C.c_double)),
                                                       cm.ctypes.data_as(C.POINTER(C.c_double)) if cm is not None else None))
        self.n_mol = len(molecules)
        dev = self.ctx.device
        self.predict = torch.empty(self.n_mol, dtype=torch.float32, device=dev)
        self.loss = torch.empty(self.n_mol, dtype=torch.float32, device=dev)
        self.feature = torch.empty((self.n_mol, int(self.lib.gf_smp_feature_width(self.handle))), dtype=torch.float32, device=dev)

    def _flat(self, t, name):
        """params / grads must be exactly the flat model: float32, contiguous, on the context's device, n_params long."""
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                and t.numel() == self.n_params and t.device == self.ctx.device):
            raise TypeError("%s must be a contiguous float32 tensor of %d elements on %s" % (name, self.n_params, self.ctx.device))
        return C.c_void_p(t.data_ptr())

    def backward_features(self, params, grads, d_feature, accumulate=False):
        """Physics tower: the reverse sweep from the gradient of the feature rows (what the head's backward returns)."""
        self._flat(params, "params")
        self._flat(grads, "grads")
        if not (d_feature.is_cuda and d_feature.dtype == torch.float32 and d_feature.is_contiguous() and d_feature.shape == self.feature.shape):
            raise TypeError("d_feature must be a contiguous float32 CUDA tensor shaped like the feature rows")
        self.ctx.check(self.lib.gf_smp_backward_features(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()),
                                                         C.c_void_p(d_feature.data_ptr()), 1 if accumulate else 0))
        return grads

    def forward(self, params, targets=None):
        self._flat(params, "params")
        if self.cfg.physics:
            if targets is not None:
                raise TypeError("a physics tower has no loss of its own: targets go to the head")
            self.ctx.check(self.lib.gf_smp_forward(self.handle, C.c_void_p(params.data_ptr()), None, None, None,
                                                   C.c_void_p(self.feature.data_ptr())))
            return self.feature
        if targets is not None and not (targets.is_cuda and targets.dtype == torch.float32 and targets.is_contiguous()
                                        and targets.numel() == self.n_mol):
            raise TypeError("targets must be a contiguous float32 CUDA tensor with one value per molecule (%d)" % self.n_mol)
        t = C.c_void_p(targets.data_ptr()) if targets is not None else None
        self.ctx.check(self.lib.gf_smp_forward(self.handle, C.c_void_p(params.data_ptr()), t,
                                               C.c_void_p(self.predict.data_ptr()), C.c_void_p(self.loss.data_ptr()),
                                               C.c_void_p(self.feature.data_ptr())))
        return self.predict, self.loss, self.feature

    def backward(self, params, grads, accumulate=False):
        self._flat(params, "params")
        self._flat(grads, "grads")
        self.ctx.check(self.lib.gf_smp_backward(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()),
                                                1 if accumulate else 0))
        return grads

    def adam_step(self, params, grads, learning_rate, nBatch):
        """Adam::Learn(learning_rate, nBatch) as SMP_omega::BatchLearn applies it (SMP_omega.h:820-821); grads = batch sum."""
        self._flat(params, "params")
        self._flat(grads, "grads")
        self.ctx.check(self.lib.gf_smp_adam_step(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()),
                                                 float(learning_rate), int(nBatch)))
        return params

    def momentum_step(self, params, grads, learning_rate, nBatch, gamma=0.9):
        """Momentum::Learn(learning_rate, nBatch) (Momentum.h:64-71): the optimiser of SMP_2D_ver6-8."""
        self._flat(params, "params")
        self._flat(grads, "grads")
        self.ctx.check(self.lib.gf_smp_momentum_step(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()),
                                                     float(learning_rate), int(nBatch), float(gamma)))
        return params

    def adam_reset(self):
        """zero state for every optimiser of the handle, and no recorded kind"""
        self.ctx.check(self.lib.gf_smp_adam_reset(self.handle))

    def optimiser_step(self, params, grads, kind, learning_rate, nBatch, gamma=0.9, beta1=0.0, beta2=0.0, rho=0.0, epsilon=0.0):
        """sgd->Learn(learning_rate, nBatch) for kind "adam", "momentum", "sgd", "adamax" or "adadelta" (or gf_optim_config's number);
        constants left at 0 are the classes' defaults.  A kind other than the handle's last one is refused until adam_reset()."""
        self._flat(params, "params")
        self._flat(grads, "grads")
        cfg = _lib.OptimConfig(_lib.OPTIMISERS.get(kind, kind), int(nBatch), float(learning_rate), float(gamma), float(beta1), float(beta2),
                               float(rho), float(epsilon))
        self.ctx.check(self.lib.gf_smp_optimiser_step(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()), C.byref(cfg)))
        return params

    def regularise(self, params, grads, norm, lam, times=1):
        """L1Regularization (norm 1) / L2Regularization (norm 2): grads += times * the term of backward(); returns the value"""
        self._flat(params, "params")
        self._flat(grads, "grads")
        value = C.c_double(0.0)
        self.ctx.check(self.lib.gf_smp_regularise(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()), int(norm), float(lam),
                                                  int(times), C.byref(value)))
        return value.value

    def param_blocks(self):
        """offsets [blocks + 1] of the blocks the class registers with sgd->add, into the flat parameter vector"""
        if getattr(self, "nClass", 0):
            return _lib.param_blocks("gf_smp_classifier_config_param_blocks", C.byref(self.cfg), self.nClass)
        return _lib.param_blocks("gf_smp_config_param_blocks", C.byref(self.cfg))

    def fit(self, params, grads, targets, nIterations, learning_rate, epsilon=0.0, kind=0, optimiser="adam", gamma=0.9):
        """The classes' iterative training calls on the prepared batch (gf_smp_fit): kind 0 = BatchLearn(nBatch, molecule, target,
        nIterations, learning_rate, epsilon), kind 1 = Learn(molecule, target, ...) on a batch of one sample.  optimiser "adam",
        "momentum" (with gamma), "sgd", "adamax" or "adadelta" (the classes' default constants).  targets: one float32 per sample on the
        device (None for the Gram auto-encoder).  Returns (report, decisions): the dict of gf_smp_fit_report and one entry per iteration
        run -- 1 kept, 2 restored, 3 restored and left, 4 left on error < epsilon."""
        self._flat(params, "params")
        self._flat(grads, "grads")
        if optimiser not in _lib.OPTIMISERS:
            raise ValueError("fit: optimiser %r (one of %s)" % (optimiser, ", ".join(sorted(_lib.OPTIMISERS))))
        cfg = _lib.FitConfig(int(kind), _lib.OPTIMISERS[optimiser], int(nIterations), float(learning_rate), float(epsilon), float(gamma))
        rep = _lib.FitReport()
        log = (C.c_ubyte * max(1, int(nIterations)))()
        t = C.c_void_p(targets.data_ptr()) if targets is not None else None
        self.ctx.check(self.lib.gf_smp_fit(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()), t, C.byref(cfg),
                                           C.byref(rep), log))
        report = {name: getattr(rep, name) for name, _ in _lib.FitReport._fields_}
        return report, list(log[:rep.iterations])

    def parameters_snapshot(self, params):
        """The classes' cache_parameters(): the values of params into the handle's cache (optimiser state is not part of it)."""
        self._flat(params, "params")
        self.ctx.check(self.lib.gf_smp_parameters_snapshot(self.handle, C.c_void_p(params.data_ptr())))

    def parameters_rollback(self, params):
        """The classes' restore_parameters(): the cached values back into params."""
        self._flat(params, "params")
        self.ctx.check(self.lib.gf_smp_parameters_rollback(self.handle, C.c_void_p(params.data_ptr())))
        return params

    def uniform_init(self):
        """Initial weights exactly as SMP_omega's constructor draws them from rand() (host numpy array; call srand first)."""
        out = np.zeros(self.n_params, dtype=np.float32)
        st = self.lib.gf_smp_uniform_init_host(C.byref(self.cfg), out.ctypes.data_as(C.POINTER(C.c_float)))
        if st != 0:
            raise RuntimeError("gf_smp_uniform_init_host failed")
        return out

    def save_model(self, params, path):
        """SMP_omega::save_model (SMP_omega.h:1033-1042): text checkpoint the reference's load_model reads."""
        self.ctx.check(self.lib.gf_smp_save_model(self.handle, C.c_void_p(params.data_ptr()), str(path).encode()))

    def load_model(self, params, path):
        """SMP_omega::load_model (SMP_omega.h:1044-1055) into the flat device parameter buffer."""
        self.ctx.check(self.lib.gf_smp_load_model(self.handle, C.c_void_p(params.data_ptr()), str(path).encode()))
        return params

    def set_fused(self, on=True):
        """Fused level kernels (default) vs the op-by-op pipeline; both give the same results within fp32 rounding."""
        self.ctx.check(self.lib.gf_smp_set_fused(self.handle, 1 if on else 0))

    def device_bytes(self):
        """(bytes held by the current batch, bytes the handle's pool keeps in total)."""
        used, res = C.c_size_t(0), C.c_size_t(0)
        self.ctx.check(self.lib.gf_smp_device_bytes(self.handle, C.byref(used), C.byref(res)))
        return int(used.value), int(res.value)

    def single_vertex_launches(self):
        """Launches so far of the level-1 kernels for single-vertex sources (they run under the general kernels' launch names)."""
        return int(self.lib.gf_smp_single_vertex_launches(self.handle))

    def empty_row_calls(self):
        """Level passes so far, forward or backward, that neither stored nor read O / dO of the level's empty rows (gf_smp_empty_row_calls)."""
        return int(self.lib.gf_smp_empty_row_calls(self.handle))

    def level_projected(self, level):
        """The level's projected matrix as the last pass left it, [rows][2 C] on the device: O after a forward, dO after a backward."""
        rows = self.level_sizes(level)[1]
        out = torch.empty((rows, 2 * self.cfg.nChanels), dtype=torch.float32, device=self.ctx.device)
        self.ctx.check(self.lib.gf_smp_level_projected_f32(self.handle, level, C.c_void_p(out.data_ptr())))
        torch.cuda.synchronize()
        return out

    def receptive_field(self, mol, level, v):
        buf = (C.c_int * 4096)()
        n = self.lib.gf_smp_receptive_field(self.handle, mol, level, v, buf, 4096)
        return list(buf[:n])

    def activation(self, mol, level, v):
        """f_level[v] of molecule `mol` after forward(): numpy [s, s, C] (level[l]->f[v]->value in the reference)."""
        s = len(self.receptive_field(mol, level, v))
        ch = self.cfg.nChanels
        if self.cfg.physics:   # a physics tower halves its channels from level to level (SMP_omega_physics.h:141-156)
            for _ in range(level):
                ch = max(1, ch // 2)
        out = np.empty((s, s, ch), dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out

    def reduced_adjacency(self, mol, level, v):
        """Reduced adjacency [s, s] of f_level[v] (level[l]->adj[v] in the reference), level >= 1."""
        s = len(self.receptive_field(mol, level, v))
        out = np.empty((s, s), dtype=np.float32)
        n = self.lib.gf_smp_read_reduced_adjacency(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_reduced_adjacency(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out

    def set_grad_allreduce(self, on=True):
        """Data-parallel runs (ctx.dist_init): backward() leaves the gradient summed over all ranks (default) or local."""
        self.ctx.check(self.lib.gf_smp_set_grad_allreduce(self.handle, 1 if on else 0))

    def level_sizes(self, level):
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        self.ctx.check(self.lib.gf_smp_level_sizes(self.handle, level, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def level_present_rows(self, level):
        """rows (a, b) of the level whose slab row is not structurally zero (gf_smp_level_present_rows)"""
        return int(self.lib.gf_smp_level_present_rows(self.handle, level))

    def level_pairs(self, level):
        """(node, neighbour) pairs of the level = sum of its receptive-field sizes (gf_smp_level_pairs)"""
        return int(self.lib.gf_smp_level_pairs(self.handle, level))

    def level_covered_rows(self, level):
        """rows (b, c) of the level that some source covers (gf_smp_level_covered_rows)"""
        return int(self.lib.gf_smp_level_covered_rows(self.handle, level))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gf_smp_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SMPGamma(SMPOmega):
    """Batched SMP_gamma (GraphFlow/SMP_gamma.h): the SMP_omega DAG with RisiContraction_4, no receptive-field cap and no
    reduced adjacency.  Parameters in registration order: H[C, F(D+1)], (K_l[4C, C], b_l[C]) for l = 1..L, W[C]."""

    def __init__(self, nLevels, nChanels, nFeatures, nDepth, max_nVertices, has_WL_ordering=True, ctx=None):
        super().__init__(nLevels, nChanels, nFeatures, nDepth, max_nVertices, has_WL_ordering, ctx=ctx, nContractions=4)


class SMPTheta(SMPOmega):
    """Batched SMP_theta (GraphFlow/SMP_theta.h), the first-order member of the family: f_l[v] is a matrix [s, C]; the children of a
    vertex are its neighbours within one hop; lambda1, lambda2 and the bias b exist per field size.  Parameters in registration order:
    H[C, F(D+1)]; for l = 1..L: (lambda1_s, lambda2_s, b_s[C]) for s = 1..max_nVertices, then K_l[2C, C]; W[C]."""

    def __init__(self, max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.cfg = self.config(max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(max_nVertices, max_receptive_field, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True):
        return SMPConfig(nLevels, nChanels, nFeatures, nDepth, max_receptive_field, 1 if has_WL_ordering else 0, 0, 0, 0, 1, max_nVertices)

    def activation(self, mol, level, v):
        """f_level[v] of molecule `mol` after forward(): numpy [s, C] (level[l]->f[v]->value in the reference)."""
        s = len(self.receptive_field(mol, level, v))
        out = np.empty((s, self.cfg.nChanels), dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class SMP1D(SMPTheta):
    """Batched SMP_1D (version 1), SMP_1D_ver2 (2) and SMP_1D_ver3 (3) of GraphFlow/SMP_1D*.h, and with nClass >= 2 their classifiers
    (SMP_1D_classification, SMP_1D_ver3_classification; a version-2 classifier is the same read-out on SMP_1D_ver2).  First order as
    SMP_theta, without a cap and without its [2C, C] matrix:
      1: z = lambda1_s S + lambda2_s sumS + b_s, C channels at every level, LeakyReLU slope 0.01;
      2: z = [lambda1_s S | lambda2_s sumS] + b_s, the channels double per level (C << l), slope 0;
      3: z = [lambda1_s S K_eye | lambda2_s sumS K_one] + b_s, likewise.
    Parameters in registration order: H[C, F(D+1)]; for l = 1..L: (lambda1_s, lambda2_s, b_s[C_l]) for s = 1..max_nVertices, then for
    version 3 K_eye and K_one [C_{l-1}, C_{l-1}]; W[C_L], or W[nClass, C_L] for a classifier.  The optimiser is Momentum: step().
    A classifier's forward(params, labels) returns (arg-max label, log p[label], graph_feature); scores() the logits and probabilities."""

    def __init__(self, version, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True, nClass=0, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.version, self.nClass = int(version), int(nClass)
        self.cfg = self.config(version, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering)
        h = C.c_void_p()
        if self.nClass:
            self.ctx.check(self.lib.gf_smp_create_classifier(self.ctx.handle, C.byref(self.cfg), self.nClass, C.byref(h)))
        else:
            self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(version, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True):
        if version not in (1, 2, 3):
            raise ValueError("SMP1D: version %r (1: SMP_1D, 2: SMP_1D_ver2, 3: SMP_1D_ver3)" % (version,))
        return SMPConfig(nLevels, nChanels, nFeatures, nDepth, max_nVertices, 1 if has_WL_ordering else 0, 0, 0, 0, 1 + version, max_nVertices)

    def level_channels(self, level):
        return self.cfg.nChanels if self.version == 1 else self.cfg.nChanels << level

    def step(self, params, grads, learning_rate, nBatch, gamma=0.9):
        """Momentum::Learn(learning_rate, nBatch) as the classes' BatchLearn applies it; grads = the batch sum of backward()."""
        return self.momentum_step(params, grads, learning_rate, nBatch, gamma)

    def scores(self):
        """(scores, probability) of a classifier's last forward, [nMol, nClass] each."""
        if not self.nClass:
            raise TypeError("SMP1D.scores: not a classifier (nClass = 0)")
        return SMPClassifier.scores(self)

    def uniform_init(self):
        """Initial weights exactly as the reference constructor draws them from rand() (host numpy array; call srand first)."""
        return SMPClassifier.uniform_init(self) if self.nClass else SMPOmega.uniform_init(self)

    def activation(self, mol, level, v):
        """f_level[v] of molecule `mol` after forward(): numpy [s, C_level]."""
        s = len(self.receptive_field(mol, level, v))
        out = np.empty((s, self.level_channels(level)), dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class SMP2D(SMP1D):
    """Batched SMP_2D (form "2d") and SMP_2D_ver4 (form "ver4") of GraphFlow/SMP_2D.h, SMP_2D_ver4.h, and with n_class >= 2 their
    classifiers (SMP_2D_classification, SMP_2D_ver4_classification): the second-order steerable models, gf_smp_config.steerable_2d.
    f_l[v] is [s, s, C_l]; with S = the children's tensors summed on the positions of phi_l(v) plus scalar_l * adj_v, col = its column sums:
      "2d":   z = lambda1_s S + lambda2_s col + b_s, C channels at every level;
      "ver4": z = [lambda1_s S | lambda2_s col] + b_s, the channels double per level (C << l);
      "ver5": z = K_l [lambda1_s S | lambda2_s col] + b_s (SMP_2D_ver5, steerable_2d = 5): ver4's level projected back to C channels by a
              learned K_l[C, 2C], so the width stays constant; nChanels <= 128; no classifier (n_class is refused).
    Parameters in registration order: H[C, F(D+1)]; for l = 1..L: (lambda1_s[C_{l-1}], lambda2_s[C_{l-1}], b_s[C_l]) for
    s = 1..max_nVertices, then ("ver5" only) K_l[C, 2C], then scalar_l[C_{l-1}]; W[C_L], or W[n_class, C_L] for a classifier.  The optimiser
    is Momentum: step().
    A classifier's forward(params, labels) returns (arg-max label, log p[label], graph_feature); scores() the logits and probabilities."""

    FORMS = {"2d": 1, "ver4": 2, "ver5": 5}

    def __init__(self, form, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True, n_class=0, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.form, self.nClass = form, int(n_class)
        self.cfg = self.config(form, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering)
        h = C.c_void_p()
        if self.nClass:
            self.ctx.check(self.lib.gf_smp_create_classifier(self.ctx.handle, C.byref(self.cfg), self.nClass, C.byref(h)))
        else:
            self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(form, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True):
        if form not in SMP2D.FORMS:
            raise ValueError("SMP2D: form %r (\"2d\": SMP_2D, \"ver4\": SMP_2D_ver4, \"ver5\": SMP_2D_ver5)" % (form,))
        return SMPConfig(nLevels, nChanels, nFeatures, nDepth, max_nVertices, 1 if has_WL_ordering else 0, 0, 0, 0, 0, max_nVertices,
                         SMP2D.FORMS[form])

    def level_channels(self, level):
        return self.cfg.nChanels << level if self.form == "ver4" else self.cfg.nChanels

    def scores(self):
        """(scores, probability) of a classifier's last forward, [nMol, n_class] each."""
        if not self.nClass:
            raise TypeError("SMP2D.scores: not a classifier (n_class = 0)")
        return SMPClassifier.scores(self)

    def activation(self, mol, level, v):
        """f_level[v] of molecule `mol` after forward(): numpy [s, s, C_level]."""
        s = len(self.receptive_field(mol, level, v))
        out = np.empty((s, s, self.level_channels(level)), dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class SMPUnrestricted(SMP1D):
    """Batched Unrestricted_SMP_1D (form "1d"), Unrestricted_SMP_1D_ver2 ("1d_ver2") and Unrestricted_SMP_2D ("2d") of
    GraphFlow/Unrestricted_SMP_*.h, gf_smp_config.unrestricted = 1, 2, 3: SMP_1D, SMP_1D_ver2 and SMP_2D with a dense learned filter per
    field size s.  With S = the children's activations summed on the positions of phi_l(v) (form "2d": on both indices, plus scalar_l * adj_v):
      "1d":      z[i, c] = sum_k W_s[i, k] S[k, c] + b_s[c], C channels at every level, LeakyReLU slope 0.01;
      "1d_ver2": z[i] = [(W1_s S)[i] | (W2_s S)[i]] + b_s, the channels double per level (C << l), slope 0;
      "2d":      z[i, j, c] = sum_k W_s[i, k, c] S[k, j, c] + b_s[c], f_l[v] is [s, s, C], slope 0.01.
    Parameters in registration order: H[C, F(D+1)]; for l = 1..L: for s = 1..max_nVertices (W_s[s, s] | W1_s, W2_s[s, s] | W_s[s, s, C],
    then b_s[C_l]), for "2d" then scalar_l[C]; W[C_L].  Every gradient is the plain derivative.  The optimiser is Momentum: step().
    There are no classifiers of these forms."""

    FORMS = {"1d": 1, "1d_ver2": 2, "2d": 3}

    def __init__(self, form, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.form, self.nClass = form, 0
        self.cfg = self.config(form, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(form, max_nVertices, nLevels, nChanels, nFeatures, nDepth, has_WL_ordering=True):
        if form not in SMPUnrestricted.FORMS:
            raise ValueError("SMPUnrestricted: form %r (\"1d\": Unrestricted_SMP_1D, \"1d_ver2\": Unrestricted_SMP_1D_ver2, \"2d\": "
                             "Unrestricted_SMP_2D)" % (form,))
        return SMPConfig(nLevels, nChanels, nFeatures, nDepth, max_nVertices, 1 if has_WL_ordering else 0, 0, 0, 0, 0, max_nVertices, 0,
                         SMPUnrestricted.FORMS[form])

    def level_channels(self, level):
        return self.cfg.nChanels << level if self.form == "1d_ver2" else self.cfg.nChanels

    def activation(self, mol, level, v):
        """f_level[v] of molecule `mol` after forward(): numpy [s, C_level], or [s, s, C] for form "2d"."""
        s = len(self.receptive_field(mol, level, v))
        shape = (s, s, self.cfg.nChanels) if self.form == "2d" else (s, self.level_channels(level))
        out = np.empty(shape, dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class SMPNeighbourhood(SMP1D):
    """Batched NeuralFingerprint (form "fingerprint"), GCN_1D ("gcn_1d") and GCN_2D ("gcn_2d") of GraphFlow/NeuralFingerprint.h, GCN_1D.h,
    GCN_2D.h, gf_smp_config.neighbourhood = 1, 2, 3: the baselines of the CCN / SMP models.  One vector h_l[v] [nHiddens] per vertex:
      h_0[v] = softmax(W1_0 x[v]);  h_l[v] = softmax(W1_l x[v] + W2_l n_l[v]),  n_l[v] = the aggregate of h_{l-1} over N_l(v);
      "fingerprint": x = the vertex's features (nDepth must be 0), N_l(v) = {u: adj[v, u] > 0}, sum;
      "gcn_1d":      x = the shell sums up to nDepth, N_l(v) = {u: dist(v, u) <= min(l, max_Radius)}, sum;
      "gcn_2d":      x likewise, N_l(v) = {u: dist(v, u) <= l} (max_Radius is not read), RisiLayer2D;
      "gcn_3d":      GCN_3D (GraphFlow/GCN_3D.h, neighbourhood = 6): x and N_l(v) as "gcn_1d" (max_Radius is read), n_l[v] = the nHiddens largest
                     entries of RisiLayer3D's H^3 triple products over the members, ascending (KMax); 0 under three members; nHiddens <= 64.
    predict = <W, sum_v h_L[v]>, squared loss.  Parameters in registration order: W1_0[H, F']; for l = 1..L: W1_l[H, F'], W2_l[H, H]; W[H],
    F' = nFeatures (nDepth + 1).  The softmax gradient is the classes' diagonal rule.  nLevels = 0 is a model.  nHiddens <= 128.  The optimiser
    is Momentum: step().  There are no classifiers of these forms."""

    FORMS = {"fingerprint": 1, "gcn_1d": 2, "gcn_2d": 3, "gcn_3d": 6}

    def __init__(self, form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius=1, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.form, self.nClass = form, 0
        self.cfg = self.config(form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius=1):
        if form not in SMPNeighbourhood.FORMS:
            raise ValueError("SMPNeighbourhood: form %r (\"fingerprint\": NeuralFingerprint, \"gcn_1d\": GCN_1D, \"gcn_2d\": GCN_2D, "
                             "\"gcn_3d\": GCN_3D)" % (form,))
        return SMPConfig(nLevels, nHiddens, nFeatures, nDepth, max_nVertices, 0, 0, 0, 0, 0, max_nVertices, 0, 0,
                         SMPNeighbourhood.FORMS[form], max_Radius)

    def level_channels(self, level):
        return self.cfg.nChanels

    def activation(self, mol, level, v):
        """h_level[v] of molecule `mol` after forward(): numpy [nHiddens]."""
        out = np.empty(self.cfg.nChanels, dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class SMPGatedNeighbourhood(SMPNeighbourhood):
    """Batched GRU_GCN_1D (form "gru_gcn_1d") and GRU_GCN_2D ("gru_gcn_2d") of GraphFlow/GRU_GCN_1D.h, GRU_GCN_2D.h,
    gf_smp_config.neighbourhood = 4, 5: GCN_1D / GCN_2D's features and aggregates with a GRU cell as the level's update and a gated read-out.
      h_0[v] = softmax(W x[v]);  n = the aggregate of h_{l-1} over N_l(v) = {u: dist(v, u) <= min(l, max_Radius)} (both forms), hp = h_{l-1}[v]:
      z = sigmoid(W_z n + U_z hp), r = sigmoid(W_r n + U_r hp), c = tanh(W_h n + U_h (r hp)), h_l[v] = (1 - z) hp + z c;
      graph_feature = tanh(sum_v sigmoid(W_g h_L[v]) tanh(U_g h_L[v])), predict = <U, graph_feature>, squared loss.
    Parameters in registration order, shared by all levels: W[H, F']; W_z, U_z, W_r, U_r, W_h, U_h, W_g, U_g [H, H]; U[H].  nLevels = 0 is a
    model.  nHiddens <= 64.  The optimiser is Momentum: step().  There are no classifiers of these forms.
    "gru_gcn_3d" is GRU_GCN_3D (GraphFlow/GRU_GCN_3D.h, neighbourhood = 7): the same cell with n = the nHiddens largest entries of RisiLayer3D
    over the members (KMax, ascending; 0 under three members)."""

    FORMS = {"gru_gcn_1d": 4, "gru_gcn_2d": 5, "gru_gcn_3d": 7}

    @staticmethod
    def config(form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius=1):
        if form not in SMPGatedNeighbourhood.FORMS:
            raise ValueError("SMPGatedNeighbourhood: form %r (\"gru_gcn_1d\": GRU_GCN_1D, \"gru_gcn_2d\": GRU_GCN_2D, "
                             "\"gru_gcn_3d\": GRU_GCN_3D)" % (form,))
        return SMPConfig(nLevels, nHiddens, nFeatures, nDepth, max_nVertices, 0, 0, 0, 0, 0, max_nVertices, 0, 0,
                         SMPGatedNeighbourhood.FORMS[form], max_Radius)


class SMPDistance(SMPNeighbourhood):
    """Batched GCN_1D_Distance (form "gcn_1d_distance"), GCN_2D_Distance ("gcn_2d_distance") and GCN_3D_Distance ("gcn_3d_distance") of
    GraphFlow/GCN_*D_Distance.h, gf_smp_config.distance_channel = 1 with neighbourhood = 2, 3, 6: the only models that read a molecule's
    distance matrix.  Two copies of the softmax level of "gcn_1d" / "gcn_2d" / "gcn_3d" run side by side over the same neighbour lists
    N_l(v) = {u: dist(v, u) <= min(l, max_Radius)} (all three read max_Radius), each with weights of its own:
      the vertex channel reads x_v[v] = the shell sums [F'], the distance channel x_d[v] = column v of the distance matrix, padded with
      zeros to max_nVertices and sorted ascending (on the device);
      graph feature = [sum_v h^v_L[v] | sum_v h^d_L[v]] (2 nHiddens), predict = <W, graph feature>, squared loss.
    Parameters in registration order: for l = 0..L: W1v_l[H, F'], W1d_l[H, M], and for l > 0 W2v_l[H, H], W2d_l[H, H]; W[2 H].
    save_model / load_model read and write the classes' files, whose order differs (channel by channel).  prepare() takes molecules as
    (adj, feature, distance) triples, distance float[V, V]; activation(mol, l, v) is [h^v_l[v] | h^d_l[v]].  The optimiser is Momentum: step()."""

    FORMS = {"gcn_1d_distance": 2, "gcn_2d_distance": 3, "gcn_3d_distance": 6}

    @staticmethod
    def config(form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius=1):
        if form not in SMPDistance.FORMS:
            raise ValueError("SMPDistance: form %r (\"gcn_1d_distance\": GCN_1D_Distance, \"gcn_2d_distance\": GCN_2D_Distance, "
                             "\"gcn_3d_distance\": GCN_3D_Distance)" % (form,))
        return SMPConfig(nLevels, nHiddens, nFeatures, nDepth, max_nVertices, 0, 0, 0, 0, 0, max_nVertices, 0, 0,
                         SMPDistance.FORMS[form], max_Radius, 0, 0, 0, 0, 1)

    @staticmethod
    def pack(molecules, coulomb=None):
        """The flat host arrays gf_smp_prepare_distance takes: vertex counts, adjacency, feature and distance matrices back to back."""
        pk = SMPOmega.pack(molecules)
        pk["distance"] = np.concatenate([np.ascontiguousarray(m[2], dtype=np.float64).ravel() for m in molecules])
        assert pk["distance"].size == pk["adj"].size
        return pk

    def prepare(self, molecules, coulomb=None):
        """molecules: list of (adj int[V, V], feature float[V, F], distance float[V, V]) or the dict pack() returns.  Blocking."""
        if coulomb is not None:
            raise TypeError("SMPDistance.prepare: the distance models have no Coulomb adjacency")
        pk = molecules if isinstance(molecules, dict) else self.pack(molecules)
        nV, adj, feat, dist = pk["nV"], pk["adj"], pk["feature"], pk["distance"]
        self.ctx.check(self.lib.gf_smp_prepare_distance(self.handle, len(nV), nV.ctypes.data_as(C.POINTER(C.c_int)),
                                                        adj.ctypes.data_as(C.POINTER(C.c_int)), feat.ctypes.data_as(C.POINTER(C.c_double)),
                                                        dist.ctypes.data_as(C.POINTER(C.c_double))))
        self.n_mol = len(nV)
        dev = self.ctx.device
        self.predict = torch.empty(self.n_mol, dtype=torch.float32, device=dev)
        self.loss = torch.empty(self.n_mol, dtype=torch.float32, device=dev)
        self.feature = torch.empty((self.n_mol, 2 * self.cfg.nChanels), dtype=torch.float32, device=dev)

    def activation(self, mol, level, v):
        """[h^v_level[v] | h^d_level[v]] of molecule `mol` after forward(): numpy [2 nHiddens]."""
        out = np.empty(2 * self.cfg.nChanels, dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class SMPKernelPairs(SMPNeighbourhood):
    """Batched GCN_1D_Kernel (form "gcn_1d_kernel"), GCN_2D_Kernel ("gcn_2d_kernel") and GCN_3D_Kernel ("gcn_3d_kernel") of
    GraphFlow/GCN_*D_Kernel.h, gf_smp_config.readout = 1 with neighbourhood = 2, 3, 6: kernel learning on pairs of graphs.  Graphs X and Y go
    through the levels of "gcn_1d" / "gcn_2d" / "gcn_3d" with the same weights, N_l(v) = {u: dist(v, u) <= min(l, max_Radius)} in all three
    (GCN_2D_Kernel reads max_Radius):
      graph feature = [sum_v h^X_L[v] | sum_v h^Y_L[v]] (2 nHiddens), predict = <W, graph feature>, squared loss.
    Parameters in registration order: W1_0[H, F']; for l = 1..L: W1_l[H, F'], W2_l[H, H]; W[2 H].  The arguments are the classes' constructor's.
    prepare(graphs_x, graphs_y) takes two lists of (adj, feature) of equal length; X_p and Y_p may differ in size.  forward() returns predict,
    loss [nPairs] and the features [nPairs, 2 H]; receptive_field / activation / level_sizes count graph 2 p for X_p and 2 p + 1 for Y_p.
    The optimiser is Momentum: step()."""

    FORMS = {"gcn_1d_kernel": 2, "gcn_2d_kernel": 3, "gcn_3d_kernel": 6}

    def __init__(self, form, nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius, ctx=None):
        super().__init__(form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius, ctx=ctx)

    @staticmethod
    def config(form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius=1):
        if form not in SMPKernelPairs.FORMS:
            raise ValueError("SMPKernelPairs: form %r (\"gcn_1d_kernel\": GCN_1D_Kernel, \"gcn_2d_kernel\": GCN_2D_Kernel, "
                             "\"gcn_3d_kernel\": GCN_3D_Kernel)" % (form,))
        return SMPConfig(nLevels, nHiddens, nFeatures, nDepth, max_nVertices, 0, 0, 0, 0, 0, max_nVertices, 0, 0,
                         SMPKernelPairs.FORMS[form], max_Radius, 0, 0, 0, 0, 0, 1)

    def prepare(self, graphs_x, graphs_y=None, coulomb=None):
        """graphs_x, graphs_y: lists of (adj int[V, V], feature float[V, F]) of equal length (or the dicts pack() returns).  Blocking."""
        if graphs_y is None or coulomb is not None:
            raise TypeError("SMPKernelPairs.prepare(graphs_x, graphs_y): a pair model takes two lists of graphs and no Coulomb adjacency")
        px = graphs_x if isinstance(graphs_x, dict) else self.pack(graphs_x)
        py = graphs_y if isinstance(graphs_y, dict) else self.pack(graphs_y)
        if len(px["nV"]) != len(py["nV"]):
            raise ValueError("SMPKernelPairs.prepare: %d graphs X, %d graphs Y" % (len(px["nV"]), len(py["nV"])))
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self.ctx.check(self.lib.gf_smp_prepare_pairs(self.handle, len(px["nV"]), px["nV"].ctypes.data_as(ip), px["adj"].ctypes.data_as(ip),
                                                     px["feature"].ctypes.data_as(dp), py["nV"].ctypes.data_as(ip), py["adj"].ctypes.data_as(ip),
                                                     py["feature"].ctypes.data_as(dp)))
        self.n_mol = len(px["nV"])   # (pairs: what targets, predict and loss count)
        dev = self.ctx.device
        self.predict = torch.empty(self.n_mol, dtype=torch.float32, device=dev)
        self.loss = torch.empty(self.n_mol, dtype=torch.float32, device=dev)
        self.feature = torch.empty((self.n_mol, 2 * self.cfg.nChanels), dtype=torch.float32, device=dev)


class GCA1D(SMPNeighbourhood):
    """Batched GCA_1D (GraphFlow/GCA_1D.h, LinearGram.h), gf_smp_config.readout = 2 with neighbourhood = 2: the graph auto-encoder on
    GCN_1D's levels.  There is no W and no target:
      G[x, y] = <h_L[x], h_L[y]>;  loss = 0.5 sum (G - adj)^2 with the adjacency taken by VALUE (an entry of 2 counts as 2, an asymmetric
      matrix as written);  dh_L[x] = sum_y (E[x, y] + E[y, x]) h_L[y],  E = G - adj.
    Parameters: W1_0[H, F']; for l = 1..L: W1_l[H, F'], W2_l[H, H].  The arguments are the class's constructor's.  forward(params) returns the
    per-molecule loss; gram() the list of V x V matrices of the last forward (Predict); backward() works after any forward, once per forward.
    The optimiser is Momentum: step()."""

    def __init__(self, nLevels, max_nVertices, nFeatures, nHiddens, nDepth, max_Radius, ctx=None):
        super().__init__("gca_1d", nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius, ctx=ctx)

    @staticmethod
    def config(form, nLevels, nHiddens, nFeatures, nDepth, max_nVertices, max_Radius=1):
        if form != "gca_1d":
            raise ValueError("GCA1D: form %r (\"gca_1d\": GCA_1D)" % (form,))
        return SMPConfig(nLevels, nHiddens, nFeatures, nDepth, max_nVertices, 0, 0, 0, 0, 0, max_nVertices, 0, 0, 2, max_Radius, 0, 0, 0, 0, 0, 2)

    def prepare(self, molecules, coulomb=None):
        super().prepare(molecules, coulomb)
        nV = molecules["nV"] if isinstance(molecules, dict) else [len(m[0]) for m in molecules]
        self.n_vertices = [int(v) for v in nV]

    def forward(self, params, targets=None):
        if targets is not None:
            raise TypeError("GCA1D.forward: the auto-encoder's target is the batch's own adjacency")
        self._flat(params, "params")
        self.ctx.check(self.lib.gf_smp_forward(self.handle, C.c_void_p(params.data_ptr()), None, None, C.c_void_p(self.loss.data_ptr()), None))
        return self.loss

    def gram(self):
        """The Gram matrices of the last forward(): a list of numpy [V, V] float32 arrays, one per molecule."""
        flat = torch.empty(sum(v * v for v in self.n_vertices), dtype=torch.float32, device=self.ctx.device)
        self.ctx.check(self.lib.gf_smp_gram(self.handle, C.c_void_p(flat.data_ptr())))
        host, out, at = flat.cpu().numpy(), [], 0
        for v in self.n_vertices:
            out.append(host[at:at + v * v].reshape(v, v))
            at += v * v
        return out


class GCNMW(SMPNeighbourhood):
    """Batched GCN_MW (GraphFlow/GCN_MW.h, gf_smp_config.matrix_form = 2): the Kipf-Welling GCN in matrix form on the row-list GEMM level.
      A-hat = D^-1/2 (A + I) D^-1/2;  h_0 = LeakyReLU((A-hat x) W_0);  h_l = LeakyReLU((A-hat h_{l-1}) W_l);  x = the shell sums up to nDepth;
      predict = <W, sum_v h_L[v]>, squared loss.  Parameters in registration order: W_0[F', H]; W_l[H, H] for l = 1..L; W[H], F' = nFeatures
    (nDepth + 1).  nLevels = 0 is a model.  The optimiser is Momentum: step().  receptive_field(mol, l, v) gives the non-zero columns of row v
    of A-hat, activation(mol, l, v) h_l[v]."""

    def __init__(self, nLevels, max_nVertices, nFeatures, nHiddens, nDepth, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.form, self.nClass = "gcn_mw", 0
        self.cfg = self.config(nLevels, max_nVertices, nFeatures, nHiddens, nDepth)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(nLevels, max_nVertices, nFeatures, nHiddens, nDepth):
        return SMPConfig(nLevels, nHiddens, nFeatures, nDepth, max_nVertices, 0, 0, 0, 0, 0, max_nVertices, 0, 0, 0, 0, 2, 0, 0, 0)


class LCNN(GCNMW):
    """Batched LCNN (PATCHY-SAN, GraphFlow/LCNN.h, gf_smp_config.matrix_form = 1) on the row-list GEMM level.  Every molecule is padded to
    nVertices vertices; order = the class's exchange sort by the shell-sum rows, seq[i] = the first nNeighbors real vertices around rank
    position i by (hop distance, rank), padded with the molecule's vertex count;
      c1[i] = [x[seq[i][0]] | ..] F1 + b1, a1 = LeakyReLU(c1);  c2[i] = [a1[seq[i][0]] | ..] F2 + b2 (a1 is indexed by the sequence's vertex
      ids, as the class does);  dense = Dm vec(c2);  predict = <W, dense>, squared loss; the graph feature is dense.
    Parameters in registration order: F1[k, F', C1], b1[C1], F2[k, C1, C2], b2[C2], Dm[nDense, V C2], W[nDense].  prepare() refuses a
    full-size molecule one of whose vertices reaches fewer than nNeighbors vertices (the class reads past its matrix there).
    receptive_field(mol, l, i) gives the sequence of rank position i (level 0: the vertex at that position), activation(mol, 1, i) a1[i],
    activation(mol, 2, i) c2[i]."""

    def __init__(self, nVertices, nFeatures, nNeighbors, nDepth, nChanels1, nChanels2, nDense, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.form, self.nClass = "lcnn", 0
        self.cfg = self.config(nVertices, nFeatures, nNeighbors, nDepth, nChanels1, nChanels2, nDense)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(nVertices, nFeatures, nNeighbors, nDepth, nChanels1, nChanels2, nDense):
        return SMPConfig(2, nChanels1, nFeatures, nDepth, nVertices, 0, 0, 0, 0, 0, nVertices, 0, 0, 0, 0, 1, nNeighbors, nChanels2, nDense)

    def level_channels(self, level):
        return self.cfg.nChanels2 if level == 2 else self.cfg.nChanels

    def activation(self, mol, level, v):
        """a1[v] (level 1, [nChanels1]) or c2[v] (level 2, [nChanels2]) of rank position v of molecule `mol` after forward()."""
        out = np.empty(self.level_channels(level), dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class CGCN1D(SMPNeighbourhood):
    """Batched CGCN_1D (GraphFlow/CGCN_1D.h, gf_smp_config.covariant = 1): the covariant graph convolution network on the whole-network
    vertex level.  A vertex carries one vector of length M = max_nVertices, indexed by the molecule's vertex ids:
      h_0[v] = e_v <x[v], H>;  n_l[v] = sum of h_{l-1}[u] over N(v) = {u: adj[u, v] > 0};  h_l[v] = LeakyReLU(mask_l(v) * (F_l n_l[v])),
      mask_l(v) = {i: dist(i, v) <= l};  x = the shell sums up to nDepth;  predict = the sum of the components of sum_v h_L[v], squared loss.
    Parameters in registration order: H[F'], F_l[M, M] for l = 1..L, F' = nFeatures (nDepth + 1); there is no W.  nLevels = 0 is a model.
    One forward and one backward launch for all levels.  The optimiser is Momentum: step().  receptive_field(mol, l, v) gives mask_l(v),
    activation(mol, l, v) h_l[v] [M]."""

    COVARIANT = 1

    def __init__(self, nLevels, max_nVertices, nFeatures, nDepth, ctx=None):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.form, self.nClass = "cgcn_%dd" % self.COVARIANT, 0
        self.cfg = self.config(nLevels, max_nVertices, nFeatures, nDepth)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    @classmethod
    def config(cls, nLevels, max_nVertices, nFeatures, nDepth):
        return SMPConfigCovariant(nLevels, 1, nFeatures, nDepth, max_nVertices, 0, 0, 0, 0, 0, max_nVertices, covariant=cls.COVARIANT)

    def level_channels(self, level):
        return self.cfg.max_nVertices

    def activation(self, mol, level, v):
        """h_level[v] of molecule `mol` after forward(): numpy [max_nVertices]."""
        out = np.empty(self.cfg.max_nVertices, dtype=np.float32)
        n = self.lib.gf_smp_read_activation(self.handle, mol, level, v, out.ctypes.data_as(C.c_void_p), out.size)
        if n != out.size:
            raise RuntimeError("gf_smp_read_activation(%d, %d, %d) returned %d" % (mol, level, v, n))
        return out


class CGCN2D(CGCN1D):
    """Batched CGCN_2D (GraphFlow/CGCN_2D.h, gf_smp_config.covariant = 2): CGCN1D with RisiLayer2D as the aggregate,
      n_l[v][i] = sum over u in N(v) of h_{l-1}[u][i] * (sum over the OTHER members w of N(v) of sum_k h_{l-1}[w][k]),
    zero with fewer than two neighbours; the exclusive sums are evaluated directly."""

    COVARIANT = 2


class SMPClassifier(SMPOmega):
    """The classification models of GraphFlow (SMP_2D_ver6_classification: nContractions=10, custom_matmul=True;
    SMP_2D_ver7_classification: 50, True) through gf_smp_create_classifier: the levels of the regression model, read out by
    MatVecMul(W[nClass, C]) + LogLoss.  Parameters in registration order: H, (K_l, b_l) for l = 1..L, W[nClass, C].
    forward(params, targets) takes the labels as floats and returns (predict = arg-max label as a float, loss = log p[label],
    at most 0 -- the reference's sign -- and graph_feature); scores() gives the logits and probabilities of that forward."""

    def __init__(self, nClass, nLevels, nChanels, nFeatures, nDepth, max_receptive_field, has_WL_ordering=True, ctx=None,
                 nContractions=10, custom_matmul=True):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.nClass = int(nClass)
        self.cfg = SMPConfig(nLevels, nChanels, nFeatures, nDepth, max_receptive_field, 1 if has_WL_ordering else 0,
                             nContractions, 1 if custom_matmul else 0, 0)
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_create_classifier(self.ctx.handle, C.byref(self.cfg), self.nClass, C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_param_count(h)
        self.n_mol = 0

    def scores(self):
        """(scores, probability) of the last forward: predict->value and LogLoss::probability, [nMol, nClass] each."""
        dev = self.ctx.device
        z = torch.empty((self.n_mol, self.nClass), dtype=torch.float32, device=dev)
        p = torch.empty((self.n_mol, self.nClass), dtype=torch.float32, device=dev)
        self.ctx.check(self.lib.gf_smp_class_scores(self.handle, C.c_void_p(z.data_ptr()), C.c_void_p(p.data_ptr())))
        return z, p

    def uniform_init(self):
        """Initial weights exactly as the reference classifier's constructor draws them from rand() (call srand first)."""
        out = np.zeros(self.n_params, dtype=np.float32)
        st = self.lib.gf_smp_classifier_uniform_init_host(C.byref(self.cfg), self.nClass, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st != 0:
            raise RuntimeError("gf_smp_classifier_uniform_init_host failed")
        return out


class SMPModelConfig(C.Structure):
    _fields_ = [("nTowers", C.c_int), ("nLevels", C.c_int), ("nChanels", C.c_int), ("max_receptive_field", C.c_int),
                ("nFeatures", C.c_int * 2), ("nKept", C.c_int), ("nContractions", C.c_int), ("first_order", C.c_int),
                ("max_nVertices", C.c_int * 2), ("ccn_1d", C.c_int), ("nChanels_decay", C.c_double)]


class SMPModel:
    """The _physics (one tower) / _pairgraphs (two towers, nKept > 0: SMP_sigma_pairgraphs) models of GraphFlow through
    gf_smp_model_*.  nContractions = 4: SMP_gamma_physics / SMP_gamma_pairgraphs (RisiContraction_4, K_l[4 C_{l-1}, C_l]).
    first_order=True with max_nVertices (an int, or one per tower): SMP_theta_physics / SMP_theta_pairgraphs.
    ccn_1d=True with nChanels_decay: CCN_1D (see CCN1D).
    Parameters / gradients: one flat fp32 tensor in the class's registration order."""

    def __init__(self, nLevels, nChanels, max_receptive_field, nFeatures, nKept=0, ctx=None, nContractions=18, first_order=False,
                 max_nVertices=0, ccn_1d=False, nChanels_decay=0.0):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        self.cfg = SMPModel.config(nLevels, nChanels, max_receptive_field, nFeatures, nKept, nContractions, first_order, max_nVertices,
                                   ccn_1d, nChanels_decay)
        self._adam = None
        h = C.c_void_p()
        self.ctx.check(self.lib.gf_smp_model_create(self.ctx.handle, C.byref(self.cfg), C.byref(h)))
        self.handle = h
        self.n_params = self.lib.gf_smp_model_param_count(h)
        self.n_mol = 0

    @staticmethod
    def config(nLevels, nChanels, max_receptive_field, nFeatures, nKept=0, nContractions=18, first_order=False, max_nVertices=0,
               ccn_1d=False, nChanels_decay=0.0):
        """the gf_smp_model_config of a model (gf_smp_model_config_param_count takes it without a device)"""
        feats = list(nFeatures) if isinstance(nFeatures, (list, tuple)) else [nFeatures]
        maxV = list(max_nVertices) if isinstance(max_nVertices, (list, tuple)) else [max_nVertices, 0]
        return SMPModelConfig(len(feats), nLevels, nChanels, max_receptive_field, (C.c_int * 2)(*(feats + [0])[:2]), nKept,
                              0 if first_order else nContractions, 1 if first_order else 0, (C.c_int * 2)(*(maxV + [0])[:2]),
                              1 if ccn_1d else 0, float(nChanels_decay))

    @staticmethod
    def _pack(graphs):
        nV = np.array([len(g[0]) for g in graphs], dtype=np.int32)
        adj = np.concatenate([np.ascontiguousarray(g[0], dtype=np.int32).ravel() for g in graphs])
        feat = np.concatenate([np.ascontiguousarray(g[1], dtype=np.float64).ravel() for g in graphs])
        return nV, adj, feat

    def prepare(self, graphs1, graphs2=None):
        a = self._pack(graphs1)
        b = self._pack(graphs2) if graphs2 is not None else (None, None, None)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None  # noqa: E731
        self.ctx.check(self.lib.gf_smp_model_prepare(self.handle, len(graphs1), ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(b[0]), ptr(b[1]), ptr(b[2])))
        self.n_mol = len(graphs1)
        dev = self.ctx.device
        self.predict = torch.empty(self.n_mol, dtype=torch.float32, device=dev)
        self.loss = torch.empty(self.n_mol, dtype=torch.float32, device=dev)

    def set_mode(self, train=True):
        self.ctx.check(self.lib.gf_smp_model_set_mode(self.handle, 1 if train else 0))

    def set_fused(self, on=True):
        """False: every tower level op by op (promotion + contraction kernels + K-projection), the parity yardstick."""
        self.ctx.check(self.lib.gf_smp_model_set_fused(self.handle, 1 if on else 0))

    def uniform_init_host(self):
        """weights_initialization(): the initial weights the reference class draws from rand() (call srand first)."""
        out = np.empty(self.n_params, dtype=np.float32)
        self.ctx.check(self.lib.gf_smp_model_uniform_init_host(self.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def forward(self, params, targets=None):
        t = C.c_void_p(targets.data_ptr()) if targets is not None else None
        self.ctx.check(self.lib.gf_smp_model_forward(self.handle, C.c_void_p(params.data_ptr()), t, C.c_void_p(self.predict.data_ptr()),
                                                     C.c_void_p(self.loss.data_ptr())))
        return self.predict, self.loss

    def backward(self, params, grads, accumulate=False):
        self.ctx.check(self.lib.gf_smp_model_backward(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()),
                                                      1 if accumulate else 0))
        return grads

    def adam_step(self, params, grads, learning_rate, nBatch):
        """Adam::Learn(learning_rate, nBatch) as the classes' BatchLearn applies it, over the whole registration-order vector; grads =
        the batch sum of backward().  The moments live with this object."""
        if self._adam is None:
            self._adam = [torch.zeros_like(params), torch.zeros_like(params), 0]
        m, v, n = self._adam
        self.ctx.check(self.lib.gf_adam_step_f32(self.ctx.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()),
                                                 C.c_void_p(m.data_ptr()), C.c_void_p(v.data_ptr()), self.n_params, float(learning_rate),
                                                 int(nBatch), n))
        self._adam[2] = n + self.n_params
        return params

    def _flat(self, params, grads):
        for t, name in ((params, "params"), (grads, "grads")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self.n_params):
                raise TypeError("%s must be a contiguous float32 CUDA tensor of %d elements" % (name, self.n_params))

    def optimiser_step(self, params, grads, kind, learning_rate, nBatch, gamma=0.9, beta1=0.0, beta2=0.0, rho=0.0, epsilon=0.0):
        """SMPOmega.optimiser_step on the composite handle; the state lives in the HANDLE (kind "adam": not adam_step()'s moments), and
        the handle keeps the kind of its first step"""
        self._flat(params, grads)
        cfg = _lib.OptimConfig(_lib.OPTIMISERS.get(kind, kind), int(nBatch), float(learning_rate), float(gamma), float(beta1), float(beta2),
                               float(rho), float(epsilon))
        self.ctx.check(self.lib.gf_smp_model_optimiser_step(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()), C.byref(cfg)))
        return params

    def regularise(self, params, grads, norm, lam, times=1):
        self._flat(params, grads)
        value = C.c_double(0.0)
        self.ctx.check(self.lib.gf_smp_model_regularise(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()), int(norm),
                                                        float(lam), int(times), C.byref(value)))
        return value.value

    def param_blocks(self):
        return _lib.param_blocks("gf_smp_model_config_param_blocks", C.byref(self.cfg))

    def fit(self, params, grads, targets, nIterations, learning_rate, epsilon=0.0, kind=0, optimiser="adam"):
        """The classes' iterative training calls (gf_smp_model_fit; see SMPOmega.fit) with Adam -- or "sgd", "adamax", "adadelta" --, whose
        state lives in the HANDLE here, not with adam_step().  Returns (report, decisions)."""
        self._flat(params, grads)
        if optimiser not in _lib.OPTIMISERS:
            raise ValueError("fit: optimiser %r (one of %s)" % (optimiser, ", ".join(sorted(_lib.OPTIMISERS))))
        cfg = _lib.FitConfig(int(kind), _lib.OPTIMISERS[optimiser], int(nIterations), float(learning_rate), float(epsilon), 0.0)
        rep = _lib.FitReport()
        log = (C.c_ubyte * max(1, int(nIterations)))()
        self.ctx.check(self.lib.gf_smp_model_fit(self.handle, C.c_void_p(params.data_ptr()), C.c_void_p(grads.data_ptr()),
                                                 C.c_void_p(targets.data_ptr()), C.byref(cfg), C.byref(rep), log))
        report = {name: getattr(rep, name) for name, _ in _lib.FitReport._fields_}
        return report, list(log[:rep.iterations])

    def save_model(self, params, path):
        """The classes' save_model: every parameter value in registration order as text, which their load_model reads.  Nine significant
        digits: load_model gives back the same float32 bits."""
        with open(str(path), "w") as f:
            f.write("".join("%.9g " % x for x in params.detach().cpu().numpy()))

    def load_model(self, path):
        """The classes' load_model: the flat parameter tensor on the context's device from a text checkpoint (ours or the reference's)."""
        with open(str(path)) as f:
            vals = np.array(f.read().split(), dtype=np.float64)
        if vals.size != self.n_params:
            raise ValueError("load_model: %s holds %d values, the model has %d parameters" % (path, vals.size, self.n_params))
        return torch.as_tensor(vals.astype(np.float32)).to(self.ctx.device)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.gf_smp_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CCN1D(SMPModel):
    """Batched CCN_1D (GraphFlow/CCN_1D.h), the first-order covariant compositional network on a pair of graphs: two SMP_theta towers
    whose widths decay, C_0 = nChanels, C_l = max(ceil(C_{l-1} * nChanels_decay), 16); every vertex's feature row divided by its L1 norm
    (a row of zeros is refused at prepare()); a head nTotal -> max(ceil(nTotal * decay), 16) -> max(ceil(that * decay), 16) -> 1.
    Parameters in registration order: H_1[C, F_1], H_2[C, F_2]; for l = 1..L: (lambda1_s, lambda2_s, b_s[C_l]) for s = 1..max_nVertices_1
    and K1_l[2 C_{l-1}, C_l], then the same for tower 2; W1, W2, W3.  The constructor takes the reference's argument list."""

    def __init__(self, max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1, nFeatures_2, nChanels_decay,
                 ctx=None):
        super().__init__(nLevels, nChanels, max_receptive_field, [nFeatures_1, nFeatures_2], ctx=ctx, first_order=True,
                         max_nVertices=[max_nVertices_1, max_nVertices_2], ccn_1d=True, nChanels_decay=nChanels_decay)

    @staticmethod
    def config(max_nVertices_1, max_nVertices_2, max_receptive_field, nLevels, nChanels, nFeatures_1, nFeatures_2, nChanels_decay):
        return SMPModel.config(nLevels, nChanels, max_receptive_field, [nFeatures_1, nFeatures_2], first_order=True,
                               max_nVertices=[max_nVertices_1, max_nVertices_2], ccn_1d=True, nChanels_decay=nChanels_decay)
