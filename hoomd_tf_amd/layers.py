"""Counterpart of ``hoomd/htf/layers.py``: RBFExpansion, WCARepulsion, EDSLayer, plus the
declarative pair-MLP (RBF -> Dense -> Dense -> Dense) that config C3 evaluates on MFMA, and the
per-particle descriptor network DescriptorMLP (RBF channels summed over the neighbors -> Dense stack)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, cgmap, ops, simmodel
from ._lib import lib, check
from .initializers import mlp_params


class RBFExpansion:
    """layers.py:7-49: ``exp(-(d - mu)^2 / gap)`` on an evenly spaced grid of ``count``
    centres from ``low`` to ``high`` (inclusive); gap = centre spacing (not squared)."""

    def __init__(self, low, high, count):
        self.low, self.high, self.count = float(low), float(high), int(count)
        self.centers = np.linspace(self.low, self.high, self.count).astype(np.float32)
        self.gap = np.float32(self.centers[1] - self.centers[0])

    def get_config(self):
        return {'low': self.low, 'high': self.high, 'count': self.count}

    def __call__(self, inputs):
        if isinstance(inputs, simmodel.SafeNorm) or (isinstance(inputs, torch.Tensor) and inputs.requires_grad):
            # the distances of compute()'s neighbor tensor (or anything else on an autograd graph): the expansion in torch ops, so
            # that whatever the model builds from it -- a descriptor summed over the neighbors and fed to Dense layers, a per-pair
            # network written by hand -- is differentiable by compute_nlist_forces (the reference's layer is a TF op like any
            # other: layers.py:36-49).  [.., count] floats: the generic route, not a fused kernel (htf.PairMLP is that).
            if isinstance(inputs, simmodel.SafeNorm):
                t = inputs.nlist.ad[:, :, :3] + inputs.delta
                inputs = torch.sqrt((t * t).sum(dim=2))
            simmodel._trace_log().append({"op": "rbf"})
            c = torch.as_tensor(self.centers, dtype=inputs.dtype, device=inputs.device)
            d = inputs[..., None] - c
            return torch.exp(-(d * d) / float(self.gap))
        x = inputs.to(torch.float32).contiguous()
        ops._dev(x, "inputs")
        simmodel._trace_log().append({"op": "rbf"})
        out = torch.empty(tuple(x.shape) + (self.count,), dtype=torch.float32, device=x.device)
        check(lib.htf_rbf_expansion(x.data_ptr(), x.numel(), self.low, self.high, self.count, out.data_ptr(),
                                    ops._stream(x)))
        return out


class Dense:
    """tf.keras.layers.Dense for the per-particle networks of the force path (example 08): ``x W + b``,
    glorot-uniform kernel, zero bias, ``activation=None`` unless given ('tanh').  Built on first call, like
    Keras.  Applied to the symbolic top-k features it stays symbolic (three of them lower to one kernel);
    applied to a tensor it is a torch matmul."""

    def __init__(self, units, activation=None, seed=0):
        self.units, self.activation, self.seed = int(units), activation, int(seed)
        self.kernel = self.bias = None
        self.version = 0

    def build(self, fan_in):
        if self.kernel is None:
            rng = np.random.default_rng(self.seed)
            lim = np.sqrt(6.0 / (fan_in + self.units))
            self.kernel = rng.uniform(-lim, lim, size=(fan_in, self.units)).astype(np.float32)
            self.bias = np.zeros(self.units, dtype=np.float32)

    def get_weights(self):
        return [] if self.kernel is None else [self.kernel.copy(), self.bias.copy()]

    def set_weights(self, ws):
        k, b = np.asarray(ws[0], dtype=np.float32), np.asarray(ws[1], dtype=np.float32)
        if k.shape[1] != self.units or b.shape != (self.units,):
            raise ValueError("Dense(%d): weight shapes %r, %r do not fit" % (self.units, k.shape, b.shape))
        self.kernel, self.bias = k.copy(), b.copy()
        self.version += 1

    def __call__(self, x):
        if isinstance(x, simmodel.TopRinv):
            self.build(x.k)
            return simmodel.DenseOut(x, [self])
        if isinstance(x, simmodel.DenseOut):
            self.build(x.layers[-1].units)
            return simmodel.DenseOut(x.top, x.layers + [self])
        t = x.tensor() if hasattr(x, "tensor") and callable(x.tensor) else x
        self.build(int(t.shape[-1]))
        y = t @ torch.as_tensor(self.kernel, dtype=t.dtype, device=t.device) + torch.as_tensor(self.bias, dtype=t.dtype, device=t.device)
        return torch.tanh(y) if self.activation == "tanh" else y


class WCARepulsion:
    """layers.py:52-98: trainable WCA repulsion ``(sigma/r)^6`` inside ``2^(1/3) sigma``,
    clipped to [0, 10].  Called on the neighbor list; returns the pair energy.  ``sigma`` is
    a trainable scalar weight with regulariser ``-regularization_strength * sigma``; it lives
    on the device once the layer takes part in training."""
    name = 'wca-repulsion'

    def __init__(self, sigma, regularization_strength=1e-3):
        self._sigma0 = float(np.float32(sigma))
        self.regularization_strength = regularization_strength
        self.w = None  # device weight, created on first training use

    @property
    def sigma(self):
        return float(self.w[0]) if self.w is not None else self._sigma0

    def get_config(self):
        return {'sigma': float(self.sigma)}

    def get_weights(self):
        return [np.array([self.sigma], dtype=np.float32)]

    def set_weights(self, ws):
        v = float(np.asarray(ws[0]).reshape(-1)[0])
        if self.w is not None:
            self.w[0] = v
        self._sigma0 = float(np.float32(v))

    # trainable-layer protocol used by tfcompute's training step
    nonneg_mask = 0

    @property
    def l1_reg(self):
        return (-float(self.regularization_strength),)

    def make_trainable(self, device):
        if self.w is None:
            self.w = torch.tensor([self._sigma0], dtype=torch.float32, device=device)
        return self.w

    @property
    def trainable_weights(self):
        return [self.w] if self.w is not None else []

    def potential(self):
        """The layer's own potential: kept while the layer lives, rebuilt when sigma is reset on the host
        or the device weight appears."""
        key = ("theta", id(self.w)) if self.w is not None else ("sigma", self._sigma0)
        if getattr(self, "_pot", None) is None or self._pot[0] != key:
            self._pot = (key, ops.Potential.wca(self.sigma, theta=self.w))
        return self._pot[1]

    def __call__(self, nlist):
        return simmodel.WCAPair(simmodel._as_nlist(nlist), self.sigma, layer=self)


class LJLayer:
    """The trainable Lennard-Jones layer of example 06 and build_examples.py:336-359: weights
    ``w = [sig, eps]`` (NonNeg constraint); called on ``r = safe_norm(nlist[:, :, :3], axis=2)``
    it returns the pair energy ``w[0] * 4 * (r6**2 - r6) / 2`` with ``r6 = w[1]**6 / r**6``."""
    name = 'lj'
    nonneg_mask = 0b11
    l1_reg = (0.0, 0.0)

    def __init__(self, sig, eps, device="cuda"):
        self.start = [sig, eps]
        self.w = torch.tensor([sig, eps], dtype=torch.float32, device=device)

    def get_config(self):
        return {'sig': self.start[0], 'eps': self.start[1]}

    def get_weights(self):
        return [self.w.detach().cpu().numpy().copy()]

    def set_weights(self, ws):
        self.w.copy_(torch.as_tensor(np.asarray(ws[0], dtype=np.float32).reshape(2)))

    def make_trainable(self, device):
        return self.w

    @property
    def trainable_weights(self):
        return [self.w]

    def potential(self):
        """The layer's own potential (reads ``self.w`` on the device at every launch)."""
        if getattr(self, "_pot", None) is None:
            w = self.w.cpu().numpy()
            self._pot = ops.Potential.lj_param(float(w[0]), float(w[1]), theta=self.w)
        return self._pot

    def __call__(self, r):
        if not isinstance(r, simmodel.SafeNorm):
            raise ValueError("LJLayer expects r = safe_norm(nlist[:, :, :3], axis=2)")
        return simmodel.LJParamEnergy(r.nlist, self)


class SoftRDFCV:
    """Differentiable stand-in for one RDF bin: cv = (1/N) sum_i sum_j
    exp(-(r_ij - r0)^2 / gap), r = safe_norm, padded slots masked -- a single RBFExpansion
    channel summed over the neighbor list.  Call it on the nlist; feed the result to EDSLayer."""

    def __init__(self, r0, gap):
        self.r0, self.gap = float(r0), float(gap)

    def get_config(self):
        return {'r0': self.r0, 'gap': self.gap}

    def __call__(self, nlist):
        return simmodel.PairCV(simmodel._as_nlist(nlist), self.r0, self.gap)


class PairMLP:
    """safe_norm -> RBFExpansion(low, high, K) -> Dense(H1) -> Dense(H2) -> Dense(1), masked
    with the nlist_rinv criterion and halved per pair (SURVEY 8(a) closed forms).  Keras
    Dense defaults: glorot-uniform kernels, zero biases, ``activation=None``; pass
    ``activation='tanh'`` for the C3 benchmark model.
    ``precision``: how the dense layers meet the matrix cores.  ``"split16"`` (default): every fp32 operand as hi + lo in
    fp16 (2^-22), three partial products on the fp16 MFMA -- the fp32 evaluator's accuracy (same tolerances against the
    fp64 oracle, tests/test_gpu_parity.py::test_pair_mlp_split_operands) at 2.5x its speed; weights and activations must
    stay inside fp16's range (|x| < 6e4: always true of a tanh network with sane weights).  ``"fp32"``: exact fp32 products
    on the fp32 MFMA.  ``"split"``: three bf16 parts, six partial products (no range limit).  ``"bf16"``: plain bf16
    operands, reduced precision."""

    name = 'pair-mlp'
    nonneg_mask = 0
    l1_reg = (0.0,)
    _KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")

    def __init__(self, K=32, H1=64, H2=64, low=0.0, high=3.0, activation=None, seed=3, precision="split16"):
        self.low, self.high = float(low), float(high)
        self.activation = activation or "linear"
        self.precision = precision
        self.params = mlp_params(seed=seed, K=K, H1=H1, H2=H2)
        self.w = None      # flat device weights (Keras get_weights() order) once the potential exists
        self._pot = None
        self._seen = None  # self.w._version the operand images were last built from

    def _flat(self):
        return np.concatenate([np.asarray(self.params[k], dtype=np.float32).ravel() for k in self._KEYS])

    def make_trainable(self, device="cuda"):
        if self.w is None:
            self.w = torch.tensor(self._flat(), dtype=torch.float32, device=device)
        return self.w

    @property
    def trainable_weights(self):
        return [self.w] if self.w is not None else []

    def potential(self):
        """One persistent potential reading ``self.w``: an optimizer step or set_weights only
        rebuilds its operand images on the device (htf_potential_refresh)."""
        if self._pot is None:
            self._pot = ops.Potential.pair_mlp(self.params, self.low, self.high, activation=self.activation,
                                               precision=self.precision, theta=self.make_trainable())
        self.refresh_if_stale()
        return self._pot

    def after_update(self):
        if self._pot is not None:
            self._pot.refresh()
            self._seen = self.w._version

    def refresh_if_stale(self):
        """``self.w`` written by anybody but the training step (an in-place op on ``trainable_weights[0]``, an optimizer of the
        user's own): the operand images are rebuilt from it before the next launch."""
        if self._pot is not None and self._seen != self.w._version:
            self.after_update()

    def _sync_host(self):
        if self.w is None:
            return
        flat, o = self.w.detach().cpu().numpy(), 0
        for k in self._KEYS:
            n = self.params[k].size
            self.params[k] = flat[o:o + n].reshape(self.params[k].shape).copy()
            o += n

    def get_weights(self):
        self._sync_host()
        return [self.params[k].copy() for k in self._KEYS]

    def set_weights(self, ws):
        for k, w in zip(self._KEYS, ws):
            if np.shape(w) != self.params[k].shape:
                raise ValueError("shape mismatch for %s" % k)
        for k, w in zip(self._KEYS, ws):
            self.params[k] = np.asarray(w, dtype=np.float32).copy()
        if self.w is not None:
            self.w.copy_(torch.from_numpy(self._flat()))
            self.after_update()

    def save_weights(self, path):
        self._sync_host()
        np.savez(path, **self.params)

    def load_weights(self, path):
        with np.load(path) as z:
            self.set_weights([z[k] for k in self._KEYS])

    def __call__(self, nlist):
        return simmodel.MLPEnergy(simmodel._as_nlist(nlist), self)


class DescriptorMLP:
    """A descriptor network of Behler-Parrinello / SchNet form, evaluated in one HIP kernel (include/htf_bp.h).

    Called on the neighbor list it returns the symbolic per-particle energy ``E_i``; ``compute_nlist_forces(nlist, E)``
    gives the forces ``2 sum_j dE_i/dx_ij`` with ``E_i`` in column 3, and the generic route's virial when asked::

        G_i[t*K + k] = sum_j [r_ij > 3e-6] [t_ij = t] exp(-(r_ij - mu_k)^2 / gap)    r_ij = safe_norm(x_ij)
        E_i = W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3

    ``mu = linspace(low, high, K)`` and ``gap = mu_1 - mu_0`` exactly as RBFExpansion builds them; ``t_ij = rint(nlist[i, j, 3])``
    when ``n_types > 1`` (a type outside ``[0, n_types)`` contributes nothing), 0 otherwise.  ``activation``: 'tanh' or
    'linear' for both hidden layers.  The weights (``mlp_params(seed, K=n_types*K, H1, H2)``, Keras order) live in one flat
    fp32 device tensor ``w`` that the kernel reads at every call: ``set_weights``, ``load_weights`` and in-place writes to
    ``w`` take effect at the next call.  The energy takes no part in arithmetic with other energies (it raises): evaluate
    each term with its own ``compute_nlist_forces`` and add the forces.

    ``r_cut=rc`` multiplies every Gaussian by the cosine cutoff ``fc(r) = 0.5 (cos(pi r / rc) + 1)`` for ``r < rc`` and 0
    beyond, so that a neighbor entering or leaving at ``rc`` changes neither energy nor force; ``rc``
    (rounded to fp32) should not exceed the ``r_cut`` of the neighbor list, which is not checked.  ``None``: no cutoff.
    ``n_species=S`` keeps one network per particle species, Behler-Parrinello's one network per element: ``w`` holds S
    networks of P floats, network ``s`` at ``w[s P:(s + 1) P]`` initialised from ``mlp_params(seed + s, ...)``, and row ``i`` is
    evaluated by network ``rint(species_i)``.  The species come with the call -- ``layer(nlist, positions)`` (column 3 of a
    [B, 4] tensor, or a [B] tensor), ``forces(x, species=...)``, ``loss_gradient(x, labels, species=...)`` -- and a value
    outside ``[0, S)`` raises; with ``S = 1`` they are ignored.  Each call partitions the rows by species on the device
    (one read-back of the S counts, cached while the same species tensor is passed) and launches once per species present.

    ``trainable=True`` makes the layer learn by force matching (htf_bp_loss_grad): under ``tfcompute.attach(...,
    train=True)`` every batch is one ``loss_gradient`` sweep -- the sum of squared residuals of (F_i, E_i) against the
    labels and its gradient with respect to ``w``, one pass over the pair vectors -- and one optimizer step on ``w``, on
    the device.  ``loss_gradient`` is also the offline entry: with ``iter_from_trajectory`` and ``ops.optimizer_step`` on
    ``w`` it trains from stored frames.  The centres and their spacing are not trained.  With the default
    ``trainable=False`` a training run raises.

    ``conservative=True`` makes ``compute_nlist_forces`` return the forces of the total energy, ``F = -d(sum_i E_i)/dr``
    (``total_forces``, include/htf_cforce.h), instead of the row operator's ``2 sum_j dE_i/dx_ij``: ``E_j`` also depends on
    ``r_i`` through ``G_j``, and two sweeps add that term -- the first writes ``g_i = dE_i/dG_i`` for every row, the second
    gathers ``g_j`` for every slot.  They conserve momentum and ``KE + sum_i E_i``.  The second sweep needs the particle in
    each slot: ``htf.Nlist(tensor, index)``, which ``tfcompute`` provides for the step's own list; offline,
    ``compute_nlist(..., sorted=True, return_types=False)[:, :, 3]`` is the index that goes with the ``return_types=True``
    tensor (both calls produce the same slots).  With ``n_types > 1`` it also needs the rows' own types:
    ``layer(nlist, positions)``.  The forces are exact when the list is symmetric within the descriptor's range -- full
    lists, no overflow, ``r_cut`` not above the list's cutoff -- which is not checked.  Energies are the row operator's, bit
    for bit.  Under slab domain decomposition (``domain.SlabDomain``) the second sweep also gathers from ghost particles, whose
    rows of ``g`` their owners compute: one more forward halo between the two sweeps (``SlabDomain.halo_rows``, ``total_forces``'
    ``n_ghost`` and ``halo``) makes every rank's forces the single-domain forces, and the force-matching sweeps below exchange
    the residual the same way and all-reduce ``accum``.  Not with batches, a mapped list or a ``BrickDomain``: each raises.

    ``trainable="total"`` is force matching on those forces (htf_ct_loss_grad, include/htf_ctrain.h) and implies
    ``conservative=True``: the layer is fitted to the force definition it runs with.  Under ``tfcompute.attach(...,
    train=True)`` every step is one ``total_loss_gradient`` sweep on the step's own list, index and ``total_forces`` output,
    and one optimizer step; offline, ``total_loss_gradient(x, labels, index)`` with ``iter_from_trajectory`` and the index
    above.  The sweep is ``loss_gradient``'s with one gathered residual per slot; it needs no types of the rows' own.
    ``trainable=True`` with ``conservative=True`` raises: that sweep differentiates the row operator.

    ``l_max=1`` or ``2`` (with ``conservative=True``; include/htf_angular.h) adds angular channels: beside ``G`` the network
    reads ``A_i[c] = |sum_j w u_ij|^2 = sum_jj' w w' cos(theta_jij')`` and, for ``l_max=2``, ``Q_i[c] = ||sum_j w u_ij (outer)
    u_ij||_F^2 = sum_jj' w w' cos^2(theta_jij')`` per channel ``c = t K + k``, with ``w = fc(r_ij) e_k(r_ij)`` and ``u_ij`` the
    direction of the pair vector.  The input is ``[G | A | Q]``, ``D = n_types K (1 + l_max)`` values, the weights are
    ``mlp_params(seed + s, K=D, H1, H2)``, and ``total_forces`` / ``compute_nlist_forces`` / ``descriptor`` run the angular
    kernels; everything said about ``conservative=True`` holds.  The row operator has no angular form (``forces`` and
    ``loss_gradient`` raise, as do ``trainable=True`` and ``trainable="total"``, whose sweeps are those of an ``l_max=0``
    layer).  ``l_max=0`` is the layer without the argument.

    ``trainable="angular"`` (with ``l_max=1`` or ``2``; htf_at_loss_grad, include/htf_atrain.h) is force matching on the
    angular conservative forces and implies ``conservative=True``, as ``"total"`` does for ``l_max=0``: under
    ``tfcompute.attach(..., train=True)`` every step is one ``angular_loss_gradient`` sweep on the step's own list, index and
    ``total_forces`` output, and one optimizer step; offline, ``angular_loss_gradient(x, labels, index)`` with
    ``iter_from_trajectory``.  The sweep is ``total_loss_gradient``'s over the wider input, its tangent ``[Gdot | Adot | Qdot]``
    formed from the moments and their tangents; it is callable on any layer with ``l_max > 0``.  With ``l_max=0`` the value
    raises and names ``trainable="total"``.

    ``n_models=M`` (2 to 8, with ``conservative=True``; include/htf_committee.h) makes the layer a committee: M members of this
    one architecture, member ``m`` and species ``s`` initialised from ``mlp_params(seed + m S + s, ...)``, ``w`` holding
    ``[M][S][P]`` floats and ``get_weights`` / ``set_weights`` / ``save_weights`` / ``load_weights`` carrying a leading axis of
    length M ahead of the species axis.  ``total_forces`` and ``compute_nlist_forces`` return the mean model, ``Fbar_i = (1/M)
    sum_m F_i^m`` with ``Ebar_i`` in column 3 and the mean virial when asked, each ``F_i^m`` being the conservative forces above
    for member ``m``'s weights, and leave in ``layer.deviation`` the [B, 2] fp32 tensor of that call (``None`` before the first),
    the per-particle model deviation that tells when the model extrapolates::

        devF_i = sqrt((1/M) sum_m |F_i^m - Fbar_i|^2)        devE_i = sqrt((1/M) sum_m (E_i^m - Ebar_i)^2)

    in the population form, computed as written (mean first, then the differences): members that agree have deviation 0.  A
    model returns it as a second output (``return f, self.desc.deviation``) and finds it in ``tfcompute.outputs``;
    ``total_forces(..., members=True)`` also returns the [M, B, 4] fp32 tensor of ``(F_i^m, E_i^m)``.  The two sweeps read the
    slots, form ``G_i`` and evaluate every exponential once for all members; only the dense stack and the gathered ``g_j`` run M
    times.  The first sweep keeps all M networks in LDS, ``4 (M P4 + K4 + 1024)`` bytes (P4: ``D (H1 + 1) + H1 (H2 + 1) + H1 + 2 H2
    + 1`` floats, rounded up to a multiple of 4, K4 likewise); a committee above 160 KiB raises at construction.
    ``layer.member(m)`` is a plain ``DescriptorMLP`` whose ``w`` is a view of member ``m``'s slice: ``forces``,
    ``total_forces``, ``descriptor``, ``total_loss_gradient`` and ``ops.optimizer_step`` on it evaluate and train that member in
    place, and the committee sees the new weights at its next call -- one member at a time, offline.  Not covered, each
    raises: angular channels (``l_max > 0``), ``trainable=True``, ``"total"`` or ``"angular"`` on the committee itself, slab or
    brick domains (``n_ghost > 0``), and the row-operator and single-network sweep methods, which point to ``member(m)``.
    ``n_models=1`` is the layer without the argument.

    ``trainable="committee"`` (with ``n_models >= 2`` and ``l_max = 0``; htf_cmt_loss_grad, include/htf_cmt_train.h) trains the
    committee where it runs and implies ``conservative=True``: every member is fitted on its own to the same labels, the loss
    being ``sum_m SSR^m``.  ``committee_loss_gradient(x, labels, index)`` is ``total_loss_gradient`` for all members in one
    sweep -- one wave per member on the same rows, the waves sharing the exponentials and the descriptor --
    and returns ``accum`` [M, 1 + P]; it is callable on any committee.  Under ``tfcompute.attach(..., train=True)`` every step
    is that sweep on the step's own list, index and members' forces, and M optimizer steps, member ``m`` on its slice of ``w``
    with its own optimizer state; the loss metric reads the mean of the members' losses.  The sweep keeps all M networks and
    six exchange lines and 256 slot terms per member in LDS, ``4 (M (P4 + 640) + K4)`` bytes; above 160 KiB the constructor raises.  In the run,
    ``n_species > 1``, several ranks and batches raise; offline the method covers species.
    Limits: ``n_types * K * (1 + l_max) <= 64``, ``H1, H2 <= 64``, at most 256 neighbor slots."""

    name = 'descriptor-mlp'
    _KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")
    MAX_D, MAX_H, MAX_NN = 64, 64, 256
    MAX_MODELS, MAX_COMMITTEE_LDS = 8, 160 * 1024   # include/htf_committee.h
    deviation = None    # a committee's (devF_i, devE_i) [B, 2] of its last total_forces call
    nonneg_mask = 0     # what the optimizer step reads of a trainable layer: no weight is constrained or regularised
    l1_reg = (0.0,)

    def __init__(self, K=16, H1=32, H2=32, low=0.0, high=3.0, n_types=1, activation="tanh", seed=3, device=None,
                 trainable=False, r_cut=None, n_species=1, conservative=False, l_max=0, n_models=1):
        K, H1, H2, n_types, n_species = int(K), int(H1), int(H2), int(n_types), int(n_species)
        if isinstance(l_max, bool) or int(l_max) != l_max or int(l_max) not in (0, 1, 2):
            raise ValueError("DescriptorMLP: l_max must be 0, 1 or 2, not %r" % (l_max,))
        self.l_max = l_max = int(l_max)
        if (isinstance(n_models, bool) or not isinstance(n_models, (int, np.integer))
                or not 1 <= int(n_models) <= self.MAX_MODELS):
            raise ValueError("DescriptorMLP: n_models must be an integer in [1, %d], not %r: a larger committee is several "
                             "layers, each evaluated with its own total_forces" % (self.MAX_MODELS, n_models))
        self.n_models = n_models = int(n_models)
        committee = isinstance(trainable, str) and trainable == "committee"
        if committee:
            if n_models < 2:
                raise ValueError("DescriptorMLP: trainable=\"committee\" trains the members of a committee and needs n_models >= 2, "
                                 "not n_models = %d; trainable=\"total\" fits one network" % n_models)
            if l_max:
                raise ValueError("DescriptorMLP: trainable=\"committee\" needs l_max = 0, not l_max = %d: the committee's sweeps "
                                 "have no angular form" % l_max)
            conservative = True   # the forces of the total energy, fitted and run alike
        if n_models > 1:
            if l_max:
                raise NotImplementedError("DescriptorMLP: n_models = %d does not go with l_max = %d: a committee of angular "
                                          "networks is a follow-up; M layers of l_max = %d, one total_forces each, evaluate it"
                                          % (n_models, l_max, l_max))
            if trainable is not False and not committee:
                raise NotImplementedError("DescriptorMLP: n_models = %d does not go with trainable=%r: training a committee in "
                                          "the running simulation is a follow-up; member(m, trainable=\"total\") is a view of "
                                          "member m that total_loss_gradient and ops.optimizer_step train in place"
                                          % (n_models, trainable))
            if not conservative:
                raise ValueError("DescriptorMLP: n_models = %d needs conservative=True: the deviation is defined on the forces "
                                 "of the total energy (total_forces)" % n_models)
        if isinstance(trainable, str):
            if trainable not in ("total", "angular", "committee"):
                raise ValueError("DescriptorMLP: trainable must be False, True, 'total', 'angular' or 'committee', not %r"
                                 % (trainable,))
            if trainable == "angular" and not l_max:
                raise ValueError("DescriptorMLP: trainable=\"angular\" fits the angular channels and needs l_max = 1 or 2; "
                                 "trainable=\"total\" fits the conservative forces of an l_max = 0 layer")
            self.trainable, self.conservative = trainable, True   # the forces of the total energy, fitted and run alike
        else:
            self.trainable, self.conservative = bool(trainable), bool(conservative)
            if self.trainable and self.conservative:
                raise ValueError("DescriptorMLP: conservative=True cannot go with trainable=True, whose force-matching sweep "
                                 "differentiates the row operator's forces: trainable=\"total\" fits the conservative forces")
        if l_max:
            if self.trainable and self.trainable != "angular":
                raise NotImplementedError("DescriptorMLP: trainable=%r does not go with l_max = %d: the force-matching sweep on the "
                                          "angular conservative forces, the follow-up to the angular channels, is "
                                          "trainable=\"angular\" (angular_loss_gradient)" % (trainable, l_max))
            if not self.conservative:
                raise ValueError("DescriptorMLP: l_max = %d needs conservative=True: the row operator has no angular form" % l_max)
        if r_cut is not None:
            r_cut = float(np.float32(r_cut))
            if not (np.isfinite(r_cut) and r_cut > 0):
                raise ValueError("DescriptorMLP: r_cut = %r must be finite and positive (None: no cutoff)" % (r_cut,))
        if n_species < 1:
            raise ValueError("DescriptorMLP: n_species = %d; at least one network" % n_species)
        self.r_cut, self.n_species = r_cut, n_species
        activation = activation or "linear"
        if activation not in ("tanh", "linear"):
            raise ValueError("DescriptorMLP: activation must be 'tanh' or 'linear', not %r" % (activation,))
        if K < 2:
            raise ValueError("DescriptorMLP: K = %d; the Gaussian width is the spacing of at least two centres" % K)
        if n_types < 1 or n_types * K > self.MAX_D:
            raise ValueError("DescriptorMLP: n_types * K = %d * %d channels; the kernel takes 1 to %d" % (n_types, K, self.MAX_D))
        if n_types * K * (1 + l_max) > self.MAX_D:
            raise ValueError("DescriptorMLP: n_types * K * (1 + l_max) = %d * %d * %d network inputs; the kernel takes 1 to %d"
                             % (n_types, K, 1 + l_max, self.MAX_D))
        if not (1 <= H1 <= self.MAX_H and 1 <= H2 <= self.MAX_H):
            raise ValueError("DescriptorMLP: hidden widths %d, %d outside [1, %d]" % (H1, H2, self.MAX_H))
        rbf = RBFExpansion(low, high, K)
        if not rbf.gap > 0:
            raise ValueError("DescriptorMLP: high = %g must exceed low = %g" % (rbf.high, rbf.low))
        self.K, self.H1, self.H2, self.n_types, self.activation = K, H1, H2, n_types, activation
        self.low, self.high, self.centers, self.gap = rbf.low, rbf.high, rbf.centers, rbf.gap
        self.Dr = n_types * K                 # radial channels; the network reads [G | A | Q]
        self.D = self.Dr * (1 + l_max)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        if n_models > 1:
            need = self.committee_lds_bytes(n_models, K, n_types, H1, H2)
            if need > self.MAX_COMMITTEE_LDS:
                raise ValueError("DescriptorMLP: a committee of %d networks of %d x %d x %d needs %d bytes of LDS for its first "
                                 "sweep, above the %d bytes of one compute unit: fewer members, or narrower networks"
                                 % (n_models, self.D, H1, H2, need, self.MAX_COMMITTEE_LDS))
            need = self.committee_train_lds_bytes(n_models, K, n_types, H1, H2)
            if committee and need > self.MAX_COMMITTEE_LDS:
                raise ValueError("DescriptorMLP: the training sweep of a committee of %d networks of %d x %d x %d needs %d bytes "
                                 "of LDS, above the %d bytes of one compute unit: fewer members, or narrower networks; "
                                 "member(m, trainable=\"total\") trains one member at a time"
                                 % (n_models, self.D, H1, H2, need, self.MAX_COMMITTEE_LDS))
        ps = [mlp_params(seed=seed + s, K=self.D, H1=H1, H2=H2) for s in range(n_models * n_species)]   # [M][S]
        self._shapes = [ps[0][k].shape for k in self._KEYS]
        self.P = sum(int(np.prod(sh)) for sh in self._shapes)   # floats of one network
        self.w = torch.tensor(np.concatenate([p[k].ravel() for p in ps for k in self._KEYS]), dtype=torch.float32, device=device)
        self.mu = torch.tensor(self.centers, dtype=torch.float32, device=device)

    @staticmethod
    def committee_lds_bytes(n_models, K, n_types, H1, H2):
        """Dynamic LDS of the committee's first sweep (htf_cmt_grad): M networks with rows padded by one float, the centres
        and one exchange line for each of a block's 16 waves."""
        D = K * n_types
        member = (D * (H1 + 1) + H1 + H1 * (H2 + 1) + H2 + H2 + 1 + 3) & ~3
        return 4 * (n_models * member + ((K + 3) & ~3) + 16 * 64)

    @staticmethod
    def committee_train_lds_bytes(n_models, K, n_types, H1, H2):
        """Dynamic LDS of the committee's training sweep (htf_cmt_loss_grad): per member the network with rows padded by one
        float, six exchange lines and one row of 256 slot terms; and the centres."""
        D = K * n_types
        member = (D * (H1 + 1) + H1 + H1 * (H2 + 1) + H2 + H2 + 1 + 3) & ~3
        return 4 * (n_models * (member + 6 * 64 + 256) + ((K + 3) & ~3))

    def member(self, m, trainable=False):
        """Member ``m`` of a committee as a plain ``DescriptorMLP`` of the same configuration (``n_models=1``, ``trainable`` as
        given) whose ``w`` is a view of this layer's ``w[m S P:(m + 1) S P]``: evaluating it runs the single-network kernels
        on that member, and training it in place (``total_loss_gradient`` and ``ops.optimizer_step`` on the view) changes what
        the committee computes at its next call."""
        if isinstance(m, bool) or int(m) != m or not 0 <= int(m) < self.n_models:
            raise ValueError("DescriptorMLP: member(%r) of a layer with n_models = %d" % (m, self.n_models))
        cfg = self.get_config()
        cfg.pop("n_models", None)
        cfg.pop("trainable", None)
        lay = DescriptorMLP(device="cpu", trainable=trainable, **cfg)
        n = self.n_species * self.P
        lay.w = self.w[int(m) * n:(int(m) + 1) * n]
        lay.mu = self.mu
        return lay

    def _no_committee(self, what):
        if self.n_models > 1:
            raise NotImplementedError("DescriptorMLP: %s() is a single network's; on a committee (n_models = %d) member(m).%s() "
                                      "evaluates member m, and total_forces() the mean model and its deviation"
                                      % (what, self.n_models, what))

    def get_config(self):
        cfg = {'K': self.K, 'H1': self.H1, 'H2': self.H2, 'low': self.low, 'high': self.high, 'n_types': self.n_types,
               'activation': self.activation}
        if self.trainable:
            cfg['trainable'] = self.trainable   # (True, "total", "angular" or "committee")
        if self.r_cut is not None:
            cfg['r_cut'] = self.r_cut
        if self.n_species != 1:
            cfg['n_species'] = self.n_species
        if self.conservative:
            cfg['conservative'] = True
        if self.l_max:
            cfg['l_max'] = self.l_max
        if self.n_models != 1:
            cfg['n_models'] = self.n_models
        return cfg

    def get_weights(self):
        """The six Keras arrays; with ``n_species = S > 1`` each has a leading axis of length S, and with ``n_models = M > 1``
        one of length M ahead of it."""
        lead = self._lead_axes()
        flat, out, o = self.w.detach().cpu().numpy().reshape(-1, self.P), [], 0
        for shape in self._shapes:
            n = int(np.prod(shape))
            out.append(flat[:, o:o + n].reshape(lead + tuple(shape)).copy())
            o += n
        return out

    def _lead_axes(self):
        return ((self.n_models,) if self.n_models > 1 else ()) + ((self.n_species,) if self.n_species > 1 else ())

    def set_weights(self, ws):
        ws = list(ws)
        S = self.n_models * self.n_species
        if len(ws) != len(self._KEYS):
            raise ValueError("DescriptorMLP: expected %d weight arrays, got %d" % (len(self._KEYS), len(ws)))
        for k, shape, w in zip(self._KEYS, self._shapes, ws):
            shape = self._lead_axes() + tuple(shape)
            if np.shape(w) != shape:
                raise ValueError("DescriptorMLP: shape mismatch for %s: %r, expected %r" % (k, np.shape(w), shape))
        flat = np.concatenate([np.asarray(w, dtype=np.float32).reshape(S, -1) for w in ws], axis=1).ravel()
        with torch.no_grad():
            self.w.copy_(torch.from_numpy(flat))   # (in place: the next call reads it)

    def save_weights(self, path):
        np.savez(path, **dict(zip(self._KEYS, self.get_weights())))

    def load_weights(self, path):
        with np.load(path) as z:
            self.set_weights([z[k] for k in self._KEYS])

    def _check(self, x, what="nlist"):
        ops._dev(x, what)
        if x.dim() != 3 or x.shape[2] != 4:
            raise ValueError("DescriptorMLP: %s must be [B, NN, 4], got %s" % (what, tuple(x.shape)))
        ops._dt(x)
        if x.shape[1] > self.MAX_NN:
            raise ValueError("DescriptorMLP: NN = %d neighbor slots; the kernel takes at most %d" % (x.shape[1], self.MAX_NN))
        ops._dev(self.w, "DescriptorMLP.w", torch.float32)
        if self.w.device != x.device or self.w.numel() != self.n_models * self.n_species * self.P:
            raise ValueError("DescriptorMLP: the weights (%d floats on %s) do not fit a call on %s" % (self.w.numel(), self.w.device, x.device))
        return int(x.shape[0]), int(x.shape[1])

    def _partition(self, species, x):
        """The rows of a batch grouped by species: (rows, counts) -- ``rows`` int32 [B] on the device, species 0's rows first,
        ascending inside a species (a stable sort of the rounded species); ``counts`` the S sizes on the host.  One read-back
        of the counts serves the launch sizes and the range check.  Cached while the same species tensor is passed."""
        S, B = self.n_species, int(x.shape[0])
        if species is None:
            raise ValueError("DescriptorMLP: n_species = %d needs the particles' species: layer(nlist, positions), "
                             "forces(x, species=...) or loss_gradient(x, labels, species=...)" % S)
        if (not isinstance(species, torch.Tensor) or species.device != x.device
                or tuple(species.shape) not in ((B,), (B, 4))):
            raise ValueError("DescriptorMLP: species must be a [%d] or [%d, 4] tensor on %s, got %s" % (
                B, B, x.device, tuple(species.shape) if isinstance(species, torch.Tensor) else type(species)))

        def build():
            col = species[:, 3] if species.dim() == 2 else species
            sp = torch.round(col.detach().to(torch.float64))
            idx = torch.where((sp >= 0) & (sp < S), sp, torch.full_like(sp, S)).to(torch.int64)   # (NaN: S, out of range)
            rows = torch.argsort(idx, stable=True).to(torch.int32).contiguous()
            return rows, torch.bincount(idx, minlength=S + 1).cpu().tolist()

        rows, counts = cgmap._cached("descriptor-species", (species,), x.device, build, extra=S)
        if counts[S]:
            raise ValueError("DescriptorMLP: %d of %d rows have a species outside [0, %d)" % (counts[S], B, S))
        return rows, counts[:S]

    def species_counts(self, species, x):
        """Rows per species of the batch ``x`` (the cached partition's counts); [B] for one species."""
        return [int(x.shape[0])] if self.n_species == 1 else self._partition(species, x)[1]

    def _launches(self, species, x):
        """One (species, row-list pointer, rows, weight pointer) per launch: the whole batch for one network, else one per
        species present, each with its slice of the partition and of ``w``."""
        if self.n_species == 1:
            return [(0, None, int(x.shape[0]), self.w.data_ptr())], None
        rows, counts = self._partition(species, x)
        out, o = [], 0
        for s, c in enumerate(counts):
            if c:
                out.append((s, rows.data_ptr() + 4 * o, c, self.w.data_ptr() + 4 * s * self.P))
            o += c
        return out, rows   # (rows: kept alive by the caller until its launches are queued)

    class _Args:
        """The argument groups the family's C entries share (include/htf_bp.h and its followers), formed once per call on ``x``
        (checked here): ``pair`` the pair tensor and its dtype, ``shape`` (B, NN), ``rbf`` (K, n_types, mu, gap) as the entries
        without a network take them, ``net(d_w)`` (K, n_types, H1, H2, act, w, mu, gap), ``rows(d_rows, n_rows)`` with the
        cutoff behind them (``r_cut``, 0 for none), and the stream.  A call site composes them in its entry's order."""

        def __init__(self, lay, x):
            self.B, self.NN = self.shape = lay._check(x)
            self.pair = (x.data_ptr(), ops._dt(x))
            self.rbf = (lay.K, lay.n_types, lay.mu.data_ptr(), float(lay.gap))
            self.widths = (lay.K, lay.n_types, lay.H1, lay.H2, _lib.ACT_TANH if lay.activation == "tanh" else _lib.ACT_LINEAR)
            self.r_cut = float(lay.r_cut or 0.0)
            self.stream = ops._stream(x)

        def net(self, d_w):
            return self.widths + (d_w,) + self.rbf[2:]

        def rows(self, d_rows, n_rows):
            return (d_rows, n_rows, self.r_cut)

    @staticmethod
    def _dst(out, v):
        """Forces, their dtype and the virial (or none) as the force entries take them."""
        return (out.data_ptr(), ops._dt(out), v.data_ptr() if v is not None else None)

    def forces(self, x, virial=False, species=None):
        """The kernel on a pair-vector tensor ``x`` [B, NN, 4] (fp32 or fp64): forces [B, 4] in ``x``'s dtype, and the
        [B, 3, 3] virial when ``virial``.  compute_nlist_forces calls this for the layer's energy.  ``species``: [B] or
        [B, 4] (column 3), needed when ``n_species > 1``."""
        self._no_angular("forces")
        self._no_committee("forces")
        a = self._Args(self, x)
        out = torch.empty((a.B, 4), dtype=x.dtype, device=x.device)
        v = torch.empty((a.B, 3, 3), dtype=x.dtype, device=x.device) if virial else None
        launches, rows = self._launches(species, x)
        for _, d_rows, n_rows, d_w in launches:   # every row is in exactly one list: no memset
            check(lib.htf_bp_forces(*a.pair, *a.shape, *a.net(d_w), *self._dst(out, v), *a.rows(d_rows, n_rows), a.stream))
        return (out, v) if virial else out

    def _no_angular(self, what):
        if self.l_max:
            raise ValueError("DescriptorMLP: %s() is the row operator's, which has no angular form (l_max = %d): "
                             "total_forces(x, index) evaluates this layer" % (what, self.l_max))

    @staticmethod
    def _slot_index(index, x):
        """The particle in each slot as a contiguous int32 [B, NN] on ``x``'s device; a float tensor is taken by ``rint``."""
        B, NN = int(x.shape[0]), int(x.shape[1])
        if not isinstance(index, torch.Tensor) or tuple(index.shape) != (B, NN) or index.device != x.device:
            raise ValueError("DescriptorMLP: index must be a [%d, %d] tensor on %s, got %s" % (
                B, NN, x.device, tuple(index.shape) if isinstance(index, torch.Tensor) else type(index)))
        if index.dtype != torch.int32:
            index = torch.round(index.detach()).to(torch.int32) if index.is_floating_point() else index.to(torch.int32)
        return index.contiguous()

    @staticmethod
    def _ghost_rows(n_ghost, halo, what):
        """``n_ghost`` as an int; ghost rows without a ``halo`` to fill them raise."""
        if isinstance(n_ghost, bool) or int(n_ghost) != n_ghost or int(n_ghost) < 0:
            raise ValueError("DescriptorMLP: %s(n_ghost=%r): a row count, 0 or more" % (what, n_ghost))
        n_ghost = int(n_ghost)
        if n_ghost and halo is None:
            raise ValueError("DescriptorMLP: %s(n_ghost=%d) needs halo=: the callable that fills the ghosts' rows of the table "
                             "(SlabDomain.halo_rows under domain decomposition)" % (what, n_ghost))
        if n_ghost and not callable(halo):
            raise ValueError("DescriptorMLP: %s(halo=%r) is not callable" % (what, halo))
        return n_ghost

    def total_forces(self, x, index, virial=False, types=None, species=None, n_ghost=0, halo=None, members=False):
        """The forces of the total energy, ``F = -d(sum_i E_i)/dr`` (include/htf_cforce.h), on a pair-vector tensor ``x``
        [B, NN, 4] (fp32 or fp64): [B, 4] in ``x``'s dtype with ``E_i`` (``forces``' bits) in column 3, and with ``virial``
        the [B, 3, 3] ``W_i = -1/2 sum_s x_ij (outer) phi_is``.  ``index`` [B, NN]: the particle in each slot, int32 or a float
        tensor taken by ``rint``; a value outside ``[0, B)`` leaves that slot without its reverse term.  ``types``: the rows'
        own types, [B] or [B, 4] (column 3), required when ``n_types > 1``.  ``species`` as for ``forces``.  Equal to the
        gradient when the list is symmetric within the descriptor's range (full lists, no overflow, ``r_cut`` not above the
        list's cutoff); not checked.

        ``n_ghost > 0``: ``x`` holds the rows of one domain and ``index`` also names ``n_ghost`` ghost particles, numbered
        ``B .. B + n_ghost - 1`` (include/htf_cghost.h).  The table the second sweep gathers from -- ``g``, or ``{g, p, S}`` with
        ``l_max > 0`` -- then has ``B + n_ghost`` rows: the first sweep writes rows ``[0, B)``, ``halo(table)`` is called once and
        must fill rows ``[B, B + n_ghost)`` in place with what the ghosts' owners computed, with work ordered on the current
        stream (``SlabDomain.halo_rows``), and the second sweep reads a reverse term for every index in ``[0, B + n_ghost)``.
        The rows then carry the bits the whole system's call gives them.  Without ``halo`` it raises; with ``n_ghost = 0`` the
        ``halo`` is not called.

        On a committee (``n_models = M > 1``, include/htf_committee.h) the result is the mean model: ``(Fbar_i, Ebar_i)`` and
        the mean virial, in ``x``'s dtype; ``self.deviation`` becomes this call's [B, 2] fp32 ``(devF_i, devE_i)``, and
        ``members=True`` appends the [M, B, 4] fp32 tensor of ``(F_i^m, E_i^m)`` to what is returned.  ``n_ghost > 0`` raises
        there."""
        n_ghost = self._ghost_rows(n_ghost, halo, "total_forces")
        if self.n_models > 1 and n_ghost:
            raise NotImplementedError("DescriptorMLP: a committee (n_models = %d) does not run on a domain's rows (n_ghost = %d): "
                                      "slab domains are a follow-up; member(m).total_forces(..., n_ghost=, halo=) evaluates "
                                      "one member there" % (self.n_models, n_ghost))
        if members and self.n_models == 1:
            raise ValueError("DescriptorMLP: total_forces(members=True) is a committee's (n_models > 1)")
        a = self._Args(self, x)
        B, M = a.B, self.n_models
        index = self._slot_index(index, x)
        own = None
        if self.n_types > 1:
            if types is None:
                raise ValueError("DescriptorMLP: n_types = %d needs the rows' own types: total_forces(x, index, types=...)"
                                 % self.n_types)
            if hasattr(types, "plain"):
                types = types.plain()
            if (not isinstance(types, torch.Tensor) or types.device != x.device or tuple(types.shape) not in ((B,), (B, 4))):
                raise ValueError("DescriptorMLP: types must be a [%d] or [%d, 4] tensor on %s, got %s" % (
                    B, B, x.device, tuple(types.shape) if isinstance(types, torch.Tensor) else type(types)))
            own = (types[:, 3] if types.dim() == 2 else types).detach().to(torch.float32).contiguous()
        out = torch.empty((B, 4), dtype=x.dtype, device=x.device)
        v = torch.empty((B, 3, 3), dtype=x.dtype, device=x.device) if virial else None

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=x.device)

        # the family: its two entries, the table pass 1 writes and pass 2 gathers from, and what each entry takes of its own
        dev = mem = None
        if M > 1:        # include/htf_committee.h: the two sweeps for all members at once
            grad, forces, table, e = lib.htf_cmt_grad, lib.htf_cmt_forces, f32(B, M, self.D), f32(B, M)
            dev, mem = f32(B, 2), f32(M, B, 4) if members else None
            own1, own2 = (M, self.n_species * self.P), (M, dev.data_ptr(), mem.data_ptr() if members else None)
        elif self.l_max:   # include/htf_angular.h: the table {g, p, S} per row and channel in place of g
            grad, forces, e = lib.htf_ang_grad, lib.htf_ang_forces_ghost, f32(B)
            table = f32(B + n_ghost, self.Dr, 4 if self.l_max == 1 else 10)
            own1, own2 = (self.l_max,), (self.l_max, B + n_ghost)
        else:            # include/htf_cforce.h; pass 2 by include/htf_cghost.h, whose n_table = B is the plain entry
            grad, forces, table, e = lib.htf_cf_grad, lib.htf_cf_forces_ghost, f32(B + n_ghost, self.D), f32(B)
            own1, own2 = (), (B + n_ghost,)
        launches, rows = self._launches(species, x)
        for _, d_rows, n_rows, d_w in launches:   # pass 1: every row is in exactly one list
            check(grad(*a.pair, *a.shape, *a.net(d_w), table.data_ptr(), e.data_ptr(), *a.rows(d_rows, n_rows), *own1, a.stream))
        if n_ghost:
            halo(table)
        check(forces(*a.pair, index.data_ptr(), own.data_ptr() if own is not None else None, *a.shape, *a.rbf, table.data_ptr(),
                     e.data_ptr(), *self._dst(out, v), a.r_cut, *own2, a.stream))
        if M > 1:
            self.deviation = dev
        res = (out,) + ((v,) if virial else ()) + ((mem,) if members else ())
        return res if len(res) > 1 else out

    def loss_gradient(self, x, labels, pred=None, accum=None, species=None):
        """One force-matching sweep (htf_bp_loss_grad) over a pair-vector tensor ``x`` [B, NN, 4] (fp32 or fp64) and
        ``labels`` [B, 4] (fp32 or fp64): returns ``accum`` [1 + P] fp32 on the device, {sum of squared residuals of
        (F_i, E_i), its gradient with respect to ``w``} -- what ``ops.optimizer_step(w, accum, 1 / (4 B), ...)`` consumes for
        Keras' MeanSquaredError.  ``pred`` [B, 4] fp32: the layer's ``forces(x)`` at the current weights, evaluated here
        when not given.  Two calls on the same inputs give the same bits.  With ``n_species = S > 1`` (``species`` as for
        ``forces``) ``accum`` is [S, 1 + P]: row ``s`` holds the residuals and the gradient of network ``s`` over species
        ``s``'s rows, zeros when it has none; each row steps its own slice of ``w``."""
        self._no_angular("loss_gradient")
        self._no_committee("loss_gradient")
        a = self._Args(self, x)
        pred, accum, launches, rows, scratch = self._sweep_buffers(x, labels, pred, accum, species,
                                                                   lambda: self.forces(x, species=species))
        for s, d_rows, n_rows, d_w in launches:
            check(lib.htf_bp_loss_grad(*a.pair, *a.shape, *a.net(d_w), labels.data_ptr(), ops._dt(labels), pred.data_ptr(),
                                       accum.data_ptr() + 4 * s * (1 + self.P), scratch.data_ptr(), *a.rows(d_rows, n_rows),
                                       a.stream))
        return accum

    def _sweep_buffers(self, x, labels, pred, accum, species, evaluate, members=0, scratch_floats=None):
        """What the force-matching sweeps share ahead of their C calls: the checks of ``labels``, of ``pred`` (``evaluate()``,
        in fp32, when not given) and of ``accum`` (made here when not given), the launches, one scratch buffer, and zeros in the
        rows of ``accum`` whose species is absent.  ``members=M``: the committee's sweep, whose ``pred`` and ``accum`` carry a
        leading axis of length M; ``scratch_floats(n_rows)``: the floats its entry wants for a launch (htf_bp_scratch_floats
        when not given).  Returns (pred, accum, launches, rows, scratch); ``rows`` is what ``_launches`` asks its caller to keep."""
        B = int(x.shape[0])
        lead = (members,) if members else ()
        ops._dev(labels, "labels")
        ops._dt(labels)
        if tuple(labels.shape) != (B, 4) or labels.device != x.device:
            raise ValueError("DescriptorMLP: labels must be [%d, 4] on %s, got %s on %s" % (B, x.device, tuple(labels.shape), labels.device))
        if pred is None:
            pred = evaluate()
            if pred.dtype != torch.float32:
                pred = pred.to(torch.float32)
        ops._dev(pred, "pred", torch.float32)
        if tuple(pred.shape) != lead + (B, 4) or pred.device != x.device:
            raise ValueError("DescriptorMLP: pred must be %s on %s%s, got %s on %s" % (
                list(lead + (B, 4)), x.device, " (total_forces(..., members=True))" if members else "", tuple(pred.shape), pred.device))
        S, P = self.n_species, self.P
        total = (members or 1) * S * (1 + P)
        if accum is None:
            accum = torch.empty(lead + ((S, 1 + P) if S > 1 else (1 + P,)), dtype=torch.float32, device=x.device)
        ops._dev(accum, "accum", torch.float32)
        if accum.numel() != total or accum.device != x.device or (members and not accum.is_contiguous()):
            raise ValueError("DescriptorMLP: accum must hold %d %sfloats on %s" % (total, "contiguous " if members else "", x.device))
        launches, rows = self._launches(species, x)
        # one scratch buffer for the largest species: the launches run one after the other on the stream
        # (htf_bp_scratch_floats sized for D = K n_types (1 + l_max) inputs: P is this layer's)
        n_max = max([n for _, _, n, _ in launches] or [0])
        floats = (scratch_floats(n_max) if scratch_floats else
                  lib.htf_bp_scratch_floats(n_max, self.K, self.n_types * (1 + self.l_max), self.H1, self.H2))
        scratch = torch.empty(max(1, int(floats)), dtype=torch.float32, device=x.device)
        present = {s for s, _, _, _ in launches}   # (every other row of accum is written by its species' launch)
        for s in range(S):
            if s not in present:
                accum.view(-1, S, 1 + P)[:, s].zero_()
        return pred, accum, launches, rows, scratch

    def _sweep(self, entry, a, index, rho, buffers, own):
        """The launches of a sweep on the forces of the total energy: ``entry`` once per species present, on the residual table
        ``rho``, with what ``_sweep_buffers`` returned; ``own``: what the entry takes of its own ahead of the stream."""
        _, accum, launches, _, scratch = buffers
        for s, d_rows, n_rows, d_w in launches:   # (d_w: species s, of member 0 in a committee; its row of accum likewise)
            check(entry(*a.pair, index.data_ptr(), *a.shape, *a.net(d_w), rho.data_ptr(), accum.data_ptr() + 4 * s * (1 + self.P),
                        scratch.data_ptr(), *a.rows(d_rows, n_rows), *own, a.stream))
        return accum

    def total_loss_gradient(self, x, labels, index, types=None, pred=None, accum=None, species=None, n_ghost=0, halo=None):
        """One force-matching sweep on the forces of the total energy (htf_ct_loss_grad, include/htf_ctrain.h): ``accum`` as
        ``loss_gradient`` returns it -- [1 + P], or [S, 1 + P] with zero rows for absent species -- for the residuals of
        ``total_forces(x, index, ...)`` against ``labels`` [B, 4], so that the fit and a ``conservative=True`` run see the same
        model.  ``index`` as for ``total_forces``; a slot whose index is outside ``[0, B)`` has no reverse term, as there.
        ``pred`` [B, 4] fp32: ``total_forces`` at the current weights, evaluated here (with ``types``, which the sweep itself
        does not need) when not given.  The residual ``pred - labels`` is formed in fp32 with torch and every row's is read:
        ``x`` holds the whole system.  Two calls on the same inputs give the same bits.  Callable on any layer, like
        ``total_forces``.

        ``n_ghost > 0`` (as for ``total_forces``): ``x`` holds one domain's rows; the residual table has ``B + n_ghost`` rows,
        ``halo(rho)`` fills the ghosts' rows with their owners' residuals, and ``pred``, when not given, is ``total_forces``
        with the same ``n_ghost`` and ``halo``.  ``accum`` then holds this domain's rows' share: the sum over the domains is the
        whole system's sweep."""
        self._no_committee("total_loss_gradient")
        if self.l_max:
            raise NotImplementedError("DescriptorMLP: total_loss_gradient() is the sweep of an l_max = 0 layer; with l_max = %d its "
                                      "follow-up angular_loss_gradient(x, labels, index) is the force-matching sweep" % self.l_max)
        return self._conservative_sweep(x, labels, index, types, pred, accum, species, n_ghost, halo, "total_loss_gradient")

    def angular_loss_gradient(self, x, labels, index, types=None, pred=None, accum=None, species=None, n_ghost=0, halo=None):
        """``total_loss_gradient`` for a layer with ``l_max = 1`` or ``2`` (htf_at_loss_grad, include/htf_atrain.h): one
        force-matching sweep on the forces of the total energy with angular channels.  Argument for argument the same: ``accum``
        [1 + P], or [S, 1 + P] with zero rows for absent species, holds {SSR, d SSR / d theta} per network for the residuals of
        ``total_forces(x, index, ...)`` against ``labels`` [B, 4]; ``pred`` [B, 4] fp32 is ``total_forces`` at the current
        weights, evaluated here when not given; the residual is formed in fp32 with torch; a slot whose index is outside
        ``[0, B)`` has no reverse term.  Two calls on the same inputs give the same bits.  Callable on any layer with
        ``l_max > 0``, trainable or not; with ``l_max = 0`` it raises.  ``n_ghost`` and ``halo`` as for ``total_loss_gradient``."""
        self._no_committee("angular_loss_gradient")
        if not self.l_max:
            raise ValueError("DescriptorMLP: angular_loss_gradient() is the sweep of the angular channels (l_max = 1 or 2); "
                             "total_loss_gradient(x, labels, index) is the sweep of this l_max = 0 layer")
        return self._conservative_sweep(x, labels, index, types, pred, accum, species, n_ghost, halo, "angular_loss_gradient")

    def _conservative_sweep(self, x, labels, index, types, pred, accum, species, n_ghost=0, halo=None, what="total_loss_gradient"):
        """The sweep on the forces of the total energy for this layer's ``l_max``: htf_ct_loss_grad, or htf_at_loss_grad; with
        ghost rows their twins of include/htf_cghost.h on the residual table of ``B + n_ghost`` rows."""
        n_ghost = self._ghost_rows(n_ghost, halo, what)
        a = self._Args(self, x)
        index = self._slot_index(index, x)
        buffers = self._sweep_buffers(
            x, labels, pred, accum, species,
            lambda: self.total_forces(x, index, types=types, species=species, n_ghost=n_ghost, halo=halo))
        n_table = a.B + n_ghost
        rho = torch.empty((n_table, 4), dtype=torch.float32, device=x.device)
        torch.sub(buffers[0].detach(), labels.detach().to(torch.float32), out=rho[:a.B])
        if n_ghost:
            halo(rho)
        if self.l_max:
            return self._sweep(lib.htf_at_loss_grad_ghost, a, index, rho, buffers, (self.l_max, n_table))
        return self._sweep(lib.htf_ct_loss_grad_ghost, a, index, rho, buffers, (n_table,))

    def committee_loss_gradient(self, x, labels, index, types=None, pred=None, accum=None, species=None):
        """``total_loss_gradient`` for every member of a committee in one sweep (htf_cmt_loss_grad, include/htf_cmt_train.h):
        returns ``accum`` [M, 1 + P] fp32 on the device -- [M, S, 1 + P] with ``n_species = S > 1``, zero rows for an absent
        species -- whose row ``m`` holds {SSR^m, d SSR^m / d theta^m} for the residuals of member ``m``'s forces against
        ``labels`` [B, 4]: what ``member(m, trainable="total").total_loss_gradient(x, labels, index, pred=pred[m])`` returns,
        without reading the pair vectors, the index and the neighbors' residuals M times.  Every member is fitted on its own to
        the same labels; ``ops.optimizer_step(w[m P:(m + 1) P], accum[m], 1 / (4 B), ...)`` steps member ``m``.  ``pred``
        [M, B, 4] fp32: the members tensor of ``total_forces(x, index, ..., members=True)`` at the current weights, evaluated
        here (with ``types``) when not given.  The residual table [B, M, 4] is formed in fp32 with torch and every row's is
        read: ``x`` holds the whole system.  Two calls on the same inputs give the same bits, and row ``m`` depends on member
        ``m``'s weights and residuals alone.  Callable on any committee, trainable or not; a single network raises."""
        if self.n_models < 2:
            raise ValueError("DescriptorMLP: committee_loss_gradient() is a committee's (n_models > 1); "
                             "total_loss_gradient(x, labels, index) is the sweep of this single network")
        a = self._Args(self, x)
        index = self._slot_index(index, x)
        M, S, P = self.n_models, self.n_species, self.P
        buffers = self._sweep_buffers(
            x, labels, pred, accum, species, lambda: self.total_forces(x, index, types=types, species=species, members=True)[-1],
            members=M, scratch_floats=lambda n: lib.htf_cmt_scratch_floats(n, self.K, self.n_types, self.H1, self.H2, M))
        # [B][M][4]: a particle's residuals are one record of 16 M bytes
        rho = (buffers[0].detach() - labels.detach().to(torch.float32).unsqueeze(0)).permute(1, 0, 2).contiguous()
        return self._sweep(lib.htf_cmt_loss_grad, a, index, rho, buffers, (M, S * P, S * (1 + P)))   # (members S P floats apart)

    def descriptor(self, nlist):
        """The network input [B, D] alone (the kernel's first stage), in the dtype of the pair-vector tensor: G, or
        [G | A | Q] with ``l_max > 0``."""
        self._no_committee("descriptor")
        x = simmodel._as_nlist(nlist).tensor
        a = self._Args(self, x)
        out = torch.empty((a.B, self.D), dtype=x.dtype, device=x.device)
        entry, own = (lib.htf_ang_descriptor, (self.l_max,)) if self.l_max else (lib.htf_bp_descriptor, ())
        check(entry(*a.pair, *a.shape, *a.rbf, out.data_ptr(), ops._dt(out), a.r_cut, *own, a.stream))
        simmodel._trace_log().append({"op": "descriptor"})   # (no replay: a model calling it keeps the eager path)
        return out

    def __call__(self, nlist, positions=None):
        nl = simmodel._as_nlist(nlist)
        if len(nl.shape) != 3 or nl.shape[2] != 4:
            raise ValueError("DescriptorMLP: nlist must be [B, NN, 4], got %s" % (tuple(nl.shape),))
        if nl.shape[1] > self.MAX_NN:
            raise ValueError("DescriptorMLP: NN = %d neighbor slots; the kernel takes at most %d" % (nl.shape[1], self.MAX_NN))
        if self.n_species > 1 and positions is None:
            raise ValueError("DescriptorMLP: n_species = %d needs the particles' species: layer(nlist, positions)" % self.n_species)
        return simmodel.DescriptorEnergy(nl, self, positions if self.n_species > 1 else None,
                                         positions=positions if self.conservative else None)


class EDSLayer:
    """layers.py:101-195.  Call it on the collective variable every step; returns alpha,
    the EDS coupling constant.  The running mean / ssd / TF1-Adam state lives on the
    device and advances in a one-thread kernel, so a device-resident CV never visits
    the host."""

    def __init__(self, set_point, period, learning_rate=1e-2, cv_scale=1.0, name='eds-layer', device="cuda"):
        if isinstance(set_point, (int, np.integer)) and not isinstance(set_point, bool):
            raise ValueError('EDS only works with floats, not dtype' + str(type(set_point)))
        self.set_point = float(set_point)
        self.period = int(period)
        self.cv_scale = float(cv_scale)
        self.learning_rate = float(learning_rate)
        self.name = name
        self.state = torch.zeros(8, dtype=torch.float32, device=device)

    def get_config(self):
        return {'set_point': self.set_point, 'period': self.period, 'cv_scale': self.cv_scale,
                'learning_rate': self.learning_rate}

    @property
    def alpha(self):
        return self.state[2]

    @property
    def mean(self):
        return self.state[0]

    @property
    def n(self):
        return int(self.state[5].item())

    def __call__(self, cv):
        if isinstance(cv, simmodel.PairCV):
            return simmodel.DeferredAlpha(self, cv)  # advances when the biased energy is lowered
        if not isinstance(cv, torch.Tensor):
            cv = torch.tensor(float(cv), dtype=torch.float32, device=self.state.device)
        cv = cv.detach().to(torch.float32).reshape(1).contiguous()
        check(lib.htf_eds_update(self.state.data_ptr(), cv.data_ptr(), self.set_point, self.period,
                                 self.learning_rate, self.cv_scale, ops._stream(self.state)))
        simmodel._trace_log().append({"stateful": self.name})
        return self.state[2]
