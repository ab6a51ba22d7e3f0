"""``DeviationSelector``: the "select" step of an active-learning loop, on the device (include/htf_select.h, csrc/select.hip).

A committee ``DescriptorMLP(conservative=True, n_models=M)`` leaves the per-particle model deviation ``layer.deviation``
[N, 2] = (devF_i, devE_i) after every ``total_forces``.  ``update`` classifies the frame by the largest of them -- accurate
below ``lo``, failed from ``hi`` on (or NaN), a candidate in between -- and keeps the candidates' positions and box in a buffer
of ``capacity`` frames: three launches on the current stream, no read-back, so that the step loop never waits.  ``frames`` and
``trajectory`` hand the stored frames over for labelling and for ``iter_from_trajectory``.
"""
import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .ops import _stream

_POLICIES = {"first": _lib.SEL_FIRST, "largest": _lib.SEL_LARGEST}
_QUANTITIES = {"force": _lib.SEL_FORCE, "energy": _lib.SEL_ENERGY}
_COUNTERS = ("seen", "accurate", "candidate", "failed", "stored", "dropped", "replaced")


class DeviationSelector:
    """Frames picked by committee deviation (the DP-GEN rule), held on the device.

    ``n_particles``: rows N of every frame; ``capacity``: frames the buffer holds, 1 to 65 536; ``lo``, ``hi``: the thresholds,
    0 <= lo <= hi, lo finite, taken as fp32 like the deviations (``hi = inf``: nothing fails but a NaN); ``quantity``: "force"
    (column 0 of the deviation) or "energy" (column 1); ``policy``: what a candidate meets when the buffer is full -- "first"
    drops it, "largest" lets it replace the stored frame of the smallest deviation (the lowest slot among equals) if its own is
    strictly larger; ``dtype``: fp32 or fp64, of the positions and the box it is given and keeps; ``max_blocks``: a cap on the
    reduction's grid (None: the library's), there for testing.

    Per update, s = max_i d_i and a = the lowest i with d_i = s (a NaN anywhere: s is NaN and a the lowest index holding one);
    exact, so that no launch shape changes them.  Counters: seen = accurate + candidate + failed, candidate = stored + replaced
    + dropped, stored <= capacity.
    """

    def __init__(self, n_particles, capacity, lo, hi=float("inf"), quantity="force", policy="first", dtype=torch.float32,
                 device=None, max_blocks=None):
        for name, v in (("n_particles", n_particles), ("capacity", capacity)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("DeviationSelector: %s must be an integer, not %r" % (name, v))
        if n_particles < 1:
            raise ValueError("DeviationSelector: n_particles = %d; a frame holds at least one particle" % n_particles)
        if not 1 <= capacity <= _lib.SEL_MAX_CAPACITY:
            raise ValueError("DeviationSelector: capacity = %d outside [1, %d]" % (capacity, _lib.SEL_MAX_CAPACITY))
        if quantity not in _QUANTITIES:
            raise ValueError("DeviationSelector: quantity must be 'force' or 'energy', not %r" % (quantity,))
        if policy not in _POLICIES:
            raise ValueError("DeviationSelector: policy must be 'first' or 'largest', not %r" % (policy,))
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("DeviationSelector: dtype must be torch.float32 or torch.float64, not %r" % (dtype,))
        lo, hi = float(np.float32(lo)), float(np.float32(hi))
        if not (np.isfinite(lo) and 0.0 <= lo <= hi):
            raise ValueError("DeviationSelector: thresholds must be 0 <= lo <= hi with lo finite, not lo = %r, hi = %r" % (lo, hi))
        if max_blocks is None:
            max_blocks = 0
        elif isinstance(max_blocks, bool) or not isinstance(max_blocks, (int, np.integer)) or not 1 <= max_blocks <= _lib.SEL_MAX_BLOCKS:
            raise ValueError("DeviationSelector: max_blocks must be None or an integer in [1, %d], not %r"
                             % (_lib.SEL_MAX_BLOCKS, max_blocks))
        self.n_particles, self.capacity, self.lo, self.hi = int(n_particles), int(capacity), lo, hi
        self.quantity, self.policy, self.dtype, self.max_blocks = quantity, policy, dtype, int(max_blocks)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        # all zeros is the empty selector (include/htf_select.h); the frame buffers are named by the state alone
        self._state = torch.zeros(int(lib.htf_sel_state_words(self.capacity)), dtype=torch.int32, device=self.device)
        self._frames = torch.zeros((self.capacity, self.n_particles, 4), dtype=dtype, device=self.device)
        self._boxes = torch.zeros((self.capacity, 3, 3), dtype=dtype, device=self.device)
        self.last = self._state[_lib.SEL_LAST:_lib.SEL_LAST + 2].view(torch.float32)

    def _check(self, t, name, shape, dtype):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("DeviationSelector.update: %s must be a CUDA/HIP device tensor (the selector has no CPU path)" % name)
        if t.device != self.device:
            raise ValueError("DeviationSelector.update: %s is on %s, the selector on %s" % (name, t.device, self.device))
        if tuple(t.shape) != shape:
            hint = ""
            if len(shape) == 2 and t.dim() == 2 and t.shape[1] == shape[1]:
                hint = ": the selector was built for n_particles = %d" % self.n_particles
            raise ValueError("DeviationSelector.update: %s must be [%s], got %s%s"
                             % (name, ", ".join(str(s) for s in shape), tuple(t.shape), hint))
        if t.dtype != dtype:
            raise ValueError("DeviationSelector.update: %s must be %s, got %s" % (name, dtype, t.dtype))
        if not t.is_contiguous():
            raise ValueError("DeviationSelector.update: %s must be contiguous" % name)
        return t

    def update(self, deviation, positions, box=None):
        """Classify the frame by ``deviation`` [N, 2] fp32 (``layer.deviation``) and, if it is a candidate with a place in the
        buffer, keep ``positions`` [N, 4] (a tensor or the ``PositionsInput`` of ``compute``) and ``box`` [3, 3] (None: zeros),
        both of the selector's dtype.  Enqueues on the current stream and returns None; never synchronises, never allocates."""
        N = self.n_particles
        plain = getattr(positions, "plain", None)
        if callable(plain):
            positions = plain()
        dev = self._check(deviation, "deviation", (N, 2), torch.float32)
        pos = self._check(positions, "positions", (N, 4), self.dtype)
        if box is not None:
            box = self._check(box, "box", (3, 3), self.dtype)
        check(lib.htf_sel_update(dev.data_ptr(), N, _QUANTITIES[self.quantity], self.lo, self.hi, _POLICIES[self.policy],
                                 self.capacity, self._state.data_ptr(), pos.data_ptr(), None if box is None else box.data_ptr(),
                                 _lib.HTF_F32 if self.dtype == torch.float32 else _lib.HTF_F64, self._frames.data_ptr(),
                                 self._boxes.data_ptr(), self.max_blocks, _stream(self._state)))

    def reset(self):
        """Counters and buffer emptied, on the current stream."""
        if self.device.type != "cuda":
            self._state.zero_()
            return
        check(lib.htf_sel_reset(self._state.data_ptr(), self.capacity, _stream(self._state)))

    def counts(self):
        """The seven counters as a dict of ints (one read-back)."""
        c = self._state[:len(_COUNTERS)].cpu().numpy().view(np.uint32)
        return {name: int(v) for name, v in zip(_COUNTERS, c)}

    def frames(self):
        """The stored frames as CPU numpy arrays, ordered by stamp ascending: ``positions`` [n, N, 4], ``box`` [n, 3, 3] (the
        selector's dtype), ``s`` [n] fp32, ``argmax`` [n] and ``stamp`` [n] (the 0-based ordinal of the update), n = stored."""
        state = self._state.cpu().numpy()
        cap, h = self.capacity, _lib.SEL_HEADER_WORDS
        n = int(state.view(np.uint32)[_lib.SEL_STORED])
        s = state[h:h + n].view(np.float32)
        a = state[h + cap:h + cap + n].view(np.uint32)
        stamp = state[h + 2 * cap:h + 2 * cap + n].view(np.uint32)
        order = np.argsort(stamp, kind="stable")
        return {"positions": self._frames[:n].cpu().numpy()[order], "box": self._boxes[:n].cpu().numpy()[order],
                "s": s[order].copy(), "argmax": a[order].astype(np.int64), "stamp": stamp[order].astype(np.int64)}

    def trajectory(self):
        """The stored frames as an ``ArrayTrajectory`` for ``iter_from_trajectory``: positions from columns 0 to 2, dimensions
        [Lx, Ly, Lz, 90, 90, 90] from each stored box (``box[1] - box[0]``), types from column 3 of the first stored frame."""
        from .trajectory import ArrayTrajectory
        f = self.frames()
        n = len(f["stamp"])
        if n == 0:
            raise ValueError("DeviationSelector.trajectory: no frame is stored")
        box = f["box"]
        if np.any(box[:, 2] != 0):
            raise ValueError("DeviationSelector.trajectory: a stored box has a non-zero tilt row %s (only orthorhombic boxes are "
                             "supported)" % (box[np.any(box[:, 2] != 0, axis=1)][0, 2].tolist(),))
        dims = np.concatenate([box[:, 1] - box[:, 0], np.full((n, 3), 90.0, box.dtype)], axis=1)
        return ArrayTrajectory(f["positions"][:, :, :3], dims, types=f["positions"][0, :, 3].astype(np.int64))
