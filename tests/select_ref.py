"""A NumPy statement of include/htf_select.h, taken literally: what htf.DeviationSelector is compared with, exactly.

``SelectorRef`` has the selector's constructor, ``update``, ``counts``, ``frames``, ``last`` and ``reset``; it takes and returns
numpy arrays.  The thresholds are rounded to fp32, as the deviations are.  ``refused_equal`` counts, beyond the selector's seven
counters, the candidates that policy "largest" dropped because their s equalled the smallest stored one: the tests use it to
show that a sequence exercises that rule."""
import numpy as np

COUNTERS = ("seen", "accurate", "candidate", "failed", "stored", "dropped", "replaced")


class SelectorRef:
    def __init__(self, n_particles, capacity, lo, hi=float("inf"), quantity="force", policy="first", dtype=np.float32,
                 device=None, max_blocks=None):
        assert quantity in ("force", "energy") and policy in ("first", "largest")
        self.n_particles, self.capacity = int(n_particles), int(capacity)
        self.lo, self.hi = np.float32(lo), np.float32(hi)
        assert np.isfinite(self.lo) and 0 <= self.lo <= self.hi
        self.column = 0 if quantity == "force" else 1
        self.policy, self.dtype = policy, np.dtype(dtype)
        self.reset()

    def reset(self):
        self.c = dict.fromkeys(COUNTERS, 0)
        self.slots = []            # per slot: dict(positions, box, s, argmax, stamp)
        self.last = np.zeros(2, np.float32)
        self.refused_equal = 0
        self.classes = []          # the class of every update since the reset, in order

    def update(self, deviation, positions, box=None):
        deviation, positions = np.asarray(deviation), np.asarray(positions)
        assert deviation.shape == (self.n_particles, 2) and deviation.dtype == np.float32
        assert positions.shape == (self.n_particles, 4) and positions.dtype == self.dtype
        d = deviation[:, self.column]
        nan = np.isnan(d)
        a = int(np.argmax(nan)) if nan.any() else int(np.argmax(d))     # (argmax: the first of equal maxima)
        s = d[a]
        stamp = self.c["seen"]
        self.c["seen"] += 1
        self.last = np.array([s, np.float32(a)], np.float32)
        if np.isnan(s) or (np.isfinite(self.hi) and s >= self.hi):
            self.c["failed"] += 1
            self.classes.append("failed")
            return
        if s < self.lo:
            self.c["accurate"] += 1
            self.classes.append("accurate")
            return
        self.c["candidate"] += 1
        self.classes.append("candidate")
        box = np.zeros((3, 3), self.dtype) if box is None else np.asarray(box)
        assert box.shape == (3, 3) and box.dtype == self.dtype
        frame = dict(positions=positions.copy(), box=box.copy(), s=np.float32(s), argmax=a, stamp=stamp)
        if len(self.slots) < self.capacity:
            self.slots.append(frame)
            self.c["stored"] += 1
            return
        if self.policy == "largest":
            stored = np.array([f["s"] for f in self.slots], np.float32)
            j = int(np.argmin(stored))                                  # (argmin: the lowest slot of equal minima)
            if s > stored[j]:
                self.slots[j] = frame
                self.c["replaced"] += 1
                return
            if s == stored[j]:
                self.refused_equal += 1
        self.c["dropped"] += 1

    def counts(self):
        return dict(self.c)

    def frames(self):
        fs = sorted(self.slots, key=lambda f: f["stamp"])
        N = self.n_particles
        return {"positions": np.array([f["positions"] for f in fs], self.dtype).reshape(len(fs), N, 4),
                "box": np.array([f["box"] for f in fs], self.dtype).reshape(len(fs), 3, 3),
                "s": np.array([f["s"] for f in fs], np.float32),
                "argmax": np.array([f["argmax"] for f in fs], np.int64),
                "stamp": np.array([f["stamp"] for f in fs], np.int64)}
