"""tests/select_ref.SelectorRef, the NumPy statement of include/htf_select.h, on sequences worked by hand: every expected
value below is written out, none is computed.  No GPU."""
import numpy as np

from select_ref import SelectorRef

INF, NAN = float("inf"), float("nan")


def _frame(col, k, N=4, column=0, dtype=np.float32):
    """deviation [N, 2] with `col` in `column` (the other column holds 99, which must not matter), positions filled with k."""
    d = np.full((N, 2), 99.0, np.float32)
    d[:, column] = col
    return d, np.full((N, 4), float(k), dtype), np.full((3, 3), 10.0 + k, dtype)


def _run(ref, cols, **kw):
    for k, col in enumerate(cols):
        ref.update(*_frame(col, k, **kw))
    return ref


def test_class_boundaries():
    """lo = 0.5, hi = 2: s = lo is a candidate, s = hi failed, a NaN failed; just below lo accurate, just below hi a candidate."""
    below_lo, below_hi = np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(2), np.float32(0))
    ref = _run(SelectorRef(4, 8, 0.5, 2.0), [[0.1, 0.5, 0.2, 0.0], [0.0, 0.1, 2.0, 0.3], [0.1, NAN, 0.2, 0.3],
                                             [below_lo, 0, 0, 0], [0, 0, 0, below_hi], [INF, 0, 0, 0], [0, 0, 0, 0]])
    assert ref.classes == ["candidate", "failed", "failed", "accurate", "candidate", "failed", "accurate"]
    assert ref.counts() == dict(seen=7, accurate=2, candidate=2, failed=3, stored=2, dropped=0, replaced=0)
    f = ref.frames()
    assert f["s"].tolist() == [0.5, float(below_hi)] and f["argmax"].tolist() == [1, 3] and f["stamp"].tolist() == [0, 4]
    assert (f["positions"][0] == 0).all() and (f["positions"][1] == 4).all()
    assert (f["box"][0] == 10).all() and (f["box"][1] == 14).all()
    assert ref.last.tolist() == [0.0, 0.0]


def test_hi_inf():
    """hi = inf: no number fails, +inf is a candidate; a NaN still fails.  lo = 0: a frame of zeros is a candidate."""
    ref = _run(SelectorRef(4, 8, 0.0), [[0, 0, 0, 0], [1, INF, 2, INF], [NAN, INF, 0, 0], [3, 1, 3, 2]])
    assert ref.classes == ["candidate", "candidate", "failed", "candidate"]
    f = ref.frames()
    assert f["s"].tolist() == [0.0, INF, 3.0] and f["argmax"].tolist() == [0, 1, 0] and f["stamp"].tolist() == [0, 1, 3]
    assert ref.counts() == dict(seen=4, accurate=0, candidate=3, failed=1, stored=3, dropped=0, replaced=0)


def test_last_nan_and_ties():
    """``last`` is (s, a) of the last update whatever its class; the lowest index of equal maxima; the lowest NaN beats any
    number and any later NaN."""
    ref = SelectorRef(6, 2, 1.0, 5.0)
    for col, want in (([0.2, 0.7, 0.7, 0.1, 0.7, 0.0], (np.float32(0.7), 1.0)), ([3, 1, 3, 3, 0, 2], (3.0, 0.0)),
                      ([9, 9, NAN, 0, 9, NAN], (NAN, 2.0)), ([0, 0, 0, 0, 0, 8], (8.0, 5.0))):
        ref.update(*_frame(col, 0, N=6))
        assert (np.isnan(ref.last[0]) if np.isnan(want[0]) else ref.last[0] == want[0]) and ref.last[1] == want[1]
    assert ref.classes == ["accurate", "candidate", "failed", "failed"]


def test_energy_column_and_dtype():
    """quantity = "energy" reads column 1 (column 0 holds 99 here and would fail every frame); fp64 frames stay fp64."""
    ref = _run(SelectorRef(4, 2, 0.5, 2.0, quantity="energy", dtype=np.float64), [[0.1, 0.2, 0.3, 0.4], [0.6, 0.2, 0.6, 0.1]],
               column=1, dtype=np.float64)
    assert ref.classes == ["accurate", "candidate"]
    f = ref.frames()
    assert f["positions"].dtype == np.float64 and f["box"].dtype == np.float64 and f["s"].dtype == np.float32
    assert f["s"].tolist() == [float(np.float32(0.6))] and f["argmax"].tolist() == [0] and f["stamp"].tolist() == [1]


def test_first_overflow():
    """capacity 2, "first": the third and fourth candidates are dropped, larger or not."""
    ref = _run(SelectorRef(4, 2, 1.0, policy="first"), [[1, 0, 0, 0], [0, 2, 0, 0], [0, 0, 9, 0], [0.5, 0, 0, 0], [0, 0, 0, 3]])
    assert ref.counts() == dict(seen=5, accurate=1, candidate=4, failed=0, stored=2, dropped=2, replaced=0)
    f = ref.frames()
    assert f["s"].tolist() == [1.0, 2.0] and f["stamp"].tolist() == [0, 1] and f["argmax"].tolist() == [0, 1]
    assert (f["positions"][0] == 0).all() and (f["positions"][1] == 1).all()


def test_largest_replacement():
    """capacity 3, "largest".  s per update: 2, 1, 1 fill slots 0, 1, 2.  Then 1: equal to the smallest, dropped and counted as
    refused.  Then 1.5: the smallest is 1 in slots 1 and 2, the tie goes to slot 1 (stamp 1 leaves).  Then 0.5 (lo = 0.25):
    smaller than every stored s, dropped.  Then 3: replaces slot 2 (s = 1, stamp 2).  Then 1.5: equals the smallest now, refused.
    Stored at the end: slot 0 (2, stamp 0), slot 1 (1.5, stamp 4), slot 2 (3, stamp 6)."""
    ref = _run(SelectorRef(4, 3, 0.25, policy="largest"),
               [[2, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [1, 0, 0, 0], [0, 1.5, 0, 0], [0.5, 0, 0, 0], [0, 0, 0, 3], [1.5, 1.5, 0, 0]])
    assert ref.counts() == dict(seen=8, accurate=0, candidate=8, failed=0, stored=3, dropped=3, replaced=2)
    assert ref.refused_equal == 2
    assert [s["stamp"] for s in ref.slots] == [0, 4, 6]
    f = ref.frames()
    assert f["stamp"].tolist() == [0, 4, 6] and f["s"].tolist() == [2.0, 1.5, 3.0] and f["argmax"].tolist() == [0, 1, 3]
    assert [float(p[0, 0]) for p in f["positions"]] == [0.0, 4.0, 6.0] and [float(b[0, 0]) for b in f["box"]] == [10.0, 14.0, 16.0]


def test_largest_keeps_inf():
    """A stored +inf is never the one to leave, and an +inf does not replace an +inf."""
    ref = _run(SelectorRef(4, 1, 0.0, policy="largest"), [[1, 0, 0, 0], [INF, 0, 0, 0], [0, INF, 0, 0], [5, 0, 0, 0]])
    assert ref.counts() == dict(seen=4, accurate=0, candidate=4, failed=0, stored=1, dropped=2, replaced=1)
    assert ref.refused_equal == 1 and ref.frames()["stamp"].tolist() == [1] and ref.frames()["argmax"].tolist() == [0]


def test_box_none_and_reset():
    ref = SelectorRef(4, 2, 0.0)
    d, p, _ = _frame([1, 2, 3, 4], 7)
    ref.update(d, p)
    assert (ref.frames()["box"] == 0).all() and ref.frames()["box"].shape == (1, 3, 3)
    ref.reset()
    assert ref.counts() == dict.fromkeys(("seen", "accurate", "candidate", "failed", "stored", "dropped", "replaced"), 0)
    f = ref.frames()
    assert f["positions"].shape == (0, 4, 4) and f["box"].shape == (0, 3, 3) and f["s"].shape == (0,)
    assert ref.last.tolist() == [0.0, 0.0] and ref.classes == []
    ref.update(d, p)
    assert ref.frames()["stamp"].tolist() == [0] and ref.frames()["argmax"].tolist() == [3]
