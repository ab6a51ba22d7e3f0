"""The cell-binned route of compute_nlist on the host: the C ABI table of include/htf_nlist.h, the grid rule, and the
argument checks of ``ArrayTrajectory`` / ``iter_from_trajectory`` that need no device.  No GPU."""
import numpy as np
import pytest


def test_nlist_abi_table(htf):
    """The cell route's entry points are a fifth table, the symbols of include/htf_nlist.h, exported by the library and
    bound under whichever binding is active, sharing no name with the other four tables."""
    import ctypes
    import os
    import re
    from helpers import ROOT
    hdr = open(os.path.join(ROOT, "include", "htf_nlist.h")).read()
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_nlist_\w+)\s*\(", hdr)))
    assert names == sorted(htf._lib.NLIST_PROTOTYPES) and len(names) == 2
    raw = ctypes.CDLL(htf._lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(htf._lib.lib, n)
    others = (set(htf._lib.PROTOTYPES) | set(htf._lib.STANDIN_PROTOTYPES) | set(htf._lib.CG_PROTOTYPES)
              | set(htf._lib.GEOM_PROTOTYPES))
    assert not set(names) & others


def test_nlist_pybind_module_exports_table(htf):
    import importlib
    import os
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.NLIST_PROTOTYPES:
        assert hasattr(mod, n)


def test_nlist_header_is_plain_c():
    """include/htf_nlist.h compiles as C99 beside htf_amd.h."""
    import os
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_nlist.h"\n'
                             'int main(void){int (*f)(const float *, unsigned, unsigned, const float *, float, unsigned, unsigned, '
                             'unsigned, unsigned, int, int, const unsigned char *, unsigned *, float *, int *, htf_stream) = '
                             'htf_nlist_cells_forward; unsigned long long (*g)(unsigned, unsigned) = htf_nlist_cells_scratch_words; '
                             '(void)f; (void)g; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_scratch_words_grow_with_m_and_cells(htf):
    w = htf._lib.lib.htf_nlist_cells_scratch_words
    assert w(1000, 27) >= 6 * 1000 + 3 * 28
    assert w(2000, 27) > w(1000, 27) and w(1000, 1000) > w(1000, 27)
    assert w(1 << 20, 1 << 20) % 4 == 0


def test_cell_grid_rule(htf):
    from hoomd_tf_amd import cgmap
    f32 = np.float32
    assert cgmap._cell_grid(1000, [12.0] * 3, f32(2.0)) == (5, 5, 5)
    assert cgmap._cell_grid(1000, [7.0] * 3, f32(2.0)) == (3, 3, 3)
    assert cgmap._cell_grid(1000, [6.0] * 3, f32(2.0)) is None          # 6 / (2 + margin) < 3
    assert cgmap._cell_grid(1000, [6.0] * 3, f32(1.99)) == (3, 3, 3)
    assert cgmap._cell_grid(1000, [31.0, 9.5, 14.25], f32(2.5)) == (12, 3, 5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert cgmap._cell_grid(1000, [12.0] * 3, bad) is None
        assert cgmap._cell_grid(1000, [12.0, bad, 12.0], 2.0) is None
    # capped at max(27, M) cells, never below 3 per dimension, never narrower than r_cut + margin
    for M, L, r in ((10, 1e4, 1.0), (1000, 1e3, 0.5), (50, 30.0, 1.0), (10 ** 6, 100.0, 0.3)):
        g = cgmap._cell_grid(M, [L] * 3, f32(r))
        assert np.prod(g) <= max(27, M) and min(g) >= 3
        assert all(L / n >= r + cgmap._CELL_MARGIN * (L + r) for n in g)
    assert cgmap._nlist_route(max(cgmap.NLIST_CELLS_MIN_M, 1), [6.0] * 3, 2.0) == "all-pairs"


# ------------------------------------------------------------------------------------------------ ArrayTrajectory
def _frames(F=3, N=5):
    rng = np.random.default_rng(0)
    return rng.random((F, N, 3)).astype(np.float32) * 4


def test_array_trajectory_surface(htf):
    P = _frames()
    vel = P * 2
    t = htf.ArrayTrajectory(P, [4, 4, 4, 90, 90, 90], types=["b", "a", "b", "c", "a"], forces=-P, velocities=vel)
    g = t.select_atoms("all")
    assert len(g) == 5 and list(g.atoms.types) == ["b", "a", "b", "c", "a"]
    steps = []
    for ts in t.trajectory:
        np.testing.assert_array_equal(g.positions, P[ts.frame])
        np.testing.assert_array_equal(ts.positions, P[ts.frame])
        np.testing.assert_array_equal(ts.forces, -P[ts.frame])
        np.testing.assert_array_equal(ts.velocities, vel[ts.frame])
        np.testing.assert_array_equal(ts.dimensions, [4, 4, 4, 90, 90, 90])
        steps.append(ts.frame)
    assert steps == [0, 1, 2] and len(t.trajectory) == 3
    dims = np.array([[4, 4, 4, 90, 90, 90], [5, 5, 5, 90, 90, 90], [6, 4, 5, 90, 90, 90]])
    t2 = htf.ArrayTrajectory(P, dims)
    assert [float(ts.dimensions[0]) for ts in t2.trajectory] == [4, 5, 6]
    assert next(iter(t2.trajectory)).forces is None


def test_type_column(htf):
    from hoomd_tf_amd import trajectory
    P = _frames()
    col = trajectory._type_column(htf.ArrayTrajectory(P, [4] * 3 + [90] * 3, types=["b", "a", "b", "c", "a"]).select_atoms("all"))
    np.testing.assert_array_equal(col[:, 0], [1, 0, 1, 2, 0])
    col = trajectory._type_column(htf.ArrayTrajectory(P, [4] * 3 + [90] * 3, types=[7, 3, 3, 9, 7]).select_atoms("all"))
    np.testing.assert_array_equal(col[:, 0], [1, 0, 0, 2, 1])
    col = trajectory._type_column(htf.ArrayTrajectory(P, [4] * 3 + [90] * 3).select_atoms("all"))
    assert col.shape == (5, 1) and not col.any() and col.dtype == np.float32


@pytest.mark.parametrize("kw", [
    dict(positions=np.zeros((3, 5, 2))),
    dict(positions=np.zeros((5, 3))),
    dict(positions=np.zeros((0, 5, 3))),
    dict(positions=np.zeros((3, 5, 3), dtype=bool)),
    dict(dimensions=[4, 4, 4, 90, 90]),
    dict(dimensions=np.zeros((2, 6)) + 4),
    dict(dimensions=[4, 0, 4, 90, 90, 90]),
    dict(dimensions=[4, np.nan, 4, 90, 90, 90]),
    dict(types=["a", "b"]),
    dict(types=[0.5] * 5),
    dict(forces=np.zeros((3, 4, 3))),
    dict(forces=np.zeros((2, 5, 3))),
    dict(velocities=np.zeros((3, 5))),
])
def test_array_trajectory_validation(htf, kw):
    args = dict(positions=_frames(), dimensions=[4, 4, 4, 90, 90, 90])
    args.update(kw)
    with pytest.raises(ValueError):
        htf.ArrayTrajectory(**args)


def test_selection_and_skew_errors(htf):
    t = htf.ArrayTrajectory(_frames(), [4, 4, 4, 90, 90, 90])
    with pytest.raises(ValueError):
        t.select_atoms("name CA")
    with pytest.raises(ValueError):
        next(htf.iter_from_trajectory(4, t, selection="type 1"))
    with pytest.raises(ValueError):
        next(htf.iter_from_trajectory(4, t, period=0))
    skewed = htf.ArrayTrajectory(_frames(), [4, 4, 4, 90, 90, 60])
    with pytest.raises(htf.SkewedBoxError):
        next(htf.iter_from_trajectory(4, skewed))
    # a skewed frame later in the trajectory raises when it is reached, after the first frames were skipped
    dims = np.array([[4, 4, 4, 90, 90, 90]] * 2 + [[4, 4, 4, 80, 90, 90]])
    with pytest.raises(htf.SkewedBoxError):
        next(htf.iter_from_trajectory(4, htf.ArrayTrajectory(_frames(), dims), start=2))
