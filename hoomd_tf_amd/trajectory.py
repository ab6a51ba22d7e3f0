"""The offline path (utils.iter_from_trajectory of hoomd-tf): ``SimModel.compute`` driven from stored frames, no simulation.

``iter_from_trajectory`` reads a trajectory through the small part of an MDAnalysis ``Universe`` it needs and yields
``[nlist, positions, box]`` per frame, so that ``model(inputs)`` runs as in upstream's examples 05, 08, 09 and 10.
``ArrayTrajectory`` offers the same surface over numpy arrays: arrays and universes go through one code path, and
MDAnalysis is never required.
"""
import numpy as np
import torch

from ._lib import SkewedBoxError
from .cgmap import compute_nlist


class _Timestep:
    """One frame of an ``ArrayTrajectory``: ``frame``, ``dimensions`` [6], ``positions`` [N, 3] and, when the trajectory
    has them, ``forces`` and ``velocities`` [N, 3] (else None)."""

    def __init__(self, frame, dimensions, positions, forces, velocities):
        self.frame = frame
        self.dimensions = dimensions
        self.positions = positions
        self.forces = forces
        self.velocities = velocities


class _Reader:
    def __init__(self, owner):
        self._o = owner

    def __len__(self):
        return self._o.n_frames

    def __iter__(self):
        o = self._o
        for f in range(o.n_frames):
            o._frame = f
            yield _Timestep(f, o._dims[f].copy(), o._pos[f], None if o._forces is None else o._forces[f],
                            None if o._vel is None else o._vel[f])


class _Atoms:
    def __init__(self, owner):
        self._o = owner

    @property
    def types(self):
        if self._o._types is None:
            raise AttributeError("this trajectory has no atom types")
        return self._o._types

    def __len__(self):
        return self._o.n_atoms


class _Group:
    """The selected atoms: ``positions`` of the current frame and ``atoms.types``."""

    def __init__(self, owner):
        self._o = owner
        self.atoms = _Atoms(owner)

    @property
    def positions(self):
        return self._o._pos[self._o._frame]

    def __len__(self):
        return self._o.n_atoms


def _float_array(a, name, shape_tail):
    a = np.asarray(a)
    if a.dtype.kind not in "fiu":
        raise ValueError("%s must hold numbers, got dtype %s" % (name, a.dtype))
    a = a.astype(np.float32)
    if a.ndim != 1 + len(shape_tail) or tuple(a.shape[1:]) != shape_tail:
        raise ValueError("%s must be [F%s], got %s" % (name, "".join(", %d" % s for s in shape_tail), tuple(a.shape)))
    return a


class ArrayTrajectory:
    """A trajectory held in arrays, with the surface of an MDAnalysis ``Universe`` that ``iter_from_trajectory`` reads:
    ``select_atoms('all')`` (its ``.positions`` and ``.atoms.types``) and ``trajectory`` (timesteps with ``.frame``,
    ``.dimensions``, ``.positions``, ``.forces``, ``.velocities``).

    positions: [F, N, 3]; dimensions: [6] (one box for every frame) or [F, 6], lengths then angles in degrees;
    types: [N] atom types (strings or integers; None: every atom is type 0); forces, velocities: [F, N, 3] or None."""

    def __init__(self, positions, dimensions, types=None, forces=None, velocities=None):
        pos = np.asarray(positions)
        if pos.ndim != 3 or pos.shape[2] != 3:
            raise ValueError("positions must be [F, N, 3], got %s" % (tuple(pos.shape),))
        F, N = int(pos.shape[0]), int(pos.shape[1])
        if F < 1 or N < 1:
            raise ValueError("positions must hold at least one frame of one atom, got %s" % (tuple(pos.shape),))
        self._pos = _float_array(pos, "positions", (N, 3))
        dims = np.asarray(dimensions)
        if dims.shape == (6,):
            dims = np.broadcast_to(dims, (F, 6))
        if dims.shape != (F, 6):
            raise ValueError("dimensions must be [6] or [%d, 6], got %s" % (F, tuple(np.shape(dimensions))))
        self._dims = _float_array(dims, "dimensions", (6,))
        if not np.all(np.isfinite(self._dims)) or np.any(self._dims[:, :3] <= 0):
            raise ValueError("dimensions must hold finite, positive box lengths")
        self._forces = None if forces is None else _float_array(forces, "forces", (N, 3))
        self._vel = None if velocities is None else _float_array(velocities, "velocities", (N, 3))
        for a, name in ((self._forces, "forces"), (self._vel, "velocities")):
            if a is not None and a.shape[0] != F:
                raise ValueError("%s must have %d frames, got %d" % (name, F, a.shape[0]))
        if types is not None:
            t = np.asarray(types)
            if t.shape != (N,):
                raise ValueError("types must be [%d], got %s" % (N, tuple(t.shape)))
            if t.dtype.kind not in "iuUSO":
                raise ValueError("types must be strings or integers, got dtype %s" % t.dtype)
            types = t
        self._types = types
        self.n_frames, self.n_atoms = F, N
        self._frame = 0
        self.trajectory = _Reader(self)

    def select_atoms(self, selection):
        if selection != "all":
            raise ValueError("ArrayTrajectory supports only selection='all', got %r" % (selection,))
        return _Group(self)


def _type_column(group):
    """Atom type indices into the sorted unique types, as float32 [N, 1]; 0 for every atom without types (utils.py:703-712)."""
    try:
        types = np.asarray(group.atoms.types)
    except (AttributeError, ValueError):     # (MDAnalysis' NoDataError is both)
        return np.zeros((len(group), 1), np.float32)
    _, inverse = np.unique(types, return_inverse=True)
    return inverse.reshape(-1, 1).astype(np.float32)


def iter_from_trajectory(nneighbor_cutoff, universe, selection='all', r_cut=10., period=1, start=0., end=None):
    """utils.py:627-749: yield ``([nlist, positions, box], ts)`` for the frames of ``universe`` with
    ``start <= ts.frame <= end`` and ``i % period == 0`` (``i`` counts every frame of the trajectory), so that
    ``model(inputs)`` runs a ``SimModel`` on stored frames.

    ``universe``: an MDAnalysis ``Universe`` or an ``ArrayTrajectory`` (only ``select_atoms``, ``.positions``,
    ``.atoms.types`` and ``trajectory`` are read; MDAnalysis is not imported).  Per yielded frame, all new device tensors:
    ``positions`` [N, 4] fp32 (xyz, type index as a float; the type index of an atom is its type's place among the sorted
    unique types, 0 for all when the atoms have none), ``box`` [3, 3] = [[0, 0, 0], [Lx, Ly, Lz], [0, 0, 0]] and
    ``nlist`` = ``compute_nlist(positions, r_cut, nneighbor_cutoff, [Lx, Ly, Lz], sorted=True, return_types=True)``.

    Departures from upstream:
    - the list is built for every frame (upstream builds it once, from frame 0, and yields it with every frame);
    - column 3 of the list is the neighbor's type, as tfcompute gives models (upstream: the neighbor's index);
    - the nearest ``nneighbor_cutoff`` neighbors are kept, nearest first (upstream's default keeps the farthest);
    - ``end=None`` means the last frame (upstream compares frame numbers with the trajectory's total time);
    - a selection other than 'all' reads the selected atoms without rewriting the universe's trajectory;
    - a box whose angles are not all 90 degrees raises ``SkewedBoxError`` (upstream produces tilt factors).
    """
    NN = int(nneighbor_cutoff)
    period = int(period)
    if period < 1:
        raise ValueError("period must be >= 1, got %d" % period)
    group = universe.select_atoms(selection)
    type_col = _type_column(group)
    device = torch.device("cuda")
    for i, ts in enumerate(universe.trajectory):
        if ts.frame < start or (end is not None and ts.frame > end) or i % period != 0:
            continue
        dims = np.asarray(ts.dimensions, dtype=np.float64).reshape(-1)
        if dims.shape[0] != 6:
            raise ValueError("a timestep's dimensions must hold six values, got %d" % dims.shape[0])
        if np.any(dims[3:6] != 90.0):
            raise SkewedBoxError("box is skewed: angles %s (only orthorhombic boxes are supported)" % (dims[3:6].tolist(),))
        L = [float(v) for v in dims[:3].astype(np.float32)]
        xyz = np.asarray(group.positions, dtype=np.float32).reshape(-1, 3)
        positions = torch.from_numpy(np.concatenate([xyz, type_col], axis=1)).to(device)
        box = torch.tensor([[0.0, 0.0, 0.0], L, [0.0, 0.0, 0.0]], dtype=torch.float32, device=device)
        nlist = compute_nlist(positions, r_cut, NN, L, sorted=True, return_types=True)
        yield [nlist, positions, box], ts
