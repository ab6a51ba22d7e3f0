"""Coarse-grained mapping (utils.py of hoomd-tf): ``sparse_mapping``, ``center_of_mass``, ``compute_nlist``.

``sparse_mapping`` builds the B x N bead-from-atom operator once, on the host.  ``center_of_mass`` and
``compute_nlist`` are per-step model ops (examples 02, 07, 09 call them inside ``SimModel.compute``): both run in the
HIP kernels of ``csrc/cg_map.hip`` (C ABI: include/htf_cg.h) and both are differentiable, so a coarse-grained energy
gives atom forces through ``compute_positions_forces``.  Models that call them step on the eager path.  Large neighbor
lists take the cell-binned search of ``csrc/nlist_cells.hip`` (include/htf_nlist.h), which returns the same bits.
"""
import math
import weakref

import numpy as np
import torch

from . import ops, standin
from ._lib import check, lib
from .simmodel import _trace_log, _unwrap

MAX_NN = 256  # include/htf_cg.h HTF_CG_MAX_NN


def sparse_mapping(molecule_mapping, molecule_mapping_index, system=None, device=None):
    """utils.py:1040-1125: the ``B x N`` mapping operator as a coalesced float32 ``torch.sparse_coo_tensor``.

    ``molecule_mapping``: one ``L x M`` matrix per molecule (L beads, M atoms); ``molecule_mapping_index``: the atom
    indices of each molecule (``find_molecules``).  With ``system`` every entry is the atom's mass (``system.vel[:, 3]``)
    over its bead's total mass; without it the matrix entries are kept.  ``device``: where the tensor lives (default:
    the system's device, else the GPU)."""
    if type(molecule_mapping[0]) != np.ndarray:
        raise TypeError('molecule_mapping should be list of numpy arrays')
    if len(molecule_mapping_index) != len(molecule_mapping):
        raise ValueError('Length of molecule_mapping_index and molecule_mapping must match')
    N = sum(len(m) for m in molecule_mapping_index)
    masses = None
    if system is not None:
        masses = system.vel[:system.N, 3].double().cpu().numpy()
    rows, cols, values = [], [], []
    total_i = 0
    for k, (mmi, mm) in enumerate(zip(molecule_mapping_index, molecule_mapping)):
        mm = np.asarray(mm)
        if mm.ndim != 2 or len(mmi) != mm.shape[1]:
            raise ValueError('Mismatch in shapes of molecule_mapping_index and molecule_mapping at index %d. '
                             'shape %d is incompatible with %s' % (k, len(mmi), mm.shape))
        b, a = np.nonzero(mm > 0)          # (row-major: bead by bead, atoms in order, as the reference's loops)
        atoms = np.asarray(mmi, dtype=np.int64)[a]
        if masses is not None:
            v = masses[atoms]
            bead_mass = np.bincount(b, weights=v, minlength=mm.shape[0])
            if np.any(bead_mass[b] == 0):
                raise ValueError('molecule %d has a bead of zero mass' % k)
            v = v / bead_mass[b]
        else:
            v = mm[b, a].astype(np.float64)
        rows.append(b + total_i)
        cols.append(atoms)
        values.append(v)
        total_i += mm.shape[0]
    B = total_i
    if device is None:
        device = system.device if system is not None else torch.device("cuda")
    idx = torch.from_numpy(np.stack([np.concatenate(rows), np.concatenate(cols)]).astype(np.int64))
    val = torch.from_numpy(np.concatenate(values).astype(np.float32))
    return torch.sparse_coo_tensor(idx, val, (B, N), dtype=torch.float32).coalesce().to(device)


# ---------------------------------------------------------------------------------------------- centre of mass
_MAPS = {}   # (tag, id(tensor), ...) -> (weakrefs, device, _versions, extra, arrays): device arrays derived from tensors


def _cached(tag, tensors, device, build, extra=None):
    """``build()``'s arrays for ``tensors`` on ``device``, built on first use and whenever one tensor's ``_version`` (or
    ``extra``) changes; kept while the tensors live.  A hit touches nothing on the device."""
    key = (tag,) + tuple(id(t) for t in tensors)
    versions = tuple(t._version for t in tensors)
    hit = _MAPS.get(key)
    alive = hit is not None and all(r() is t for r, t in zip(hit[0], tensors))
    if alive and hit[1] == device and hit[2] == versions and hit[3] == extra:
        return hit[4]
    arrays = build()
    if not alive:
        for t in tensors:
            weakref.finalize(t, _MAPS.pop, key, None)
    _MAPS[key] = (tuple(weakref.ref(t) for t in tensors), device, versions, extra, arrays)
    return arrays


def _device_maps(mapping, device):
    """The CSR and CSC copies of ``mapping`` on ``device``, built on first use and whenever the tensor's ``_version``
    changes; kept while the mapping tensor lives.  A hit touches nothing on the device."""
    if not isinstance(mapping, torch.Tensor) or mapping.dim() != 2:
        raise ValueError("mapping must be a 2-d torch tensor (sparse_mapping), got %r" % type(mapping))
    return _cached("mapping", (mapping,), device, lambda: _build_maps(mapping, device))


def _build_maps(mapping, device):
    m = mapping if mapping.layout == torch.sparse_coo else mapping.to_sparse()
    m = m.coalesce()
    B, N = int(m.shape[0]), int(m.shape[1])
    idx = m.indices().to(device)
    vals = m.values().to(device=device, dtype=torch.float32).contiguous()
    if idx.shape[1] >= 2 ** 31:
        raise ValueError("mapping has too many entries")
    rows, cols = idx[0], idx[1]      # (coalesced: sorted by row, then column -- CSR order)
    zero = torch.zeros(1, dtype=torch.int64, device=device)
    row_ptr = torch.cat([zero, torch.cumsum(torch.bincount(rows, minlength=B), 0)]).to(torch.int32)
    order = torch.argsort(cols * max(B, 1) + rows)
    col_ptr = torch.cat([zero, torch.cumsum(torch.bincount(cols, minlength=N), 0)]).to(torch.int32)
    return {"B": B, "N": N, "row_ptr": row_ptr.contiguous(), "cols": cols.to(torch.int32).contiguous(), "vals": vals,
            "col_ptr": col_ptr.contiguous(), "rows": rows[order].to(torch.int32).contiguous(),
            "vals_c": vals[order].contiguous()}


_BOXES = {}


def _box_tensor(box_size, device):
    """[Lx, Ly, Lz] as a float32 device tensor (a device tensor stays where it is: no read-back)."""
    if isinstance(box_size, torch.Tensor):
        b = _unwrap(box_size).detach()
        if b.is_cuda:
            return b.reshape(-1)[:3].to(torch.float32).contiguous()
        box_size = b.cpu().numpy()
    vals = tuple(float(v) for v in np.asarray(box_size, dtype=np.float32).reshape(-1)[:3])
    if len(vals) != 3:
        raise ValueError("box_size must hold [Lx, Ly, Lz]")
    k = (device, vals)
    if k not in _BOXES:
        _BOXES[k] = torch.tensor(vals, dtype=torch.float32, device=device)
    return _BOXES[k]


def _box_host(box_size, L):
    """The three fp32 box lengths of ``_box_tensor(box_size)`` (= ``L``) on the host: read back only when the box was given
    as a device tensor."""
    b = _unwrap(box_size)
    if isinstance(b, torch.Tensor) and b.is_cuda:
        return L.cpu().tolist()
    return [float(v) for v in np.asarray(b.cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float32).reshape(-1)[:3]]


def _sorting_enabled():
    sim = standin.current_simulation()
    if sim is None:
        return False
    lists = list(getattr(sim, "nlists", ())) + [getattr(f, "_nlist", None) for f in list(sim.forces) + list(sim.computes)]
    return any(nl is not None and getattr(nl, "sort_particles", False) for nl in lists)


def _positions(positions, name):
    p = _unwrap(positions)
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise ValueError("%s must be a CUDA/HIP device tensor (there is no CPU path)" % name)
    if p.dim() != 2 or p.shape[1] < 3:
        raise ValueError("%s must be [M, 3] or [M, 4], got %s" % (name, tuple(p.shape)))
    return p


def _f32_rows(p):
    """fp32 with unit column stride (rows may keep a stride: a [:, :3] view of an [N, 4] array is not copied)."""
    if p.dtype != torch.float32:
        p = p.to(torch.float32)
    if p.stride(1) != 1 or p.stride(0) < p.shape[1]:
        p = p.contiguous()
    return p


class _CenterOfMass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, maps, L):
        B = maps["B"]
        com = torch.empty((B, 3), dtype=torch.float32, device=x.device)
        xz = torch.empty((B, 6), dtype=torch.float32, device=x.device)
        check(lib.htf_cg_com_forward(x.data_ptr(), x.stride(0), maps["N"], B, maps["row_ptr"].data_ptr(),
                                     maps["cols"].data_ptr(), maps["vals"].data_ptr(), L.data_ptr(), com.data_ptr(),
                                     xz.data_ptr(), ops._stream(x)))
        ctx.save_for_backward(x, xz, L)
        ctx.maps = maps
        return com

    @staticmethod
    def backward(ctx, grad):
        x, xz, L = ctx.saved_tensors
        maps = ctx.maps
        g = grad.to(torch.float32).contiguous()
        gx = torch.empty((maps["N"], 3), dtype=torch.float32, device=x.device)
        check(lib.htf_cg_com_backward(x.data_ptr(), x.stride(0), maps["N"], maps["B"], maps["col_ptr"].data_ptr(),
                                      maps["rows"].data_ptr(), maps["vals_c"].data_ptr(), L.data_ptr(), xz.data_ptr(),
                                      g.data_ptr(), gx.data_ptr(), ops._stream(x)))
        return gx, None, None


def center_of_mass(positions, mapping, box_size):
    """utils.py:11-49: the periodic centre of mass of every bead, ``[B, 3]`` in (-L/2, L/2].

    theta = 2 pi p / L; X = mapping @ cos(theta), Z = mapping @ sin(theta); com = atan2(Z, X) L / (2 pi), per component.
    ``mapping``: ``sparse_mapping``'s ``B x N`` tensor (its device CSR / CSC copies are cached while it lives and rebuilt
    when it is written).  Differentiable with respect to ``positions``.  Raises ValueError while particle sorting is on
    (the mapping refers to fixed atom indices)."""
    if _sorting_enabled():
        raise ValueError('You must disable hoomd sorting to use center_of_mass!')
    p = _positions(positions, "positions")
    x = _f32_rows(p[:, :3])
    maps = _device_maps(mapping, x.device)
    if x.shape[0] != maps["N"]:
        raise ValueError("positions has %d rows but the mapping has %d columns" % (x.shape[0], maps["N"]))
    L = _box_tensor(box_size, x.device)
    _trace_log().append({"op": "center_of_mass"})   # (no replay: a model calling it keeps the eager path)
    com = _CenterOfMass.apply(x, maps, L)
    return com if p.dtype == torch.float32 else com.to(p.dtype)


# ---------------------------------------------------------------------------------------------- neighbor list
# Smallest M that takes the cell route: the smallest size of tools/nlist_probe.py's table at which it beat all-pairs on the
# MI355X (8 192: 0.09 ms against 0.16 ms; at 1 024 it lost, 0.09 ms against 0.02 ms).  DESIGN.md §0.3.
NLIST_CELLS_MIN_M = 8192
# Cell width >= r_cut + 2^-14 (L + r_cut) per dimension: the margin the exactness argument of csrc/nlist_cells.hip needs.
_CELL_MARGIN = 2.0 ** -14


def _cell_grid(M, L, r_cut):
    """(nx, ny, nz) of the cell route for ``M`` particles in the box ``L`` (three fp32 values) at cutoff ``r_cut`` (fp32),
    or None where the route does not apply: a dimension fitting fewer than 3 cells (the 27-cell stencil would wrap onto
    itself), or a cutoff or box that is not finite and positive.  The grid holds at most max(27, M) cells (scratch stays
    O(M)): the largest dimension is halved until it does, which only widens cells."""
    r = float(r_cut)
    if not (math.isfinite(r) and r > 0.0):
        return None
    n = []
    for Lc in (float(v) for v in L):
        if not (math.isfinite(Lc) and Lc > 0.0):
            return None
        w = r + _CELL_MARGIN * (Lc + r)
        k = int(Lc // w)
        while k > 0 and Lc / k < w:
            k -= 1
        if k < 3:
            return None
        n.append(k)
    cap = max(27, int(M))
    while n[0] * n[1] * n[2] > cap:
        a = n.index(max(n))
        n[a] = max(3, n[a] // 2)
    return tuple(n)


def _nlist_route(M, L, r_cut):
    """Which search ``compute_nlist`` runs for ``M`` particles, box ``L`` and cutoff ``r_cut``: ``"cells"`` or ``"all-pairs"``.
    Both return the same bits; the cell route needs M >= NLIST_CELLS_MIN_M and at least 3 cells along every dimension."""
    L32 = [float(v) for v in np.asarray(L, dtype=np.float32).reshape(-1)[:3]]
    if int(M) < NLIST_CELLS_MIN_M or _cell_grid(M, L32, np.float32(r_cut)) is None:
        return "all-pairs"
    return "cells"


class _ComputeNlist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, L, r_cut, NN, sorted_, return_types, excl, grid):
        M = x.shape[0]
        out = torch.empty((M, NN, 4), dtype=torch.float32, device=x.device)
        idx = torch.empty((M, NN), dtype=torch.int32, device=x.device)
        ex = excl.data_ptr() if excl is not None else None
        if grid is None:
            check(lib.htf_cg_nlist_forward(x.data_ptr(), x.stride(0), M, L.data_ptr(), r_cut, NN, int(sorted_), int(return_types),
                                           ex, out.data_ptr(), idx.data_ptr(), ops._stream(x)))
        else:
            nx, ny, nz = grid
            scratch = torch.empty(int(lib.htf_nlist_cells_scratch_words(M, nx * ny * nz)), dtype=torch.int32, device=x.device)
            check(lib.htf_nlist_cells_forward(x.data_ptr(), x.stride(0), M, L.data_ptr(), r_cut, nx, ny, nz, NN, int(sorted_),
                                              int(return_types), ex, scratch.data_ptr(), out.data_ptr(), idx.data_ptr(),
                                              ops._stream(x)))
        ctx.save_for_backward(idx)
        ctx.cols = x.shape[1]
        return out

    @staticmethod
    def backward(ctx, grad):
        (idx,) = ctx.saved_tensors
        M, NN = idx.shape
        g = grad.to(torch.float32).contiguous()
        gx = torch.zeros((M, ctx.cols), dtype=torch.float32, device=idx.device)
        g3 = gx if ctx.cols == 3 else torch.zeros((M, 3), dtype=torch.float32, device=idx.device)
        check(lib.htf_cg_nlist_backward(idx.data_ptr(), M, NN, g.data_ptr(), g3.data_ptr(), ops._stream(idx)))
        if g3 is not gx:
            gx[:, :3] = g3
        return gx, None, None, None, None, None, None, None


def compute_nlist(positions, r_cut, NN, box_size, sorted=False, return_types=False, exclusion_matrix=None):
    """utils.py:75-161: the all-pairs neighbor list ``[M, NN, 4]`` (float32) of ``positions`` ([M, 3] or [M, 4]).

    Pair (i, j): r = minimum image of p_j - p_i (round half to even); kept when 5e-4 <= |r| <= r_cut and the pair is not
    excluded (``exclusion_matrix`` [M, M], True = exclude, applied symmetrically).  ``sorted=True``: the NN nearest,
    nearest first; ``sorted=False``: the reference's top_k of the distances, i.e. the NN farthest in range, farthest first.
    Ties go to the lower index.  Column 3: the neighbor's index, or its type (``positions[:, 3]``) with
    ``return_types=True``.  Empty slots are zeros.  Differentiable with respect to the xyz of ``positions``.
    From NLIST_CELLS_MIN_M particles on, with at least 3 cells of width > r_cut along every dimension, the list is found by
    a cell-binned search (cost ~ M); otherwise all pairs are tested (cost ~ M^2).  Both give the same bits
    (``_nlist_route``).  A box given as a device tensor is then read back once, to choose the grid."""
    p = _positions(positions, "positions")
    if return_types and p.shape[1] == 3:
        raise ValueError('Cannot return type if positions does not have type. Make sure positions is N x 4')
    NN = int(NN)
    if not 1 <= NN <= MAX_NN:
        raise ValueError("NN must be in [1, %d], got %d" % (MAX_NN, NN))
    M = int(p.shape[0])
    if M < 1:
        raise ValueError("compute_nlist needs at least one position")
    x = _f32_rows(p[:, :4] if p.shape[1] >= 4 else p)
    L = _box_tensor(box_size, x.device)
    excl = None
    if exclusion_matrix is not None:
        e = _unwrap(exclusion_matrix)
        e = torch.as_tensor(np.asarray(e) if not isinstance(e, torch.Tensor) else e)
        if tuple(e.shape) != (M, M):
            raise ValueError("exclusion_matrix must be [%d, %d], got %s" % (M, M, tuple(e.shape)))
        excl = (e != 0).to(device=x.device, dtype=torch.uint8).contiguous()
    r32 = float(np.float32(float(r_cut)))
    grid = None
    if M >= NLIST_CELLS_MIN_M:
        grid = _cell_grid(M, _box_host(box_size, L), r32)
    _trace_log().append({"op": "compute_nlist"})    # (no replay: a model calling it keeps the eager path)
    return _ComputeNlist.apply(x, L, r32, NN, bool(sorted), bool(return_types), excl, grid)
