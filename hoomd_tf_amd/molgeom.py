"""Molecular geometry (utils.py of hoomd-tf): ``mol_bond_distance``, ``mol_angle``, ``mol_dihedral`` and the host-side
``mol_features_multiple``.

The three ops measure bonds, bond angles and dihedrals either per molecule of ``MolSimModel``'s ``[M, MN, 4]``
``mol_positions`` (molecule mode) or over index arrays into a ``[B, 3|4]`` array of beads, e.g. ``center_of_mass``'s
output (CG mode).  They run in the HIP kernels of ``csrc/mol_geom.hip`` (C ABI: include/htf_geom.h), in fp32, and are
differentiable with respect to the positions: the CG backward sums each bead's contributions in a fixed order (no
atomics), so forces are bitwise reproducible.  Models that call them step on the eager path.

Definitions (every vector minimum-imaged in the orthorhombic box ``box[1] - box[0]``):
  bond      d = |p_j - p_i|
  angle     a = p_i - p_j, b = p_k - p_j;  theta = atan2(|a x b|, a . b) in [0, pi]
  dihedral  b1 = p_j - p_i, b2 = p_k - p_j, b3 = p_l - p_k, n1 = b1 x b2, n2 = b2 x b3;
            |phi|, phi = atan2(|b2| b1 . n2, n1 . n2), in [0, pi]
Departures from upstream: the angle is the atan2 form (upstream's ``acos`` loses digits near 0 and pi and gives NaN once
the rounded cosine passes +-1); every term is its own angle or dihedral (upstream's all-atom dihedral normalises by the
norm over all molecules, its CG tensor branches sum over terms or return three numbers per dihedral); a dihedral with
n1 = 0 or n2 = 0 is 0 with a zero gradient (upstream raises 'Vectors are linear', which would need a read-back on every
call).
"""
import numpy as np
import torch

from . import ops
from ._lib import check, lib
from .cgmap import _box_tensor, _cached, _f32_rows
from .simmodel import _trace_log, _unwrap, box_size

_NAMES = {2: "mol_bond_distance", 3: "mol_angle", 4: "mol_dihedral"}


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _grad_f32(grad):
    g = grad if grad.dtype == torch.float32 else grad.to(torch.float32)
    return g, (g.stride(0) if g.dim() == 1 else 0)


class _MolTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, M, MN, slots, L):
        s = list(slots) + [0] * (4 - len(slots))
        out = torch.empty((M,), dtype=torch.float32, device=x.device)
        check(lib.htf_geom_mol_forward(x.data_ptr(), x.stride(0), M, MN, len(slots), *s, L.data_ptr(), out.data_ptr(),
                                       ops._stream(x)))
        ctx.save_for_backward(x, L)
        ctx.geom = (M, MN, len(slots), s)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, L = ctx.saved_tensors
        M, MN, K, s = ctx.geom
        g, gs = _grad_f32(grad)
        gx = torch.empty((M * MN, 3), dtype=torch.float32, device=x.device)   # (every row written by the kernel)
        check(lib.htf_geom_mol_backward(x.data_ptr(), x.stride(0), M, MN, K, *s, L.data_ptr(), g.data_ptr(), gs,
                                        gx.data_ptr(), ops._stream(x)))
        return gx, None, None, None, None


class _CGTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tab, L):
        out = torch.empty((tab["T"],), dtype=torch.float32, device=x.device)
        check(lib.htf_geom_cg_forward(x.data_ptr(), x.stride(0), x.shape[0], tab["K"], tab["T"], tab["table"].data_ptr(),
                                      L.data_ptr(), out.data_ptr(), ops._stream(x)))
        ctx.save_for_backward(x, L)
        ctx.tab = tab
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, L = ctx.saved_tensors
        tab = ctx.tab
        B, K, T = x.shape[0], tab["K"], tab["T"]
        g, gs = _grad_f32(grad)
        contrib = torch.empty((T * K, 3), dtype=torch.float32, device=x.device)
        gx = torch.empty((B, 3), dtype=torch.float32, device=x.device)         # (every row written by the kernel)
        check(lib.htf_geom_cg_backward(x.data_ptr(), x.stride(0), B, K, T, tab["table"].data_ptr(), tab["ptr"].data_ptr(),
                                       tab["rows"].data_ptr(), L.data_ptr(), g.data_ptr(), gs, contrib.data_ptr(),
                                       gx.data_ptr(), ops._stream(x)))
        return gx, None, None


# ---------------------------------------------------------------------------------------------- arguments
def _device_positions(p, name):
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise ValueError("%s must be a CUDA/HIP device tensor (there is no CPU path)" % name)
    if p.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s must be float32 or float64, got %s" % (name, p.dtype))
    return p


def _check_box(box):
    if box is None:
        raise ValueError("box is required (the [3, 3] box of compute(): box[1] - box[0] is used)")
    b = _unwrap(box)
    shape = tuple(b.shape) if isinstance(b, torch.Tensor) else np.shape(b)
    if len(shape) != 2 or shape[0] < 2 or shape[1] != 3:
        raise ValueError("box must be the [3, 3] box of compute(), got shape %s" % (shape,))
    return b if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)


def _box_L(box, device):
    """[Lx, Ly, Lz] on the device: a device box stays there (no read-back)."""
    return _box_tensor(box_size(box), device)


def _check_slots(slots, MN):
    if not all(_is_int(s) for s in slots):
        raise ValueError("type_* must be ints (slots of mol_positions), got %r" % (slots,))
    if any(not 0 <= int(s) < MN for s in slots):
        raise ValueError("type_* must be in [0, %d), got %r" % (MN, tuple(int(s) for s in slots)))
    if len(set(int(s) for s in slots)) != len(slots):
        raise ValueError("type_* must all be different, got %r" % (tuple(int(s) for s in slots),))
    return tuple(int(s) for s in slots)


def _inverted(table, B, xp):
    """The [T, K] table's inverted index: per bead, its contribution rows t*K + s in ascending order (CSR)."""
    flat = table.reshape(-1)
    if xp is np:
        rows = np.argsort(flat, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=B))])
    else:
        rows = torch.argsort(flat, stable=True)
        zero = torch.zeros(1, dtype=torch.int64, device=flat.device)
        ptr = torch.cat([zero, torch.cumsum(torch.bincount(flat, minlength=B), 0)])
    return ptr, rows


def _host_table(beads, B, device, K):
    """Index arrays on the host (ints, lists, numpy, CPU tensors): checked here and uploaded in one copy."""
    cols = []
    for b in beads:
        a = b.numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
        if a.ndim > 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError("b1..b%d must be ints or 1-d integer arrays" % K)
        cols.append(a.reshape(-1).astype(np.int64))
    T = len(cols[0])
    if any(len(c) != T for c in cols):
        raise ValueError("b1..b%d must have one length, got %s" % (K, [len(c) for c in cols]))
    table = np.stack(cols, 1)
    if table.size and (table.min() < 0 or table.max() >= B):
        raise ValueError("bead indices must be in [0, %d)" % B)
    if T * K >= 2 ** 31:
        raise ValueError("too many terms")
    if device is None:
        return None
    ptr, rows = _inverted(table, B, np)
    packed = torch.from_numpy(np.concatenate([table.reshape(-1), ptr, rows]).astype(np.int32)).to(device)
    n = T * K
    return {"K": K, "T": T, "table": packed[:n], "ptr": packed[n:n + B + 1], "rows": packed[n + B + 1:]}


def _device_table(beads, B, device, K):
    """Index tensors on the device: the table and its inverted index, cached while the tensors live (rebuilt when one is
    written in place); the range check runs when they are built."""
    ts = [_unwrap(b) for b in beads]
    for t in ts:
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError("b1..b%d must be 1-d integer tensors" % K)
        if t.device != device:
            raise ValueError("the index tensors must be on %s, got %s" % (device, t.device))
    T = int(ts[0].shape[0])
    if any(int(t.shape[0]) != T for t in ts):
        raise ValueError("b1..b%d must have one length, got %s" % (K, [int(t.shape[0]) for t in ts]))
    if T * K >= 2 ** 31:
        raise ValueError("too many terms")

    def build():
        table = torch.stack([t.to(torch.int64) for t in ts], 1)
        if T and bool(((table < 0) | (table >= B)).any()):      # (the one read-back, when the table is built)
            raise ValueError("bead indices must be in [0, %d)" % B)
        ptr, rows = _inverted(table, B, torch)
        return {"K": K, "T": T, "table": table.to(torch.int32).contiguous(), "ptr": ptr.to(torch.int32).contiguous(),
                "rows": rows.to(torch.int32).contiguous()}

    return _cached("geom", ts, device, build, extra=B)


def _cg_kind(beads, K):
    """'scalar' (all ints), 'device' (all device tensors) or 'host' (all host arrays); anything else is refused."""
    if any(b is None for b in beads):
        raise ValueError("CG=True needs b1..b%d" % K)
    ints = [_is_int(b) for b in beads]
    if all(ints):
        return "scalar"
    if any(ints):
        raise ValueError("b1..b%d must be all ints or all 1-d index arrays (no mixing, no broadcasting)" % K)
    dev = [isinstance(_unwrap(b), torch.Tensor) and _unwrap(b).is_cuda for b in beads]
    if all(dev):
        return "device"
    if any(dev):
        raise ValueError("b1..b%d must be all device tensors or all host arrays" % K)
    return "host"


def _geom(K, mol_positions, slots, CG, cg_positions, beads, box):
    name = _NAMES[K]
    if not CG:
        if mol_positions is None:
            raise ValueError('mol_positions not found. Call build_mol_rep()')
        p = _unwrap(mol_positions)
        if isinstance(p, torch.Tensor) and (p.dim() != 3 or p.shape[2] < 3):
            raise ValueError("mol_positions must be [M, MN, 3] or [M, MN, 4], got %s" % (tuple(p.shape),))
        if isinstance(p, torch.Tensor):
            slots = _check_slots(slots, int(p.shape[1]))
        box = _check_box(box)
        p = _device_positions(p, "mol_positions")
        L = _box_L(box, p.device)
        M, MN = int(p.shape[0]), int(p.shape[1])
        x = _f32_rows(p.reshape(M * MN, p.shape[2])[:, :3])
        _trace_log().append({"op": name})     # (no replay: a model calling it keeps the eager path)
        out = _MolTerms.apply(x, M, MN, slots, L)
    else:
        if cg_positions is None:
            raise ValueError('cg_positions not found.')
        p = _unwrap(cg_positions)
        if isinstance(p, torch.Tensor) and (p.dim() != 2 or p.shape[1] < 3):
            raise ValueError("cg_positions must be [B, 3] or [B, 4], got %s" % (tuple(p.shape),))
        kind = _cg_kind(beads, K)
        box = _check_box(box)
        if kind != "device" and isinstance(p, torch.Tensor) and not p.is_cuda:
            _host_table(beads, int(p.shape[0]), None, K)      # (argument errors before the device check)
        p = _device_positions(p, "cg_positions")
        L = _box_L(box, p.device)
        x = _f32_rows(p[:, :3])
        B = int(x.shape[0])
        tab = _device_table(beads, B, x.device, K) if kind == "device" else _host_table(beads, B, x.device, K)
        _trace_log().append({"op": name})     # (no replay: a model calling it keeps the eager path)
        out = _CGTerms.apply(x, tab, L)
        if kind == "scalar":
            out = out.reshape(())
    return out if p.dtype == torch.float32 else out.to(p.dtype)


# ---------------------------------------------------------------------------------------------- public ops
_MODES = """
    Molecule mode (``CG=False``): ``mol_positions`` is MolSimModel's ``[M, MN, 3|4]`` device tensor and ``type_*`` are
    slots (ints in [0, MN), all different); the result is ``[M]``, one value per molecule.
    CG mode (``CG=True``): ``cg_positions`` is a ``[B, 3|4]`` device tensor (e.g. ``center_of_mass``'s output) and ``b*``
    are all ints (a 0-d result) or all 1-d integer arrays of one length T (a ``[T]`` result).  Device tensors as ``b*``
    are checked once and their tables cached while they live; numpy arrays and lists are checked and uploaded on every
    call, so pass device tensors in a per-step model.
    ``box``: the ``[3, 3]`` box of ``compute()`` (required; only ``box[1] - box[0]`` is used, orthorhombic minimum image).
    Computed in fp32 and returned in the dtype of the positions (float32 or float64); differentiable with respect to the
    positions.  There is no CPU path: a CPU tensor or numpy positions raise ValueError."""


def mol_bond_distance(mol_positions=None, type_i=None, type_j=None, CG=False, cg_positions=None, b1=None, b2=None,
                      box=None):
    """utils.py:866-918: the bond length ``|p_j - p_i|`` (minimum image); 0, with a zero gradient, for a bond of length 0.
    """
    return _geom(2, mol_positions, (type_i, type_j), CG, cg_positions, (b1, b2), box)


def mol_angle(mol_positions=None, type_i=None, type_j=None, type_k=None, CG=False, cg_positions=None, b1=None, b2=None,
              b3=None, box=None):
    """utils.py:789-863: the bond angle at j, ``atan2(|a x b|, a . b)`` in [0, pi] with a = p_i - p_j, b = p_k - p_j
    (upstream's ``acos(a^ . b^)`` without its loss of digits near 0 and pi).  Where ``|a x b| = 0`` the value is what
    atan2 gives (0 or pi) and the gradient is zero.
    """
    return _geom(3, mol_positions, (type_i, type_j, type_k), CG, cg_positions, (b1, b2, b3), box)


def mol_dihedral(mol_positions=None, type_i=None, type_j=None, type_k=None, type_l=None, CG=False, cg_positions=None,
                 b1=None, b2=None, b3=None, b4=None, box=None):
    """utils.py:921-1037: the unsigned dihedral ``|atan2(|b2| b1 . n2, n1 . n2)|`` in [0, pi], b1 = p_j - p_i,
    b2 = p_k - p_j, b3 = p_l - p_k, n1 = b1 x b2, n2 = b2 x b3: upstream's ``acos(n1^ . n2^)`` for every term (upstream
    normalises the all-atom normals by their norm over all molecules, which is a dihedral only for one molecule).
    Where n1 = 0 or n2 = 0 (three points on a line) the value is 0 and the gradient zero; upstream raises
    ``ValueError('Vectors are linear')`` there, which would need a device read-back on every call.
    """
    return _geom(4, mol_positions, (type_i, type_j, type_k, type_l), CG, cg_positions, (b1, b2, b3, b4), box)


for _f in (mol_bond_distance, mol_angle, mol_dihedral):
    _f.__doc__ += _MODES


def mol_features_multiple(bnd_indices=None, ang_indices=None, dih_indices=None, molecules=None, beads=None):
    """utils.py:585-624, on the host: one molecule's bond / angle / dihedral index arrays repeated for ``molecules``
    molecules of ``beads`` beads each (molecule n's indices offset by ``n * beads``), as ``(-1, 2)``, ``(-1, 3)`` and
    ``(-1, 4)`` numpy arrays (empty for an index array that is None)."""
    out = []
    for ind, k in ((bnd_indices, 2), (ang_indices, 3), (dih_indices, 4)):
        reps = [] if ind is None else [np.asarray(ind) + n * beads for n in range(molecules)]
        out.append(np.asarray(reps).reshape((-1, k)))
    return tuple(out)
