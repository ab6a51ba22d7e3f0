"""What a rebuild of the stand-in neighbor list leaves behind, restated in plain NumPy (float64) from the contracts of
``include/htf_standin.h`` and the comments of ``csrc/standin.hip`` -- every product by itself, so that a test can say which one is
wrong: ``cell_of``, ``cell_start``, ``order``, the tagged sorted copy, the candidate-range table, the reference positions, the
status words and what the scratch holds afterwards.  No GPU and nothing of the library is imported here.

Also the seeded cases the tests run (``tests/test_binning_ref_cpu.py`` asserts, on this file alone, that each holds the edge it
stands for; ``tests/test_gpu_binning.py`` and ``tests/test_gpu_plan_kernels.py`` run the kernels on them), and the references of
the slab-plan kernels (``htfs_slab_classify``, ``htfs_key_sort16``, ``htfs_segment_copy``).

Everything is integer or bit-exact.  Two rules of the builders make that possible:

* No borderline coordinate.  A coordinate is borderline when its float64 scaled value s = (p - lo) / (hi - lo) * n lies within
  8 eps(dtype) n of an integer: the kernel's ((x - lo) * Linv) * n with Linv = 1 / L is five roundings of a value <= n plus the
  cast of lo, an error below 4 eps n (measured over 200 random boxes with every face and both its neighbors planted: 1.33 eps32 n
  at the worst), so away from that band float32, float64 and this file agree on the cell.  ``settle`` moves every borderline
  coordinate to its cell's centre and asserts that none is left: no position is left out of a comparison.
* Coordinates are multiples of 2^-10 (and the box lengths are dyadic).  A difference of two of them, its square and the sum of
  three squares below 4 are then exact in float32 as in float64, with or without a fused multiply-add: a pair is inside r_list in
  one precision exactly when it is in the other, and "the largest true row count" is one number.
"""
import functools

import numpy as np

DEAD = 0xFFFFFFFF              # cell_of of an inert row (x = NaN)
TAG_SIDE = 1 << 31             # the side bit of a sorted position's tag
R_LIST = 1.0
QUANTUM = 1024.0               # coordinates are multiples of 1 / QUANTUM


# ---------------------------------------------------------------------------- the range table's format, in ONE place
RANGE_CODE_SHIFT = 28
RANGE_LEN_MASK = (1 << RANGE_CODE_SHIFT) - 1
IMAGE_NONE, IMAGE_BELOW, IMAGE_ABOVE = 0, 1, 2    # through which periodic image a run is seen


def pack_ranges(start0, len0, code_y, code_z, start1, len1, code_x):
    """Four words per (cell, stencil row): (start, length) of the main x-run with the y and z image codes on the length, (start,
    length) of the run that wraps around the box in x with the x code on its length."""
    out = np.zeros(np.shape(start0) + (4,), dtype=np.uint32)
    out[..., 0] = start0
    out[..., 1] = np.asarray(len0, dtype=np.uint32) | (np.asarray(code_y, dtype=np.uint32) << RANGE_CODE_SHIFT) \
        | (np.asarray(code_z, dtype=np.uint32) << (RANGE_CODE_SHIFT + 2))
    out[..., 2] = start1
    out[..., 3] = np.asarray(len1, dtype=np.uint32) | (np.asarray(code_x, dtype=np.uint32) << RANGE_CODE_SHIFT)
    return out


def unpack_ranges(table):
    """The inverse of ``pack_ranges``: a dict of integer arrays."""
    t = np.asarray(table, dtype=np.uint32).astype(np.int64)
    return dict(start0=t[..., 0], len0=t[..., 1] & RANGE_LEN_MASK, code_y=(t[..., 1] >> RANGE_CODE_SHIFT) & 3,
                code_z=(t[..., 1] >> (RANGE_CODE_SHIFT + 2)) & 3, start1=t[..., 2], len1=t[..., 3] & RANGE_LEN_MASK,
                code_x=(t[..., 3] >> RANGE_CODE_SHIFT) & 3)


# ---------------------------------------------------------------------------- bits of a Scalar4
def int_view(pos):
    """The array read as integers of the scalar's width."""
    return pos.view(np.int32 if pos.dtype == np.float32 else np.int64)


def types_of(pos):
    """The type id in the (low) 32 bits of w."""
    return (int_view(pos)[:, 3].astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def make_pos(xyz, types, dtype):
    """[n, 4] Scalar4 rows: xyz rounded to ``dtype``, the type id's bits in w."""
    pos = np.zeros((len(xyz), 4), dtype=dtype)
    pos[:, :3] = xyz
    int_view(pos)[:, 3] = types
    return pos


# ---------------------------------------------------------------------------- the reference
def reimaged(stored_pos, box_lo, box_hi, periodic, image_L):
    """x, y, z in float64 as they are binned and copied: on a non-periodic axis with image_L > 0 the image nearest the grid's
    centre.  (Exact for the cases here: image_L is a small integer and the result needs no more bits than the stored value.)"""
    p = np.asarray(stored_pos[:, :3], dtype=np.float64).copy()
    for d in range(3):
        if not periodic[d] and image_L[d] > 0:
            centre = 0.5 * (box_lo[d] + box_hi[d])
            p[:, d] -= image_L[d] * np.rint((p[:, d] - centre) / image_L[d])
    return p


def cell_coords(p, box_lo, box_hi, ncell3):
    """c_d = clip(floor((p_d - lo_d) / (hi_d - lo_d) * n_d), 0, n_d - 1) in float64; NaN rows get 0 (the caller masks them)."""
    lo, hi, n = (np.asarray(a, dtype=np.float64) for a in (box_lo, box_hi, ncell3))
    with np.errstate(invalid="ignore"):
        s = np.floor((p - lo) / (hi - lo) * n)
    return np.clip(np.nan_to_num(s, nan=0.0), 0, n - 1).astype(np.int64)


def expected_ranges(cell_start, ncell3, stencil3, periodic):
    """The candidate-range table [ncell * rows, 4] of a grid whose cell starts are ``cell_start``."""
    (nx, ny, nz), (wx, wy, wz), (px, py, pz) = ncell3, stencil3, periodic
    cs = np.asarray(cell_start, dtype=np.int64)
    c = np.arange(nx * ny * nz)
    cx, cy, cz = (c % nx)[:, None], ((c // nx) % ny)[:, None], (c // (nx * ny))[:, None]
    r = np.arange((2 * wy + 1) * (2 * wz + 1))
    dz, dy = (r // (2 * wy + 1) - wz)[None, :], (r % (2 * wy + 1) - wy)[None, :]

    def other_axis(a, n, p):
        code = np.where(a < 0, IMAGE_BELOW, np.where(a >= n, IMAGE_ABOVE, IMAGE_NONE))
        return a % n, code, (code != IMAGE_NONE) & (not p)

    ay, code_y, out_y = other_axis(cy + dy, ny, py)
    az, code_z, out_z = other_axis(cz + dz, nz, pz)
    outside = out_y | out_z
    base = (az * ny + ay) * nx
    a0, a1 = np.maximum(cx - wx, 0), np.minimum(cx + wx, nx - 1)
    start0 = cs[base + a0]
    len0 = cs[base + a1 + 1] - start0
    # the cells that fell off either end of the main run, modulo nx (nx >= 2 wx + 1: never both ends)
    low, high = (cx - wx < 0) & bool(px), (cx + wx >= nx) & bool(px)
    b0 = np.where(low, nx + cx - wx, 0)
    b1 = np.where(low, nx - 1, np.where(high, cx + wx - nx, -1))
    code_x = np.where(low, IMAGE_BELOW, np.where(high, IMAGE_ABOVE, IMAGE_NONE)) + 0 * base
    has = (low | high) + 0 * base > 0
    start1 = np.where(has, cs[base + b0], 0)
    len1 = np.where(has, cs[base + b1 + 1] - start1, 0)
    table = pack_ranges(start0, len0, code_y + 0 * base, code_z + 0 * base, start1, len1, code_x)
    table[outside] = 0
    return table.reshape(-1, 4)


def brute_rows(p, live, box_lo, box_hi, periodic, r_list, n_rows, chunk=256):
    """Brute-force FULL neighbor rows in float64: (counts[n_rows], neighbors of row 0 ascending | of row 1 | ...).  ``p`` are the
    binned coordinates, ``live`` masks the inert rows out.  The rows are taken in chunks of neighbors-in-x, and a chunk is only
    compared with the positions within r_list of its x-extent: 12 000 positions in a second instead of a minute."""
    lo, hi = np.asarray(box_lo, dtype=np.float64), np.asarray(box_hi, dtype=np.float64)
    L = hi - lo
    idx = np.nonzero(live)[0]
    by_x = np.argsort(p[idx, 0], kind="stable")
    idx, q = idx[by_x], p[idx][by_x]
    searched = np.nonzero(idx < n_rows)[0]
    out_i, out_k = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for a in range(0, len(searched), chunk):
        sel = searched[a: a + chunk]
        xs = q[sel, 0]
        mid, half = 0.5 * (xs.min() + xs.max()), 0.5 * (xs.max() - xs.min())
        dx = q[:, 0] - mid
        if periodic[0]:
            dx -= L[0] * np.rint(dx / L[0])
        cand = np.nonzero(np.abs(dx) <= half + r_list + 1e-9)[0]
        d = q[cand][None, :, :] - q[sel][:, None, :]
        for ax in range(3):
            if periodic[ax]:
                d[..., ax] -= L[ax] * np.rint(d[..., ax] / L[ax])
        m = (d * d).sum(-1) <= r_list * r_list
        m &= idx[cand][None, :] != idx[sel][:, None]
        ii, kk = np.nonzero(m)
        out_i.append(idx[sel][ii])
        out_k.append(idx[cand][kk])
    i, k = np.concatenate(out_i), np.concatenate(out_k)
    by_row = np.lexsort((k, i))
    return np.bincount(i, minlength=n_rows)[:n_rows].astype(np.uint32), i[by_row], k[by_row].astype(np.uint32)


class Bins:
    """The products of one rebuild (see ``expected_bins``)."""


def expected_bins(stored_pos, box_lo, box_hi, ncell3, stencil3, periodic, N, type_split, image_L, r_list=None):
    """Every product of a rebuild of ``stored_pos`` ([Ntot, 4], float32 or float64, type bits in w) on the given grid.

    cell_of [Ntot] u32, cell_start [ncell + 1] u32, live, order [live] u32 (what lies behind is not written), sorted_xyz [live, 3]
    in the positions' dtype and sorted_tag [live] (w read as an integer), ranges [ncell * rows, 4] u32, ref_rows (the live rows
    below N, where ref = pos bit for bit), slot_cell [live] (the cell whose span a staging slot lies in); with ``r_list`` also
    n_neigh [N], the pairs (row_i, row_k: every row's neighbors ascending) and max_neigh, from brute force.
    """
    nx, ny, nz = ncell3
    ncell = nx * ny * nz
    Ntot = len(stored_pos)
    b = Bins()
    alive = ~np.isnan(stored_pos[:, 0])
    p = reimaged(stored_pos, box_lo, box_hi, periodic, image_L)
    c = cell_coords(p, box_lo, box_hi, ncell3)
    cell = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    b.cell_of = np.where(alive, cell, DEAD).astype(np.uint32)
    counts = np.bincount(cell[alive], minlength=ncell)
    b.cell_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    b.live = int(alive.sum())
    live_idx = np.nonzero(alive)[0]
    b.order = live_idx[np.argsort(cell[live_idx], kind="stable")].astype(np.uint32)
    b.sorted_xyz = p[b.order].astype(stored_pos.dtype)
    assert np.array_equal(b.sorted_xyz.astype(np.float64), p[b.order]), "a re-imaged coordinate does not fit the dtype"
    side = (type_split >= 0) & (types_of(stored_pos) >= type_split)
    b.sorted_tag = b.order.astype(np.int64) | (side[b.order].astype(np.int64) << 31)
    b.ranges = expected_ranges(b.cell_start, ncell3, stencil3, periodic)
    b.ref_rows = np.nonzero(alive[:N])[0]
    b.slot_cell = np.repeat(np.arange(ncell), counts).astype(np.uint32)
    b.binned_xyz, b.alive, b.Ntot = p, alive, Ntot
    if r_list is not None:
        b.n_neigh, b.row_i, b.row_k = brute_rows(p, alive, box_lo, box_hi, periodic, r_list, N)
        if type_split >= 0:   # pairs whose types lie on different sides of the split are left out
            keep = side[b.row_i] == side[b.row_k]
            b.row_i, b.row_k = b.row_i[keep], b.row_k[keep]
            b.n_neigh = np.bincount(b.row_i, minlength=N)[:N].astype(np.uint32)
        b.max_neigh = int(b.n_neigh.max()) if N else 0
    return b


# ---------------------------------------------------------------------------- builders
def borderline(x, lo, hi, n, dtype):
    """Which coordinates (float64 values of ``dtype`` numbers) lie within 8 eps n of a cell face in scaled units."""
    s = (np.asarray(x, dtype=np.float64) - lo) / (hi - lo) * n
    with np.errstate(invalid="ignore"):
        return np.abs(s - np.rint(s)) <= 8.0 * np.finfo(dtype).eps * n


def settle(xyz, box_lo, box_hi, ncell3):
    """Move every coordinate that is borderline in float32 (hence in float64 too) to its cell's centre; assert none is left."""
    xyz = np.array(xyz, dtype=np.float64)
    c = cell_coords(xyz, box_lo, box_hi, ncell3)
    for d in range(3):
        w = (box_hi[d] - box_lo[d]) / ncell3[d]
        bad = borderline(xyz[:, d], box_lo[d], box_hi[d], ncell3[d], np.float32)
        xyz[bad, d] = box_lo[d] + (c[bad, d] + 0.5) * w
        for dtype in (np.float32, np.float64):
            assert not borderline(xyz[:, d].astype(dtype), box_lo[d], box_hi[d], ncell3[d], dtype).any()
    return xyz


def quantize(x):
    return np.round(np.asarray(x, dtype=np.float64) * QUANTUM) / QUANTUM


# (cells, stencil, box lengths) -- what each grid reaches is said in tests/test_gpu_binning.py
GRIDS = {
    "3x3x3": ((3, 3, 3), (1, 1, 1), (3.0, 3.0, 3.0)),
    "5x5x5": ((5, 5, 5), (2, 2, 2), (2.5, 2.5, 2.5)),
    "5x3x1": ((5, 3, 1), (2, 1, 0), (2.5, 3.0, 2.5)),
    "16x16x8": ((16, 16, 8), (2, 2, 2), (8.0, 8.0, 4.0)),
    "17x11x11": ((17, 11, 11), (2, 2, 2), (8.5, 5.5, 5.5)),
    "13x13x12": ((13, 13, 12), (2, 2, 2), (6.5, 6.5, 6.0)),
    "21x14x14": ((21, 14, 14), (2, 2, 2), (10.5, 7.0, 7.0)),
}
# (grid, periodic, image_L)
CONFIGS = {
    "3x3x3-ppp": ("3x3x3", (1, 1, 1), (0.0, 0.0, 0.0)),
    "3x3x3-nnn": ("3x3x3", (0, 0, 0), (0.0, 0.0, 0.0)),
    "5x5x5-ppp": ("5x5x5", (1, 1, 1), (0.0, 0.0, 0.0)),
    "5x3x1-ppp": ("5x3x1", (1, 1, 1), (0.0, 0.0, 0.0)),
    "5x3x1-pnp": ("5x3x1", (1, 0, 1), (0.0, 0.0, 0.0)),
    "16x16x8-ppp": ("16x16x8", (1, 1, 1), (0.0, 0.0, 0.0)),
    "17x11x11-ppp": ("17x11x11", (1, 1, 1), (0.0, 0.0, 0.0)),
    "17x11x11-nnn": ("17x11x11", (0, 0, 0), (0.0, 0.0, 0.0)),
    "13x13x12-ppp": ("13x13x12", (1, 1, 1), (0.0, 0.0, 0.0)),
    "21x14x14-ppp": ("21x14x14", (1, 1, 1), (0.0, 0.0, 0.0)),
    "16x16x8-image": ("16x16x8", (0, 1, 1), (32.0, 0.0, 0.0)),
}
POPULATIONS = ("uniform", "crowded", "ghosts", "typed")
CROWD = 200   # members of the crowded cell, at least


class Case:
    """One seeded configuration: grid, box, float64 coordinates (multiples of 2^-10, none borderline), types, N <= Ntot."""

    def pos(self, dtype):
        return make_pos(self.xyz, self.types, dtype)

    @functools.lru_cache(maxsize=None)
    def expected(self, dtype):
        """The products, computed once per case: the stored numbers are the same in either dtype (``build_case`` asserts it, and
        tests/test_binning_ref_cpu.py that ``expected_bins`` gives the same from float32 input), so only the sorted copy's dtype
        differs."""
        if dtype != np.float64:
            b64, b = self.expected(np.float64), Bins()
            b.__dict__.update(b64.__dict__)
            b.sorted_xyz = b64.sorted_xyz.astype(dtype)
            return b
        return expected_bins(self.pos(dtype), self.lo, self.hi, self.ncell3, self.stencil3, self.periodic, self.N,
                             self.type_split, self.image_L, r_list=R_LIST)


def _seed(*names):
    return [sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) for name in names]


@functools.lru_cache(maxsize=None)
def build_case(config, population):
    grid, periodic, image_L = CONFIGS[config]
    ncell3, stencil3, Lbox = GRIDS[grid]
    rng = np.random.default_rng(_seed(config, population))
    k = Case()
    k.config, k.population = config, population
    k.ncell3, k.stencil3, k.periodic, k.image_L = ncell3, stencil3, periodic, image_L
    k.hi = tuple(0.5 * v for v in Lbox)
    k.lo = tuple(-v for v in k.hi)
    k.ncell = ncell = ncell3[0] * ncell3[1] * ncell3[2]
    lo, hi = np.array(k.lo), np.array(k.hi)
    width = (hi - lo) / np.array(ncell3)
    k.type_split = -1

    def scatter(n):
        return settle(quantize(rng.uniform(lo, hi, (n, 3))), k.lo, k.hi, ncell3)

    def cells(x):
        c = cell_coords(x, k.lo, k.hi, ncell3)
        return (c[:, 2] * ncell3[1] + c[:, 1]) * ncell3[0] + c[:, 0]

    if population == "crowded":
        # >= CROWD members in the LAST cell, none in the first, and the indices descending in cell order: the order in which the
        # scatter's atomics arrive is then the reverse of the order the contract asks for
        x = scatter(2 * ncell)
        x = x[cells(x) != 0]
        corner = hi - width
        crowd = settle(quantize(rng.uniform(corner + 0.01 * width, hi - 0.01 * width, (CROWD + 7, 3))), k.lo, k.hi, ncell3)
        x = np.concatenate([crowd, x])
        x = x[np.argsort(-cells(x), kind="stable")]
    else:
        x = scatter(3 * ncell)
    k.Ntot = Ntot = len(x)
    k.N = Ntot
    k.types = np.zeros(Ntot, dtype=np.int32)
    if population == "ghosts":
        # Ntot ~ 1.3 N: ghosts behind the local rows, inert rows (x = NaN) among both, at either end of each and a few inside
        k.N = int(round(Ntot / 1.3))
        inert = np.concatenate([[0, k.N - 1, Ntot - 1], rng.choice(Ntot, max(1, Ntot // 40), replace=False)])
        x[inert, 0] = np.nan
    if population == "typed":
        k.types = rng.integers(0, 4, Ntot).astype(np.int32)
        k.type_split = 1
    if any(image_L):
        # a tenth of the rows a whole period away along the re-imaged axis, either way
        d = int(np.nonzero(image_L)[0][0])
        far = rng.choice(Ntot, Ntot // 10, replace=False)
        far = far[~np.isnan(x[far, 0])]
        x[far, d] += image_L[d] * rng.choice([-1.0, 1.0], len(far))
    k.xyz = x
    for dtype in (np.float32, np.float64):   # the stored numbers ARE the float64 ones in either dtype
        assert np.array_equal(x.astype(dtype).astype(np.float64), x, equal_nan=True)
    return k


def planted_case(dtype):
    """Coordinates on and next to the faces of the power-of-two box lo = (-4, -4, -2), L = (8, 8, 4), n = (16, 16, 8), where
    (x - lo) / L * n is exact in either precision: (positions [n, 4], the cell each must land in -- written out here, by hand,
    not computed by ``expected_bins`` --, box_lo, box_hi, ncell3)."""
    lo, hi, n3 = (-4.0, -4.0, -2.0), (4.0, 4.0, 2.0), (16, 16, 8)
    rows, want = [], []
    one = dtype(1.0)
    for d in range(3):
        n, w = n3[d], 0.5
        plant = []   # (coordinate, cell along d)
        for f in range(n + 1):   # every face: the cell above it, hi itself clamped into the last cell
            face = dtype(lo[d] + f * w)
            plant.append((face, min(f, n - 1)))
            # one ulp above a face: the same cell whichever way x - lo rounds
            plant.append((np.nextafter(face, dtype(np.inf)), min(f, n - 1)))
        plant.append((np.nextafter(dtype(hi[d]), -one * 100), n - 1))     # one ulp below hi
        plant += [(dtype(lo[d] - 0.25), 0), (dtype(lo[d] - 100.0), 0), (np.nextafter(dtype(lo[d]), -one * 100), 0)]   # below lo
        plant += [(dtype(hi[d] + 0.25), n - 1), (dtype(hi[d] + 100.0), n - 1)]                                       # above hi
        for j, (v, cd) in enumerate(plant):
            c = [(3 * j + 1) % n3[0], (5 * j + 2) % n3[1], (7 * j + 3) % n3[2]]   # the other two axes: some cell's centre
            x = [lo[a] + (c[a] + 0.5) * 0.5 for a in range(3)]
            x[d], c[d] = v, cd
            rows.append(x)
            want.append((c[2] * n3[1] + c[1]) * n3[0] + c[0])
    for j in range(3):   # NaN in x: an inert row, whatever y and z say
        rows.append([np.nan, lo[1] + 0.25 + j, 0.25])
        want.append(DEAD)
    return make_pos(np.array(rows), np.zeros(len(rows), np.int32), dtype), np.array(want, dtype=np.uint32), lo, hi, n3


# ---------------------------------------------------------------------------- htfs_cell_sort on synthetic cell indices
SORT_NCELL = (1, 7, 8, 9, 2047, 2048, 2049, 4095, 4097, 6151)
SORT_NTOT = (0, 1, 255, 256, 257, 3000)
SORT_PATTERNS = ("uniform", "last", "descending", "dead")


def sort_case(ncell, Ntot, pattern):
    """cell_of [Ntot] u32, or None where the pattern does not apply (everything in one cell: one thread sorts a cell)."""
    rng = np.random.default_rng([ncell, Ntot, SORT_PATTERNS.index(pattern)])
    if pattern == "last":
        if Ntot > 300:
            return None
        return np.full(Ntot, ncell - 1, dtype=np.uint32)
    c = rng.integers(0, ncell, Ntot).astype(np.uint32)
    if pattern == "descending":   # the cell index falls as the particle index rises
        c = np.sort(c)[::-1].copy()
    if pattern == "dead":         # one entry in ten in no cell, the first and the last among them
        c[rng.random(Ntot) < 0.1] = DEAD
        c[:1] = DEAD
        c[-1:] = DEAD
    return c


def expected_sort(cell_of, ncell):
    """(cell_start [ncell + 1], order [live]) of a stable counting sort that leaves the dead entries out."""
    live = np.nonzero(cell_of != DEAD)[0]
    counts = np.bincount(cell_of[live].astype(np.int64), minlength=ncell)
    order = live[np.argsort(cell_of[live], kind="stable")]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32), order.astype(np.uint32)


# ---------------------------------------------------------------------------- the slab plan: htfs_slab_classify
SLAB_BOUNDS = {   # dyadic, unequal; every bound and bound +- r_ghost is a float32 number
    2: (-8.0, 2.5, 8.0),
    3: (-8.0, -3.0, 2.5, 8.0),
    4: (-8.0, -3.0, 0.0, 2.5, 8.0),
    5: (-8.0, -5.0, -1.5, 0.0, 4.25, 8.0),
}
SLAB_R_GHOST = (0.75, 3.0)   # the second is wider than half the narrowest slab of every world: class 2 (near both faces)
SLAB_N = (1, 257, 3000)


def slab_positions(world, r_ghost, N, dtype):
    """x of N particles (float64 values of ``dtype`` numbers): on every bound and one ulp either side, on bound +- r_ghost and one
    ulp either side, outside [-8, 8), the rest uniform over [-9, 9)."""
    rng = np.random.default_rng([world, int(r_ghost * 4), N])
    bounds = SLAB_BOUNDS[world]
    x = rng.uniform(-9.0, 9.0, N).astype(dtype)
    at = [bd + s for bd in bounds for s in (0.0, r_ghost, -r_ghost)]
    big = dtype(1000.0)
    plant = [f(dtype(v)) for v in at for f in (lambda v: v, lambda v: np.nextafter(v, big), lambda v: np.nextafter(v, -big))]
    plant += [dtype(-8.5), dtype(8.0), dtype(8.5), dtype(-1000.0), dtype(1000.0)]
    plant = np.array(plant, dtype=dtype)
    m = min(N, len(plant))
    where = rng.choice(N, m, replace=False)
    # (N = 1: one planted value; a different one per world and r_ghost)
    x[where] = np.roll(plant, -(world + int(r_ghost * 4)))[:m] if N < len(plant) else plant
    return x.astype(np.float64)


def expected_slab_keys(x, bounds, rank, r_ghost):
    """key = destination * 4 + class, by the header's rules in float64 (exact: every threshold is a float32 number)."""
    bounds = np.asarray(bounds, dtype=np.float64)
    world = len(bounds) - 1
    owner = (bounds[None, 1:-1] <= x[:, None]).sum(axis=1)
    left, right = (rank + world - 1) % world, (rank + 1) % world
    if world == 2:   # both faces lead to the one peer: everything that leaves travels as "right"
        dest = np.where(owner != rank, 2, 0)
    else:
        dest = np.where(owner == rank, 0, np.where(owner == left, 1, np.where(owner == right, 2, 3)))
    near_l, near_r = x < bounds[owner] + r_ghost, x >= bounds[owner + 1] - r_ghost
    cls = np.where(near_l, np.where(near_r, 2, 1), np.where(near_r, 3, 0))
    return (dest * 4 + cls).astype(np.uint32)


def admitted_keys(world):
    """The (destination, class) keys a world can produce: two slabs know "stay" and "right" only, three have no "beyond"."""
    dests = {2: (0, 2), 3: (0, 1, 2)}.get(world, (0, 1, 2, 3))
    return {d * 4 + c for d in dests for c in range(4)}


# ---------------------------------------------------------------------------- htfs_key_sort16
KEY_N = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
KEY_PATTERNS = ("uniform", "zeros", "fifteens", "alternating", "sorted", "reversed")


def key_case(N, pattern):
    rng = np.random.default_rng([N, KEY_PATTERNS.index(pattern)])
    key = rng.integers(0, 16, N)
    if pattern == "zeros":
        key[:] = 0
    elif pattern == "fifteens":
        key[:] = 15
    elif pattern == "alternating":
        key = np.where(np.arange(N) % 2 == 0, 0, 15)
    elif pattern == "sorted":
        key = np.sort(key)
    elif pattern == "reversed":
        key = np.sort(key)[::-1]
    return np.ascontiguousarray(key, dtype=np.uint32)


def expected_key_sort(key):
    """(the 17 starts, the stable argsort)."""
    start = np.concatenate([[0], np.cumsum(np.bincount(key.astype(np.int64), minlength=16))])
    return start.astype(np.uint32), np.argsort(key, kind="stable").astype(np.uint32)


# ---------------------------------------------------------------------------- htfs_segment_copy
SEGMENT_TABLES = {   # counts per segment
    "one": (5,),
    "three-first-empty": (0, 4, 3),
    "three-middle-empty": (6, 0, 2),
    "three-last-empty": (3, 5, 0),
    "sixteen": (0, 3, 1, 0, 0, 7, 2, 0, 5, 1, 1, 0, 9, 4, 6, 0),
    "all-empty": (0, 0, 0),
    "sixteen-all-empty": (0,) * 16,
}
SEGMENT_ROW_BYTES = (4, 12, 16, 32)


def segment_case(counts, n_src=None, seed=0):
    """(src_start, dst_start, count, source rows, destination rows): the segments lie in shuffled order in the source, with a gap
    of one row between them on either side, so that a row copied from or to the wrong place shows."""
    rng = np.random.default_rng([seed, len(counts), sum(counts)])
    counts = np.asarray(counts, dtype=np.uint32)
    n = len(counts)

    def lay(order):
        start, at = np.zeros(n, dtype=np.uint32), 1
        for s in order:
            start[s] = at
            at += int(counts[s]) + 1
        return start, at

    src_start, rows_src = lay(rng.permutation(n))
    dst_start, rows_dst = lay(np.arange(n))
    return src_start, dst_start, counts, rows_src, rows_dst


def expected_segment_copy(dst, src, src_start, dst_start, counts):
    """dst[dst_start[s] + j] = src[src_start[s] + j], j < count[s]; every other row of ``dst`` as it was."""
    out = dst.copy()
    for s in range(len(counts)):
        out[dst_start[s]: dst_start[s] + counts[s]] = src[src_start[s]: src_start[s] + counts[s]]
    return out
