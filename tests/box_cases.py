"""Fixtures of the general-box tests (tests/test_gpu_general_box.py, tests/test_oracle_c.py): the boxes on which every kernel that
takes an ``htf_box`` leaves its 12-instruction minimum image for HOOMD's BoxDim::minImage with per-axis ``periodic`` flags and
tilt factors -- a domain-decomposed run has periodic = 0 along each decomposed axis, and upstream's skew rule sum(tilt) < 1e-4
lets every box through whose tilt factors sum to zero or less -- and three small systems to evaluate on them.  numpy only: what a
fixture must provide is asserted on the oracle alone (``check_conditions``), so it holds without a GPU."""
import functools

import numpy as np

from helpers import brute_nlist, fcc_lattice
from oracle import htf_oracle as O

ZERO = (0.0, 0.0, 0.0)
NEG_TILT = (-0.4, 0.25, 0.1)     # sum < 0
ZERO_SUM_TILT = (0.3, -0.3, 0.0)  # sum = 0
# (id, periodic, tilt)
FLAG_CASES = [("open-z", (1, 1, 0), ZERO), ("open-x", (0, 1, 1), ZERO), ("open-y", (1, 0, 1), ZERO), ("open-xyz", (0, 0, 0), ZERO)]
TILT_CASES = [("tilt-neg", (1, 1, 1), NEG_TILT), ("tilt-zero-sum", (1, 1, 1), ZERO_SUM_TILT), ("tilt-neg-open-y", (1, 0, 1), NEG_TILT)]
BOX_CASES = FLAG_CASES + TILT_CASES
BOX_IDS = [c[0] for c in BOX_CASES]
DTYPES = [np.float32, np.float64]

# F1: the rows of test_pair_vectors_ragged_row_lengths
F1_LENS = [5, 0, 64, 1, 192, 193, 63, 300, 65, 191, 2, 0, 130, 7, 128, 129, 256, 3, 77, 190, 1, 64, 12]
F1_L = np.array([9.0, 10.0, 11.0])
F1_TABLE = ((128, 4.0), (256, 100.0), (16, 100.0))                       # (NN, r_cut)
F1_BATCHES = ((0, 23), (1, 22), (3, 13), (0, 5), (6, 2))                 # (offset, batch)
F2_RCUT, F2_RLIST, F2_NN = 3.0, 3.4, (128, 32)                           # NN = 32 overflows every row


def case(name):
    return BOX_CASES[BOX_IDS.index(name)]


@functools.lru_cache(maxsize=None)
def f1(hdt):
    """23 ragged rows of random indices (self pairs and repeats included) in a 9 x 10 x 11 box -> pos, types, L, nn, head, nl."""
    rng = np.random.default_rng(21)
    N = len(F1_LENS)
    pos = ((rng.random((N, 3)) - 0.5) * F1_L).astype(hdt)
    types = rng.integers(0, 3, N).astype(np.int32)
    nn = np.array(F1_LENS, dtype=np.int64)
    head = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.int64)
    nl = np.concatenate([rng.integers(0, N, n) for n in F1_LENS]).astype(np.int64)
    return pos, types, F1_L, nn, head, nl


def _all_pairs_nlist(pos, box, r_list, seed):
    """brute_nlist under O.min_image with ``box`` (fully periodic), rows shuffled."""
    p = pos.astype(np.float64)
    d = O.min_image(p[None, :, :] - p[:, None, :], box.astype(np.float64))
    m = (d * d).sum(axis=2) <= r_list * r_list
    np.fill_diagonal(m, False)
    rng = np.random.default_rng(seed)
    rows = [rng.permutation(np.nonzero(m[i])[0]) for i in range(len(p))]
    nn = np.array([len(r) for r in rows], dtype=np.uint32)
    head = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.uint32)
    return nn, head, np.concatenate(rows).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def f2(hdt, tilt=ZERO):
    """256 particles of a jittered fcc (a = 1.6, the system of test_pair_vectors_bit_exact) and their list within 3.4 under the fully
    periodic metric of the box -> pos, types, L, nn, head, nl.  Under a tilt the lattice is sheared into the triclinic cell and the
    list comes from an all-pairs search under O.min_image with that box."""
    pos, L = fcc_lattice(4, 1.6)
    rng = np.random.default_rng(11)
    pos[:, :3] += 0.08 * rng.standard_normal((len(pos), 3))
    types = rng.integers(0, 3, size=len(pos)).astype(np.int32)
    if tuple(tilt) == ZERO:
        pos = pos.astype(hdt)
        nn, head, nl = brute_nlist(pos, L, F2_RLIST, shuffle_seed=11)
    else:
        xy, xz, yz = tilt
        pos[:, 0] += xy * pos[:, 1] + xz * pos[:, 2]
        pos[:, 1] += yz * pos[:, 2]
        pos = pos.astype(hdt)
        nn, head, nl = _all_pairs_nlist(pos, O.make_box(L, tilt=tilt), F2_RLIST, 11)
    return pos, types, L, nn, head, nl


F3_RCUT, F3_RLIST, F3_NN = 1.5, 3.2, 32


@functools.lru_cache(maxsize=None)
def f3(hdt, tilt=ZERO):
    """F3, for bounds that leave no room for the fp32 order of a row sum: 64 dimers, one on every point of a 4 x 4 x 4 grid of
    spacing 3 whose first planes ARE the box faces, so that 37 of them reach through a face.  Each particle has ONE neighbor
    within r_cut 1.5, at distance 0.9 along a direction with no small component (its list holds the other dimers out to 3.2 as
    well): a row's force is a single pair term, so fp32 against fp64 is that term's rounding and nothing cancels.  Under a tilt
    the grid is sheared into the triclinic cell, the dimers keep their length."""
    rng = np.random.default_rng(33)
    L = np.array([12.0, 12.0, 12.0])
    xy, xz, yz = tilt
    S = np.array([[1.0, xy, xz], [0.0, 1.0, yz], [0.0, 0.0, 1.0]])
    ijk = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = (3.0 * ijk - L / 2) @ S.T
    w = np.array([0.5, 0.55, 0.65]) * rng.choice([-1.0, 1.0], (64, 3))
    w = np.stack([rng.permutation(r) for r in w])
    w *= 0.9 / np.linalg.norm(w, axis=1, keepdims=True)
    real = np.concatenate([centres + w / 2, centres - w / 2])
    frac = real @ np.linalg.inv(S).T            # back on the orthorhombic cell: wrap there, shear again
    frac -= np.round(frac / L) * L
    pos = (frac @ S.T).astype(hdt)
    pos = pos[rng.permutation(len(pos))]
    types = rng.integers(0, 3, size=len(pos)).astype(np.int32)
    nn, head, nl = _all_pairs_nlist(pos, O.make_box(L, tilt=tilt), F3_RLIST, 33)
    return pos, types, L, nn, head, nl


def fixture(which, hdt, name):
    """-> (pos, types, L, nn, head, nl), box, periodic for fixture ``which`` ("F1" / "F2" / "F3") on box case ``name``."""
    _, periodic, tilt = case(name)
    sysm = f1(hdt) if which == "F1" else (f2 if which == "F2" else f3)(hdt, tuple(tilt))
    return sysm, O.make_box(sysm[2], tilt=tilt, dtype=hdt), periodic


def kept_counts(sysm, box, periodic, r_cut, offset=0, batch=None):
    """List entries within r_cut per row (self pairs and repeats count): what the max_count side channel reports the largest of."""
    pos, types, L, nn, head, nl = sysm
    big = int(max(1, np.max(nn)))
    t = O.prepare_neighbors(pos, np.ones(len(pos), np.int32), nn, head, nl, box, r_cut, big, offset=offset, batch_size=batch,
                            periodic=periodic)
    return (t[..., 3] != 0).sum(axis=1)


def pair_index(sysm, box, periodic, r_cut, NN, offset=0, batch=None):
    """The slot-aligned index tensor: O.prepare_neighbors with the list entry stored where it stores the pair vector, -1 in the
    slots it leaves zero (entry q of a row in slot q % NN, the last writer wins)."""
    pos, types, L, nn, head, nl = sysm
    N = len(nn)
    B = N - offset if batch is None else batch
    out = np.full((B, NN), -1, dtype=np.int32)
    rc = pos.dtype.type(r_cut)
    for bi, i in enumerate(range(offset, offset + B)):
        k = np.asarray(nl)[int(head[i]): int(head[i]) + int(nn[i])].astype(np.int64)
        if len(k) == 0:
            continue
        dx = O.min_image(pos[k] - pos[i], box, periodic)
        keep = ~(dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1] + dx[:, 2] * dx[:, 2] > rc * rc)
        for q, kk in enumerate(k[keep]):
            out[bi, q % NN] = kk
    return out


def check_conditions(which, hdt, name):
    """What the fixture must provide on this box, on the oracle alone: the reference tensor differs from the plain-box reference
    of the same list in a quarter of F2's (F3's) rows / five of F1's 23, and F2 and F3 hold no contact below 0.65."""
    sysm, box, periodic = fixture(which, hdt, name)
    pos, types, L, nn, head, nl = sysm
    plain = O.make_box(L, dtype=hdt)
    for NN, r_cut in {"F1": F1_TABLE, "F2": [(n, F2_RCUT) for n in F2_NN], "F3": [(F3_NN, F3_RCUT)]}[which]:
        ref = O.prepare_neighbors(pos, types, nn, head, nl, box, r_cut, NN, periodic=periodic)
        ref0 = O.prepare_neighbors(pos, types, nn, head, nl, plain, r_cut, NN)
        rows = int((ref != ref0).any(axis=(1, 2)).sum())
        assert rows >= (5 if which == "F1" else len(pos) // 4), (which, name, NN, rows)
        if which != "F1":
            r = np.sqrt((ref[..., :3].astype(np.float64) ** 2).sum(axis=2))
            assert r[r > 0].min() >= 0.65, (name, NN, float(r[r > 0].min()))
