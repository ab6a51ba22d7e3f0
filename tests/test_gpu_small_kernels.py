"""The observable and bookkeeping kernels at their edge shapes: each HIP kernel against ``oracle/htf_oracle.py`` or a few
lines of float64 NumPy, at the sizes where a lane group, a grid-stride loop, a block tail, a dtype dispatch or a clipping
rule changes path.  Every input comes from a seeded ``numpy.random.default_rng``.

The builders below (``*_case`` / ``*_rows``) are plain NumPy and assert, on the reference side, that the edge a test
relies on is really in its data (both end bins filled, a tie pair in different lanes, ...): they run without a GPU.

Derived bounds (eps = machine epsilon of the dtype under test):
  * wrap_vector        4 eps max|r|: one rounding each for the quotient's effect, the product and the difference.
  * energy_sum         N 2^-53 sum|e|: the kernel accumulates in double.
  * reduce_partials    one fp32 ulp of float32(fsum(partials) * float64(float32(scale))).
  * bias_combine       2 eps (|f| + |alpha b|): one rounding for the product and one for the sum, fused or not.
  * rdf_finalize       against the exact volume of the fp32 shell edges: half an ulp for each cube, one rounding each for
                       the difference and the quotient (``_finalize_case``); against the oracle rtol = 1e-4 as test_rdf.
Everything else is compared bit for bit, or at the tolerance the kernel's existing test already uses.
"""
import math

import numpy as np
import pytest
import torch

from oracle import htf_oracle as O

pytestmark = pytest.mark.gpu

TDT = {"float32": torch.float32, "float64": torch.float64}
NDT = {"float32": np.float32, "float64": np.float64}
DTYPES = ["float32", "float64"]
BLOCK_NS = [1, 255, 256, 257, 1000]


def _eps(dtype):
    return float(np.finfo(NDT[dtype]).eps)


def _dev(a, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(cuda)


# ------------------------------------------------------------------------------------------------
# 1. histogram and RDF
# ------------------------------------------------------------------------------------------------
RDF_SHAPES = [(1, 1), (5, 3), (64, 7), (300, 33)]
RDF_RANGES = [(0.0, 3.5), (1.0, 2.5)]
PLANTED_R = (1.7, 0.0, 0.5, 3.8)      # inside both ranges, a padded slot, below 1.0, above 3.5 and 2.5


def rdf_case(B, NN, seed=0):
    """[B, NN, 4] float64 pair vectors (not fp32-representable: the fp64 kernel has to round them): radii uniform over
    [0.2, 4.0], one slot in eight padded (all zero), column 3 the neighbor's type 0..2.  The first slots are planted."""
    rng = np.random.default_rng(1000 * B + NN + seed)
    n = B * NN
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = rng.uniform(0.2, 4.0, n)
    rad[rng.random(n) < 0.125] = 0.0
    rad[:min(n, 4)] = PLANTED_R[:min(n, 4)]
    nl = np.zeros((n, 4))
    nl[:, :3] = u * rad[:, None]
    nl[:, 3] = np.where(rad > 0, rng.integers(0, 3, n), 0)
    return nl.reshape(B, NN, 4)


def norm32(nl32):
    """tf.norm as the histogram takes it: float32 products and sums, every one rounded on its own."""
    assert nl32.dtype == np.float32
    sq = nl32[..., :3] * nl32[..., :3]
    return np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2])


def hist_ref(nl, r_range, nb, types=None, type_i=None, type_j=None):
    """O.histogram_fixed_width over O.masked_nlist on the float32 cast of the tensor."""
    nl32 = nl.astype(np.float32)
    if type_i is not None or type_j is not None:
        nl32 = O.masked_nlist(nl32, types, type_i, type_j)
    return O.histogram_fixed_width(norm32(nl32), np.asarray(r_range, np.float32), nb)


def untyped_case(B, NN, nb, r_range):
    nl = rdf_case(B, NN)
    ref = hist_ref(nl, r_range, nb)
    assert ref.sum() == B * NN
    r = norm32(nl.astype(np.float32))
    if B * NN >= 15:      # (one slot cannot hold all of them)
        assert ref[0] > 0 and ref[-1] > 0 and np.count_nonzero(ref[1:-1]) >= 1
        assert (r == 0).any() and (r > r_range[1]).any() and (r_range[0] == 0 or ((r > 0) & (r < r_range[0])).any())
    if B * NN >= 400:
        assert np.count_nonzero(ref[1:-1]) >= min(10, nb - 2)
    return nl, ref


def row_types(pattern, B, seed=5):
    rng = np.random.default_rng(seed + B)
    if pattern == "random":
        return rng.integers(0, 3, B).astype(np.float32)
    if pattern == "runs":      # each type holds one run of B / 3 >= 64 consecutive rows: whole waves (and blocks) skip
        assert B // 3 >= 64
        return np.repeat(np.arange(3), -(-B // 3))[:B].astype(np.float32)
    if pattern == "no2":       # type 2 never occurs
        return rng.integers(0, 2, B).astype(np.float32)
    raise ValueError(pattern)


def typed_case(pattern, B, NN, r_range, type_i, type_j, nb=102):
    nl, types = rdf_case(B, NN, seed=3), row_types(pattern, B)
    ref = hist_ref(nl, r_range, nb, types, type_i, type_j)
    kept = B if type_i is None else int((types == type_i).sum())
    assert ref.sum() == kept * NN
    if pattern == "no2" and type_i == 2:
        assert kept == 0 and ref.sum() == 0
    elif B >= 64:
        assert type_i is None or 0 < kept < B
        if type_j is not None:    # slots of another type moved into bin 0 (0 - r0 clips there too)
            only_i = hist_ref(nl, r_range, nb, types, type_i, None)
            assert ref[0] > only_i[0] and ref[1:].sum() < only_i[1:].sum() and ref[1:-1].sum() > 0
    return nl, types, ref


def edge_case(nb):
    """Radii that ARE bin edges of range (0, 4): coordinates are multiples of 1/32 (3-4-5 triples and axis vectors), so every
    product, sum, root and quotient below is exact.  With 128 bins in all the edges are the multiples of 1/32 and each
    radius belongs to the bin it opens; with 128 + 2 bins the edges 0, 2 and 4 are exact."""
    k = np.arange(0, 131)
    rows = [np.stack([k / 32.0, 0 * k, 0 * k], 1), np.stack([0 * k, 0 * k, -k / 32.0], 1)]
    m = np.arange(1, 26)
    rows.append(np.stack([3 * m / 32.0, -4 * m / 32.0, 0 * m], 1))     # radius 5 m / 32
    xyz = np.concatenate(rows)
    nl = np.zeros((len(xyz), 1, 4))
    nl[:, 0, :3] = xyz
    r = norm32(nl.astype(np.float32))[:, 0].astype(np.float64)
    assert np.array_equal(r * 32, np.round(r * 32)) and r.max() > 4.0
    by_hand = np.bincount(np.minimum((r * nb).astype(np.int64) // 4, nb - 1), minlength=nb)   # integer arithmetic
    ref = hist_ref(nl, (0.0, 4.0), nb)
    np.testing.assert_array_equal(ref, by_hand)
    on_edge = (r * nb / 4 == np.floor(r * nb / 4)) & (r < 4.0)
    assert on_edge.sum() >= (250 if nb == 128 else 4)
    return nl, ref


def _histogram(nl_t, r_range, nb, types_t=None, type_i=None, type_j=None):
    from hoomd_tf_amd import ops
    from hoomd_tf_amd._lib import lib, check
    hist = torch.zeros(nb, dtype=torch.int32, device=nl_t.device)
    stride = 0 if types_t is None else types_t.stride(0)
    check(lib.htf_rdf_histogram(nl_t.data_ptr(), ops._dt(nl_t), nl_t.shape[0], nl_t.shape[1], r_range[0], r_range[1], nb,
                                types_t.data_ptr() if types_t is not None else None, stride,
                                -1 if type_i is None else type_i, -1 if type_j is None else type_j, hist.data_ptr(),
                                ops._stream(nl_t)))
    return hist


def _types_tensor(types, layout, cuda):
    if layout == "vector":
        return _dev(types, cuda)
    pos = np.full((len(types), 4), 7.0, np.float32)      # column 3 of a positions tensor: stride 4
    pos[:, 3] = types
    t = _dev(pos, cuda)[:, 3]
    assert t.stride(0) == 4
    return t


@pytest.mark.parametrize("r_range", RDF_RANGES, ids=["from0", "from1"])
@pytest.mark.parametrize("nb", [3, 102, 2048])
@pytest.mark.parametrize("B,NN", RDF_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_histogram_untyped(htf, cuda, dtype, B, NN, nb, r_range):
    nl, ref = untyped_case(B, NN, nb, r_range)
    got = _histogram(_dev(nl, cuda, TDT[dtype]), r_range, nb)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


TYPED_FORMS = [(1, None), (None, 2), (0, 1)]


@pytest.mark.parametrize("layout", ["vector", "column3"])
@pytest.mark.parametrize("type_i,type_j", TYPED_FORMS, ids=["i", "j", "ij"])
@pytest.mark.parametrize("r_range", RDF_RANGES, ids=["from0", "from1"])
@pytest.mark.parametrize("pattern,B,NN", [("random", 5, 3), ("random", 300, 33), ("runs", 300, 33)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_histogram_typed(htf, cuda, dtype, pattern, B, NN, r_range, type_i, type_j, layout):
    nl, types, ref = typed_case(pattern, B, NN, r_range, type_i, type_j)
    got = _histogram(_dev(nl, cuda, TDT[dtype]), r_range, 102, _types_tensor(types, layout, cuda), type_i, type_j)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


@pytest.mark.parametrize("type_j", [None, 0])
@pytest.mark.parametrize("dtype", DTYPES)
def test_histogram_type_i_matches_no_row(htf, cuda, dtype, type_j):
    nl, types, ref = typed_case("no2", 300, 33, (0.0, 3.5), 2, type_j)
    got = _histogram(_dev(nl, cuda, TDT[dtype]), (0.0, 3.5), 102, _types_tensor(types, "vector", cuda), 2, type_j)
    assert ref.sum() == 0 and int(got.sum()) == 0


@pytest.mark.parametrize("nb", [128, 130])
@pytest.mark.parametrize("dtype", DTYPES)
def test_histogram_radii_on_bin_edges(htf, cuda, dtype, nb):
    nl, ref = edge_case(nb)
    got = _histogram(_dev(nl, cuda, TDT[dtype]), (0.0, 4.0), nb)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)


FINALIZE_CASES = [(nbins, rr) for rr in RDF_RANGES for nbins in (1, 3, 100, 257, 2046)]


def _finalize_case(nbins, r_range):
    """Random counts, the oracle's shells (O.compute_rdf's own lines) and the exact volumes of those fp32 shell edges.

    One ulp of a cube moves a shell volume by ulp(r^3) / (3 r^2 dr) <= eps r / (3 dr): 8.1e-5 for the last of 2046 bins
    of (0, 3.5), 1.35e-4 for the last of 2046 bins of (1.0, 2.5).  NumPy's float32 power is not correctly rounded, so in
    that second case the oracle's own two cubes decide a comparison at rtol = 1e-4, not the kernel: it is compared with
    the exact volumes only (``exact`` and ``bound``, which hold for every case).  The kernel rounds each cube once."""
    rng = np.random.default_rng(nbins)
    hist = rng.integers(0, 5000, nbins + 2).astype(np.int32)
    rr = np.asarray(r_range, dtype=np.float32)
    shell = np.linspace(rr[0], rr[1], nbins + 1).astype(np.float32)
    rs = (shell[1:] + shell[:-1]) * np.float32(0.5)
    vols = shell[1:] ** 3 - shell[:-1] ** 3
    rdf = hist[1:-1].astype(np.float32) / vols
    assert shell[-1] == rr[1] and shell[0] == rr[0] and np.all(vols > 0) and np.count_nonzero(hist[1:-1]) >= min(nbins, 1)
    hi, lo = shell[1:].astype(np.float64), shell[:-1].astype(np.float64)
    exact = hist[1:-1] / (hi ** 3 - lo ** 3)
    half_ulps = 0.5 * (np.spacing((hi ** 3).astype(np.float32)) + np.spacing((lo ** 3).astype(np.float32))).astype(np.float64)
    bound = np.abs(exact) * (half_ulps / (hi ** 3 - lo ** 3) + 2 * 2.0 ** -24) * 1.01
    comparable = float(rr[1]) / (float(rr[1] - rr[0]) / nbins) * 2.0 ** -23 / 3 < 1e-4
    return hist, rdf, rs, exact, bound, comparable


@pytest.mark.parametrize("nbins,r_range", FINALIZE_CASES)
def test_rdf_finalize(htf, cuda, nbins, r_range):
    from hoomd_tf_amd import simmodel
    hist, rdf, rs, exact, bound, against_oracle = _finalize_case(nbins, r_range)
    assert against_oracle or (nbins, r_range) == (2046, (1.0, 2.5))
    got_rdf, got_rs = simmodel.rdf_from_histogram(_dev(hist, cuda), *r_range)
    got_rdf, got_rs = got_rdf.cpu().numpy(), got_rs.cpu().numpy()
    assert got_rdf.shape == (nbins,) and got_rs.shape == (nbins,)
    np.testing.assert_allclose(got_rs, rs, rtol=1.2e-7, atol=0)
    err = np.abs(got_rdf.astype(np.float64) - exact)
    nz = rdf != 0
    print("rdf_finalize nbins=%d range=%s: max err / bound %.3f, max relative distance to the oracle %.3g"
          % (nbins, r_range, float(np.max(err[nz] / bound[nz])), float(np.max(np.abs(got_rdf[nz] / rdf[nz] - 1)))))
    assert np.all(err <= bound)
    if against_oracle:
        np.testing.assert_allclose(got_rdf, rdf, rtol=1e-4)


@pytest.mark.parametrize("layout", ["vector", "column3"])
@pytest.mark.parametrize("type_i,type_j", [(None, None)] + TYPED_FORMS, ids=["untyped", "i", "j", "ij"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compute_rdf(htf, cuda, dtype, type_i, type_j, layout):
    from hoomd_tf_amd import simmodel
    B, NN, nbins, r_range = 300, 33, 100, (0.0, 3.5)
    typed = type_i is not None or type_j is not None
    if typed:
        nl, types, counts = typed_case("random", B, NN, r_range, type_i, type_j, nb=nbins + 2)
    else:
        (nl, counts), types = untyped_case(B, NN, nbins + 2, r_range), row_types("random", B)
    ref_rdf, ref_rs = O.compute_rdf(nl.astype(np.float32), list(r_range), types if typed else None, nbins, type_i, type_j)
    nl_t, types_t = _dev(nl, cuda, TDT[dtype]), _types_tensor(types, layout, cuda)
    rdf, rs = htf.compute_rdf(nl_t, list(r_range), type_tensor=types_t if typed else None, nbins=nbins, type_i=type_i, type_j=type_j)
    np.testing.assert_allclose(rdf.cpu().numpy(), ref_rdf, rtol=1e-4)
    np.testing.assert_allclose(rs.cpu().numpy(), ref_rs, rtol=1.2e-7)
    # the counts behind it are the direct call's: the same histogram through the same finalize gives the same bits
    direct = _histogram(nl_t, r_range, nbins + 2, types_t if typed else None, type_i, type_j)
    np.testing.assert_array_equal(direct.cpu().numpy(), counts)
    d_rdf, d_rs = simmodel.rdf_from_histogram(direct, *r_range)
    assert torch.equal(rdf, d_rdf) and torch.equal(rs, d_rs)
    assert np.count_nonzero(counts[1:-1]) >= 10


# ------------------------------------------------------------------------------------------------
# 2. RBFExpansion
# ------------------------------------------------------------------------------------------------
RBF_RANGES = [(0.0, 2.0), (-1.5, 4.0), (0.5, 0.75)]


def rbf_case(low, high, count, n_random, shape=None):
    """fp32 inputs: ``n_random`` values over [low - 1, high + 1] followed by every centre; the float64 reference."""
    rng = np.random.default_rng(count * 1000 + n_random)
    c, gap = O.rbf_centers(low, high, count)
    assert c[-1] == np.float32(high) and c[0] == np.float32(low) and gap > 0
    x = np.concatenate([rng.uniform(low - 1, high + 1, n_random).astype(np.float32), c])
    if shape is not None:
        x = x[:int(np.prod(shape))].reshape(shape)
    ref = O.rbf_expansion(x.astype(np.float64), low, high, count)
    return x, ref, c


def _rbf(htf, x_t, low, high, count):
    got = htf.RBFExpansion(low, high, count)(x_t)
    return got.tensor() if hasattr(got, "tensor") and callable(got.tensor) else got


@pytest.mark.parametrize("low,high", RBF_RANGES)
@pytest.mark.parametrize("count", [2, 10, 33])
def test_rbf_counts_and_ranges(htf, cuda, count, low, high):
    x, ref, c = rbf_case(low, high, count, 64)
    on_centre = ref[64:, :][np.arange(count), np.arange(count)]
    assert np.all(on_centre == 1.0) and x[-1] == np.float32(high)
    got = _rbf(htf, _dev(x, cuda), low, high, count).cpu().numpy()
    assert got.shape == (64 + count, count) and got.dtype == np.float32
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=1e-7)
    assert np.all(got[64:, :][np.arange(count), np.arange(count)] == 1.0)     # x on a centre, the last one (= high) included


@pytest.mark.parametrize("numel", [1, 257, 104900])
def test_rbf_sizes(htf, cuda, numel):
    count = 10
    x, ref, _ = rbf_case(0.0, 2.0, count, numel - count if numel > count else numel)
    x, ref = x[:numel], ref[:numel]
    assert x.size == numel and (numel * count > 4096 * 256) == (numel == 104900)     # the last one runs the grid-stride loop
    got = _rbf(htf, _dev(x, cuda), 0.0, 2.0, count).cpu().numpy()
    assert got.shape == (numel, count)
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=1e-7)


def test_rbf_keeps_the_input_shape(htf, cuda):
    x, ref, _ = rbf_case(-1.5, 4.0, 10, 7 * 5 * 3, shape=(7, 5, 3))
    got = _rbf(htf, _dev(x, cuda), -1.5, 4.0, 10)
    assert tuple(got.shape) == (7, 5, 3, 10)
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=2e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------------
# 3. wrap_vector
# ------------------------------------------------------------------------------------------------
BOXES = {"pow2": (4.0, 8.0, 16.0), "odd": (3.0, 5.5, 7.25)}


def wrap_random_case(L, n, dtype):
    """Vectors up to +-3.6 box lengths, none within 0.01 box lengths of a half-box tie; the float64 reference on the
    values the kernel gets."""
    rng = np.random.default_rng(n)
    q = rng.uniform(-3.6, 3.6, (n, 3))
    near_tie = np.abs(q - np.round(q)) >= 0.48
    q[near_tie] = np.trunc(q[near_tie]) + 0.25 * np.sign(q[near_tie])
    bs = np.asarray(L)
    r = (q * bs).astype(NDT[dtype])
    q = r.astype(np.float64) / bs
    assert np.all(np.abs(q - np.round(q)) < 0.49) and (n < 85 or np.abs(q).max() > 3.0)
    return r, O.wrap_vector(r.astype(np.float64), O.make_box(L))


def wrap_tie_case(L, dtype):
    """Every combination of +-0.5, +-1.5, +-2.5, +-3.5 box lengths in a power-of-two box: all arithmetic is exact."""
    h = np.array([s * (k + 0.5) for k in range(4) for s in (1, -1)])
    q = np.stack(np.meshgrid(h, h, h, indexing="ij"), -1).reshape(-1, 3)
    r = (q * np.asarray(L)).astype(NDT[dtype])
    ref = O.wrap_vector(r, O.make_box(L, dtype=NDT[dtype]))
    assert ref.dtype == NDT[dtype] and np.all(np.abs(ref) == np.asarray(L) / 2) and (ref > 0).any() and (ref < 0).any()
    # rint / tf.math.round go to the EVEN image: 0.5 and 2.5 box lengths keep their sign, 1.5 and 3.5 change it
    assert np.array_equal(np.sign(ref), np.sign(q) * np.where(np.floor(np.abs(q)) % 2 == 0, 1, -1))
    return r, ref


@pytest.mark.parametrize("n", [1, 85, 86, 1000])
@pytest.mark.parametrize("box", ["pow2", "odd"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_vector_random(htf, cuda, dtype, box, n):
    L = BOXES[box]
    r, ref = wrap_random_case(L, n, dtype)
    got = htf.wrap_vector(_dev(r, cuda), _dev(O.make_box(L), cuda))
    assert got.dtype == TDT[dtype] and tuple(got.shape) == (n, 3)
    np.testing.assert_allclose(got.cpu().numpy().astype(np.float64), ref, rtol=0, atol=4 * _eps(dtype) * np.abs(r).max())
    assert np.all(np.abs(got.cpu().numpy()) <= np.asarray(L) / 2 * (1 + 1e-6))


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_vector_half_box_ties(htf, cuda, dtype):
    L = BOXES["pow2"]
    r, ref = wrap_tie_case(L, dtype)
    box = _dev(O.make_box(L), cuda)
    got = htf.wrap_vector(_dev(r, cuda), box).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    assert np.array_equal(np.signbit(got), np.signbit(ref))
    # the torch route a tensor on an autograd graph takes gives the same values
    on_graph = _dev(r, cuda).requires_grad_(True)
    np.testing.assert_array_equal(htf.wrap_vector(on_graph, box).detach().cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------
# 4. topk_desc
# ------------------------------------------------------------------------------------------------
TOPK_NK = [(1, 1), (63, 63), (64, 1), (65, 8), (128, 128), (129, 16), (255, 200), (256, 256)]
TOPK_BS = [1, 3, 4, 5, 9]
TOPK_KINDS = ["normal", "equal", "five", "monotone", "zeros", "inf"]


def topk_rows(kind, B, n, k):
    rng = np.random.default_rng(B * 1000 + n)
    if kind == "normal":
        x = rng.standard_normal((B, n))
        assert n == 1 or ((x > 0).any() and (x < 0).any())
    elif kind == "equal":
        x = np.repeat(np.where(np.arange(B) % 2 == 0, 1.5, -1.5)[:, None], n, 1)
    elif kind == "five":      # ties across lanes (index % 64) and across a lane's slots (index // 64)
        x = rng.choice([-2.5, -1.0, 0.0, 0.75, 3.0], (B, n))
        def tie_spans(row, part):
            return any(len(set(part(np.flatnonzero(row == v)))) > 1 for v in np.unique(row))
        if n >= 6:
            assert all(tie_spans(row, lambda i: i % 64) for row in x)
        if n > 64:
            assert all(tie_spans(row, lambda i: i // 64) for row in x)
    elif kind == "monotone":  # even rows strictly increasing, odd rows strictly decreasing
        ramp = (np.arange(n) - n / 2 + 0.25) * 0.37
        x = np.where(np.arange(B)[:, None] % 2 == 0, ramp[None, :], -ramp[None, :])
    elif kind == "zeros":     # -0.0 ahead of +0.0 in index order: equal values, so the lower index goes first
        x = rng.choice([0.0, -0.0, -1.0, -3.5], (B, n))
        x[:, 0] = -0.0
        if n > 1:
            x[:, 1] = 0.0
            assert np.all(np.signbit(x[:, 0]) & ~np.signbit(x[:, 1]) & (x[:, 0] == x[:, 1]))
        if n >= 63:
            assert (x < 0).any() and np.all((x == 0).sum(1) > 2)
    elif kind == "inf":
        x = rng.standard_normal((B, n))
        x[:, 2::9] = np.inf
        x[:, 4::11] = -np.inf
        if n >= 63:
            assert np.all(np.isposinf(x).sum(1) > 1) and np.all(np.isneginf(x).sum(1) > 1)
    x = x.astype(np.float32)
    idx = np.argsort(-x, axis=1, kind="stable")[:, :k]
    return x, idx, np.take_along_axis(x, idx, 1)


@pytest.mark.parametrize("kind", TOPK_KINDS)
@pytest.mark.parametrize("n,k", TOPK_NK)
def test_topk_desc(htf, cuda, n, k, kind):
    for B in TOPK_BS:
        x, idx, vals = topk_rows(kind, B, n, k)
        got_v, got_i = htf.ops.topk_desc(_dev(x, cuda), k)
        np.testing.assert_array_equal(got_i.cpu().numpy(), idx, err_msg="B = %d" % B)
        # the values are the ORIGINAL bits (the sign of a zero included)
        np.testing.assert_array_equal(got_v.cpu().numpy().view(np.int32), vals.view(np.int32), err_msg="B = %d" % B)


def test_topk_desc_rejects(htf, cuda):
    x = torch.zeros((2, 257), dtype=torch.float32, device=cuda)
    with pytest.raises(ValueError):
        htf.ops.topk_desc(x[:, :8].contiguous(), 0)
    with pytest.raises(ValueError):
        htf.ops.topk_desc(x[:, :8].contiguous(), 9)
    with pytest.raises(ValueError):
        htf.ops.topk_desc(x, 4)


# ------------------------------------------------------------------------------------------------
# 5. bookkeeping kernels
# ------------------------------------------------------------------------------------------------
PAIRS = [("float32", "float32"), ("float64", "float32"), ("float64", "float64"), ("float32", "float64")]
INT_OF = {"float32": np.int32, "float64": np.int64}


def stuffed(n, dtype, seed):
    """HOOMD positions: random xyz, w = the BITS of the type id 0..6 (a denormal; ops.stuff_types' layout)."""
    rng = np.random.default_rng(seed)
    ids = np.arange(n) % 7
    p = np.zeros((n, 4), NDT[dtype])
    p[:, :3] = rng.uniform(-20, 20, (n, 3))
    p[:, 3] = ids.astype(INT_OF[dtype]).view(NDT[dtype])
    assert np.array_equal(p[:, 3].view(INT_OF[dtype]), ids) and (n < 2 or np.all(p[1:7, 3] != 0))
    return p, ids


@pytest.mark.parametrize("N", BLOCK_NS)
@pytest.mark.parametrize("src_dtype,dest_dtype", PAIRS)
def test_copy3(htf, cuda, src_dtype, dest_dtype, N):
    dest, ids = stuffed(N + 5, dest_dtype, 1)
    on_device = htf.ops.stuff_types(_dev(dest[:, :3], cuda), _dev(ids, cuda), TDT[dest_dtype])
    np.testing.assert_array_equal(on_device.cpu().numpy().view(INT_OF[dest_dtype]), dest.view(INT_OF[dest_dtype]))
    src = np.random.default_rng(N).uniform(-50, 50, (N + 2, 4)).astype(NDT[src_dtype])
    got = htf.ops.copy3(on_device, _dev(src, cuda), N).cpu().numpy()
    np.testing.assert_array_equal(got[:N, :3], src[:N, :3].astype(NDT[dest_dtype]))
    np.testing.assert_array_equal(got[:, 3].view(INT_OF[dest_dtype]), ids)                                  # the stuffed type, as bits
    np.testing.assert_array_equal(got[N:].view(INT_OF[dest_dtype]), dest[N:].view(INT_OF[dest_dtype]))      # rows N.. untouched


@pytest.mark.parametrize("unstuff4", [True, False])
@pytest.mark.parametrize("N", BLOCK_NS)
@pytest.mark.parametrize("src_dtype,dest_dtype", PAIRS)
def test_copy_positions(htf, cuda, src_dtype, dest_dtype, N, unstuff4):
    src, ids = stuffed(N + 7, src_dtype, 2)
    src_t = _dev(src, cuda)
    for offset in (0, 3, len(src) - N):
        got = htf.ops.copy_positions(src_t, offset=offset, N=N, unstuff4=unstuff4, out_dtype=TDT[dest_dtype])
        assert got.dtype == TDT[dest_dtype] and tuple(got.shape) == (N, 4)
        got = got.cpu().numpy()
        want = src[offset:offset + N].astype(NDT[dest_dtype])       # xyz and, not un-stuffed, w: the cast of what is stored
        if unstuff4:
            want[:, 3] = ids[offset:offset + N]                    # the type id as a number
        np.testing.assert_array_equal(got.view(INT_OF[dest_dtype]), want.view(INT_OF[dest_dtype]), err_msg="offset %d" % offset)


def energy_case(N, dtype):
    rng = np.random.default_rng(N + 11)
    f = np.full((N, 4), 1e30, NDT[dtype])                          # x, y, z: garbage that would swamp any sum
    f[:, 3] = (10.0 ** rng.uniform(-3, 3, N)) * rng.choice([-1.0, 1.0], N)
    e = f[:, 3].astype(np.float64)
    assert N < 63 or ((e > 0).any() and (e < 0).any() and np.abs(e).min() < 1e-2 and np.abs(e).max() > 1e2)
    return f, math.fsum(e), N * 2.0 ** -53 * float(np.abs(e).sum())


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_energy_sum(htf, cuda, dtype, N):
    f, ref, bound = energy_case(N, dtype)
    got = float(htf.ops.energy_sum(_dev(f, cuda)).item())
    assert abs(got - ref) <= bound, (got, ref, bound)


@pytest.mark.parametrize("dtype", DTYPES)
def test_energy_sum_of_no_rows(htf, cuda, dtype):
    """N = 0 of an allocated array (a torch tensor without rows has no pointer to hand over): the sum is 0, not what was there."""
    from hoomd_tf_amd import ops
    from hoomd_tf_amd._lib import lib, check
    f, _, _ = energy_case(8, dtype)
    f_t = _dev(f, cuda)
    out = torch.full((1,), 7.0, dtype=torch.float64, device=cuda)
    check(lib.htf_energy_sum(f_t.data_ptr(), ops._dt(f_t), 0, out.data_ptr(), ops._stream(f_t)))
    assert float(out.item()) == 0.0


@pytest.mark.parametrize("scale", [1.0, 1.0 / 777.0])
@pytest.mark.parametrize("n", [1, 63, 64, 1000, 1024, 1025, 3000])
def test_reduce_partials(htf, cuda, n, scale):
    rng = np.random.default_rng(n)
    buf = np.full(n + 9, 1e30, np.float32)                          # behind n: must not be read
    buf[:n] = (rng.standard_normal(n) + 0.5) * 10.0 ** rng.uniform(-2, 2, n)
    total = math.fsum(buf[:n].astype(np.float64))
    assert abs(total) > 1e-3 * float(np.abs(buf[:n]).sum())         # no cancellation: an fp32 ulp of the result dwarfs the double sum's error
    ref = np.float32(total * np.float64(np.float32(scale)))
    out = torch.full((1,), -5.0, dtype=torch.float32, device=cuda)
    htf.ops.reduce_partials(_dev(buf, cuda), n, scale, out)
    assert abs(float(out.item()) - float(ref)) <= float(np.spacing(np.abs(ref))), (float(out.item()), float(ref))


@pytest.mark.parametrize("N", BLOCK_NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_combine(htf, cuda, dtype, N):
    rng = np.random.default_rng(N + 3)
    f = rng.uniform(-5, 5, (N, 4)).astype(NDT[dtype])
    b = rng.uniform(-5, 5, (N, 4)).astype(NDT[dtype])
    alpha, cv = np.float32(-0.37251), np.float32(4.1873)
    term = float(alpha) * np.concatenate([b[:, :3].astype(np.float64), np.full((N, 1), float(cv))], 1)
    ref = f.astype(np.float64) + term
    got = htf.ops.bias_combine(_dev(f, cuda), _dev(b, cuda), _dev(np.array([alpha]), cuda), _dev(np.array([cv]), cuda)).cpu().numpy()
    assert got.dtype == NDT[dtype]
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 2 * _eps(dtype) * (np.abs(f) + np.abs(term)))


@pytest.mark.parametrize("slack", [0, 3])
@pytest.mark.parametrize("N", BLOCK_NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_virial(htf, cuda, dtype, N, slack):
    rng = np.random.default_rng(N + slack)
    pitch = N + slack
    src9 = rng.standard_normal((N, 9)).astype(NDT[dtype])
    src9[:, [3, 6, 7]] = [1e6, 2e6, 3e6]                            # the lower triangle must not land anywhere
    dest = rng.standard_normal(6 * pitch).astype(NDT[dtype])
    ref = O.receive_virial(dest.copy(), src9, pitch, 0, N)
    assert np.abs(ref).max() < 100 and not np.array_equal(ref, dest)
    got = htf.ops.add_virial(_dev(dest, cuda), _dev(src9, cuda), N, pitch).cpu().numpy()
    np.testing.assert_array_equal(got.view(INT_OF[dtype]), ref.view(INT_OF[dtype]))


@pytest.mark.parametrize("N", BLOCK_NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_scalar4(htf, cuda, dtype, N):
    rng = np.random.default_rng(N)
    a, b = rng.standard_normal((N, 4)).astype(NDT[dtype]), rng.standard_normal((N, 4)).astype(NDT[dtype])
    got = htf.ops.add_scalar4(_dev(a, cuda), _dev(b, cuda)).cpu().numpy()
    np.testing.assert_array_equal(got.view(INT_OF[dtype]), (a + b).view(INT_OF[dtype]))


def check_nlist_case(B, NN, planted, dtype):
    """Random fills of four kinds of slot -- dx > 0 (the only kind that counts), dx < 0, dx = 0 with dy != 0, empty -- with
    row ``planted`` full of dx > 0 and one slot of every other row not counting: the maximum NN lives in that row alone."""
    rng = np.random.default_rng(B * 100 + NN)
    kind = rng.integers(0, 4, (B, NN))
    kind[np.arange(B), rng.integers(0, NN, B)] = rng.integers(1, 4, B)
    kind[planted] = 0
    nl = np.zeros((B, NN, 4), NDT[dtype])
    nl[..., 0] = np.where(kind == 0, rng.uniform(1e-30, 3, (B, NN)), np.where(kind == 1, -rng.uniform(0.1, 3, (B, NN)), 0.0))
    nl[..., 1] = np.where(kind != 3, rng.uniform(0.1, 2, (B, NN)), 0.0)
    nl[..., 3] = np.where(kind != 3, rng.integers(0, 3, (B, NN)), 0.0)
    counts = (nl[..., 0] > 0).sum(1)
    assert counts[planted] == NN and np.all(np.delete(counts, planted) < NN) and O.check_nlist_count(nl) == NN
    if (B - 1) * NN >= 30:
        assert (nl[..., 0] < 0).any() and ((nl[..., 0] == 0) & (nl[..., 1] != 0)).any() and (np.abs(nl[..., :3]).sum(-1) == 0).any()
    return nl


@pytest.mark.parametrize("NN", [1, 15, 16, 17, 63, 65])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 65])
@pytest.mark.parametrize("dtype", DTYPES)
def test_check_nlist(htf, cuda, dtype, B, NN):
    for planted in sorted({0, B // 2, B - 1}):
        nl = check_nlist_case(B, NN, planted, dtype)
        assert htf.ops.check_nlist(_dev(nl, cuda)) == O.check_nlist_count(nl), "maximum planted in row %d" % planted
    if B > 1:       # no row full: the maximum is some row's partial count
        nl[planted, NN // 2, 0] = -1.0
        assert htf.ops.check_nlist(_dev(nl, cuda)) == O.check_nlist_count(nl)


@pytest.mark.parametrize("dtype", DTYPES)
def test_check_nlist_empty_and_uncounted(htf, cuda, dtype):
    nl = np.zeros((33, 17, 4), NDT[dtype])
    assert htf.ops.check_nlist(_dev(nl, cuda)) == 0
    nl[..., 0], nl[..., 1] = -1.0, 2.0                  # every slot holds a neighbor, none with dx > 0
    nl[5, :, 0] = 0.0
    assert O.check_nlist_count(nl) == 0 and htf.ops.check_nlist(_dev(nl, cuda)) == 0


def _radial_close(got, ref):
    """test_positions_forces_radial's bound: |d| <= 1e-5 + 2e-5 |ref|."""
    got = got.astype(np.float64)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - ref) <= 1e-5 + 2e-5 * np.abs(ref)), float(np.max(np.abs(got - ref) / (1e-5 + 2e-5 * np.abs(ref))))


def radial_case(N, seed, lo, hi, types):
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((N, 3))
    p = np.zeros((N, 4), np.float32)
    p[:, :3] = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(lo, hi, (N, 1))
    p[:, 3] = rng.choice(types, N)
    return p


@pytest.mark.parametrize("power", [-16, -1, 2, 16])
@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_positions_radial_row_at_the_origin(htf, cuda, dtype, ncomp, power):
    p = radial_case(257, 1, 0.5, 2.0, [0.0, 1.0])
    p[[0, 100, 256]] = 0.0                              # at the origin with type 0: |p| = 0 for either ncomp
    ref = O.positions_radial_model(p.astype(np.float64), power=power, ncomp=ncomp)
    assert np.all(ref[[0, 100, 256]] == 0.0) and np.all(np.isfinite(ref))
    got = htf.ops.positions_forces_radial(_dev(p, cuda, TDT[dtype]), power=power, ncomp=ncomp).cpu().numpy()
    assert np.all(got[[0, 100, 256]] == 0.0)
    _radial_close(got, ref)


@pytest.mark.parametrize("power", [-16, 16])
@pytest.mark.parametrize("ncomp", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_positions_radial_extreme_powers(htf, cuda, dtype, ncomp, power):
    p = radial_case(1000, 2, 0.85, 1.0, [0.0, 0.5])     # |p| in [0.85, 1.12] over three or four columns
    norm = np.linalg.norm(p[:, :ncomp].astype(np.float64), axis=1)
    assert norm.min() > 0.84 and norm.max() < 1.13 and (norm < 1).any() and ((norm > 1).any() or ncomp == 3)
    ref = O.positions_radial_model(p.astype(np.float64), coef=0.75, power=power, ncomp=ncomp)
    assert np.abs(ref).max() > 3
    got = htf.ops.positions_forces_radial(_dev(p, cuda, TDT[dtype]), coef=0.75, power=power, ncomp=ncomp).cpu().numpy()
    _radial_close(got, ref)


@pytest.mark.parametrize("power", [-1, -2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_positions_radial_three_columns_against_four(htf, cuda, dtype, power):
    p = radial_case(300, 3, 0.5, 3.0, [1.0, 2.0])       # a non-zero type in every row: the two norms differ everywhere
    ref3 = O.positions_radial_model(p.astype(np.float64), power=power, ncomp=3)
    ref4 = O.positions_radial_model(p.astype(np.float64), power=power, ncomp=4)
    assert np.all(np.abs(ref3[:, 3] - ref4[:, 3]) > 1e-2 * np.abs(ref3[:, 3]))
    p_t = _dev(p, cuda, TDT[dtype])
    _radial_close(htf.ops.positions_forces_radial(p_t, power=power, ncomp=3).cpu().numpy(), ref3)
    _radial_close(htf.ops.positions_forces_radial(p_t, power=power, ncomp=4).cpu().numpy(), ref4)
