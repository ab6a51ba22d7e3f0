"""The conservative htf.DescriptorMLP on one domain's rows on the MI355X (include/htf_cghost.h; total_forces /
total_loss_gradient / angular_loss_gradient with ``n_ghost`` and ``halo``): a system decomposed by hand, in one process.

The systems are tests/test_gpu_desc_total.py's jittered lattices (symmetric lists by geometry, exact fp32 pair vectors: that
module asserts both): config a, 6^3 particles, list cutoff 1.8, NN = 37, and b256, 7^3, cutoff 2.9, NN = 256 (four slots per
lane).  Particle id = ix n^2 + iy n + iz, so the local rows L -- lattice x-index below ``layers`` -- are the first |L| rows; the
ghosts are every other particle a slot of a local row names, numbered from |L| up in ascending id.  ``halo`` copies the ghosts'
rows out of the whole system's table (pass 1 of the whole system through the C entries; the whole system's residual).

No atomics and fixed-order sums: a row's bits depend on its slots, its indices and the gathered rows alone, so the decomposed
rows carry the whole system's BITS.  Everything here is an equality except the sum of two domains' sweeps, whose partials are
added in another order: there the bound is twice what each fp32 sweep meets against fp64 (test_gpu_desc_total_train.py: 2e-4 of
the largest gradient entry, 1e-5 on the SSR)."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_desc_angular as A
import test_gpu_desc_total as T

pytestmark = pytest.mark.gpu
TOL_F, TOL_G, TOL_SSR = 2e-5, 2e-4, 1e-5


# ------------------------------------------------------------------------------------------------ the decomposition
@functools.lru_cache(maxsize=None)
def _domain(config, layers=None, upper=False):
    """(rows [nL] long: the local particles, ghosts [nG] long, idx_loc [nL, NN] int32) of the slab of lattice x-index below
    ``layers`` (n / 2 when None), or with ``upper`` its complement."""
    p, L, rc_list, x, idx = T._system(config)
    n = T.CONFIGS[config][0]
    N = len(p)
    ix = torch.arange(N, device=p.device) // (n * n)
    assert torch.equal(torch.floor(p[:, 0] + 0.5).long() % n, ix)   # (the id is the lattice index: jitter < 0.5)
    local = (ix * 2 < n) if layers is None else (ix < layers)
    if upper:
        local = ~local
    rows = torch.nonzero(local)[:, 0]
    named = idx[rows].long()
    named = torch.unique(named[named >= 0])
    ghosts = named[~local[named]]
    assert len(rows) > 0 and len(ghosts) > 0 and len(rows) + len(ghosts) <= N
    remap = torch.full((N,), -1, dtype=torch.int32, device=p.device)
    remap[rows] = torch.arange(len(rows), dtype=torch.int32, device=p.device)
    remap[ghosts] = len(rows) + torch.arange(len(ghosts), dtype=torch.int32, device=p.device)
    idx_loc = torch.where(idx[rows] >= 0, remap[idx[rows].long().clamp(min=0)], torch.full_like(idx[rows], -1)).contiguous()
    assert bool((idx_loc[idx[rows] >= 0] >= 0).all())
    return rows, ghosts, idx_loc


def _layer(htf, l_max=0, **kw):
    return A._layer(htf, l_max=l_max, **kw) if l_max else T._layer(htf, **kw)


def _act(htf, lay):
    return htf._lib.ACT_TANH if lay.activation == "tanh" else htf._lib.ACT_LINEAR


def _pass1(htf, lay, x):
    """(table, energy) of the whole system by the C entries of pass 1, as total_forces calls them: g [B, D], or {g, p, S}
    [B, Dr, 4 or 10] with l_max > 0."""
    from hoomd_tf_amd import ops
    L, B, NN = htf._lib, x.shape[0], x.shape[1]
    e = torch.empty((B,), dtype=torch.float32, device=x.device)
    common = (x.data_ptr(), ops._dt(x), B, NN, lay.K, lay.n_types, lay.H1, lay.H2, _act(htf, lay), lay.w.data_ptr(), lay.mu.data_ptr(),
              float(lay.gap))
    if lay.l_max:
        t = torch.empty((B, lay.Dr, 4 if lay.l_max == 1 else 10), dtype=torch.float32, device=x.device)
        L.check(L.lib.htf_ang_grad(*common, t.data_ptr(), e.data_ptr(), None, B, float(lay.r_cut or 0.0), lay.l_max, ops._stream(x)))
    else:
        t = torch.empty((B, lay.D), dtype=torch.float32, device=x.device)
        L.check(L.lib.htf_cf_grad(*common, t.data_ptr(), e.data_ptr(), None, B, float(lay.r_cut or 0.0), ops._stream(x)))
    return t, e


def _pass2(htf, lay, x, idx, types, table, e, n_table=None, virial=True):
    """Pass 2 by the C entries: the twin (n_table None) or the entry of include/htf_cghost.h.  -> (forces [B, 4], virial [B, 9])."""
    from hoomd_tf_amd import ops
    L, B, NN = htf._lib, x.shape[0], x.shape[1]
    out = torch.full((B, 4), float("nan"), dtype=x.dtype, device=x.device)
    v = torch.full((B, 9), float("nan"), dtype=x.dtype, device=x.device) if virial else None
    own = types.to(torch.float32).contiguous() if lay.n_types > 1 else None
    head = (x.data_ptr(), ops._dt(x), idx.data_ptr(), own.data_ptr() if own is not None else None, B, NN, lay.K, lay.n_types,
            lay.mu.data_ptr(), float(lay.gap), table.data_ptr(), e.data_ptr(), out.data_ptr(), ops._dt(out),
            v.data_ptr() if virial else None, float(lay.r_cut or 0.0))
    if lay.l_max:
        head += (lay.l_max,)
    twin, ghost = ((L.lib.htf_ang_forces, L.lib.htf_ang_forces_ghost) if lay.l_max else (L.lib.htf_cf_forces, L.lib.htf_cf_forces_ghost))
    L.check(twin(*head, ops._stream(x)) if n_table is None else ghost(*head, n_table, ops._stream(x)))
    return out, v


def _sweep(htf, lay, x, idx, rho, rows=None, n_table=None):
    """The force-matching sweep by the C entries on a residual table: the twin (n_table None) or the entry of htf_cghost.h."""
    from hoomd_tf_amd import ops
    L, B, NN = htf._lib, x.shape[0], x.shape[1]
    n_rows = B if rows is None else len(rows)
    accum = torch.full((1 + lay.P,), float("nan"), dtype=torch.float32, device=x.device)
    scratch = torch.empty(max(1, int(L.lib.htf_bp_scratch_floats(n_rows, lay.K, lay.n_types * (1 + lay.l_max), lay.H1, lay.H2))),
                          dtype=torch.float32, device=x.device)
    head = (x.data_ptr(), ops._dt(x), idx.data_ptr(), B, NN, lay.K, lay.n_types, lay.H1, lay.H2, _act(htf, lay), lay.w.data_ptr(),
            lay.mu.data_ptr(), float(lay.gap), rho.data_ptr(), accum.data_ptr(), scratch.data_ptr(),
            rows.data_ptr() if rows is not None else None, n_rows, float(lay.r_cut or 0.0))
    if lay.l_max:
        head += (lay.l_max,)
    twin, ghost = ((L.lib.htf_at_loss_grad, L.lib.htf_at_loss_grad_ghost) if lay.l_max
                   else (L.lib.htf_ct_loss_grad, L.lib.htf_ct_loss_grad_ghost))
    L.check(twin(*head, ops._stream(x)) if n_table is None else ghost(*head, n_table, ops._stream(x)))
    return accum


class Halo:
    """``halo(table)`` for a hand-made domain: the ghosts' rows of the whole system's tables, chosen by the shape of a row; a row
    shape in ``zero`` is filled with zeros instead (an exchange that was forgotten).  Counts its calls and checks what it is handed:
    the rows [0, nL) already hold the local particles' rows of the same whole-system table."""

    def __init__(self, rows, ghosts, tables, zero=()):
        self.rows, self.ghosts, self.zero, self.calls = rows, ghosts, tuple(zero), []
        self.tables = {tuple(t.shape[1:]): t for t in tables}
        assert len(self.tables) == len(tables)

    def __call__(self, table):
        whole = self.tables[tuple(table.shape[1:])]
        nL, nG = len(self.rows), len(self.ghosts)
        assert table.shape[0] == nL + nG and table.dtype == torch.float32 and table.is_contiguous()
        assert torch.equal(table[:nL], whole[self.rows])
        self.calls.append(tuple(table.shape[1:]))
        if tuple(table.shape[1:]) in self.zero:
            table[nL:].zero_()
        else:
            table[nL:] = whole[self.ghosts]


def _labels(B, cuda, seed):
    return torch.from_numpy(0.05 * np.random.default_rng(seed).standard_normal((B, 4))).to(torch.float32).to(cuda)


CASES = [(16, 1), (6, 3), (6, 1)]   # (K, n_types): K = 16 gathers float4, K = 6 single floats; three types need the rows' own


def _case_layer(htf, l_max, K, n_types, cut, rc_list, seed=5):
    return _layer(htf, l_max=l_max, K=K, n_types=n_types, high=rc_list, r_cut=0.9 * rc_list if cut else None, seed=seed + n_types)


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("K,n_types", CASES)
@pytest.mark.parametrize("l_max", [0, 1, 2])
def test_ghost_entries_with_the_twins_table_give_the_twins_bits(htf, cuda, l_max, K, n_types, dtype):
    """n_table = B: htf_cf_forces_ghost / htf_ang_forces_ghost and htf_ct_loss_grad_ghost / htf_at_loss_grad_ghost write what
    htf_cf_forces / htf_ang_forces and htf_ct_loss_grad / htf_at_loss_grad write, with and without a row list; and the layer's
    default path is those bits."""
    p, L, rc_list, x, idx = T._system("a")
    lay = _case_layer(htf, l_max, K, n_types, True, rc_list)
    xx, types, B = x.to(dtype), p[:, 3].contiguous(), len(p)
    table, e = _pass1(htf, lay, xx)
    f, v = _pass2(htf, lay, xx, idx, types, table, e)
    fg, vg = _pass2(htf, lay, xx, idx, types, table, e, n_table=B)
    assert torch.isfinite(f).all() and torch.isfinite(v).all() and f[:, :3].abs().max().item() > 1e-3
    assert torch.equal(fg, f) and torch.equal(vg, v)
    lf, lv = lay.total_forces(xx, idx, virial=True, types=types)
    assert torch.equal(lf, f) and torch.equal(lv.reshape(B, 9), v)
    rho = (f.to(torch.float32) - _labels(B, cuda, 3)).contiguous()
    rows = torch.arange(B - 1, -1, -2, dtype=torch.int32, device=cuda).contiguous()
    for r in (None, rows):
        a = _sweep(htf, lay, xx, idx, rho, rows=r)
        assert torch.isfinite(a).all() and a[1:].abs().max().item() > 0
        assert torch.equal(_sweep(htf, lay, xx, idx, rho, rows=r, n_table=B), a)


# ------------------------------------------------------------------------------------------------ 2. forces, decomposed by hand
def _decomposed_forces(htf, cuda, config, l_max, K, n_types, cut, dtype, layers=None):
    p, L, rc_list, x, idx = T._system(config)
    rows, ghosts, idx_loc = _domain(config, layers)
    lay = _case_layer(htf, l_max, K, n_types, cut, rc_list)
    xx, types = x.to(dtype), p[:, 3].contiguous()
    whole_f, whole_v = lay.total_forces(xx, idx, virial=True, types=types)
    table, e = _pass1(htf, lay, xx)
    halo = Halo(rows, ghosts, [table])
    x_loc, t_loc = xx[rows].contiguous(), types[rows].contiguous()
    f, v = lay.total_forces(x_loc, idx_loc, virial=True, types=t_loc, n_ghost=len(ghosts), halo=halo)
    assert len(halo.calls) == 1 and f.dtype == dtype and f.shape == (len(rows), 4) and v.shape == (len(rows), 3, 3)
    assert whole_f[rows, :3].abs().max().item() > 1e-3
    assert torch.equal(f, whole_f[rows]) and torch.equal(v, whole_v[rows])
    # without the virial: the same launch family, the same bits
    assert torch.equal(lay.total_forces(x_loc, idx_loc, types=t_loc, n_ghost=len(ghosts), halo=halo), whole_f[rows])
    return lay, (rows, ghosts, idx_loc), (f, whole_f)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("K,n_types", CASES)
@pytest.mark.parametrize("l_max", [0, 1, 2])
def test_decomposed_forces_are_the_whole_systems_bits(htf, cuda, l_max, K, n_types, cut, dtype):
    """Rows L of the whole system's total_forces -- forces, energy and virial -- from (x[L], remapped index, the ghosts' table
    rows): torch.equal."""
    lay, (rows, ghosts, idx_loc), _ = _decomposed_forces(htf, cuda, "a", l_max, K, n_types, cut, dtype)
    # both faces of the slab have ghosts (layers n - 1 through the periodic image, and n / 2), and interior rows have none
    n = T.CONFIGS["a"][0]
    assert set((ghosts // (n * n)).tolist()) == {n // 2, n - 1}
    assert bool((idx_loc < len(rows)).all(dim=1).any()) and bool((idx_loc >= len(rows)).any(dim=1).any())


@pytest.mark.parametrize("l_max", [0, 2])
def test_decomposed_forces_four_slots_per_lane(htf, cuda, l_max):
    """7^3, cutoff 2.9, NN = 256: every slot register of a lane is in use, ghosts are two lattice layers deep on either side."""
    _decomposed_forces(htf, cuda, "b256", l_max, 16, 1, True, torch.float32)


@pytest.mark.parametrize("l_max", [0, 1, 2])
def test_one_ghost_layer_serves_both_faces(htf, cuda, l_max):
    """Five of the six lattice layers are local: the sixth is the periodic neighbor of layer 0 and the neighbor of layer 4, so
    every ghost is gathered by rows on both faces of the slab."""
    lay, (rows, ghosts, idx_loc), _ = _decomposed_forces(htf, cuda, "a", l_max, 6, 3, True, torch.float32, layers=5)
    n = T.CONFIGS["a"][0]
    assert set((ghosts // (n * n)).tolist()) == {n - 1}
    layer_of_row = (rows // (n * n))[:, None].expand_as(idx_loc)
    for g in range(len(rows), len(rows) + len(ghosts)):
        assert set(layer_of_row[idx_loc == g].tolist()) == {0, n - 2}


# ------------------------------------------------------------------------------------------------ 3. the sweeps, decomposed by hand
def _decomposed_sweep(htf, cuda, l_max, K, n_types, cut, dtype, zero=(), near=False):
    """-> (layer, whole-system accum, [accum of the lower half, accum of the upper half]); asserts bit contract (c): each half
    equals the twin entry on the whole system with the half's row list.  Labels: noise of size 0.05 (the residual is then mostly
    the energy's, as in test_gpu_desc_total_train.py), or with ``near`` the prediction plus that noise (force and energy
    residuals of one size)."""
    p, L, rc_list, x, idx = T._system("a")
    lay = _case_layer(htf, l_max, K, n_types, cut, rc_list, seed=6)
    xx, types, B = x.to(dtype), p[:, 3].contiguous(), len(p)
    table, _ = _pass1(htf, lay, xx)
    pred = lay.total_forces(xx, idx, types=types).to(torch.float32)
    labels = _labels(B, cuda, 7 + n_types) + (pred if near else 0.0)
    sweep = lay.angular_loss_gradient if l_max else lay.total_loss_gradient
    whole = sweep(xx, labels, idx, types=types)
    rho = (pred - labels).contiguous()
    halves = []
    for upper in (False, True):
        rows, ghosts, idx_loc = _domain("a", None, upper)
        halo = Halo(rows, ghosts, [table, rho], zero=zero)
        got = sweep(xx[rows].contiguous(), labels[rows].contiguous(), idx_loc, types=types[rows].contiguous(),
                    n_ghost=len(ghosts), halo=halo)
        assert halo.calls == [tuple(table.shape[1:]), (4,)]   # (pred through total_forces with the same halo, then the residual)
        assert got.shape == whole.shape and torch.isfinite(got).all()
        if not zero:
            want = _sweep(htf, lay, xx, idx, rho, rows=rows.to(torch.int32).contiguous())
            assert torch.equal(got, want), "rows %s: max diff %.3g" % ("upper" if upper else "lower", (got - want).abs().max().item())
            # a prediction handed in is the one evaluated inside
            again = Halo(rows, ghosts, [rho])
            assert torch.equal(sweep(xx[rows].contiguous(), labels[rows].contiguous(), idx_loc, pred=pred[rows].contiguous(),
                                     n_ghost=len(ghosts), halo=again), got) and again.calls == [(4,)]
        halves.append(got)
    return lay, whole, halves


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("K,n_types", CASES)
@pytest.mark.parametrize("l_max", [0, 1, 2])
def test_decomposed_sweeps(htf, cuda, l_max, K, n_types, cut, dtype):
    """Each half's sweep on (x_loc, idx_loc) with the residual halo is, bit for bit, the existing entry on the whole system with
    the half's row list; the halves added in fp64 are the whole system's sweep to twice the bound a sweep meets against fp64."""
    lay, whole, halves = _decomposed_sweep(htf, cuda, l_max, K, n_types, cut, dtype)
    total, ref = halves[0].double() + halves[1].double(), whole.double()
    scale, err = ref[1:].abs().max().item(), (total[1:] - ref[1:]).abs().max().item()
    print("l_max %d K %d T %d cut %s %s: max|sum of halves - whole| = %.3g of %.3g (ratio %.3g); SSR %.9g vs %.9g"
          % (l_max, K, n_types, cut, dtype, err, scale, err / scale, total[0].item(), ref[0].item()))
    assert scale > 0 and err <= 2 * TOL_G * scale
    assert abs(total[0].item() - ref[0].item()) <= 2 * TOL_SSR * ref[0].item()


# ------------------------------------------------------------------------------------------------ 4. the tests can fail
def test_a_forgotten_halo_moves_the_forces(htf, cuda):
    """Ghost rows left at zero: some boundary row's force moves by more than 100 x the bound of tests/test_gpu_desc_total.py.
    The precondition is stated on the fp64 formula of include/htf_cforce.h (the local rows' formula on (x_loc, idx_loc) has no
    reverse term for an index >= |L|), not on the kernels."""
    p, L, rc_list, x, idx = T._system("a")
    rows, ghosts, idx_loc = _domain("a")
    lay = _case_layer(htf, 0, 6, 3, True, rc_list)
    types = p[:, 3].contiguous()
    F = T.formula(lay, x, idx, types.long())[0]
    F_cut = T.formula(lay, x[rows].contiguous(), idx_loc, types[rows].long())[0]
    moved = (F[rows] - F_cut).abs().max(dim=1)[0]
    bound = 100 * TOL_F * F.abs().max().item()
    boundary = (idx_loc >= len(rows)).any(dim=1)
    print("formula: max move %.3g, bound %.3g, rows moved %d of %d boundary rows" % (moved.max().item(), bound, int((moved > bound).sum()), int(boundary.sum())))
    assert moved.max().item() > bound and bool((moved[~boundary] < 1e-12).all())
    table, e = _pass1(htf, lay, x)
    whole = lay.total_forces(x, idx, types=types)
    lost = lay.total_forces(x[rows].contiguous(), idx_loc, types=types[rows].contiguous(), n_ghost=len(ghosts),
                            halo=Halo(rows, ghosts, [table], zero=[tuple(table.shape[1:])]))
    diff = (lost[:, :3].double() - whole[rows, :3].double()).abs().max(dim=1)[0]
    assert diff.max().item() > bound and torch.equal(lost[~boundary], whole[rows][~boundary])
    T._close(lost[:, :3], F_cut, "forces without the ghosts' rows")
    # the energy column needs no halo
    assert torch.equal(lost[:, 3], whole[rows, 3])


@pytest.mark.parametrize("l_max", [0, 2])
def test_a_forgotten_residual_halo_moves_the_gradient(htf, cuda, l_max):
    """The ghosts' residuals left at zero (the table of pass 1 exchanged as it should be): the sum of the halves leaves the whole
    system's gradient by more than 100 x the sweeps' bound -- the pattern of the "forgot rho_j" checks.  The labels are the
    prediction plus noise: against labels of noise alone the energy residual is E_i itself, its term 2 sum_i rho_iE in the
    gradient of b3 is the largest entry by far (the scale the bound is stated in), and it needs no halo."""
    lay, whole, halves = _decomposed_sweep(htf, cuda, l_max, 16, 1, True, torch.float32, zero=[(4,)], near=True)
    total, ref = halves[0].double() + halves[1].double(), whole.double()
    scale, err = ref[1:].abs().max().item(), (total[1:] - ref[1:]).abs().max().item()
    print("l_max %d: zeroed residual halo moves the gradient by %.3g of %.3g (ratio %.3g)" % (l_max, err, scale, err / scale))
    assert err > 100 * TOL_G * scale
    assert abs(total[0].item() - ref[0].item()) <= 2 * TOL_SSR * ref[0].item()   # (the SSR is the local rows' own)


# ------------------------------------------------------------------------------------------------ 5. edges
@pytest.mark.parametrize("l_max", [0, 1, 2])
def test_index_outside_the_table(htf, cuda, l_max):
    """An index >= n_table or negative on a live slot of a boundary row: no reverse term, nothing read -- the bits of the whole
    system with -1 in the same slots.  The sweep treats the same slots as m = 0."""
    p, L, rc_list, x, idx = T._system("a")
    rows, ghosts, idx_loc = _domain("a")
    lay = _case_layer(htf, l_max, 6, 3, True, rc_list)
    types, nL, n_table = p[:, 3].contiguous(), len(rows), len(rows) + len(ghosts)
    boundary = torch.nonzero((idx_loc >= nL).any(dim=1))[:4, 0]
    bad = [n_table, n_table + 5, -7, 2 ** 31 - 1]
    idx_w, idx_l = idx.clone(), idx_loc.clone()
    for r, value in zip(boundary.tolist(), bad):
        s = int(torch.nonzero(idx_loc[r] >= nL)[0, 0])   # a slot that names a ghost
        idx_l[r, s], idx_w[rows[r], s] = value, -1
    table, e = _pass1(htf, lay, x)
    whole = lay.total_forces(x, idx_w, virial=True, types=types)
    assert not torch.equal(whole[0][rows], lay.total_forces(x, idx, types=types)[rows])   # (the dropped terms are not zero)
    halo = Halo(rows, ghosts, [table])
    got = lay.total_forces(x[rows].contiguous(), idx_l, virial=True, types=types[rows].contiguous(), n_ghost=len(ghosts), halo=halo)
    assert torch.equal(got[0], whole[0][rows]) and torch.equal(got[1], whole[1][rows])
    labels = _labels(len(p), cuda, 9)
    rho = (whole[0].to(torch.float32) - labels).contiguous()
    sweep = lay.angular_loss_gradient if l_max else lay.total_loss_gradient
    acc = sweep(x[rows].contiguous(), labels[rows].contiguous(), idx_l, pred=whole[0][rows].to(torch.float32).contiguous(),
                n_ghost=len(ghosts), halo=Halo(rows, ghosts, [rho]))
    assert torch.equal(acc, _sweep(htf, lay, x, idx_w, rho, rows=rows.to(torch.int32).contiguous()))


@pytest.mark.parametrize("l_max", [0, 1])
def test_no_ghost_rows_no_halo_call(htf, cuda, l_max):
    """n_ghost = 0 with a halo given: the halo is never called and the bits are the default path's."""
    p, L, rc_list, x, idx = T._system("a")
    lay = _case_layer(htf, l_max, 6, 3, True, rc_list)
    types, labels = p[:, 3].contiguous(), _labels(len(p), cuda, 11)

    def halo(table):
        raise AssertionError("halo called for n_ghost = 0")

    f, v = lay.total_forces(x, idx, virial=True, types=types)
    fg, vg = lay.total_forces(x, idx, virial=True, types=types, n_ghost=0, halo=halo)
    assert torch.equal(fg, f) and torch.equal(vg, v)
    sweep = lay.angular_loss_gradient if l_max else lay.total_loss_gradient
    assert torch.equal(sweep(x, labels, idx, types=types, n_ghost=0, halo=halo), sweep(x, labels, idx, types=types))


@pytest.mark.parametrize("l_max", [0, 1, 2])
def test_zero_rows_with_ghost_rows(htf, cuda, l_max):
    """B = 0: nothing is launched on the pair tensor, the halo still gets its table of n_ghost rows, the sweep returns zeros."""
    lay = _layer(htf, l_max=l_max, K=8, n_types=2)
    seen = []
    for dt in (torch.float32, torch.float64):
        x = torch.zeros((0, 32, 4), dtype=dt, device=cuda)
        index, types = torch.zeros((0, 32), dtype=torch.int32, device=cuda), torch.zeros((0,), device=cuda)
        f, v = lay.total_forces(x, index, virial=True, types=types, n_ghost=3, halo=lambda t: seen.append(tuple(t.shape)))
        assert f.shape == (0, 4) and v.shape == (0, 3, 3) and f.dtype == dt
        sweep = lay.angular_loss_gradient if l_max else lay.total_loss_gradient
        acc = sweep(x, torch.zeros((0, 4), dtype=dt, device=cuda), index, types=types, n_ghost=3,
                    halo=lambda t: seen.append(tuple(t.shape)))
        assert acc.shape == (1 + lay.w.numel(),) and (acc == 0).all()
    row = (lay.Dr, 4 if l_max == 1 else 10) if l_max else (lay.D,)
    assert seen == [(3,) + row, (3,) + row, (3, 4)] * 2
