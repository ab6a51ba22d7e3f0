"""tests/brick_ref.py checked without a GPU: every seeded case holds the edge it stands for, the NumPy reference equals the torch
restatement (``BrickDomain(backend="torch")``) bit for bit, and one tiny plan is typed out by hand so that the two cannot be wrong
together unnoticed."""
import types

import numpy as np
import pytest
import torch

import brick_ref as R

TORCH = {"f32": torch.float32, "f64": torch.float64}
REPLICA = [g for g in R.GEOMETRIES if R.GEOMETRIES[g][3]]
RANKS = [g for g in R.GEOMETRIES if not R.GEOMETRIES[g][3]]
OVERFLOWS = {"over_mig": R.BF_MIG_OVERFLOW, "over_int": R.BF_INT_OVERFLOW, "over_bnd": R.BF_BND_OVERFLOW, "over_ghost": R.BF_GHOST_OVERFLOW}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(np.asarray(b, dtype=a.dtype)))


def _carried_by(geom, c):
    return sum(R.msg_takes_class(geom, m, c) for m in range(geom["n_msg"]))


# ------------------------------------------------------------------------------------------------ the cases hold their edges
@pytest.mark.parametrize("gid,dt", R.case_ids())
def test_thresholds_reach_every_key_and_class(gid, dt):
    """At least one row in every destination key and every class the geometry can have (class 2 along a thin axis, and with both
    axes thin a row in all eight messages), with inert rows at rows 0, 1, every 7th and the last."""
    case = R.cases(gid, dt)["thresholds"]
    g = case.geom
    r = case.run()[0]
    inert = np.isnan(case.pos[:, 0])
    n_in = int(np.nonzero(~inert)[0].max()) + 2     # the interleaved rows; what follows pads the arrays to their capacity
    assert inert[0] and inert[1] and inert[n_in - 1] and all(inert[i] for i in range(0, n_in, 7))
    keys = set(int(k) for k in r["key"])
    want = set(range(g["n_msg"] + 2))
    for d in range(g["ndim"]):       # two bricks of real ranks along an axis: everything that leaves travels "up"
        if g["p"][d] == 2 and not g["replica"]:
            want -= {1 + m for m, o in enumerate(R.offsets(g["ndim"])) if o[d] == -1}
    assert keys == want
    classes = set(int(k) for k in R.class_keys(r["cand_pos"], g, case.bounds))
    per_axis = []
    for d in range(g["ndim"]):   # a brick wider than 2 r_ghost has no row near both faces, a thinner one none away from both
        w = case.bounds[d][g["me"][d] + 1] - case.bounds[d][g["me"][d]]
        per_axis.append({0, 1, 3} if w > 2 * g["r_ghost"] else ({1, 3} if w == 2 * g["r_ghost"] else {1, 2, 3}))
    possible = {k0 + 4 * k1 for k0 in per_axis[0] for k1 in (per_axis[1] if g["ndim"] == 2 else {0})}
    assert classes == possible, (sorted(classes), sorted(possible))
    carried = set(_carried_by(g, c) for c in classes)
    if gid == "thin3x3":
        assert 2 in [c & 3 for c in classes] and {1, 2, 3, 5} <= carried
    if gid == "thin3x3-both":
        assert 10 in classes and {3, 5, 8} <= carried
    if g["p"][0] == 2 and g["replica"]:   # the minimum-image face choice: rows either side of the point opposite the brick's centre
        b, me = case.bounds[0], g["me"][0]
        far = 0.5 * (b[me] + b[me + 1]) + R.BOX_L / 2
        far = far if far < b[2] else far - R.BOX_L
        x = case.pos[:, 0].astype(np.float64)
        assert set(int(k) for k in r["key"][(np.abs(x - far) < 1e-2)]) == {1, 2}


@pytest.mark.parametrize("gid,dt", R.case_ids())
def test_cases_are_what_they_claim(gid, dt):
    cs = R.cases(gid, dt)
    for name, case in cs.items():
        g, res = case.geom, case.run()
        n_msg = g["n_msg"]
        for r in res:
            assert (r["flags"] & ~R.BF_LOST) == (case.flags & ~R.BF_LOST), (name, r["flags"])
        kind = name.rstrip("0123456789")
        if kind in OVERFLOWS:
            assert res[0]["flags"] == OVERFLOWS[kind] == int(res[0]["counts"][R.BC_FLAGS]), name
            by = int(name[len(kind):])
            c = res[0]["counts"]
            n_int, n_bnd = int(c[R.BC_CLASS + 1]), int(c[R.BC_N_CAND] - c[R.BC_CLASS + 1])
            if kind == "over_int":
                assert n_int == g["cap_int"] + by
            if kind == "over_bnd":
                assert n_bnd == g["cap_bnd"] + by and by < R.ghost_rows(g)   # (the halo pack reads pos[cap_int + n_bnd - 1])
            if kind == "over_ghost":
                need = [sum(int(c[R.BC_CLASS + k + 1] - c[R.BC_CLASS + k]) for k in range(1, R.n_classes(g)) if R.msg_takes_class(g, m, k))
                        for m in range(n_msg)]
                over = [n - g["ghost_cap"][m] for m, n in enumerate(need)]
                assert max(over) == by and all(o in (by, 0) or o < 0 for o in over), over
                assert np.any(res[0]["row_slots"][:int(c[R.BC_N_BND])] == R.NONE)
            if kind == "over_mig":
                start = res[0]["start1"]
                over = [int(start[2 + m] - start[1 + m]) - (g["mig_cap"][m] - 1) for m in range(n_msg)]
                assert max(over) == by and all(o in (by, 0) or o < 0 for o in over), over
        if name == "exact_fit":
            c = res[0]["counts"]
            assert res[0]["flags"] == 0 and int(c[R.BC_N_INT]) == g["cap_int"] and int(c[R.BC_N_BND]) == g["cap_bnd"]
            assert [int(v) for v in c[R.BC_MSG:R.BC_MSG + n_msg]] == g["ghost_cap"][:n_msg]
            # every migration message exactly full: the ones a replica rank sends (and so receives); at a real rank the ones it
            # receives (what it sends depends on its neighbors' side of the cut: two bricks send nothing "down")
            held = res[0]["mig_counts"] if g["replica"] else [int(R.header_view(res[0]["mig_recv"])[g["mig_off"][m]]) for m in range(n_msg)]
            assert held == [v - 1 for v in g["mig_cap"][:n_msg]]
        if name == "empty":
            assert np.all(res[0]["key"] == n_msg + 1) and int(res[0]["counts"][R.BC_N_CAND]) == 0 and res[0]["inert"].all()
        if name == "no_interior":
            assert int(res[0]["counts"][R.BC_N_INT]) == 0 and int(res[0]["counts"][R.BC_N_BND]) > 0
        if name.startswith("no_boundary"):
            assert int(res[0]["counts"][R.BC_N_BND]) == 0 and int(res[0]["counts"][R.BC_N_INT]) > 0
            assert not np.any(R.header_view(res[0]["mig_send"])[g["mig_off"][:n_msg]])        # every message empty
            assert (g["cap_bnd"] == 0) == (name == "no_boundary_cap0")
        if name == "one_row":
            assert R.cap(g) == 3
        if name.startswith("tile"):
            assert R.cap(g) + R.mig_rows(g) == int(name[4:])
        if name == "lost":
            r = res[0]
            assert r["flags"] == R.BF_LOST and r["lost"].sum() == 1
            i = int(np.nonzero(r["lost"])[0][0])
            assert r["key"][i] == 0 and np.any(r["vel"][:, 2] == case.vel[i, 2])    # key 0: it stays a candidate, and is placed
    assert ("lost" in cs) == gid.startswith("ends5")
    assert cs["thresholds"].rounds == 3 and cs["tile1025"].rounds == 3
    last = cs["thresholds"].run()[-1]["counts"]
    assert int(last[R.BC_REBUILDS]) == 3 and int(last[R.BC_N_ARRIVED]) > int(cs["thresholds"].run()[0]["counts"][R.BC_N_ARRIVED]) > 0


# ------------------------------------------------------------------------------------------------ reference == torch restatement
def _domain(gid, dt, case):
    """A BrickDomain on CPU tensors with the case's geometry and capacities."""
    from hoomd_tf_amd.brick import BrickDomain
    g = case.geom
    n_msg = g["n_msg"]
    grid, coords, fractions = [1, 1, 1], [0, 0, 0], {}
    for d in range(g["ndim"]):
        a, p = g["axis"][d], g["p"][d]
        grid[a], coords[a] = p, g["me"][d]
        fractions[a] = [(case.bounds[d][c] - R.BOX_LO) / R.BOX_L for c in range(1, p)]
    lo = [R.BOX_LO] * 3
    s = types.SimpleNamespace(N=1, n_ghost=0, box3x3=np.array([lo, [R.BOX_LO + R.BOX_L] * 3, [0.0] * 3]), periodic=(1, 1, 1),
                              device=torch.device("cpu"), pos=torch.zeros((1, 4), dtype=TORCH[dt]), vel=torch.zeros((1, 4), dtype=TORCH[dt]))
    rank = coords[0] + grid[0] * (coords[1] + grid[1] * coords[2])
    dom = BrickDomain(s, 0 if g["replica"] else rank, tuple(grid), r_ghost=g["r_ghost"], fractions=fractions, replica=bool(g["replica"]),
                      coords=tuple(coords), n_global=1000, backend="torch", transport="torch", local_grid=not g["halo_wrap"])
    assert tuple(dom.coords) == tuple(coords) and dom.n_msg == n_msg and dom.offsets == R.offsets(g["ndim"])
    for d in range(g["ndim"]):
        assert np.array_equal(dom.bounds[g["axis"][d]], case.bounds[d][:g["p"][d] + 1])
    assert np.array_equal(dom.shift, np.array(g["shift"][:n_msg])) and np.array_equal(dom.mig_shift, np.array(g["mig_shift"][:n_msg]))
    assert int(dom.halo_wrap) == g["halo_wrap"] and int(dom.mig_wrap) == g["mig_wrap"]
    # the case's capacities instead of the constructor's
    dom.cap_int, dom.cap_bnd, dom.cap = g["cap_int"], g["cap_bnd"], R.cap(g)
    dom.ghost_cap, dom.ghost_off = g["ghost_cap"][:n_msg], g["ghost_off"][:n_msg]
    dom.mig_cap, dom.mig_off = g["mig_cap"][:n_msg], g["mig_off"][:n_msg]
    dom.n_ghost_cap, dom.mig_rows = R.ghost_rows(g), R.mig_rows(g)
    dom.cand = dom.cap + dom.mig_rows
    t = TORCH[dt]
    s.pos = torch.full((dom.cap + dom.n_ghost_cap, 4), -777.0, dtype=t)
    s.vel = torch.full((dom.cap, 4), -777.0, dtype=t)
    s.N, s.n_ghost = dom.cap, dom.n_ghost_cap
    dom.mig_send = torch.zeros((dom.mig_rows, 8), dtype=t)
    dom.mig_recv = torch.zeros((dom.mig_rows, 8), dtype=t)
    dom.halo_send = torch.empty((dom.n_ghost_cap, 4), dtype=t)
    return dom, s


def _defined_words(g):
    w = [R.BC_N_INT, R.BC_N_BND, R.BC_N_CAND, R.BC_N_ARRIVED, R.BC_FLAGS, R.BC_REBUILDS]
    w += list(range(R.BC_MSG, R.BC_MSG + g["n_msg"])) + list(range(R.BC_CLASS, R.BC_CLASS + R.n_classes(g) + 1))
    return w + list(range(R.BC_SLOT, R.BC_SLOT + 16 * R.MAX_MSG))


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("gid", REPLICA)
def test_reference_equals_torch_restatement(gid, dt):
    """Replica geometries, every case without a flag, every round: local arrays, migration messages, all the counts (BC_CLASS, BC_MSG
    and BC_SLOT included) and the halo message, bit for bit."""
    n = 0
    for name, case in R.cases(gid, dt).items():
        res = case.run()
        if any(r["flags"] for r in res) or case.planted is not None:
            continue
        g = case.geom
        dom, s = _domain(gid, dt, case)
        words = _defined_words(g)
        for r in res:
            s.pos[:dom.cap] = torch.from_numpy(r["pos_in"])
            s.vel[:] = torch.from_numpy(r["vel_in"])
            c_in = r["counts_in"].copy()
            dom.counts = torch.from_numpy(c_in.view(np.int32).copy())
            dom.rebuild()
            assert _same(r["pos"], s.pos[:dom.cap].numpy()) and _same(r["vel"], s.vel.numpy()), (name, "local rows")
            got = dom.counts.numpy().view(np.uint32)
            assert np.array_equal(got[words], r["counts"][words]), (name, "counts")
            send = dom.mig_send.numpy()
            assert _same(r["mig_send"][r["mig_mask"]], send[r["mig_mask"]]), (name, "migration rows")
            off = g["mig_off"][:g["n_msg"]]
            assert np.array_equal(R.header_view(send)[off], R.header_view(r["mig_send"])[off]), (name, "migration headers")
            assert _same(r["halo_send"], dom.halo_send.numpy()), (name, "halo message")
            assert _same(r["halo_direct"], s.pos[dom.cap:].numpy()), (name, "ghost region")
            n += 1
    assert n >= 10


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("gid", RANKS)
def test_reference_keys_equal_torch_restatement(gid, dt):
    """Real-rank geometries (their transport needs ranks): destination keys, the lost mask and class keys only."""
    for name, case in R.cases(gid, dt).items():
        dom, s = _domain(gid, dt, case)
        for r in case.run():
            key, lost = dom._dest_keys_torch(torch.from_numpy(r["pos_in"]))
            assert np.array_equal(key.numpy(), r["key"]) and np.array_equal(lost.numpy(), r["lost"]), name
            k2 = dom._class_keys_torch(torch.from_numpy(np.ascontiguousarray(r["cand_pos"])))
            assert np.array_equal(k2.numpy(), R.class_keys(r["cand_pos"], case.geom, case.bounds)), name
            assert np.all(np.diff(k2.numpy()) >= 0)    # (the candidates are in class order)


# ------------------------------------------------------------------------------------------------ typed out by hand
@pytest.mark.parametrize("dt", list(R.DTYPES))
def test_hand_written_slab3(dt):
    """slab3: bricks [-8, -3 | -3, 3 | 3, 8], this rank the middle one, r_ghost 1.5, a replica (what leaves through the high face
    comes back 6 lower).  Twelve rows; everything below is worked out by hand from include/htf_standin.h."""
    dtype = R.DTYPES[dt]
    nan = np.nan
    geom, bounds = R.geometry("slab3-w0")
    g = R.with_caps(geom, 4, 8, 4, 3)
    x = [nan, 0.0, -3.0, 3.0, -3.25, 1.5, -1.5, nan, 2.0, -7.0, 7.5, -2.0]
    pos = np.array([[v, v if v != v else 0.5, v if v != v else -0.25, 0.0 if v != v else 2.0] for v in x], dtype=dtype)
    vel = np.array([[0, 0, 0, 1] if v != v else [i, 0.5, 0, 1] for i, v in enumerate(x)], dtype=dtype)
    key, lost = R.dest_keys(pos, g, bounds)
    #                 inert: 3   stay: 0   through the low face (message 0): 1   through the high face (message 1): 2
    assert key.tolist() == [3, 0, 0, 2, 1, 0, 0, 3, 0, 1, 2, 0] and not lost.any()
    start1, order1 = R.key_sort(key, 16)
    assert order1.tolist() == [1, 2, 5, 6, 8, 11, 4, 9, 3, 10, 0, 7] and start1.tolist() == [0, 6, 8, 10] + [12] * 13
    send, mask, n_mig, flags = R.pack_migrants(pos, vel, key, g)
    assert n_mig == [2, 2] and flags == 0 and mask.tolist() == [False, True, True, False, True, True]
    assert R.header_view(send)[[0, 3]].tolist() == [2, 2]
    assert send[[1, 2, 4, 5], 0].tolist() == [2.75, -1.0, -3.0, 1.5]       # message 0 shifted by +6, message 1 by -6
    assert send[[1, 2, 4, 5], 4].tolist() == [4, 9, 3, 10]
    recv = R.deliver(send, g)
    assert recv[[1, 2, 4, 5], 4].tolist() == [3, 10, 4, 9]
    m = R.merge(pos, vel, key, recv, g, bounds, R.fresh_counts())
    # candidates: stayed 1 2 5 6 8 11 | from the high neighbor 4 9 | from the low neighbor 3 10
    #   x          0 -3 1.5 -1.5 2 -2 |  2.75 -1                   |  -3 1.5
    #   class      0  1  3   0   3  1 |  3     0                   |   1  3
    assert m["cand_vel"][:, 0].tolist() == [1, 6, 9, 2, 11, 3, 5, 8, 4, 10]
    assert m["vel"][:, 0].tolist() == [1, 6, 9, 0, 2, 11, 3, 5, 8, 4, 10, 0]
    want_x = [0.0, -1.5, -1.0, nan, -3.0, -2.0, -3.0, 1.5, 2.0, 2.75, 1.5, nan]
    assert _same(m["pos"][:, 0], np.array(want_x, dtype=dtype))
    assert m["inert"].tolist() == [False] * 3 + [True] + [False] * 7 + [True]
    assert _same(m["pos"][3], np.array([nan, nan, nan, 0], dtype=dtype)) and m["vel"][3].tolist() == [0, 0, 0, 1]
    assert m["pos"][9].tolist() == [2.75, 0.5, -0.25, 2.0]
    c = m["counts"]
    assert c[[R.BC_N_INT, R.BC_N_BND, R.BC_N_CAND, R.BC_N_ARRIVED, R.BC_FLAGS, R.BC_REBUILDS]].tolist() == [3, 7, 10, 4, 0, 1]
    assert c[R.BC_MSG:R.BC_MSG + 2].tolist() == [3, 4] and c[R.BC_CLASS:R.BC_CLASS + 5].tolist() == [0, 3, 6, 6, 10]
    slot = c[R.BC_SLOT:R.BC_SLOT + 128].reshape(16, 8)
    assert slot[1, :2].tolist() == [0, R.NONE] and slot[2, :2].tolist() == [3, 0] and slot[3, :2].tolist() == [R.NONE, 0]
    assert np.all(slot[0] == R.NONE) and np.all(slot[4:] == R.NONE) and np.all(slot[:, 2:] == R.NONE)
    halo, direct = R.pack_halo(m["pos"], c, g)
    assert _same(halo[:, 0], np.array([3.0, 4.0, 3.0, nan, -4.5, -4.0, -3.25, -4.5], dtype=dtype))
    assert _same(direct[:, 0], np.array([-4.5, -4.0, -3.25, -4.5, 3.0, 4.0, 3.0, nan], dtype=dtype))
    assert halo[4].tolist() == [-4.5, 0.5, -0.25, 2.0] and _same(halo[3], np.array([nan, nan, nan, 0], dtype=dtype))
    rs = R.row_slots(c, g)
    assert rs[:, 0].tolist() == [0, 1, 2] + [R.NONE] * 5 and rs[:, 1].tolist() == [R.NONE] * 3 + [0, 1, 2, 3, R.NONE]
    assert np.all(rs[:, 2:] == R.NONE)
    # and the torch restatement on the same rows
    case = R.Case("hand", g, bounds, pos, vel)
    dom, s = _domain("slab3-w0", dt, case)
    s.pos[:12], s.vel[:] = torch.from_numpy(pos), torch.from_numpy(vel)
    dom.counts = torch.zeros(R.BC_WORDS, dtype=torch.int32)
    dom.rebuild()
    assert _same(np.array(want_x, dtype=dtype), s.pos[:12, 0].numpy()) and s.vel[:, 0].tolist() == [1, 6, 9, 0, 2, 11, 3, 5, 8, 4, 10, 0]
    assert _same(direct, s.pos[12:].numpy())
    assert np.array_equal(dom.counts.numpy().view(np.uint32)[_defined_words(g)], c[_defined_words(g)])
