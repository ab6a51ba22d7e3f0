"""The brick kernels (csrc/brick.hip) against the NumPy reference of tests/brick_ref.py, driven through the C entry points on
hand-filled ``htfs_brick`` geometries: the two-brick branches, axes other than x-first, the wrapped neighbors, lost rows, rows on
every threshold and one ulp either side, class key 2, every overflow, empty and degenerate plans, candidate counts either side of
the sort tile.  Every comparison is bit for bit (NaN with NaN); every array has guard rows either side, checked after every call."""
import ctypes as C

import numpy as np
import pytest
import torch

import brick_ref as R

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f64": torch.float64}
GUARD = 8
FSENT = -777.0              # floats no kernel writes
ISENT = 0x5A5A5A5A          # words no kernel writes (brick_ref.fresh_counts fills the reference's counts with the same)
GARBAGE = 0x2B2B2B2B
NEIGH = 7
IDS = ["%s-%s" % p for p in R.case_ids()]


def _stream(dev):
    from hoomd_tf_amd.ops import raw_stream
    return C.c_void_p(raw_stream(dev.index))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want):
    """Bit for bit, any NaN equal to any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(_bits(got)[~gn], _bits(want)[~wn])


class Guarded:
    """A device array with GUARD rows of sentinel in front of it and behind it."""

    def __init__(self, rows, width, dtype, fill, dev):
        shape = (rows + 2 * GUARD,) + ((width,) if width else ())
        self.fill = fill
        self.buf = torch.full(shape, fill, dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + rows]
        self.rows = rows

    def ptr(self, row=0):
        return self.t.data_ptr() + row * (self.t.stride(0) * self.t.element_size() if self.rows else 0)

    def set(self, a, first=0):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        self.t[first:first + len(a)] = torch.from_numpy(a).to(self.t.device)

    def get(self):
        a = self.t.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == self.fill).all()) and bool((b[GUARD + self.rows:] == self.fill).all())


def _isent32():
    return int(np.array(ISENT, dtype=np.uint32).view(np.int32))


class Harness:
    """The device side of one case: geometry, bounds, local arrays, messages, counts and the scratch of a rebuild."""

    def __init__(self, htf, dev, case, dt):
        self.lib, self.dev, self.case, self.g = htf._lib, dev, case, case.geom
        lib, g = self.lib, self.g
        self.code = lib.HTF_F32 if dt == "f32" else lib.HTF_F64
        self.np = R.DTYPES[dt]
        t, i32 = TORCH[dt], torch.int32
        self.cap, self.ghost, self.mig = R.cap(g), R.ghost_rows(g), R.mig_rows(g)
        self.cand = self.cap + self.mig
        self.geom = self.brick(g)
        a = self.a = {}
        a["bounds"] = Guarded(2 * (R.MAX_P + 1), 0, t, FSENT, dev)
        a["bounds"].set(case.bounds.astype(self.np).reshape(-1))
        a["pos"] = Guarded(self.cap + self.ghost, 4, t, FSENT, dev)
        a["vel"] = Guarded(self.cap, 4, t, FSENT, dev)
        a["counts"] = Guarded(R.BC_WORDS, 0, i32, _isent32(), dev)
        a["counts"].set(R.fresh_counts(ISENT))
        a["mig_send"] = Guarded(self.mig, 8, t, FSENT, dev)
        a["mig_recv"] = Guarded(self.mig, 8, t, FSENT, dev)
        a["halo"] = Guarded(self.ghost, 4, t, FSENT, dev)
        a["n_neigh"] = Guarded(self.cap, 0, i32, _isent32(), dev)
        a["n_neigh"].t[:] = NEIGH
        a["row_slots"] = Guarded(max(g["cap_bnd"], 1), R.MAX_MSG, i32, _isent32(), dev)
        garbage = int(np.array(GARBAGE, dtype=np.uint32).view(np.int32))
        for name, rows, width in (("key", self.cand, 0), ("order", self.cand, 0), ("start1", 17, 0), ("start2", 33, 0)):
            a[name] = Guarded(rows, width, i32, _isent32(), dev)
            a[name].t[:] = garbage
        # the caller's contract (BrickDomain._make_device_state): sort_scratch is 32 words per 1024-candidate tile, zeroed
        a["scratch"] = Guarded(32 * ((self.cand + 1023) // 1024), 0, i32, _isent32(), dev)
        a["scratch"].t[:] = 0
        for name in ("tmp_pos", "tmp_vel"):
            a[name] = Guarded(self.cand, 4, t, FSENT, dev)
            a[name].t[:] = 12345.0
        w = self.work = lib.BrickWork()
        w.key, w.order, w.sort_scratch = a["key"].ptr(), a["order"].ptr(), a["scratch"].ptr()
        w.start1, w.start2, w.tmp_pos, w.tmp_vel = a["start1"].ptr(), a["start2"].ptr(), a["tmp_pos"].ptr(), a["tmp_vel"].ptr()
        self.s = _stream(dev)

    def brick(self, g):
        b = self.lib.Brick()
        b.ndim, b.n_msg, b.replica, b.r_ghost = g["ndim"], g["n_msg"], g["replica"], g["r_ghost"]
        b.cap_int, b.cap_bnd, b.halo_wrap, b.mig_wrap = g["cap_int"], g["cap_bnd"], g["halo_wrap"], g["mig_wrap"]
        for d in range(2):
            b.axis[d], b.p[d], b.me[d] = g["axis"][d], g["p"][d], g["me"][d]
        for m in range(R.MAX_MSG):
            b.ghost_cap[m], b.ghost_off[m], b.mig_cap[m], b.mig_off[m] = g["ghost_cap"][m], g["ghost_off"][m], g["mig_cap"][m], g["mig_off"][m]
            for c in range(3):
                b.shift[m][c], b.mig_shift[m][c] = g["shift"][m][c], g["mig_shift"][m][c]
        for c in range(3):
            b.box_lo[c], b.box_L[c] = g["box_lo"][c], g["box_L"][c]
        return b

    def ghost_ptr(self):
        return self.a["pos"].ptr(self.cap)

    def load(self, pos, vel, counts=None):
        self.a["pos"].set(pos)
        self.a["vel"].set(vel)
        if counts is not None:
            self.a["counts"].set(counts)

    def sync_and_check_guards(self, what):
        torch.cuda.synchronize()
        bad = [k for k, v in self.a.items() if not v.intact()]
        assert not bad, (self.case.name, what, "wrote outside", bad)

    # ---- the entry points
    def migrate_pack(self, geom=None):
        a = self.a
        self.lib.check(self.lib.lib.htfs_brick_migrate_pack(C.byref(geom or self.geom), a["pos"].ptr(), a["vel"].ptr(), self.code, a["bounds"].ptr(),
                                                            C.byref(self.work), a["mig_send"].ptr(), a["counts"].ptr(), self.s))

    def migrate_merge(self, n_neigh=True, geom=None):
        a = self.a
        self.lib.check(self.lib.lib.htfs_brick_migrate_merge(C.byref(geom or self.geom), a["pos"].ptr(), a["vel"].ptr(), self.code, a["bounds"].ptr(),
                                                             C.byref(self.work), a["mig_recv"].ptr(), a["n_neigh"].ptr() if n_neigh else None,
                                                             a["counts"].ptr(), self.s))

    def pack_halo(self, send=True, direct=False, geom=None, direct_ptr=None):
        a = self.a
        self.lib.check(self.lib.lib.htfs_brick_pack_halo(C.byref(geom or self.geom), a["pos"].ptr(), self.code, a["counts"].ptr(),
                                                         a["halo"].ptr() if send else None,
                                                         (direct_ptr or self.ghost_ptr()) if direct else None, self.s))

    def row_slots(self, geom=None):
        self.lib.check(self.lib.lib.htfs_brick_row_slots(C.byref(geom or self.geom), self.a["counts"].ptr(), self.a["row_slots"].ptr(), self.s))

    def deliver(self, r):
        """mig_recv as the exchange leaves it: a replica rank's own message m in the slot of source offset n_msg - 1 - m (copied on the
        device, "don't care" rows and all); the planted messages of a rank with real neighbors."""
        g, a = self.g, self.a
        if self.case.planted is not None:
            a["mig_recv"].set(r["mig_recv"])
            return
        for m in range(g["n_msg"]):
            j = g["n_msg"] - 1 - m
            a["mig_recv"].t[g["mig_off"][j]:g["mig_off"][j] + g["mig_cap"][j]] = a["mig_send"].t[g["mig_off"][m]:g["mig_off"][m] + g["mig_cap"][m]]

    # ---- comparisons with one round of the reference
    def check_pack(self, r):
        g, a, name = self.g, self.a, self.case.name
        n_msg = g["n_msg"]
        assert np.array_equal(a["key"].get()[:self.cap], r["key"].astype(np.uint32)), (name, "destination keys")
        assert np.array_equal(a["start1"].get(), r["start1"].astype(np.uint32)), (name, "start1")
        assert np.array_equal(a["order"].get()[:self.cap], r["order1"].astype(np.uint32)), (name, "order")
        send = a["mig_send"].get()
        off = g["mig_off"][:n_msg]
        assert np.array_equal(R.header_view(send)[off], R.header_view(r["mig_send"])[off]), (name, "migration headers")
        assert _same(send[r["mig_mask"]], r["mig_send"][r["mig_mask"]]), (name, "migration rows")
        assert np.array_equal(a["counts"].get(), r["counts_pack"]), (name, "flags after the pack", int(a["counts"].get()[R.BC_FLAGS]))

    def check_merge(self, r, n_neigh=True):
        a, name = self.a, self.case.name
        got = a["counts"].get()
        bad = np.nonzero(got != r["counts"])[0]
        assert len(bad) == 0, (name, "counts", [(int(w), int(got[w]), int(r["counts"][w])) for w in bad[:8]])
        pos = a["pos"].get()
        assert _same(pos[:self.cap], r["pos"]), (name, "positions")
        assert _same(a["vel"].get(), r["vel"]), (name, "velocities")
        assert np.all(pos[self.cap:] == FSENT), (name, "the ghost region is not the rebuild's to write")
        want = np.where(r["inert"], 0, NEIGH) if n_neigh else np.full(self.cap, NEIGH)
        assert np.array_equal(a["n_neigh"].get(), want.astype(np.uint32)), (name, "n_neigh")


def _cases(gid, dt, only=None):
    cs = R.cases(gid, dt)
    return [c for n, c in cs.items() if only is None or only(n)]


def _not_over(name):
    return not name.startswith("over_")


@pytest.mark.parametrize("gid,dt", R.case_ids(), ids=IDS)
def test_migrate_pack(htf, cuda, gid, dt):
    """htfs_brick_migrate_pack on every round's input: destination keys, start1, the stable order, every defined row of mig_send and
    its header word, FLAGS (LOST, MIG_OVERFLOW) -- and not one other word of the counts."""
    for case in _cases(gid, dt):
        h = Harness(htf, cuda, case, dt)
        for r in case.run():
            h.load(r["pos_in"], r["vel_in"], r["counts_in"])
            h.migrate_pack()
            h.sync_and_check_guards("migrate_pack")
            h.check_pack(r)


@pytest.mark.parametrize("gid,dt", R.case_ids(), ids=IDS)
def test_migrate_merge(htf, cuda, gid, dt):
    """htfs_brick_migrate_merge behind the pack, the rounds chained on the device state (moved between rounds as the reference
    moves its own): local arrays, all BC_WORDS of the counts, n_neigh zeroed on inert rows and untouched on live ones; the first
    round once more with d_n_neigh = NULL."""
    for case in _cases(gid, dt, _not_over):
        for n_neigh in ((True, False) if case.name in ("thresholds", "one_row") else (True,)):
            h = Harness(htf, cuda, case, dt)
            res = case.run()
            pos, vel = res[0]["pos_in"], res[0]["vel_in"]
            for r in (res if n_neigh else res[:1]):
                assert _same(pos, r["pos_in"]) and _same(vel, r["vel_in"])
                h.load(pos, vel)
                h.migrate_pack()
                h.deliver(r)
                h.migrate_merge(n_neigh)
                h.sync_and_check_guards("migrate_merge")
                h.check_merge(r, n_neigh)
                h.a["n_neigh"].t[:] = NEIGH
                vel = h.a["vel"].get()
                pos = R.move(h.a["pos"].get()[:h.cap], vel, case.geom)


@pytest.mark.parametrize("gid,dt", R.case_ids(), ids=IDS)
def test_pack_halo(htf, cuda, gid, dt):
    """htfs_brick_pack_halo on the reference's plan, three ways -- send only, direct only, both: the messages bit for bit, inert
    rows behind each count, nothing else written (slab3-w1-me0: a message that leaves the box is wrapped back into it)."""
    for case in _cases(gid, dt, _not_over):
        r = case.run()[-1]
        for send, direct in ((True, False), (False, True), (True, True)):
            h = Harness(htf, cuda, case, dt)
            h.load(r["pos"], r["vel"], r["counts"])
            h.pack_halo(send, direct)
            h.sync_and_check_guards("pack_halo")
            pos = h.a["pos"].get()
            assert _same(pos[:h.cap], r["pos"]) and np.array_equal(h.a["counts"].get(), r["counts"])
            if send:
                assert _same(h.a["halo"].get(), r["halo_send"]), (case.name, "send")
            else:
                assert np.all(h.a["halo"].get() == FSENT)
            if direct:
                assert _same(pos[h.cap:], r["halo_direct"]), (case.name, "direct")
            else:
                assert np.all(pos[h.cap:] == FSENT)


@pytest.mark.parametrize("gid,dt", R.case_ids(), ids=IDS)
def test_row_slots(htf, cuda, gid, dt):
    """htfs_brick_row_slots against the reference: rows past N_BND all 0xFFFFFFFF; without a boundary segment the call returns OK and
    leaves its output alone."""
    seen_cap0 = False
    for case in _cases(gid, dt, _not_over):
        r = case.run()[-1]
        h = Harness(htf, cuda, case, dt)
        h.load(r["pos"], r["vel"], r["counts"])
        h.row_slots()
        h.sync_and_check_guards("row_slots")
        got = h.a["row_slots"].get()
        if case.geom["cap_bnd"] == 0:
            assert np.all(got == ISENT), case.name
            seen_cap0 = True
            continue
        assert np.array_equal(got, r["row_slots"]), case.name
        assert np.all(got[int(r["counts"][R.BC_N_BND]):] == R.NONE)
        assert np.array_equal(h.a["counts"].get(), r["counts"])
    assert seen_cap0 == ("no_boundary_cap0" in R.cases(gid, dt))


def _dyadic_forces(h, r):
    """Velocities as the plan left them (dyadic), forces that are small dyadic numbers of the row index."""
    i = np.arange(h.cap)
    f = np.stack([((i % 9) - 4) * 0.125, ((i % 5) - 2) * 0.25, ((i % 7) - 3) * 0.5, np.zeros(h.cap)], axis=1).astype(h.np)
    return torch.from_numpy(f).to(h.dev)


def _box(lib):
    lo, hi = R.BOX_LO, R.BOX_LO + R.BOX_L
    return lib.make_box(np.array([[lo] * 3, [hi] * 3, [0.0] * 3]), (1, 1, 1))


DT = 2.0 ** -6


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("cap_int", [255, 256, 257])
@pytest.mark.parametrize("gid", ["slab3-w1-me0", "thin3x3", "yz"])
def test_nve_halo_equals_step_then_pack(htf, cuda, gid, cap_int, dt):
    """htfs_brick_nve_halo == htfs_nve_step over the local rows, then htfs_brick_pack_halo on the advanced positions: positions,
    velocities and both message buffers whole (the inert tails are the ones the rebuild's pack left).  cap_int 255, 256, 257: the
    first workgroup holds a boundary row, holds none (it skips the table), and the second one holds a single interior row."""
    lib = htf._lib
    case = R.planned_case(gid, dt, cap_int)
    r = case.run()[0]
    box = _box(lib)
    for send, direct in ((True, True), (True, False), (False, True)):
        one, two = Harness(htf, cuda, case, dt), Harness(htf, cuda, case, dt)
        force = _dyadic_forces(one, r)
        for h in (one, two):
            h.load(r["pos"], r["vel"], r["counts"])
            h.pack_halo(send, direct)            # the rebuild's own pack: the tails
        a = one.a
        lib.check(lib.lib.htfs_brick_nve_halo(C.byref(one.geom), a["pos"].ptr(), a["vel"].ptr(), force.data_ptr(), one.code, DT, C.byref(box),
                                              a["counts"].ptr(), a["halo"].ptr() if send else None, one.ghost_ptr() if direct else None, one.s))
        b = two.a
        lib.check(lib.lib.htfs_nve_step(b["pos"].ptr(), b["vel"].ptr(), force.data_ptr(), two.code, two.cap, DT, C.byref(box), two.s))
        two.pack_halo(send, direct)
        one.sync_and_check_guards("nve_halo")
        two.sync_and_check_guards("nve_step + pack_halo")
        assert _same(a["pos"].get(), b["pos"].get()), "positions and ghost region"
        assert _same(a["vel"].get(), b["vel"].get()) and _same(a["halo"].get(), b["halo"].get())
        assert not _same(a["pos"].get()[:one.cap], r["pos"])           # (it did move)
        assert np.array_equal(a["counts"].get(), r["counts"])


def _peer(lib, h, dev):
    """One block laid out as brick.py::_make_peer lays it out (inbox [2][ghost rows] Scalar4, then the signal words), this rank its
    own neighbor in every direction; the state words in ordinary device memory."""
    esz = 4 * np.dtype(h.np).itemsize
    up = lambda n: (int(n) + 255) // 256 * 256  # noqa: E731
    inbox, signal = 0, up(2 * h.ghost * esz)
    total = up(signal + 2 * R.MAX_MSG * 4)
    ptr = C.c_void_p()
    if lib.lib.htfs_shared_alloc(total, 1, C.byref(ptr)) != 0:       # (no fine-grained memory: plain device memory, as brick.py)
        lib.check(lib.lib.htfs_shared_alloc(total, 0, C.byref(ptr)))
    state = torch.zeros(4, dtype=torch.int32, device=dev)
    p = lib.Peer()
    for m in range(h.g["n_msg"]):
        p.inbox[m], p.signal[m] = ptr.value + inbox, ptr.value + signal
    p.my_inbox, p.my_signal, p.state, p.spin_limit = ptr.value + inbox, ptr.value + signal, state.data_ptr(), 1 << 22
    return p, state, ptr.value


@pytest.mark.parametrize("dt", list(R.DTYPES))
@pytest.mark.parametrize("gid", ["slab3-w0", "slab3-w1-me0", "thin3x3"])
def test_peer_route_equals_direct(htf, cuda, gid, dt):
    """The rank as its own neighbor through the inbox: htfs_brick_pack_halo_peer then htfs_brick_unpack_halo on one stream, three
    exchanges (both inbox halves, both parities), then three more packed by htfs_brick_nve_halo_peer: the ghost region has the bits
    of the direct route every time, no timeout is counted or flagged.  The pack always precedes the unpack: nothing ever waits."""
    lib = htf._lib
    case = R.cases(gid, dt)["thresholds"]
    r = case.run()[-1]
    box = _box(lib)
    via, ref = Harness(htf, cuda, case, dt), Harness(htf, cuda, case, dt)
    peer, state, block = _peer(lib, via, cuda)
    try:
        force = _dyadic_forces(via, r)
        for h in (via, ref):
            h.load(r["pos"], r["vel"], r["counts"])
        ref.pack_halo(False, True)
        for exchange in range(1, 7):
            a, b = via.a, ref.a
            if exchange <= 3:
                if exchange > 1:     # other positions every time: the boundary rows drift by a dyadic step
                    for h in (via, ref):
                        h.a["pos"].t[:h.cap, :3] += 2.0 ** -5
                lib.check(lib.lib.htfs_brick_pack_halo_peer(C.byref(via.geom), a["pos"].ptr(), via.code, a["counts"].ptr(), C.byref(peer), via.s))
                ref.pack_halo(False, True)
            else:
                lib.check(lib.lib.htfs_brick_nve_halo_peer(C.byref(via.geom), a["pos"].ptr(), a["vel"].ptr(), force.data_ptr(), via.code, DT,
                                                           C.byref(box), a["counts"].ptr(), C.byref(peer), via.s))
                lib.check(lib.lib.htfs_brick_nve_halo(C.byref(ref.geom), b["pos"].ptr(), b["vel"].ptr(), force.data_ptr(), ref.code, DT,
                                                      C.byref(box), b["counts"].ptr(), None, ref.ghost_ptr(), ref.s))
            lib.check(lib.lib.htfs_brick_unpack_halo(C.byref(via.geom), a["pos"].ptr(), via.code, C.byref(peer), a["counts"].ptr(), via.s))
            via.sync_and_check_guards("peer exchange %d" % exchange)
            ref.sync_and_check_guards("direct exchange %d" % exchange)
            got, want = a["pos"].get(), b["pos"].get()
            assert _same(got[:via.cap], want[:via.cap]) and _same(a["vel"].get(), b["vel"].get())
            assert _same(got[via.cap:], want[via.cap:]), ("ghost region", exchange)
            assert np.isnan(want[via.cap:, 0]).any() and not np.isnan(want[via.cap:, 0]).all()
            st = state.cpu().numpy()
            assert st[0] == exchange and st[1] == 0 and st[2] == 0, st
            assert np.array_equal(a["counts"].get(), r["counts"]) and not int(r["counts"][R.BC_FLAGS]) & R.BF_HALO_TIMEOUT
    finally:
        torch.cuda.synchronize()
        lib.check(lib.lib.htfs_shared_free(block))


@pytest.mark.parametrize("gid,dt", R.case_ids(), ids=IDS)
def test_overflows(htf, cuda, gid, dt):
    """Each capacity overflowed by 1 and by 5 rows, alone.  What a flagged plan promises: exactly its flag; the clamped header count,
    N_INT, N_BND and MSG[m]; the first cap_int and cap_bnd rows of the class-sorted candidates placed; not a store outside the
    arrays, by the rebuild or by the halo pack and the row-slot table that follow it.  After a ghost overflow also the message -- its
    first ghost_cap[m] rows in class order -- and 0xFFFFFFFF in the row-slot table for the rows that were cut off.
    (A boundary overflow makes the halo pack READ pos[cap_int + n_bnd - 1], past the local rows: the overflow is at most 5 rows,
    fewer than the ghost region behind them.)"""
    over = _cases(gid, dt, lambda n: n.startswith("over_"))
    assert len(over) >= 6
    for case in over:
        r = case.run()[0]
        g = case.geom
        h = Harness(htf, cuda, case, dt)
        h.load(r["pos_in"], r["vel_in"])
        h.migrate_pack()
        h.deliver(r)
        h.migrate_merge()
        h.sync_and_check_guards("rebuild")
        assert R.header_view(h.a["mig_send"].get())[g["mig_off"][:g["n_msg"]]].tolist() == r["mig_counts"], case.name
        c = h.a["counts"].get()
        assert int(c[R.BC_FLAGS]) == case.flags == r["flags"], (case.name, int(c[R.BC_FLAGS]))
        for w in [R.BC_N_INT, R.BC_N_BND] + list(range(R.BC_MSG, R.BC_MSG + g["n_msg"])):
            assert c[w] == r["counts"][w], (case.name, w)
        assert int(c[R.BC_N_INT]) <= g["cap_int"] and int(c[R.BC_N_BND]) <= g["cap_bnd"]
        pos = h.a["pos"].get()
        assert _same(pos[:h.cap], r["pos"]) and _same(h.a["vel"].get(), r["vel"]), (case.name, "rows placed")
        ni, nb, n_int = int(c[R.BC_N_INT]), int(c[R.BC_N_BND]), int(r["counts"][R.BC_CLASS + 1])
        assert _same(pos[:ni], r["cand_pos"][:ni]) and _same(pos[g["cap_int"]:g["cap_int"] + nb], r["cand_pos"][n_int:n_int + nb])
        assert r["flags"] & R.BF_BND_OVERFLOW == 0 or R.cap(g) + 5 <= len(pos)
        h.pack_halo(True, False)
        h.row_slots()
        h.sync_and_check_guards("halo pack and row slots of a flagged plan")
        if case.flags == R.BF_GHOST_OVERFLOW:
            halo = h.a["halo"].get()
            assert _same(halo, r["halo_send"]), case.name
            for m in range(g["n_msg"]):
                rows = R.halo_rows(r["counts"], g, m)
                assert len(rows) <= g["ghost_cap"][m] and _same(halo[g["ghost_off"][m]:g["ghost_off"][m] + len(rows), 3], r["pos"][rows, 3])
            assert np.array_equal(h.a["row_slots"].get(), r["row_slots"]), case.name


def _mutations():
    def m(name, match, fn):
        return pytest.param(match, fn, id=name)

    def set_(**kw):
        def fn(b):
            for k, v in kw.items():
                setattr(b, k, v)
        return fn

    def item(field, i, v):
        def fn(b):
            getattr(b, field)[i] = v(getattr(b, field)[i]) if callable(v) else v
        return fn

    def both(*fns):
        def fn(b):
            for f in fns:
                f(b)
        return fn
    return [m("ndim1_with_8_messages", "messages", set_(n_msg=8)),
            m("ndim2_with_2_messages", "messages", set_(ndim=2)),
            m("one_brick", "bricks", item("p", 0, 1)),
            m("me_past_the_end", "coordinate", item("me", 0, 3)),
            m("me_negative", "coordinate", item("me", 0, -1)),
            m("mig_cap_1", "no room", both(item("mig_cap", 0, 1), item("mig_cap", 1, 1))),
            m("ghost_cap_0", "no room", both(item("ghost_cap", 0, 0), item("ghost_cap", 1, 0))),
            m("unequal_ghost_caps", "opposite", item("ghost_cap", 0, lambda v: v + 1)),
            m("unequal_mig_caps", "opposite", item("mig_cap", 1, lambda v: v + 1)),
            m("gap_between_migration_messages", "does not follow", item("mig_off", 1, lambda v: v + 1)),
            m("gap_between_halo_messages", "does not follow", item("ghost_off", 1, lambda v: v + 1)),
            m("first_message_not_at_row_0", "row 0", both(item("mig_off", 0, 1))),
            m("no_local_rows", "no local rows", set_(cap_int=0, cap_bnd=0))]


@pytest.mark.parametrize("match,mutate", _mutations())
def test_bad_geometry_is_refused(htf, cuda, match, mutate):
    """Every requirement of check_geom: each entry point raises ValueError, launches nothing and leaves every output its sentinel."""
    lib = htf._lib
    case = R.cases("slab3-w0", "f32")["thresholds"]
    r = case.run()[0]
    h = Harness(htf, cuda, case, "f32")
    h.load(r["pos_in"], r["vel_in"])
    before = {k: v.buf.view(torch.int32).clone() for k, v in h.a.items()}
    bad = h.brick(case.geom)
    mutate(bad)
    box, a = _box(lib), h.a
    force = torch.zeros((h.cap, 4), dtype=torch.float32, device=cuda)
    calls = [lambda: h.migrate_pack(bad), lambda: h.migrate_merge(True, bad), lambda: h.pack_halo(True, True, bad), lambda: h.row_slots(bad),
             lambda: lib.check(lib.lib.htfs_brick_nve_halo(C.byref(bad), a["pos"].ptr(), a["vel"].ptr(), force.data_ptr(), h.code, DT, C.byref(box),
                                                           a["counts"].ptr(), a["halo"].ptr(), h.ghost_ptr(), h.s))]
    for call in calls:
        with pytest.raises(ValueError, match=match):
            call()
    torch.cuda.synchronize()
    for k, v in h.a.items():
        assert torch.equal(v.buf.view(torch.int32), before[k]), k
