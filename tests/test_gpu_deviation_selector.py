"""htf.DeviationSelector on the MI355X (csrc/select.hip, include/htf_select.h) against tests/select_ref.SelectorRef.

Every comparison is exact: the selector compares and copies, it rounds nothing, and (s, a) is the greatest element of a total
order, the same whatever the grid.  Counters, s, argmax and stamp are compared as numbers, positions and boxes byte for byte.

The sequences are designed, not sampled: a frame's deviation is a seeded random column scaled below half of the frame's target
s, with the target written at chosen rows.  Before a case touches the GPU it asserts on the reference that it is not vacuous: all
three classes occur, candidates are dropped and, for policy "largest", frames are replaced and a replacement is refused on an
equal s."""
import numpy as np
import pytest
import torch

from select_ref import SelectorRef

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
LO, HI = 0.5, 2.0
# the target s of the 16 updates.  With hi = 2: 2.0 and +inf fail; with hi = inf both are candidates.  0.5 is lo exactly (a
# candidate), 0.25 and 0.125 are accurate, the NaN frame fails.  Worked through for capacity 1 and 3 in test_select_ref_cpu's
# manner: "largest" replaces in every combination and meets an s equal to its smallest stored one (update 6, 12, 14 or 15).
TARGETS = (1.0, 0.25, LO, 0.75, HI, NAN, LO, 1.5, INF, 1.0, 0.125, 1.75, 1.0, 1.0, 1.75, INF)
DUPLICATED = (7, 8, 12)      # updates whose maximum stands at three rows (N permitting)

NP_DTYPE = {torch.float32: np.float32, torch.float64: np.float64}


def _sequence(N, column, dtype, targets=TARGETS, seed=0):
    """[(deviation [N, 2] fp32, positions [N, 4], box [3, 3])] with max / NaN of `column` as designed; the other column holds
    values on every side of the thresholds (a NaN among them) that must not matter."""
    rng = np.random.default_rng(1000 * N + seed)
    frames = []
    for k, t in enumerate(targets):
        d = np.empty((N, 2), np.float32)
        d[:, 1 - column] = 3.0 * rng.random(N, dtype=np.float32)
        d[rng.integers(N), 1 - column] = NAN if k % 3 == 0 else INF
        if np.isnan(t):
            d[:, column] = 100.0 * rng.random(N, dtype=np.float32)
            d[min(5, N - 1), column] = NAN
            d[min(2, N - 1), column] = NAN
        else:
            scale = np.float32(0.5 * t) if np.isfinite(t) else np.float32(1e30)
            d[:, column] = scale * rng.random(N, dtype=np.float32)
            # the row of the maximum: the last row, the first, then anywhere (N = 1300 under max_blocks = 2: every trip of the stride)
            at = N - 1 if k == 0 else 0 if k == 2 else N // 4 if k in DUPLICATED else int(rng.integers(N))
            d[at, column] = t
            if k in DUPLICATED:       # N = 1300: rows 325, 975 and 1299, one in each trip of two blocks
                d[at + N // 2, column] = t
                d[N - 1, column] = t
        pos = rng.standard_normal((N, 4)).astype(dtype)
        pos[:, 3] = np.arange(N) % 3
        L = dtype(5.0 + 0.25 * k)
        box = np.array([[-L / 2] * 3, [L / 2] * 3, [0, 0, 0]], dtype)
        frames.append((d, pos, box))
    return frames


def _reference(N, capacity, hi, quantity, policy, dtype, frames):
    ref = SelectorRef(N, capacity, LO, hi, quantity=quantity, policy=policy, dtype=dtype)
    lasts = []
    for d, p, b in frames:
        ref.update(d, p, b)
        lasts.append(ref.last.copy())
    return ref, lasts


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_equal(sel, ref):
    assert sel.counts() == ref.counts()
    got, want = sel.frames(), ref.frames()
    assert np.array_equal(got["stamp"], want["stamp"]) and np.array_equal(got["argmax"], want["argmax"])
    assert _same_bytes(got["s"], want["s"])
    assert _same_bytes(got["positions"], want["positions"]) and _same_bytes(got["box"], want["box"])


def _feed(sel, frames, lasts, cuda):
    for (d, p, b), last in zip(frames, lasts):
        assert sel.update(torch.from_numpy(d).to(cuda), torch.from_numpy(p).to(cuda), torch.from_numpy(b).to(cuda)) is None
        got = sel.last.cpu().numpy()
        assert np.array_equal(got, last, equal_nan=True), (got, last)


# (N, max_blocks): 1 300 rows are six blocks by default and, under max_blocks = 2, two blocks of three trips each
SHAPES = [(1, None), (63, None), (64, None), (65, None), (257, None), (1300, 2), (1300, None)]
KINDS = [("force", torch.float32, HI), ("energy", torch.float64, INF), ("force", torch.float64, INF), ("energy", torch.float32, HI)]


@pytest.mark.parametrize("quantity,dtype,hi", KINDS)
@pytest.mark.parametrize("policy", ["first", "largest"])
@pytest.mark.parametrize("capacity", [1, 3])
@pytest.mark.parametrize("N,max_blocks", SHAPES)
def test_sequences(htf, cuda, N, max_blocks, capacity, policy, quantity, dtype, hi):
    column = 0 if quantity == "force" else 1
    frames = _sequence(N, column, NP_DTYPE[dtype])
    ref, lasts = _reference(N, capacity, hi, quantity, policy, NP_DTYPE[dtype], frames)
    # not vacuous, on the reference alone
    c = ref.counts()
    assert 12 <= len(frames) <= 16 and set(ref.classes) == {"accurate", "candidate", "failed"}
    assert c["dropped"] > 0 and c["stored"] == capacity and c["seen"] == c["accurate"] + c["candidate"] + c["failed"]
    assert c["candidate"] == c["stored"] + c["replaced"] + c["dropped"]
    if policy == "largest":
        assert c["replaced"] > 0 and ref.refused_equal > 0
    assert ref.classes[2] == "candidate" and lasts[2][0] == np.float32(LO)                 # s = lo exactly
    assert ref.classes[4] == ("failed" if hi == HI else "candidate") and lasts[4][0] == np.float32(HI)   # s = hi exactly
    assert ref.classes[8] == ("failed" if hi == HI else "candidate") and np.isinf(lasts[8][0])
    assert np.isnan(lasts[5][0]) and lasts[5][1] == min(2, N - 1) and ref.classes[5] == "failed"
    for k in DUPLICATED:
        col = frames[k][0][:, column]
        if N >= 3:
            assert (col == col.max()).sum() == 3
        assert lasts[k][1] == np.flatnonzero(col == col.max())[0]

    sel = htf.DeviationSelector(N, capacity, LO, hi, quantity=quantity, policy=policy, dtype=dtype, max_blocks=max_blocks)
    assert sel.last.is_cuda and sel.last.shape == (2,) and sel.last.dtype == torch.float32
    _feed(sel, frames, lasts, cuda)
    _assert_equal(sel, ref)
    # reset() and the same sequence: the same result
    sel.reset()
    assert sel.counts() == dict.fromkeys(c, 0) and sel.frames()["positions"].shape == (0, N, 4)
    assert sel.last.cpu().tolist() == [0.0, 0.0]
    _feed(sel, frames, lasts, cuda)
    _assert_equal(sel, ref)


def test_grid_does_not_matter(htf, cuda):
    """(s, a) under max_blocks = 1, 2, 3, 5 and the default on 1 300 rows, maxima duplicated across the trips: the same bits."""
    N = 1300
    d = np.random.default_rng(5).random((N, 2), dtype=np.float32)
    d[[300, 700, 1299], 0] = 2.5
    d[[1290, 40], 1] = NAN
    dev, pos = torch.from_numpy(d).to(cuda), torch.zeros((N, 4), device=cuda)
    for quantity, want in (("force", [2.5, 300.0]), ("energy", [NAN, 40.0])):
        for mb in (1, 2, 3, 5, None):
            sel = htf.DeviationSelector(N, 1, 0.0, quantity=quantity, max_blocks=mb)
            sel.update(dev, pos)
            assert np.array_equal(sel.last.cpu().numpy(), np.array(want, np.float32), equal_nan=True), (quantity, mb)


def test_box_none_and_positions_input(htf, cuda):
    """box=None stores zeros; the PositionsInput that compute receives is taken as the tensor it is."""
    from hoomd_tf_amd.simmodel import PositionsInput
    N = 65
    (d, p, b), = _sequence(N, 0, np.float32, targets=(1.0,))
    sel = htf.DeviationSelector(N, 2, LO)
    sel.update(torch.from_numpy(d).to(cuda), PositionsInput.wrap(torch.from_numpy(p).to(cuda)))
    f = sel.frames()
    assert _same_bytes(f["positions"], p[None]) and _same_bytes(f["box"], np.zeros((1, 3, 3), np.float32))
    with pytest.raises(ValueError, match="box"):
        sel.trajectory()     # (no box lengths: ArrayTrajectory refuses them)


def test_error_paths(htf, cuda):
    N = 8
    sel = htf.DeviationSelector(N, 2, LO)
    dev, pos, box = torch.zeros((N, 2), device=cuda), torch.zeros((N, 4), device=cuda), torch.zeros((3, 3), device=cuda)
    wide = torch.zeros((N, 8), device=cuda)
    for bad in (dict(deviation=torch.zeros((N, 3), device=cuda)), dict(deviation=torch.zeros((N,), device=cuda)),
                dict(deviation=dev.double()), dict(deviation=dev.cpu()), dict(deviation=wide[:, :2]),
                dict(deviation=torch.zeros((N + 1, 2), device=cuda), positions=torch.zeros((N + 1, 4), device=cuda)),
                dict(positions=torch.zeros((N, 3), device=cuda)), dict(positions=torch.zeros((N - 1, 4), device=cuda)),
                dict(positions=pos.double()), dict(positions=pos.cpu()), dict(positions=wide[:, :4]),
                dict(positions=torch.zeros((4, N), device=cuda).t()), dict(positions=pos.cpu().numpy()),
                dict(box=box.double()), dict(box=box.cpu()), dict(box=torch.zeros((3, 4), device=cuda)), dict(box=torch.zeros(9, device=cuda)),
                dict(box=torch.zeros((3, 6), device=cuda)[:, ::2])):
        a = dict(dict(deviation=dev, positions=pos, box=box), **bad)
        with pytest.raises(ValueError, match="DeviationSelector.update"):
            sel.update(a["deviation"], a["positions"], a["box"])
    with pytest.raises(ValueError, match="n_particles = 8"):
        sel.update(torch.zeros((N + 1, 2), device=cuda), torch.zeros((N + 1, 4), device=cuda))
    sel64 = htf.DeviationSelector(N, 2, LO, dtype=torch.float64)
    with pytest.raises(ValueError, match="float64"):
        sel64.update(dev, pos, box.double())
    with pytest.raises(ValueError, match="float64"):
        sel64.update(dev, pos.double(), box)
    # nothing of the above reached the device
    assert sel.counts()["seen"] == 0 and sel64.counts()["seen"] == 0
    with pytest.raises(ValueError, match="no frame is stored"):
        sel.trajectory()
    # a tilted box is stored as it is and refused by trajectory()
    tilted = torch.tensor([[0.0, 0, 0], [4.0, 4, 4], [0.0, 0.5, 0]], device=cuda)
    one = torch.ones((N, 2), device=cuda)
    sel.update(one, pos, tilted)
    assert np.array_equal(sel.frames()["box"][0], tilted.cpu().numpy())
    with pytest.raises(ValueError, match="tilt"):
        sel.trajectory()


def test_replay(htf, cuda):
    """One update captured on static buffers -- a single chain of three kernels, no forked stream -- and replayed six times with
    new contents copied in between: SelectorRef fed the same six frames.  A capture admits neither a synchronisation nor an
    allocation, so update has neither."""
    N, capacity = 300, 2
    frames = _sequence(N, 0, np.float32, targets=(1.0, 0.25, 0.75, 1.5, NAN, 0.75), seed=1)
    ref, lasts = _reference(N, capacity, HI, "force", "largest", np.float32, frames)
    assert ref.counts()["replaced"] > 0 and ref.counts()["dropped"] > 0 and set(ref.classes) == {"accurate", "candidate", "failed"}
    sel = htf.DeviationSelector(N, capacity, LO, HI, policy="largest")
    dev, pos, box = torch.zeros((N, 2), device=cuda), torch.zeros((N, 4), device=cuda), torch.zeros((3, 3), device=cuda)
    sel.update(dev, pos, box)      # (the kernels' code objects load here, not under capture)
    sel.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sel.update(dev, pos, box)
    assert sel.counts()["seen"] == 0    # a capture records, it does not run
    for (d, p, b), last in zip(frames, lasts):
        dev.copy_(torch.from_numpy(d))
        pos.copy_(torch.from_numpy(p))
        box.copy_(torch.from_numpy(b))
        g.replay()
        assert np.array_equal(sel.last.cpu().numpy(), last, equal_nan=True)
    _assert_equal(sel, ref)


# ------------------------------------------------------------------------------------------------ through tfcompute
_RUN = {}


def _nve_run(htf, cuda):
    """Six NVE steps of 500 particles under a committee of 3 (test_gpu_desc_committee.test_nve_through_tfcompute), the model
    calling two selectors after the forces: lo = 0, hi = inf, capacity 4, "first" -- every frame a candidate -- and one whose lo
    lies above every deviation.  Run once, read by the two tests below."""
    if _RUN:
        return _RUN
    from test_gpu_desc_committee import _committee
    from test_gpu_desc_total import _sim
    lay = _committee(htf, 3, K=16, high=2.0, r_cut=2.0, seed=71)
    sim, sysm, L = _sim(htf, cuda, 73)
    sel = htf.DeviationSelector(sysm.N, 4, 0.0, policy="first")
    sel_high = htf.DeviationSelector(sysm.N, 4, 1e30, policy="first")

    class M(htf.SimModel):
        def setup(self):
            self.desc = lay
            self.positions, self.deviations, self.boxes = [], [], []

        def compute(self, nlist, positions, box):
            f = htf.compute_nlist_forces(nlist, self.desc(nlist, positions))
            self.positions.append(positions.detach().clone())
            self.deviations.append(self.desc.deviation.detach().clone())
            self.boxes.append(box.detach().clone())
            sel.update(self.desc.deviation, positions, box)
            sel_high.update(self.desc.deviation, positions, box)
            return f

    model = M(128)
    tfc = htf.tfcompute(model)
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    sim.run(6)
    torch.cuda.synchronize()
    _RUN.update(lay=lay, sysm=sysm, L=L, sel=sel, sel_high=sel_high, model=model)
    return _RUN


def test_through_tfcompute(htf, cuda):
    from test_gpu_desc_committee import _check_against
    from test_gpu_desc_total import _descriptor, _network
    r = _nve_run(htf, cuda)
    lay, sysm, L, sel, model = r["lay"], r["sysm"], r["L"], r["sel"], r["model"]
    assert len(model.positions) == 6
    c = sel.counts()
    assert (c["stored"], c["dropped"], c["candidate"], c["seen"], c["replaced"]) == (4, 2, 6, 6, 0)
    f = sel.frames()
    assert f["stamp"].tolist() == [0, 1, 2, 3]
    for k in range(4):
        assert _same_bytes(f["positions"][k], model.positions[k].cpu().numpy())
        assert _same_bytes(f["box"][k], model.boxes[k].cpu().numpy())
        col = model.deviations[k][:, 0]
        assert f["s"][k] == col.max().item() and f["argmax"][k] == int(torch.nonzero(col == col.max())[0, 0])
    assert not _same_bytes(f["positions"][0], f["positions"][3])      # the particles moved
    last = model.deviations[5][:, 0]
    assert sel.last.cpu().tolist() == [last.max().item(), float(torch.nonzero(last == last.max())[0, 0])]
    # the selector does not disturb the step: the last forces are the mean over the members of the all-pairs fp64 gradient
    force = sysm.force[:sysm.N].double()
    Fm, Em = [], []
    for m in range(3):
        q = model.positions[5][:, :3].double().requires_grad_(True)
        d = q[None, :, :] - q[:, None, :]
        d = d - L * torch.round(d.detach() / L)
        off = ~torch.eye(sysm.N, dtype=torch.bool, device=cuda)
        one = lay.member(m)
        G = _descriptor(one, d * off[..., None].to(d.dtype), torch.zeros((sysm.N, sysm.N), dtype=torch.float64, device=cuda))[0]
        E = _network(one, G, torch.zeros(sysm.N, dtype=torch.long, device=cuda))
        (g,) = torch.autograd.grad(E.sum(), q)
        Fm.append(-g)
        Em.append(E.detach())
    _check_against(force, model.deviations[5], torch.stack(Fm), torch.stack(Em))
    # select -> (label) -> train offline: the stored frames as a trajectory
    items = list(htf.iter_from_trajectory(128, sel.trajectory(), r_cut=2.5))
    assert len(items) == 4
    for k, ((nlist, positions, box), ts) in enumerate(items):
        assert ts.frame == k and positions.shape == (sysm.N, 4) and nlist.shape == (sysm.N, 128, 4)
        assert _same_bytes(positions[:, :3].cpu().numpy(), np.ascontiguousarray(f["positions"][k][:, :3]))
        assert torch.equal(positions[:, 3].cpu(), model.positions[0][:, 3].cpu())
        assert box[1].cpu().tolist() == (model.boxes[k][1] - model.boxes[k][0]).cpu().tolist()


def test_through_tfcompute_all_accurate(htf, cuda):
    r = _nve_run(htf, cuda)
    sel = r["sel_high"]
    assert max(d[:, 0].max().item() for d in r["model"].deviations) < sel.lo
    c = sel.counts()
    assert (c["accurate"], c["stored"], c["seen"], c["candidate"], c["failed"]) == (6, 0, 6, 0, 0)
    assert sel.frames()["positions"].shape == (0, r["sysm"].N, 4)
    with pytest.raises(ValueError, match="no frame is stored"):
        sel.trajectory()
