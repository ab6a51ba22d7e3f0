"""The check step without its check launch: the integrator of the step before it fills the displacement word
(``htfs_nve_step_check`` / ``nve_check_kernel``), the check is the five gated launches alone (``htfs_rebuild_nlist_gated``), and the
two status words ride to the host on the check step's force launch (the step epilogue's mail) where they had a copy of their own.

Kernel level: route A is what the step did before -- ``htfs_nve_step``, then ``htfs_check_rebuild_nlist`` -- route B the two new
calls, on copies of the same state; everything either leaves behind must be equal bit for bit, the displacement word also to
``htfs_max_displacement2`` on the stored positions.  Step level: ``FusedStep`` with and without ``HTF_NO_CHECK_IN_STEP=1``.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import ROOT
from test_check_step_launches import (COARSE, FINE, DTYPES, _List, _assert_clean, _check_new, _pair, _positions, _same, _stream,
                                      _word_ref)

DT = 0.05


class _State:
    """Positions, velocities and forces of one route; the velocities move a row by up to ``DT`` per axis and step."""

    def __init__(self, pos, rng, dtype, dev, force_scale=0.1):
        n = pos.shape[0]
        mk = lambda a: torch.tensor(np.concatenate([a, np.zeros((n, 1))], axis=1), dtype=dtype, device=dev)  # noqa: E731
        self.pos = pos.clone()
        self.vel = mk(rng.uniform(-1.0, 1.0, (n, 3)))
        self.force = mk(rng.uniform(-force_scale, force_scale, (n, 3)))

    def copy(self):
        c = object.__new__(_State)
        c.pos, c.vel, c.force = self.pos.clone(), self.vel.clone(), self.force.clone()
        return c


def _nve(htf, l, st, dt=DT):
    htf._lib.check(htf._lib.lib.htfs_nve_step(st.pos.data_ptr(), st.vel.data_ptr(), st.force.data_ptr(), l.code, l.N, float(dt),
                                              C.byref(l.desc.box), _stream(htf, l.dev)))


def _nve_check(htf, l, st, dt=DT):
    htf._lib.check(htf._lib.lib.htfs_nve_step_check(st.pos.data_ptr(), st.vel.data_ptr(), st.force.data_ptr(), l.code, l.N, float(dt),
                                                    C.byref(l.desc.box), C.byref(l.desc), l.disp.data_ptr(), _stream(htf, l.dev)))


def _gated(htf, l, pos, thr2, clean, h_stat=None, by_mail=False):
    htf._lib.check(htf._lib.lib.htfs_rebuild_nlist_gated(C.byref(l.desc), pos.data_ptr(), l.code, l.N, l.Ntot, int(clean), l.disp.data_ptr(),
                                                         float(thr2), l.stat.data_ptr(), None if h_stat is None else h_stat.data_ptr(),
                                                         int(by_mail), _stream(htf, l.dev)))


def _route_a(htf, l, st, thr2, clean, dt=DT):
    """The step as it was: integrator, then the check that measures for itself.  -> the word htfs_max_displacement2 finds."""
    _nve(htf, l, st, dt)
    word = _word_ref(htf, l, st.pos)
    _check_new(htf, l, st.pos, thr2, clean=clean)
    return word


def _route_b(htf, l, st, thr2, clean, dt=DT):
    """The integrator that measures, then the gated launches alone.  The work words are zero before and must be zero behind the
    integrator's launch already."""
    _nve_check(htf, l, st, dt)
    torch.cuda.synchronize()
    assert int(l.work().abs().sum()) == 0, "work words left dirty by the integrator's launch"
    word = np.float32(l.disp.item())
    _gated(htf, l, st.pos, thr2, clean)
    return word


def _bits(t):
    return t.view(torch.uint8) if t.is_floating_point() else t


def _same_route(a, b, la, lb, what=""):
    assert torch.equal(_bits(a.pos), _bits(b.pos)), "positions differ " + what
    assert torch.equal(_bits(a.vel), _bits(b.vel)), "velocities differ " + what
    sa, sb = la.state(), lb.state()
    for k in sa:
        assert torch.equal(_bits(sa[k]), _bits(sb[k])), "%s differs %s" % (k, what)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("N,grid,pitch", [(1, COARSE, 8), (1000, FINE, 64), (1025, FINE, 64), (4097, FINE, 128)],
                         ids=["n1", "n1000", "n1025", "n4097"])
def test_same_bits_as_integrator_then_check(htf, cuda, dtype, N, grid, pitch):
    """N = 1 and 1000: the one block's ticket is the last; 1025: a second, nearly empty block; 4097: five."""
    rng = np.random.default_rng(100 + N)
    ref, pos = _positions(rng, N, grid[2], dtype, cuda)
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    a = _State(pos, rng, dtype, cuda)
    b = a.copy()
    word_a = _route_a(htf, old, a, 0.0, clean=False)
    # (garbage in the counts and cursors: the gated call zeroes what it needs zero; the work words are the integrator's to find zero)
    new.scratch[2 * new.ncell: 2 * new.ncell + 2] = 0
    word_b = _route_b(htf, new, b, 0.0, clean=False)
    assert word_a > 0 and word_b.tobytes() == word_a.tobytes()
    _same_route(a, b, old, new)
    assert int(new.stat[1]) == 1 and int(new.stat[0]) <= pitch
    _assert_clean(new)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_gate_just_closed_and_just_open(htf, cuda, dtype):
    """The threshold AT the published word holds the rebuild back and nothing is touched; one ulp below opens it: route A's state."""
    N, grid, pitch = 1025, FINE, 64
    rng = np.random.default_rng(13)
    ref, pos = _positions(rng, N, grid[2], dtype, cuda)
    st = _State(pos, rng, dtype, cuda)
    probe_l, _ = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    probe = st.copy()
    _nve(htf, probe_l, probe)
    word = _word_ref(htf, probe_l, probe.pos)
    assert word > 0
    # closed
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    b = st.copy()
    new.scratch[: 2 * new.ncell + 2] = 0
    before = new.state()
    scratch_before = new.scratch.clone()
    assert _route_b(htf, new, b, float(word), clean=True).tobytes() == word.tobytes()
    after = new.state()
    assert np.float32(after.pop("disp").item()) == word
    before.pop("disp")
    _same(after, before, "after a closed check")
    assert torch.equal(new.scratch, scratch_before) and torch.equal(new.cell_of, torch.full_like(new.cell_of, -7))
    assert torch.equal(b.pos, probe.pos) and torch.equal(b.vel, probe.vel)
    # open, from the same start
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    a, b = st.copy(), st.copy()
    below = float(np.nextafter(word, np.float32(0.0)))
    assert _route_a(htf, old, a, below, clean=False) == word
    new.scratch[: 2 * new.ncell + 2] = 0
    _route_b(htf, new, b, below, clean=True)
    _same_route(a, b, old, new, "after an open check")
    assert int(new.stat[1]) == 1
    _assert_clean(new)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_three_periods_on_one_list(htf, cuda, dtype):
    """Open, closed, open on one list with nothing zeroed from the host in between: the integrator's launch and the gated launches
    leave work words and counts clean every time."""
    N, grid, pitch = 4097, FINE, 128
    rng = np.random.default_rng(14)
    ref, pos = _positions(rng, N, grid[2], dtype, cuda)
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    a = _State(pos, rng, dtype, cuda, force_scale=0.0)
    b = a.copy()
    new.scratch[: 2 * new.ncell + 2] = 0
    # rows move by dt * v, |v| <= 1 per axis: 0.01 sqrt(3) from the new reference positions stays under 0.2, 0.21 of some row's does not
    thr = 0.04
    expect = []
    for k, (dt, thr2) in enumerate(((0.05, 0.0), (0.01, thr), (0.2, thr))):
        word_a = _route_a(htf, old, a, thr2, clean=(k > 0), dt=dt)
        word_b = _route_b(htf, new, b, thr2, clean=True, dt=dt)
        assert word_b.tobytes() == word_a.tobytes()
        _same_route(a, b, old, new, "after period %d" % k)
        _assert_clean(new)
        expect.append(bool(word_a > np.float32(thr2)))
    assert expect == [True, False, True] and int(new.stat[1]) == 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_inert_rows(htf, cuda, dtype):
    """Rows whose x is NaN, in the middle and as the one row of the last block: they have not moved, the word is finite and route A's."""
    N, grid, pitch = 1025, FINE, 64
    rng = np.random.default_rng(17)
    ref, pos = _positions(rng, N, grid[2], dtype, cuda)
    pos[100:130, 0] = float("nan")
    ref[100:130, 0] = float("nan")
    pos[1024, 0] = float("nan")
    new, old = _pair(htf, cuda, dtype, N, N, grid, pitch, ref)
    a = _State(pos, rng, dtype, cuda)
    a.vel[100:130] = 0
    a.vel[1024] = 0
    b = a.copy()
    word_a = _route_a(htf, old, a, 0.0, clean=False)
    new.scratch[2 * new.ncell: 2 * new.ncell + 2] = 0
    word_b = _route_b(htf, new, b, 0.0, clean=False)
    assert word_a > 0 and np.isfinite(word_b) and word_b.tobytes() == word_a.tobytes()
    _same_route(a, b, old, new)
    _assert_clean(new)
    assert int(new.cell_start[-1]) == N - 31


def test_argument_checks_without_a_gpu(htf, tmp_path):
    """A stand-alone host program on the new entries: null pointers are refused before anything is launched, N = 0 is a no-op."""
    src = tmp_path / "t.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "htf_standin.h"
int main(void) {
    htfs_nlist nl;
    htf_box box;
    float word = 0.f;
    unsigned stat[2] = {0u, 0u}, scratch[64];
    char pos[64] = {0}, ref[64] = {0};
    int bad = 0;
    memset(&nl, 0, sizeof nl);
    memset(&box, 0, sizeof box);
    memset(scratch, 0, sizeof scratch);
    box.hi[0] = box.hi[1] = box.hi[2] = 1.0;
    nl.box = box;
    nl.ncell3[0] = nl.ncell3[1] = nl.ncell3[2] = 1;
    bad += htfs_nve_step_check(NULL, pos, pos, HTF_F32, 1, 0.1, &box, &nl, &word, NULL) == HTF_OK;
    bad += htfs_nve_step_check(pos, pos, pos, HTF_F32, 1, 0.1, &box, NULL, &word, NULL) == HTF_OK;
    bad += htfs_nve_step_check(pos, pos, pos, HTF_F32, 1, 0.1, &box, &nl, NULL, NULL) == HTF_OK;
    bad += htfs_nve_step_check(pos, pos, pos, HTF_F32, 1, 0.1, &box, &nl, &word, NULL) == HTF_OK;   /* no ref, no scratch */
    bad += htfs_rebuild_nlist_gated(NULL, pos, HTF_F32, 1, 1, 1, &word, 0.0, stat, NULL, 0, NULL) == HTF_OK;
    bad += htfs_rebuild_nlist_gated(&nl, pos, HTF_F32, 1, 1, 1, &word, 0.0, stat, NULL, 0, NULL) == HTF_OK;  /* no ref, no scratch */
    nl.ref = ref;
    nl.scratch = scratch;
    bad += htfs_nve_step_check(pos, pos, pos, 77, 1, 0.1, &box, &nl, &word, NULL) == HTF_OK;        /* bad dtype */
    bad += htfs_rebuild_nlist_gated(&nl, NULL, HTF_F32, 1, 1, 1, &word, 0.0, stat, NULL, 0, NULL) == HTF_OK;
    bad += htfs_rebuild_nlist_gated(&nl, pos, HTF_F32, 1, 1, 1, NULL, 0.0, stat, NULL, 0, NULL) == HTF_OK;
    bad += htfs_rebuild_nlist_gated(&nl, pos, HTF_F32, 1, 1, 1, &word, 0.0, NULL, NULL, 0, NULL) == HTF_OK;
    bad += htfs_nve_step_check(pos, pos, pos, HTF_F32, 0, 0.1, &box, &nl, &word, NULL) != HTF_OK;   /* N = 0: nothing to do */
    bad += htfs_rebuild_nlist_gated(&nl, pos, HTF_F32, 0, 0, 1, &word, 0.0, stat, NULL, 1, NULL) != HTF_OK;
    printf("%d\n", bad);
    return bad;
}
''')
    exe = tmp_path / "t"
    lib_dir = os.path.dirname(htf._lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lhtf_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.check_output([str(exe)], text=True, timeout=120).split() == ["0"]


# ---------------------------------------------------------------------------------------------------------------- step level
def _system(htf, dev, r_buff, period, dtype=torch.float32, kT=1.2, jitter=0.03):
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(6, 0.8442)          # 4 * 6^3 = 864 particles
    rng = np.random.default_rng(21)
    pos = pos + jitter * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    sysm = standin.System(pos, L, dtype=dtype, device=dev)
    sysm.randomize_velocities(kT=kT, seed=5)
    nl = standin.CellNlist(sysm, r_cut=2.5, r_buff=r_buff, check_period=period, device_decision=True)
    nl.build()
    ctx = htf.Context(r_cut=2.5, nneighs=96, scalar_dtype=dtype, max_n=sysm.N, fused=2)
    ctx.set_potential(htf.Potential.lj())
    fs = standin.FusedStep(sysm, nl, ctx, standin.NVE(sysm, 0.004))
    return sysm, nl, ctx, fs


@pytest.mark.gpu
def test_status_words_ride_on_the_force_launch(htf, cuda):
    """After an open check the pinned pair is the device pair -- delivered by the check step's FORCE launch: the pair is overwritten
    from the host between the check's enqueue and that launch -- and after a closed one it is unchanged."""
    sysm, nl, ctx, fs = _system(htf, cuda, r_buff=0.08, period=5)
    assert fs.available and fs._mail_ok
    for ts in range(5):
        fs.step(ts)
    assert nl._armed is not None and nl._armed[0] == 5 and nl._armed[1]
    torch.cuda.synchronize()
    assert int(nl._stat[1]) == 0                       # (the check of step 0 found nothing moved)
    nl.compute(5)
    assert nl._armed is None and nl._mail_pending == 5    # the gated launches alone, no copy
    nl._stat_host.fill_(-1)
    fs.forces_and_integrate(5)
    torch.cuda.synchronize()
    k_words = nl._stat.cpu().clone()
    assert int(k_words[1]) == 1 and 0 < int(k_words[0]) <= nl.pitch and torch.equal(nl._stat_host, k_words)
    sysm.vel.zero_()                                   # nothing moves r_buff / 2 in the next five steps
    for ts in range(6, 10):
        fs.step(ts)
    nl.compute(10)
    assert nl._mail_pending == 10
    fs.forces_and_integrate(10)
    torch.cuda.synchronize()
    assert torch.equal(nl._stat.cpu(), k_words) and torch.equal(nl._stat_host, k_words)


@pytest.mark.gpu
def test_row_overflow_is_reported_at_the_next_check(htf, cuda):
    """A pitch set too small: the check of step 5 overflows its rows, its force launch delivers the words, the check of step 10 raises."""
    sysm, nl, ctx, fs = _system(htf, cuda, r_buff=0.08, period=5)
    nl.pitch = 8                                       # pretend the rows were sized far too small (empty rows until the rebuild)
    nl.n_neigh = torch.zeros(sysm.N, dtype=torch.int32, device=cuda)
    nl.head_list = torch.zeros(sysm.N, dtype=torch.int32, device=cuda)
    nl.nlist = torch.zeros(sysm.N * 8, dtype=torch.int32, device=cuda)
    for ts in range(5):
        fs.step(ts)
    nl.compute(5)
    assert nl._mail_pending == 5
    fs.forces_and_integrate(5)
    for ts in range(6, 10):
        fs.step(ts)
    with pytest.raises(RuntimeError, match="row overflow"):
        nl.compute(10)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_a_position_written_behind_the_arming_step_is_measured(htf, cuda):
    """The word the integrator left is for the positions IT stored: a write into them afterwards, and the check measures again."""
    sysm, nl, ctx, fs = _system(htf, cuda, r_buff=0.4, period=5, kT=0.5)
    for ts in range(5):
        fs.step(ts)
    assert nl._armed is not None
    torch.cuda.synchronize()
    assert nl.device_builds() == 0                     # (0.2 in five steps of 0.004 takes a velocity of 10)
    row = int(torch.argmin(sysm.pos[:, 0]))
    sysm.pos[row, 0] += 0.3                            # in place, far enough to trip the check, still inside the box
    nl.compute(5)
    assert nl._mail_pending is None                    # the full form: it measured, and copied its words
    fs.forces_and_integrate(5)
    torch.cuda.synchronize()
    assert nl.device_builds() == 1
    # ... and without the write the armed form is taken and nothing is rebuilt
    for ts in range(6, 10):
        fs.step(ts)
    nl.compute(10)
    assert nl._mail_pending == 10
    fs.forces_and_integrate(10)
    torch.cuda.synchronize()
    assert nl.device_builds() == 1
    # a capture never takes the armed form (a replayed period always measures what it finds), nor does another timestep or a build
    for ts in range(11, 15):
        fs.step(ts)
    state = nl._armed
    assert state is not None and state[0] == 15
    nl._capturing = True
    assert nl._take_armed(15) is None
    nl._capturing = False
    nl._armed = state
    assert nl._take_armed(16) is None
    nl._armed = state
    nl.build()
    assert nl._armed is None


_CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import hoomd_tf_amd as htf
from hoomd_tf_amd import standin
period, out = int(sys.argv[2]), sys.argv[3]
dev = torch.device("cuda:0")
pos, L, a = standin.fcc_positions(6, 0.8442)
rng = np.random.default_rng(21)
pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
pos -= np.round(pos / L) * L
sysm = standin.System(pos, L, dtype=torch.float32, device=dev)
sysm.randomize_velocities(kT=1.2, seed=5)
nl = standin.CellNlist(sysm, r_cut=2.5, r_buff=0.05, check_period=period, device_decision=True)
nl.build()
ctx = htf.Context(r_cut=2.5, nneighs=96, scalar_dtype=torch.float32, max_n=sysm.N, fused=2)
ctx.set_potential(htf.Potential.lj())
fs = standin.FusedStep(sysm, nl, ctx, standin.NVE(sysm, 0.004))
assert fs.available
armed = 0
for ts in range(20):
    armed += int(nl._armed is not None)
    fs.step(ts)
torch.cuda.synchronize()
torch.save(dict(pos=sysm.pos.cpu(), vel=sysm.vel.cpu(), force=sysm.force.cpu(), n_neigh=nl.n_neigh.cpu(),
                builds=nl.device_builds(), armed=armed), out)
'''


def _child_run(tmp_path, period, no_check_in_step):
    out = tmp_path / ("p%d_%d.pt" % (period, int(no_check_in_step)))
    env = dict(os.environ)
    env.pop("HTF_NO_CHECK_IN_STEP", None)
    if no_check_in_step:
        env["HTF_NO_CHECK_IN_STEP"] = "1"
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(period), str(out)], env=env, check=True, timeout=300)
    return torch.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("period,armed_checks", [(5, 3), (4, 0)], ids=["odd", "even"])
def test_trajectory_equals_the_one_with_a_check_launch(cuda, tmp_path, period, armed_checks):
    """20 steps with rebuilds in two fresh processes, with and without HTF_NO_CHECK_IN_STEP=1: the same bits.  Period 5: the checks of
    steps 5, 10 and 15 find their word armed; period 4 (even: the step before a check is a one-launch step): the path is not taken."""
    new = _child_run(tmp_path, period, False)
    old = _child_run(tmp_path, period, True)
    assert new["armed"] == armed_checks and old["armed"] == 0
    assert new["builds"] == old["builds"] and new["builds"] >= 2
    for k in ("pos", "vel", "force", "n_neigh"):
        assert torch.equal(new[k], old[k]), k
