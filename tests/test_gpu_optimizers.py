"""The device optimizers (``htf_optimizer_step``: one thread, P <= 8; ``htf_optimizer_step_n``: one thread per parameter, any P)
against tests/optimizer_ref.py, step by step: theta, m, v and every scalar of the state after EVERY step.

The float64 rule restarts each step from the device's own theta (read back), so that errors of theta do not accumulate; m and v
run free in float64, because the moving averages contract.  Tolerances are the reference's own rounding spread on the case at
hand (``optimizer_ref.spread``: the float32 twin's largest distance from the float64 rule over all steps and parameters of the
case) times DEVICE_FACTOR = 4, which covers a powf, sqrtf and division a few ulp from libm's and another contraction of the same
expression:

    theta:  4 E_up lr + 1 ulp(theta)        m: 4 E_m gscale_k        v: 4 E_v gscale_k^2
    schedule word: 4 E_schedule, relative   loss sum: 4 E_loss       t, n_steps, last loss: exact

No step and no parameter is left out of an assertion.

The spreads the tests compute, per case, as E_up / E_m / E_v (E_up alone for SGD, which has no moments); every case prints its own:

every step, 40 steps, seeds 100 + P
  defaults SGD   P=1 5.6e-11  P=2 4.9e-11  P=8 1.7e-07  P=9 9.0e-08  P=255 3.7e-07  P=256 4.7e-07  P=257 7.3e-07  P=6337 7.4e-07
  defaults Adam  P=1 3.3e-06/2.5e-08/2.5e-09  P=2 3.3e-06/4.6e-08/3.1e-09  P=8 3.4e-06/5.7e-08/8.0e-09  P=9 3.2e-06/9.8e-08/1.0e-08
                 P=255 3.5e-06/8.6e-08/1.5e-08  P=256 3.5e-06/8.4e-08/1.4e-08  P=257 3.5e-06/1.0e-07/2.0e-08  P=6337 3.6e-06/1.3e-07/1.6e-08
  defaults Nadam P=1 2.6e-06/2.4e-08/4.6e-09  P=2 2.7e-06/6.7e-08/1.1e-08  P=8 3.6e-06/5.4e-08/8.5e-09  P=9 3.5e-06/9.9e-08/1.2e-08
                 P=255 3.6e-06/1.0e-07/2.9e-08  P=256 3.7e-06/1.4e-07/1.9e-08  P=257 3.8e-06/1.2e-07/1.7e-08  P=6337 3.9e-06/1.7e-07/3.2e-08
                 E_schedule 2.7e-07
  sharp    SGD   P=1 6.5e-11  P=2 6.9e-11  P=8 1.4e-07  P=9 7.1e-08  P=255 5.7e-07  P=256 5.6e-07  P=257 5.6e-07  P=6337 5.7e-07
  sharp    Adam  P=1 1.5e-08/6.7e-08/1.4e-07  P=2 8.0e-09/1.0e-07/1.4e-07  P=8 1.7e-07/1.2e-07/1.7e-07  P=9 2.3e-07/9.5e-08/2.1e-07
                 P=255 3.7e-07/1.4e-07/2.5e-07  P=256 2.7e-07/1.4e-07/4.1e-07  P=257 3.5e-07/1.4e-07/2.8e-07  P=6337 3.1e-07/1.9e-07/3.8e-07
  sharp    Nadam P=1 1.9e-08/6.6e-08/1.1e-07  P=2 9.5e-09/5.0e-08/1.8e-07  P=8 3.3e-07/8.3e-08/1.9e-07  P=9 2.4e-07/7.1e-08/2.5e-07
                 P=255 4.2e-07/1.2e-07/3.2e-07  P=256 3.5e-07/9.9e-08/3.2e-07  P=257 3.8e-07/1.2e-07/3.5e-07  P=6337 5.0e-07/1.8e-07/5.2e-07
                 E_schedule 3.2e-07
  E_loss 2.9e-06 to 8.0e-06 (one loss column per P)
400 steps, seeds 200 + P (theta alone is asserted): E_up  defaults Adam P=2 2.4e-06, P=257 3.5e-06;  defaults Nadam P=2 3.5e-06,
  P=257 3.8e-06;  sharp Nadam P=2 3.3e-07, P=257 4.1e-07
regulariser and NonNeg, P = 8, 40 steps:  SGD 7.4e-08   Adam 3.3e-06/1.2e-07/6.3e-09   Nadam 3.4e-06/1.1e-07/1.7e-08
both forms, first 8 of seed 41:           SGD 1.6e-07   Adam 3.3e-06/6.3e-08/7.9e-09   Nadam 3.3e-06/4.5e-08/1.5e-08
bounds, 5 steps, seeds 300 + P, P = 1 .. 257:  SGD 1.8e-11 .. 3.6e-07   Adam 2.6e-06 .. 3.5e-06 / 5.1e-09 .. 5.9e-08 / 2.9e-11 .. 1.6e-09
                                               Nadam 3.0e-06 .. 4.0e-06 / 6.6e-09 .. 5.0e-08 / 1.2e-10 .. 1.7e-09
(E_up of Adam and Nadam is set by the first few steps, where 1 - beta_2^t cancels; the small SGD figures at P <= 3 are parameters
whose gradient scale happens to be small: E_up is absolute.)  The fixed kernels stay inside every one of these bounds with the
factor 4 as it stands.
"""
import numpy as np
import pytest
import torch

import optimizer_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats of pattern on either side of every device array
SCALE = 0.5


def _pattern(n, dev):
    return torch.arange(n, dtype=torch.float32, device=dev) * 0.5 + 1.0e6


def _guarded(n, dev, offset=0):
    """n floats ``offset`` floats into a tensor whose surrounding GUARD floats hold a pattern: (whole tensor, the view)."""
    whole = _pattern(GUARD + offset + n + GUARD, dev)
    return whole, whole[GUARD + offset:GUARD + offset + n]


def _guards_intact(whole, offset, n):
    want = _pattern(whole.numel(), whole.device)
    lo, hi = GUARD + offset, GUARD + offset + n
    return bool(torch.equal(whole[:lo], want[:lo])) and bool(torch.equal(whole[hi:], want[hi:]))


def _desc(htf, kind, h):
    d = htf._lib.OptimizerDesc()
    d.kind, d.lr, d.beta1, d.beta2, d.epsilon, d.nonneg_mask = kind, h.lr, h.beta1, h.beta2, h.eps, h.nonneg_mask
    for k, x in enumerate(() if h.l1_reg is None else h.l1_reg):
        d.l1_reg[k] = x
    assert (d.lr, d.beta1, d.beta2, d.epsilon) == (h.lr, h.beta1, h.beta2, h.eps)      # the descriptor holds the floats of Hyper
    return d


SENTINEL = -123.5


class Device:
    """theta, the accum rows of every step and the state of one optimizer, each inside a guarded tensor."""

    def __init__(self, htf, dev, kind, hyper, case, theta_offset=0, sentinels=False):
        self.htf, self.P, self.offset, self.desc = htf, case["P"], theta_offset, _desc(htf, kind, hyper)
        P, steps = self.P, case["steps"]
        self.n_state = htf.ops.optimizer_state_floats(P)
        assert self.n_state == R.state_floats(P)
        self.theta_all, self.theta = _guarded(P, dev, theta_offset)
        self.accum_all, accum = _guarded(steps * (1 + P), dev)
        self.state_all, self.state = _guarded(self.n_state, dev)
        self.theta.copy_(torch.from_numpy(case["theta"]))
        accum.copy_(torch.from_numpy(case["accum"].reshape(-1)))
        self.accum = accum.view(steps, 1 + P)
        self.accum_given = self.accum_all.clone()
        st = np.zeros(self.n_state, np.float32)
        self.untouched = np.zeros(self.n_state, bool)      # words of the state that no step may change
        self.untouched[R.AT_PAD:R.HEADER_FLOATS] = True
        if P <= R.ONE_THREAD_MAX_P:
            self.untouched[P:8] = self.untouched[8 + P:16] = True
        else:
            self.untouched[:16] = True                      # the vector form keeps m and v behind the header
        if sentinels:
            st[self.untouched] = SENTINEL
        self.state_given = st
        self.state.copy_(torch.from_numpy(st))
        self.m_at, self.v_at = R.moments_at(P)

    def step(self, s):
        self.htf.ops.optimizer_step(self.theta, self.accum[s], SCALE, self.state, self.desc)
        return self.theta.cpu().numpy(), self.state.cpu().numpy()

    def assert_bounds(self):
        assert _guards_intact(self.theta_all, self.offset, self.P), "theta's surroundings were written"
        assert _guards_intact(self.state_all, 0, self.n_state), "the state's surroundings were written"
        assert torch.equal(self.accum_all, self.accum_given), "accum was written"
        got = self.state.cpu().numpy()
        assert got[self.untouched].tobytes() == self.state_given[self.untouched].tobytes(), "unused words of the state were written"


def _fail(what, step, err, bound):
    k = int(np.argmax(err - bound))
    return "%s off at step %d, parameter %d: |error| %.3g against a bound of %.3g" % (what, step + 1, k, err[k], bound[k])


def _within(what, step, got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    bound = np.broadcast_to(bound, err.shape)
    assert np.all(err <= bound), _fail(what, step, err, bound)


def _check_theta(step, got, want, E, hyper):
    _within("theta", step, got, want, R.DEVICE_FACTOR * E["E_up"] * hyper.lr + R.ulp32(want))


def _check_state(step, P, state, ref, E, gs, accum_row):
    m_at, v_at = R.moments_at(P)
    _within("m", step, state[m_at:m_at + P], ref["m"], R.DEVICE_FACTOR * E["E_m"] * gs)
    _within("v", step, state[v_at:v_at + P], ref["v"], R.DEVICE_FACTOR * E["E_v"] * gs ** 2)
    assert state[R.AT_T] == step + 1 == ref["t"] and state[R.AT_N_STEPS] == step + 1 == ref["n_steps"], "step counters at step %d" % (step + 1)
    if ref["schedule"] >= R.FLT_MIN:
        assert abs(float(state[R.AT_SCHEDULE]) / ref["schedule"] - 1.0) <= R.DEVICE_FACTOR * E["E_schedule"], \
            "schedule word %r against %r at step %d" % (state[R.AT_SCHEDULE], ref["schedule"], step + 1)
    assert abs(float(state[R.AT_LOSS_SUM]) - ref["loss_sum"]) <= R.DEVICE_FACTOR * E["E_loss"], "loss sum at step %d" % (step + 1)
    assert state[R.AT_LAST_LOSS] == accum_row[0] * np.float32(SCALE) == ref["last_loss"], "last loss at step %d" % (step + 1)


def _follow(htf, dev, kind, hyper, case, state_too=True, **kw):
    """Run the case on the device and assert every step against the float64 rule.  Returns the Device and the spread."""
    P = case["P"]
    vector = P > R.ONE_THREAD_MAX_P
    rule = hyper.without_constraints() if vector else hyper          # the vector form has neither NonNeg nor a regulariser
    E = R.spread(kind, rule, case, SCALE)
    gs = R.gradient_scale(rule, case, SCALE)
    d = Device(htf, dev, kind, hyper, case, **kw)
    ref = R.new_state(P)
    theta = case["theta"]
    for s in range(case["steps"]):
        want, _ = R.ref_step(kind, rule, ref, theta.astype(np.float64), case["accum"][s], SCALE)
        theta, state = d.step(s)
        _check_theta(s, theta, want, E, hyper)
        if state_too:
            _check_state(s, P, state, ref, E, gs, case["accum"][s])
        if case["zero_always"] is not None and hyper.l1_reg is None:
            k = case["zero_always"]
            assert theta[k].tobytes() == case["theta"][k].tobytes(), "a zero gradient moved theta at step %d" % (s + 1)
    print("P=%d kind=%d lr=%g: " % (P, kind, hyper.lr) + " ".join("%s=%.3g" % kv for kv in sorted(E.items())))
    return d, E


# ------------------------------------------------------------------------------------------------ every step, kind and form
@pytest.mark.parametrize("hname", sorted(R.HYPER_SETS))
@pytest.mark.parametrize("P", [1, 2, 8, 9, 255, 256, 257, 6337])
@pytest.mark.parametrize("name", ["SGD", "Adam", "Nadam"])
def test_every_step_follows_the_reference(htf, cuda, name, P, hname):
    case = R.make_case(P, 40, seed=100 + P)
    d, _ = _follow(htf, cuda, R.KINDS[name], R.Hyper(**R.HYPER_SETS[hname]), case)
    d.assert_bounds()


# ------------------------------------------------------------------------------------------------ long horizon
@pytest.mark.parametrize("P", [2, 257])
@pytest.mark.parametrize("name,hname", [("Adam", "defaults"), ("Nadam", "defaults"), ("Nadam", "sharp")])
def test_400_steps_follow_the_reference(htf, cuda, name, hname, P):
    """400 steps, every theta.  Nadam's float32 schedule product underflows near step 132 with the default beta_1 (and would
    again near 265 if a stored 0 restarted it); from then on 1 - 0 = 1 is the bias correction, as in Keras.  With beta_1 = 0.5
    (the second hyper set) it underflows at step 76, five times in 400 steps, and it reaches an exact 0 in BOTH forms: with
    the default beta_1 the vector form's finish kernel, which multiplies (schedule beta_1) by the bracket, two factors above
    one half each, rounds the smallest subnormal back to itself and never stores a 0 where subnormals are kept."""
    case = R.make_case(P, 400, seed=200 + P)
    d, _ = _follow(htf, cuda, R.KINDS[name], R.Hyper(**R.HYPER_SETS[hname]), case, state_too=False)
    state = d.state.cpu().numpy()
    assert state[R.AT_T] == 400 and state[R.AT_N_STEPS] == 400
    if name == "Nadam":
        stuck = hname == "defaults" and P > R.ONE_THREAD_MAX_P
        assert state[R.AT_SCHEDULE] == 0.0 or (stuck and state[R.AT_SCHEDULE] == np.float32(1.4e-45))   # 1 - 1.4e-45 is 1 all the same


# ------------------------------------------------------------------------------------------------ regulariser and NonNeg
NONNEG_MASK = 0b10100101


def _downhill_case(P, steps, seed, lr):
    """Positive gradients on every parameter and a start a few steps above zero: every theta is pushed through zero."""
    case = R.make_case(P, steps, seed)
    rng = np.random.default_rng(seed + 1)
    case["accum"][:, 1:] = (case["gscale"] * (0.2 + np.abs(rng.standard_normal((steps, P))))).astype(np.float32)
    case["theta"] = (2.0 * lr * SCALE * case["gscale"]).astype(np.float32)
    case["zero_always"] = case["zero_early"] = None
    return case


@pytest.mark.parametrize("name", ["SGD", "Adam", "Nadam"])
def test_regulariser_and_nonneg(htf, cuda, name):
    """One-thread form, P = 8: l1_reg of both signs is added unscaled; the masked parameters stop at exactly 0 while the others
    go negative; m and v of a pinned parameter keep following its (unclamped) gradient."""
    P, lr = 8, 0.01
    case = _downhill_case(P, 40, seed=31, lr=lr)
    l1 = 0.1 * SCALE * case["gscale"] * np.array([1, -1, -1, 1, 1, -1, 1, -1.0])     # below the smallest gradient, 0.2 gscale
    hyper = R.Hyper(lr, nonneg_mask=NONNEG_MASK, l1_reg=l1)
    d, _ = _follow(htf, cuda, R.KINDS[name], hyper, case)
    d.assert_bounds()
    theta = d.theta.cpu().numpy()
    masked = np.array([(NONNEG_MASK >> k) & 1 for k in range(P)], bool)
    assert np.all(theta[masked] == 0.0) and not np.signbit(theta[masked]).any()
    assert np.all(theta[~masked] < 0.0)
    # and the regulariser is in the moments: against the rule without it, m is off by far more than the tolerance
    if name != "SGD":
        plain = R.run(R.KINDS[name], R.Hyper(lr), case, SCALE)
        assert np.all(np.abs(d.state.cpu().numpy()[:P] - plain["m"][-1]) > 0.01 * SCALE * case["gscale"])


@pytest.mark.parametrize("name", ["SGD", "Adam", "Nadam"])
def test_vector_form_ignores_mask_and_regulariser(htf, cuda, name):
    """include/htf_amd.h: "nonneg_mask / l1_reg are ignored" by htf_optimizer_step_n -- bit for bit."""
    P, lr = 9, 0.01
    case = _downhill_case(P, 20, seed=32, lr=lr)
    plain = R.Hyper(lr)
    loaded = R.Hyper(lr, nonneg_mask=0xFFFFFFFF, l1_reg=[0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 0.25, -0.25])
    a = Device(htf, cuda, R.KINDS[name], plain, case)
    b = Device(htf, cuda, R.KINDS[name], loaded, case)
    for s in range(case["steps"]):
        (ta, sa), (tb, sb) = a.step(s), b.step(s)
        assert ta.tobytes() == tb.tobytes() and sa.tobytes() == sb.tobytes(), "step %d" % (s + 1)
    assert np.all(ta < 0)          # a mask would have held them at 0
    b.assert_bounds()


# ------------------------------------------------------------------------------------------------ bounds
@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("P", [1, 3, 8, 9, 256, 257])
@pytest.mark.parametrize("name", ["SGD", "Adam", "Nadam"])
def test_nothing_outside_the_arrays_is_written(htf, cuda, name, P, offset):
    """theta (also as a slice that starts 3 floats into its tensor, as tfcompute's per-species step passes it), accum and the
    state lie inside larger tensors: after 5 steps the 64 floats around each still hold their pattern, accum is as given, and
    the words of the state that this P does not use (m[P..8), v[P..8), the pad; the 16 header words of the vector form) hold the
    values they were given.  The results are those of the reference all the same."""
    case = R.make_case(P, 5, seed=300 + P)
    d, _ = _follow(htf, cuda, R.KINDS[name], R.Hyper(**R.DEFAULTS), case, theta_offset=offset, sentinels=True)
    d.assert_bounds()


# ------------------------------------------------------------------------------------------------ the two forms
@pytest.mark.parametrize("name", ["SGD", "Adam", "Nadam"])
def test_both_forms_follow_one_reference(htf, cuda, name):
    """P = 8 in the one-thread form and the first 8 parameters of a P = 9 vector on the same gradients: each within the
    tolerance of the same float64 m, v and update (not equal bits: the two kernels write Nadam's expression differently)."""
    kind, hyper = R.KINDS[name], R.Hyper(**R.DEFAULTS)
    nine = R.make_case(9, 40, seed=41)
    eight = dict(nine, P=8, theta=nine["theta"][:8].copy(), accum=np.ascontiguousarray(nine["accum"][:, :9]), gscale=nine["gscale"][:8])
    E = R.spread(kind, hyper, eight, SCALE)
    gs = R.gradient_scale(hyper, eight, SCALE)
    d8, d9 = Device(htf, cuda, kind, hyper, eight), Device(htf, cuda, kind, hyper, nine)
    ref = R.new_state(8)
    t8, t9 = eight["theta"], nine["theta"]
    for s in range(40):
        want8, upd = R.ref_step(kind, hyper, ref, t8.astype(np.float64), eight["accum"][s], SCALE)
        want9 = t9[:8].astype(np.float64) - upd
        (t8, s8), (t9, s9) = d8.step(s), d9.step(s)
        _check_theta(s, t8, want8, E, hyper)
        _check_theta(s, t9[:8], want9, E, hyper)
        _check_state(s, 8, s8, ref, E, gs, eight["accum"][s])
        _within("m of the vector form", s, s9[24:32], ref["m"], R.DEVICE_FACTOR * E["E_m"] * gs)
        _within("v of the vector form", s, s9[33:41], ref["v"], R.DEVICE_FACTOR * E["E_v"] * gs ** 2)
        assert s9[R.AT_T] == s8[R.AT_T] and s9[R.AT_LAST_LOSS] == s8[R.AT_LAST_LOSS] and s9[R.AT_LOSS_SUM] == s8[R.AT_LOSS_SUM]
