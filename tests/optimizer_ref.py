"""The device optimizers' update rules (``htf_optimizer_step``, ``htf_optimizer_step_n``) restated in plain NumPy from the
``optimizer_v2`` sources that ``hoomd_tf_amd/optimizers.py`` and ``include/htf_amd.h`` cite (TF 2.3 / 2.4 ``gradient_descent.py``,
``adam.py``, ``nadam.py``).  No GPU and nothing of the library is imported here.

Two evaluations of ONE rule (``ref_step``; the dtype is its only switch):

* float64: the reference.  Hyper-parameters are rounded to float32 first (the descriptor carries floats, and Keras casts them to
  the variable's dtype), then every operation is float64.  Gradients are the float32 words the device is given.
* float32, "the twin": every intermediate rounded to float32, in the order Keras writes the expressions on float32 variables.
  The twin is NOT a second oracle.  Its distance from the float64 rule is what float32 evaluation of these formulas costs, and
  the tests' tolerances are multiples of that distance (``spread``), never of what a kernel returns.

The state is what the header lays out: m, v, the step count t, Nadam's momentum-schedule product, the running loss sum, the
number of steps and the last loss.  The schedule product starts at 1 because t == 0, not because a stored word is 0: Keras keeps
multiplying, the float32 product underflows to exactly 0 after about 130 steps of the default beta_1, and 1 - 0 = 1 is then the
right bias correction.  ``restart_on_zero=True`` restates the rule the kernels had before (a stored 0 read as "first step"), so
that the CPU tests can show what the long-horizon GPU tests are there to catch.

Also the seeded cases the tests run (``make_case``).
"""
import functools

import numpy as np

SGD, ADAM, NADAM = 0, 1, 2                 # enum htf_optimizer_kind
KINDS = {"SGD": SGD, "Adam": ADAM, "Nadam": NADAM}
HEADER_FLOATS = 24                         # HTF_OPT_STATE_FLOATS: m[8], v[8], t, schedule, loss_sum, n_steps, last_loss, pad[3]
AT_T, AT_SCHEDULE, AT_LOSS_SUM, AT_N_STEPS, AT_LAST_LOSS, AT_PAD = 16, 17, 18, 19, 20, 21
ONE_THREAD_MAX_P = 8                       # htf_optimizer_step takes P <= 8, htf_optimizer_step_n any P


def state_floats(P):
    """ops.optimizer_state_floats, restated."""
    return HEADER_FLOATS + (2 * P if P > ONE_THREAD_MAX_P else 0)


def moments_at(P):
    """(offset of m, offset of v) in the device state of a P-parameter optimizer."""
    return (0, 8) if P <= ONE_THREAD_MAX_P else (HEADER_FLOATS, HEADER_FLOATS + P)


class Hyper:
    """learning rate, beta_1, beta_2, epsilon, NonNeg mask and d(regulariser)/d(theta), as ``htf_optimizer_desc`` holds them.
    ``fp32=True`` rounds them (and Nadam's 0.96 and 0.004) to float32 as the descriptor does; ``fp32=False`` keeps the doubles,
    for comparisons with references that compute in Python floats."""

    def __init__(self, lr, beta1=0.9, beta2=0.999, eps=1e-7, nonneg_mask=0, l1_reg=None, fp32=True):
        r = (lambda x: float(np.float32(x))) if fp32 else float
        self.lr, self.beta1, self.beta2, self.eps = r(lr), r(beta1), r(beta2), r(eps)
        self.decay_base, self.decay = r(0.96), r(0.004)
        self.nonneg_mask = int(nonneg_mask)
        self.l1_reg = None if l1_reg is None else np.array([r(x) for x in l1_reg], dtype=np.float64)

    def without_constraints(self):
        h = Hyper.__new__(Hyper)
        h.__dict__.update(self.__dict__)
        h.nonneg_mask, h.l1_reg = 0, None
        return h


DEFAULTS = dict(lr=0.01)                                          # Keras defaults beside the learning rate the tests train with
SHARP = dict(lr=0.05, beta1=0.5, beta2=0.9, eps=1e-2)             # an epsilon comparable with sqrt(v) shows where it sits
HYPER_SETS = {"defaults": DEFAULTS, "sharp": SHARP}


def new_state(P, dtype=np.float64):
    dt = np.dtype(dtype).type
    return dict(m=np.zeros(P, dtype), v=np.zeros(P, dtype), t=0, schedule=dt(1), loss_sum=dt(0), n_steps=0, last_loss=dt(0))


def ref_step(kind, hyper, state, theta, accum, scale=1.0, dtype=np.float64, restart_on_zero=False):
    """One step.  ``accum``: [loss sum, d/dtheta_0, ...] as the training sweeps leave it, rounded to float32 words; ``scale`` multiplies
    both.  g = scale * accum[1 + k] + l1_reg[k] (the regulariser's term is not scaled), the rule of ``kind``, then NonNeg on the
    masked parameters.  Updates ``state`` in place and returns (theta after the step, the rule's decrement before NonNeg), both
    in ``dtype``."""
    dt = np.dtype(dtype).type
    P = len(theta)
    theta = np.asarray(theta).astype(dtype)
    a = np.asarray(accum)
    if a.dtype != np.float64:          # (a float64 array is taken as it is: the published vectors are Python floats)
        a = a.astype(np.float32)
    a = a.astype(dtype)
    assert a.shape == (1 + P,)
    sc = dt(np.float32(scale))
    one, half = dt(1), dt(0.5)
    lr, b1, b2, eps = dt(hyper.lr), dt(hyper.beta1), dt(hyper.beta2), dt(hyper.eps)

    loss = a[0] * sc
    state["loss_sum"] = dt(state["loss_sum"] + loss)
    state["n_steps"] += 1
    state["last_loss"] = dt(loss)

    g = a[1:] * sc
    if hyper.l1_reg is not None:
        g = g + hyper.l1_reg[:P].astype(dtype)
    first = state["t"] == 0
    state["t"] += 1
    t = dt(state["t"])
    m, v = state["m"], state["v"]
    with np.errstate(under="ignore"):
        if kind == SGD:
            update = lr * g
        elif kind == ADAM:      # adam.py _prepare_local + training_ops ApplyAdam
            lr_t = lr * np.sqrt(one - np.power(b2, t)) / (one - np.power(b1, t))
            m += (g - m) * (one - b1)
            v += (g * g - v) * (one - b2)
            update = (m * lr_t) / (np.sqrt(v) + eps)
        elif kind == NADAM:     # nadam.py _prepare_local + _resource_apply_dense
            base, decay = dt(hyper.decay_base), dt(hyper.decay)
            schedule = state["schedule"]
            if first or (restart_on_zero and schedule == 0):
                schedule = one
            u_t = b1 * (one - half * np.power(base, decay * t))
            u_t1 = b1 * (one - half * np.power(base, decay * (t + one)))
            schedule_new = dt(schedule * u_t)
            schedule_next = dt(schedule_new * u_t1)
            g_prime = g / (one - schedule_new)
            m[:] = b1 * m + (one - b1) * g
            m_prime = m / (one - schedule_next)
            v[:] = b2 * v + (one - b2) * (g * g)
            v_prime = v / (one - np.power(b2, t))
            m_bar = (one - u_t) * g_prime + u_t1 * m_prime
            update = lr * m_bar / (np.sqrt(v_prime) + eps)
            state["schedule"] = schedule_new
        else:
            raise ValueError("kind %r" % (kind,))
    assert update.dtype == np.dtype(dtype) and m.dtype == np.dtype(dtype)
    new = theta - update
    for k in range(min(P, 32)):
        if (hyper.nonneg_mask >> k) & 1:
            new[k] = max(new[k], dt(0))
    return new, update


twin_step = functools.partial(ref_step, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------- seeded cases
ZERO_ALWAYS, ZERO_EARLY, EARLY_STEPS = 1, 2, 10    # which parameter's gradient is always zero / zero for the first steps


def make_case(P, steps, seed, gmin=None, gmax=None):
    """``accum`` [steps, 1 + P] float32 and a start ``theta`` (0.1 N(0, 1), float32).  Parameter k's gradients are
    ``gscale[k]`` N(0, 1) with gscale = 10^U(-3, 1), so that g g never underflows in float32.  Parameter 1 (where P >= 2) has a
    gradient that is always zero, parameter 2 (where P >= 3) one that is zero for the first ten steps; the last parameter, the
    one a dropped tail block would skip, is an ordinary one whenever P is not 2.  ``gmin``/``gmax``: |g| uniform in that range
    with a random sign instead, no zero parameter (the torch comparison).  Column 0 holds a loss sum, U(0.5, 4)."""
    rng = np.random.default_rng(seed)
    theta = (0.1 * rng.standard_normal(P)).astype(np.float32)
    accum = np.empty((steps, 1 + P), dtype=np.float32)
    accum[:, 0] = rng.uniform(0.5, 4.0, steps)
    if gmin is not None:
        gscale = np.ones(P)
        accum[:, 1:] = rng.uniform(gmin, gmax, (steps, P)) * rng.choice([-1.0, 1.0], (steps, P))
        return dict(P=P, steps=steps, theta=theta, accum=accum, gscale=gscale, zero_always=None, zero_early=None)
    gscale = 10.0 ** rng.uniform(-3.0, 1.0, P)
    accum[:, 1:] = gscale * rng.standard_normal((steps, P))
    zero_always = ZERO_ALWAYS if P > ZERO_ALWAYS else None
    zero_early = ZERO_EARLY if P > ZERO_EARLY else None
    if zero_always is not None:
        accum[:, 1 + zero_always] = 0
    if zero_early is not None:
        accum[:EARLY_STEPS, 1 + zero_early] = 0
    live = np.ones(P, bool)
    if zero_always is not None:
        live[zero_always] = False
    assert np.all(np.abs(accum[EARLY_STEPS:, 1:][:, live]) > 1e-12)       # g g stays a normal float32
    return dict(P=P, steps=steps, theta=theta, accum=accum, gscale=gscale, zero_always=zero_always, zero_early=zero_early)


def run(kind, hyper, case, scale, dtype=np.float64, **kw):
    """The rule run free over a case: per-step updates, m, v, schedule and loss sum (arrays over the steps)."""
    P, steps = case["P"], case["steps"]
    st = new_state(P, dtype)
    theta = case["theta"].astype(dtype)
    out = dict(update=np.empty((steps, P), dtype), m=np.empty((steps, P), dtype), v=np.empty((steps, P), dtype),
               schedule=np.empty(steps, dtype), loss_sum=np.empty(steps, dtype), theta=np.empty((steps, P), dtype))
    for s in range(steps):
        theta, upd = ref_step(kind, hyper, st, theta, case["accum"][s], scale, dtype=dtype, **kw)
        out["update"][s], out["m"][s], out["v"][s], out["theta"][s] = upd, st["m"], st["v"], theta
        out["schedule"][s], out["loss_sum"][s] = st["schedule"], st["loss_sum"]
    return out


FLT_MIN = float(np.finfo(np.float32).tiny)


def gradient_scale(hyper, case, scale):
    """The size of parameter k's gradient as the rule sees it: scale gscale[k] + |l1_reg[k]|."""
    gs = case["gscale"] * float(np.float32(scale))
    return gs if hyper.l1_reg is None else gs + np.abs(hyper.l1_reg[:case["P"]])


def spread(kind, hyper, case, scale):
    """The reference's own rounding spread on a case: the largest distance between the float32 twin and the float64 rule, over
    all steps and all parameters.  E_up: of the update, over lr.  E_m, E_v: of m and v, relative to the parameter's gradient
    scale and its square.  E_schedule: of the schedule product, relative, while it is a normal float32.  E_loss: of the loss
    sum, absolute."""
    r64, r32 = run(kind, hyper, case, scale, np.float64), run(kind, hyper, case, scale, np.float32)
    gs = gradient_scale(hyper, case, scale)
    normal = r32["schedule"] >= FLT_MIN
    return dict(
        E_up=float(np.max(np.abs(r32["update"].astype(np.float64) - r64["update"])) / hyper.lr),
        E_m=float(np.max(np.abs(r32["m"].astype(np.float64) - r64["m"]) / gs)),
        E_v=float(np.max(np.abs(r32["v"].astype(np.float64) - r64["v"]) / gs ** 2)),
        E_schedule=float(np.max(np.abs(r32["schedule"][normal].astype(np.float64) / r64["schedule"][normal] - 1.0), initial=0.0)),
        E_loss=float(np.max(np.abs(r32["loss_sum"].astype(np.float64) - r64["loss_sum"]))))


DEVICE_FACTOR = 4.0    # the device's powf, sqrtf and division are a few ulp from libm's, and it may contract the same expression


def ulp32(x):
    """Spacing of float32 at |x| (array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
