"""tests/optimizer_ref.py checked on its own (no GPU): the float64 rule against the published Adam / Nadam vectors and the oracle's
optimizers, the torch twin of ``Optimizer.torch()`` against it, what Nadam's schedule product does once it underflows, and the
argument refusals of the two C entries that return before anything is launched."""
import os
import subprocess

import numpy as np
import pytest

import optimizer_ref as R
from helpers import ROOT
from oracle import htf_oracle as O
from test_tf_published_vectors import GRADS, keras_nadam_steps, tf1_adam_steps


def _accum(g):
    return np.concatenate([[0.0], np.atleast_1d(g)]).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the float64 rule
def test_reference_reproduces_the_published_vectors():
    """Gradients and hyper-parameters stay Python doubles: the same arithmetic as the scalar restatements."""
    for kind, want in ((R.ADAM, tf1_adam_steps(GRADS, lr=0.001, eps=1e-7, x0=0.2)), (R.NADAM, keras_nadam_steps(GRADS, lr=0.001, x0=0.2))):
        h, st, x = R.Hyper(0.001, fp32=False), R.new_state(1), np.array([0.2])
        for g, w in zip(GRADS, want):
            x, _ = R.ref_step(kind, h, st, x, _accum(g))
            assert x[0] == pytest.approx(w, rel=1e-13, abs=1e-16)
        assert st["t"] == st["n_steps"] == len(GRADS)


@pytest.mark.parametrize("name", ["Adam", "Nadam"])
def test_reference_follows_the_oracle_over_400_steps(name):
    case = R.make_case(5, 400, seed=11)
    h, st = R.Hyper(0.01, fp32=False), R.new_state(5)
    opt = {"Adam": O.KerasAdam, "Nadam": O.KerasNadam}[name](0.01)
    x = y = case["theta"].astype(np.float64)
    for s in range(400):
        g = 0.5 * case["accum"][s, 1:].astype(np.float64)
        y = opt.step(y, g)
        x, _ = R.ref_step(R.KINDS[name], h, st, x, case["accum"][s], 0.5)
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-15)
    assert np.abs(x - case["theta"]).max() > 0.05         # ... while theta travels many steps' worth


def test_reference_sgd_regulariser_nonneg_and_loss_words():
    h = R.Hyper(0.25, nonneg_mask=0b01, l1_reg=[0.5, -0.5], fp32=False)
    st = R.new_state(2)
    x, upd = R.ref_step(R.SGD, h, st, np.array([0.5, 0.5]), np.array([3.0, 4.0, 4.0], np.float32), 0.5)
    # g = 0.5 * 4 + (0.5, -0.5) = (2.5, 1.5): the regulariser is not scaled; NonNeg after the update, on parameter 0 alone
    np.testing.assert_array_equal(upd, [0.625, 0.375])
    np.testing.assert_array_equal(x, [0.0, 0.125])
    x, _ = R.ref_step(R.SGD, h, st, np.array([0.1, 0.1]), np.array([1.0, 4.0, 4.0], np.float32), 0.5)
    np.testing.assert_array_equal(x, [0.0, 0.1 - 0.375])
    assert (st["loss_sum"], st["n_steps"], st["last_loss"], st["t"]) == (2.0, 2, 0.5, 2)


def test_hyper_parameters_are_rounded_to_float32_first():
    h = R.Hyper(**R.DEFAULTS)
    assert h.beta1 == float(np.float32(0.9)) != 0.9 and h.eps == float(np.float32(1e-7)) and h.decay == float(np.float32(0.004))
    assert R.Hyper(0.01, fp32=False).beta1 == 0.9


def test_seeded_cases_hold_what_they_stand_for():
    c = R.make_case(257, 40, seed=3)
    g = c["accum"][:, 1:]
    assert c["accum"].dtype == np.float32 and c["theta"].dtype == np.float32
    assert not g[:, R.ZERO_ALWAYS].any()
    assert not g[:R.EARLY_STEPS, R.ZERO_EARLY].any() and g[R.EARLY_STEPS:, R.ZERO_EARLY].all()
    assert g[:, [0, 255, 256]].all()                                                  # both sides of the block edge are live
    live = np.delete(np.arange(257), [R.ZERO_ALWAYS, R.ZERO_EARLY])
    gg = (g[:, live] * np.float32(0.5)) ** 2
    assert gg.dtype == np.float32 and gg.min() >= R.FLT_MIN                           # g g is a normal float32
    assert 1e-3 <= c["gscale"].min() < 1e-2 and 1.0 < c["gscale"].max() <= 10.0
    assert R.make_case(2, 5, 0)["zero_always"] == 1 and R.make_case(2, 5, 0)["zero_early"] is None
    assert R.make_case(1, 5, 0)["zero_always"] is None
    t = R.make_case(3, 300, seed=4, gmin=0.5, gmax=2.0)["accum"][:, 1:]
    assert np.abs(t).min() >= 0.5 and np.abs(t).max() <= 2.0 and (t > 0).any() and (t < 0).any()


def test_state_layout_restated():
    assert R.state_floats(8) == 24 and R.state_floats(9) == 24 + 18
    assert R.moments_at(8) == (0, 8) and R.moments_at(9) == (24, 33)


# ------------------------------------------------------------------------------------------------ Nadam's schedule product
def test_twin_schedule_underflows_to_zero_and_nothing_happens():
    """400 default Nadam steps in float32: the product of the u_t is exactly 0 from some step on, and every later update stays
    as close to the float64 rule as the earlier ones were (1 - 0 = 1 is the right bias correction).  The kernels must have this
    property; read as "first step", the stored 0 restarts the schedule and the very next update is off by half of lr."""
    case, h = R.make_case(2, 400, seed=202), R.Hyper(**R.DEFAULTS)
    r64 = R.run(R.NADAM, h, case, 0.5)
    r32 = R.run(R.NADAM, h, case, 0.5, np.float32)
    zero = np.nonzero(r32["schedule"] == 0)[0]
    first_zero = int(zero[0])                                                          # 0-based: the step after it reads a 0
    assert 100 < first_zero < 140 and np.array_equal(zero, np.arange(first_zero, 400))
    assert r64["schedule"][first_zero] > 0 and r64["schedule"][-1] == pytest.approx(0.0, abs=1e-100)
    dev = np.abs(r32["update"].astype(np.float64) - r64["update"]).max(axis=1) / h.lr
    e_before = dev[:first_zero + 1].max()
    assert 1e-6 < e_before < 1e-5
    assert dev[first_zero + 1:].max() <= e_before
    # the former rule, restated: it departs at the first step that reads the 0, and again one underflow later
    old = R.run(R.NADAM, h, case, 0.5, np.float32, restart_on_zero=True)
    dev_old = np.abs(old["update"].astype(np.float64) - r64["update"]).max(axis=1) / h.lr
    off = np.nonzero(dev_old > R.DEVICE_FACTOR * e_before)[0]
    assert off[0] == first_zero + 1 and dev_old[off[0]] > 0.3
    assert np.array_equal(old["update"][:first_zero + 1], r32["update"][:first_zero + 1])   # the steps before keep their bits
    assert (off > first_zero + 100).any()


# ------------------------------------------------------------------------------------------------ Optimizer.torch()
@pytest.mark.parametrize("name", ["SGD", "Adam", "Nadam"])
def test_torch_twin_follows_the_reference(htf, name):
    """``Optimizer.torch()`` (the autograd training route) against the float64 rule: 300 steps, float64 parameters on the CPU,
    every step's update.  torch.optim.Adam adds epsilon to sqrt(v) / sqrt(1 - beta_2^t), Keras to sqrt(v) with the correction in
    lr_t: epsilon / sqrt(1 - beta_2^t) against epsilon, a relative difference of the update below epsilon / sqrt(v).  With |g| in
    [0.5, 2], v >= (1 - beta_2) 0.25 from the first step on, sqrt(v) >= 0.0158 and the bound is 1e-7 / 0.0158 = 6.3e-6; 1e-5 is
    asserted.  torch.optim.NAdam places epsilon as Keras does (sqrt(v / (1 - beta_2^t)) + epsilon) and its momentum_decay 0.004
    on base 0.96 is Keras' schedule; what differs is that torch keeps the schedule product in a float32 tensor, one rounding of
    2^-24 per step in mu_product, which 1 / (1 - mu_product) passes on no larger while mu_product <= 0.5: far inside 1e-5."""
    import torch
    P, steps, lr = 3, 300, 0.01
    case = R.make_case(P, steps, seed=4, gmin=0.5, gmax=2.0)
    opt = getattr(htf.optimizers, name)(lr)
    w = torch.tensor(case["theta"].astype(np.float64), dtype=torch.float64, requires_grad=True)
    topt = opt.torch([w])
    h, st = R.Hyper(lr, fp32=False), R.new_state(P)
    worst = 0.0
    for s in range(steps):
        before = w.detach().numpy().copy()
        w.grad = torch.from_numpy(case["accum"][s, 1:].astype(np.float64))
        topt.step()
        got = before - w.detach().numpy()
        _, want = R.ref_step(R.KINDS[name], h, st, before, case["accum"][s])
        rel = np.abs(got - want) / np.abs(want)
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 1e-5, "step %d: %r" % (s + 1, rel)
        if name == "Adam":
            assert np.all(rel <= h.eps / np.sqrt(st["v"]) + 1e-12)                      # the derived bound itself, per parameter
    print("%s: worst relative difference of an update %.3g" % (name, worst))


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_optimizer_argument_checks_without_a_gpu(htf, tmp_path):
    """A stand-alone host program on the two entries: every call below is refused before anything is launched (the pointers
    are host memory that no kernel may see, and the program is shown no GPU)."""
    src = tmp_path / "t.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "htf_amd.h"
int main(void) {
    float theta[16] = {0}, accum[17] = {0}, state[HTF_OPT_STATE_FLOATS + 32] = {0};
    htf_optimizer_desc d;
    int bad = 0, kinds[2] = {-1, 3};
    memset(&d, 0, sizeof d);
    d.kind = HTF_OPT_ADAM;
    d.lr = 0.01f; d.beta1 = 0.9f; d.beta2 = 0.999f; d.epsilon = 1e-7f;
    bad += htf_optimizer_step(theta, 0, accum, 1.f, state, &d, NULL) != HTF_ERR_INVALID;      /* P = 0 */
    bad += htf_optimizer_step_n(theta, 0, accum, 1.f, state, &d, NULL) != HTF_ERR_INVALID;
    bad += htf_optimizer_step(theta, 9, accum, 1.f, state, &d, NULL) != HTF_ERR_INVALID;      /* P = 9 on the one-thread form */
    bad += strstr(htf_last_error(), "P=9") == NULL;
    for (int i = 0; i < 2; ++i) {
        d.kind = kinds[i];
        bad += htf_optimizer_step(theta, 2, accum, 1.f, state, &d, NULL) != HTF_ERR_INVALID;
        bad += htf_optimizer_step_n(theta, 12, accum, 1.f, state, &d, NULL) != HTF_ERR_INVALID;
    }
    d.kind = HTF_OPT_NADAM;
    bad += htf_optimizer_step(NULL, 2, accum, 1.f, state, &d, NULL) != HTF_ERR_INVALID;       /* null pointers */
    bad += htf_optimizer_step(theta, 2, NULL, 1.f, state, &d, NULL) != HTF_ERR_INVALID;
    bad += htf_optimizer_step(theta, 2, accum, 1.f, NULL, &d, NULL) != HTF_ERR_INVALID;
    bad += htf_optimizer_step(theta, 2, accum, 1.f, state, NULL, NULL) != HTF_ERR_INVALID;
    bad += htf_optimizer_step_n(NULL, 12, accum, 1.f, state, &d, NULL) != HTF_ERR_INVALID;
    bad += htf_optimizer_step_n(theta, 12, NULL, 1.f, state, &d, NULL) != HTF_ERR_INVALID;
    bad += htf_optimizer_step_n(theta, 12, accum, 1.f, NULL, &d, NULL) != HTF_ERR_INVALID;
    bad += htf_optimizer_step_n(theta, 12, accum, 1.f, state, NULL, NULL) != HTF_ERR_INVALID;
    for (int i = 0; i < 16; ++i) bad += theta[i] != 0.f || state[i] != 0.f;                   /* and nothing was written */
    printf("%d\n", bad);
    return bad;
}
''')
    exe = tmp_path / "t"
    lib_dir = os.path.dirname(htf._lib.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lhtf_amd", "-Wl,-rpath," + lib_dir])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    assert subprocess.check_output([str(exe)], text=True, timeout=120, env=env).split() == ["0"]


def test_optimizer_state_size(htf):
    import torch
    assert htf.ops.optimizer_state_floats(8) == 24 and htf.ops.optimizer_state_floats(9) == 24 + 18
    desc = htf.optimizers.Adam(0.01).desc()
    # a state one float short is refused by the Python front before the library is called (host tensors: nothing can launch)
    for P in (8, 9):
        theta, accum = torch.zeros(P), torch.zeros(1 + P)
        with pytest.raises(ValueError, match="optimizer state too small for %d parameters" % P):
            htf.ops.optimizer_step(theta, accum, 1.0, torch.zeros(htf.ops.optimizer_state_floats(P) - 1), desc)
        assert not theta.any()
