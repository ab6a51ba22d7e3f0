"""The descriptor network on the host: the argument and shape checks of htf.DescriptorMLP and the weights API (get/set,
save/load, through SimModel).  The C ABI table, the header and the code objects: tests/test_bp_cpu.py.  No GPU."""
import numpy as np
import pytest
import torch

_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")


@pytest.mark.parametrize("kw", [dict(K=33, n_types=2), dict(K=16, n_types=5), dict(K=65), dict(K=1), dict(H1=65), dict(H2=0),
                                dict(H2=65), dict(low=2.0, high=2.0), dict(low=3.0, high=1.0), dict(activation="relu"),
                                dict(n_types=0)])
def test_desc_layer_limits(htf, kw):
    with pytest.raises(ValueError):
        htf.DescriptorMLP(device="cpu", **kw)


def test_desc_layer_limits_at_the_edge(htf):
    """D = 64 and H = 64 are inside: one channel and one hidden unit per lane."""
    lay = htf.DescriptorMLP(K=16, n_types=4, H1=64, H2=64, device="cpu")
    assert lay.D == 64 and lay.w.numel() == 64 * 64 + 64 + 64 * 64 + 64 + 64 + 1
    lay = htf.DescriptorMLP(K=64, H1=1, H2=1, activation=None, device="cpu")
    assert lay.activation == "linear"


def test_desc_call_checks(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    with pytest.raises(ValueError):
        lay(torch.zeros((4, 257, 4)))               # more than four slots per lane
    with pytest.raises(ValueError):
        lay(torch.zeros((4, 16, 3)))
    e = lay(torch.zeros((4, 256, 4)))
    with pytest.raises(ValueError):
        lay.forces(torch.zeros((4, 16, 4)))         # no CPU path
    with pytest.raises(ValueError):
        lay.descriptor(torch.zeros((4, 16, 4)))
    assert isinstance(e, htf.simmodel.DescriptorEnergy) and e.reduced


def test_desc_energy_does_not_combine(htf):
    """The layer's energy takes no part in arithmetic, in either order, with constants or with other energies: a sum the
    kernel cannot form never reaches compute_nlist_forces as wrong forces."""
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    nl = htf.Nlist(torch.zeros((4, 16, 4)))
    e = lay(nl)
    lj_pair = 4.0 * (htf.nlist_rinv(nl) ** 12 - htf.nlist_rinv(nl) ** 6)
    lj = htf.reduce_sum(lj_pair, axis=1)
    for f in (lambda: e + 1.0, lambda: 1.0 + e, lambda: 2.0 * e, lambda: e * 2.0, lambda: -e, lambda: e - 1.0, lambda: e / 2.0,
              lambda: e + e, lambda: e + lj, lambda: e + lj_pair):
        with pytest.raises(TypeError):
            f()
    for f in (lambda: lj + e, lambda: lj_pair + e, lambda: lj - e):
        with pytest.raises((TypeError, RuntimeError)):
            f()


def test_desc_weights_follow_mlp_params(htf):
    from hoomd_tf_amd.initializers import mlp_params
    lay = htf.DescriptorMLP(K=6, n_types=3, H1=10, H2=7, seed=11, device="cpu")
    ref = mlp_params(seed=11, K=18, H1=10, H2=7)
    got = lay.get_weights()
    assert [g.shape for g in got] == [ref[k].shape for k in _KEYS]
    for g, k in zip(got, _KEYS):
        np.testing.assert_array_equal(g, ref[k])
    # the centres and spacing are RBFExpansion's
    rbf = htf.RBFExpansion(0.0, 3.0, 6)
    np.testing.assert_array_equal(lay.centers, rbf.centers)
    assert lay.gap == rbf.gap
    np.testing.assert_array_equal(lay.mu.numpy(), rbf.centers)


def test_desc_weights_round_trip(htf, tmp_path):
    lay = htf.DescriptorMLP(K=8, H1=12, H2=9, device="cpu")
    rng = np.random.default_rng(4)
    new = [rng.standard_normal(w.shape).astype(np.float32) for w in lay.get_weights()]
    w_before = lay.w
    lay.set_weights(new)
    assert lay.w is w_before                        # in place: whoever holds w sees the new values
    for a, b in zip(lay.get_weights(), new):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(lay.w.numpy(), np.concatenate([x.ravel() for x in new]))
    p = str(tmp_path / "desc.npz")
    lay.save_weights(p)
    other = htf.DescriptorMLP(K=8, H1=12, H2=9, seed=99, device="cpu")
    other.load_weights(p)
    for a, b in zip(other.get_weights(), new):
        np.testing.assert_array_equal(a, b)
    # an in-place write to w is what get_weights reports
    with torch.no_grad():
        lay.w[0] += 1.0
    assert lay.get_weights()[0][0, 0] == new[0][0, 0] + np.float32(1.0)
    with pytest.raises(ValueError):
        lay.set_weights(new[:5])
    with pytest.raises(ValueError):
        lay.set_weights([new[0].T] + new[1:])


def test_desc_weights_through_simmodel(htf, tmp_path):
    class M(htf.SimModel):
        def setup(self):
            self.desc = htf.DescriptorMLP(K=4, H1=5, H2=3, seed=2, device="cpu")

        def compute(self, nlist):
            return htf.compute_nlist_forces(nlist, self.desc(nlist))

    m = M(16)
    ws = m.get_weights()
    assert len(ws) == 6 and ws[0].shape == (4, 5) and ws[4].shape == (3, 1)
    new = [w + np.float32(0.5) for w in ws]
    m.set_weights(new)
    for a, b in zip(m.desc.get_weights(), new):
        np.testing.assert_array_equal(a, b)
    p = str(tmp_path / "m")
    m.save_weights(p)
    m2 = M(16)
    m2.load_weights(p)
    for a, b in zip(m2.get_weights(), new):
        np.testing.assert_array_equal(a, b)
