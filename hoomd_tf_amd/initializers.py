"""Keras-style initialisers for the pair-MLP weights (tf.keras.layers.Dense defaults:
glorot-uniform kernel, zero bias -- the defaults example 08 / NlistNN use,
build_examples.py:199-205)."""
import math

import numpy as np


def glorot_uniform(rng, fan_in, fan_out, dtype=np.float32):
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(dtype)


def mlp_params(seed=3, K=32, H1=64, H2=64, dtype=np.float32, bias_scale=0.0, H3=None):
    """RBF(K) -> H1 -> H2 -> 1 weights, numpy default_rng(seed).  With ``H3``: RBF(K) -> H1 -> H2 -> H3 -> 1,
    eight arrays, W1 to W4 drawn in that order; without it the output is what it was before the argument."""
    rng = np.random.default_rng(seed)
    p = {
        "W1": glorot_uniform(rng, K, H1, dtype), "b1": np.zeros(H1, dtype),
        "W2": glorot_uniform(rng, H1, H2, dtype), "b2": np.zeros(H2, dtype),
    }
    if H3 is None:
        p.update({"W3": glorot_uniform(rng, H2, 1, dtype), "b3": np.zeros(1, dtype)})
    else:
        p.update({"W3": glorot_uniform(rng, H2, H3, dtype), "b3": np.zeros(H3, dtype),
                  "W4": glorot_uniform(rng, H3, 1, dtype), "b4": np.zeros(1, dtype)})
    if bias_scale:
        for k in [k for k in p if k[0] == "b"]:
            p[k] = (bias_scale * rng.standard_normal(p[k].shape)).astype(dtype)
    return p
