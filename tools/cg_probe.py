"""Times the coarse-grained ops (csrc/cg_map.hip) at 131 072 atoms mapped 3:1 (43 691 beads), NN = 64, r_cut for about
40 neighbors per bead: center_of_mass forward / backward, compute_nlist forward / backward.  Device events around
``--iters`` calls per window, the median of ``--windows`` windows; one JSON line.

    python tools/cg_probe.py [--atoms 131072] [--nn 64] [--iters 20] [--windows 7]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402


def timed(fn, iters, windows):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=64)
    ap.add_argument("--neighbors", type=float, default=40.0, help="mean beads within r_cut")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cg_probe: needs a GPU")
    dev = torch.device("cuda:0")
    N = a.atoms
    L = float(N) ** (1.0 / 3.0)               # one atom per unit volume
    rng = np.random.default_rng(1)
    index = [list(range(i, min(i + 3, N))) for i in range(0, N, 3)]
    B = len(index)
    centres = rng.uniform(-L / 2, L / 2, (B, 3))
    pos = np.concatenate([centres[k] + rng.normal(0, 0.3, (len(ix), 3)) for k, ix in enumerate(index)])
    pos = (pos - np.round(pos / L) * L).astype(np.float32)
    s = htf.sparse_mapping([np.ones((1, len(ix)), np.int32) for ix in index], index, device=dev)
    r_cut = (a.neighbors / (B / L ** 3) / (4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)
    box = torch.tensor([L] * 3, device=dev)
    x = torch.from_numpy(pos).to(dev).requires_grad_(True)

    com = htf.center_of_mass(x, s, box)
    g_com = torch.randn_like(com)
    beads = com.detach().clone().requires_grad_(True)
    nl = htf.compute_nlist(beads, r_cut, a.nn, box, sorted=True)
    g_nl = torch.randn_like(nl)
    filled = (nl.detach()[:, :, :3].abs().sum(2) > 0).sum(1).float()

    res = {"atoms": N, "beads": B, "NN": a.nn, "r_cut": round(r_cut, 4), "box": round(L, 4),
           "mean_neighbors": round(float(filled.mean()), 2), "max_neighbors": int(filled.max()),
           "pair_distances": B * B}
    for name, fn in (("com_forward_ms", lambda: htf.center_of_mass(x, s, box)),
                     ("com_backward_ms", lambda: torch.autograd.grad(com, x, g_com, retain_graph=True)),
                     ("nlist_forward_ms", lambda: htf.compute_nlist(beads, r_cut, a.nn, box, sorted=True)),
                     ("nlist_backward_ms", lambda: torch.autograd.grad(nl, beads, g_nl, retain_graph=True))):
        med, lo, hi = timed(fn, a.iters, a.windows)
        res[name] = round(med, 4)
        res[name.replace("_ms", "_range_ms")] = [round(lo, 4), round(hi, 4)]
    res["nlist_forward_gpairs_per_s"] = round(B * B / (res["nlist_forward_ms"] * 1e-3) / 1e9, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
