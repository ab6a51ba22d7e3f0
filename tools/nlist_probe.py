"""Times compute_nlist on both routes (all-pairs: csrc/cg_map.hip; cell-binned: csrc/nlist_cells.hip) at density 1, r_cut for
about 40 neighbors, NN = 64, sorted, and the frames/s of iter_from_trajectory + an LJ SimModel over 100 frames.  Device
events around ``--iters`` calls per window, the median of ``--windows`` windows; the box is a host list (no read-back).
The crossover M_min of cgmap.NLIST_CELLS_MIN_M is read from this table.  One JSON line.

    python tools/nlist_probe.py [--nn 64] [--iters 10] [--windows 5] [--frames 100]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402
from hoomd_tf_amd import cgmap  # noqa: E402

SIZES = (1024, 8192, 43691, 131072)
CELLS_ONLY = (1048576,)


def timed(fn, iters, windows):
    for _ in range(2):
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
    return round(float(np.median(out)), 4)


def cloud(M, neighbors, dev, seed=1):
    L = float(M) ** (1.0 / 3.0)
    r_cut = (neighbors / (4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)
    p = np.random.default_rng(seed).uniform(-L / 2, L / 2, (M, 3)).astype(np.float32)
    return torch.from_numpy(p).to(dev), L, r_cut


class LJ(htf.SimModel):
    def compute(self, nlist, positions, box):
        rinv = htf.nlist_rinv(nlist)
        inv_r6 = rinv ** 6
        energy = htf.reduce_sum(4.0 / 2.0 * (inv_r6 * inv_r6 - inv_r6), axis=1)
        return htf.compute_nlist_forces(nlist, energy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nn", type=int, default=64)
    ap.add_argument("--neighbors", type=float, default=40.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--traj-atoms", type=int, default=131072)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nlist_probe: needs a GPU")
    dev = torch.device("cuda:0")
    rows = []
    default_min = cgmap.NLIST_CELLS_MIN_M
    for M in SIZES + CELLS_ONLY:
        x, L, r_cut = cloud(M, a.neighbors, dev)
        row = {"M": M, "L": round(L, 3), "r_cut": round(r_cut, 4), "grid": list(cgmap._cell_grid(M, [L] * 3, np.float32(r_cut)))}
        for route, min_m in (("cells", 0), ("all_pairs", 1 << 62)):
            if route == "all_pairs" and M in CELLS_ONLY:
                continue
            cgmap.NLIST_CELLS_MIN_M = min_m
            row[route + "_ms"] = timed(lambda: htf.compute_nlist(x, r_cut, a.nn, [L] * 3, sorted=True), a.iters, a.windows)
        cgmap.NLIST_CELLS_MIN_M = default_min
        if "all_pairs_ms" in row:
            row["speedup"] = round(row["all_pairs_ms"] / row["cells_ms"], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)

    # the offline path: 100 frames of 131 072 atoms through iter_from_trajectory and an LJ SimModel
    N = a.traj_atoms
    L = float(N) ** (1.0 / 3.0)
    r_cut = (a.neighbors / (4.0 / 3.0 * math.pi)) ** (1.0 / 3.0)
    rng = np.random.default_rng(2)
    base = rng.uniform(0, L, (N, 3))
    P = np.stack([base + 0.05 * rng.standard_normal((N, 3)) for _ in range(a.frames)]).astype(np.float32)
    traj = htf.ArrayTrajectory(P, [L] * 3 + [90.0] * 3, types=np.arange(N) % 2)
    model = LJ(a.nn)
    for inputs, _ in htf.iter_from_trajectory(a.nn, traj, r_cut=r_cut, end=1):
        model(inputs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for inputs, _ in htf.iter_from_trajectory(a.nn, traj, r_cut=r_cut):
        f = model(inputs)[0]
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res = {"probe": "nlist", "device": torch.cuda.get_device_name(0), "nn": a.nn, "neighbors": a.neighbors,
           "route_rule_min_m": default_min, "table": rows,
           "trajectory": {"atoms": N, "frames": n, "r_cut": round(r_cut, 4), "route": cgmap._nlist_route(N, [L] * 3, r_cut),
                          "frames_per_s": round(n / dt, 2), "ms_per_frame": round(dt / n * 1e3, 3),
                          "force_finite": bool(torch.isfinite(f).all())}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
