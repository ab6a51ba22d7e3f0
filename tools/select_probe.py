#!/usr/bin/env python3
"""Times DeviationSelector.update beside the same selection written in torch ops with a read-back per frame.

Usage:  python tools/select_probe.py [--n 131072] [--capacity 64] [--updates 200] [--windows 5] [--warmup 1] [--json PATH]

One device, one process.  A frame is a deviation tensor [N, 2] fp32 (uniform random, fixed seed) and positions [N, 4] fp32; with
lo = 0 and hi = inf every frame is a candidate, so policy "first" stores the first --capacity frames of a window and drops the
rest: both routes copy the same frames.
  (a) selector   sel.update(deviation, positions, box): three launches, nothing read back
  (b) torch      s = deviation[:, 0].max().item(); the class from s on the host; buffer[n].copy_(positions) while n < capacity:
                 what a user writes without the selector, one synchronising read-back per frame
A window is --updates updates after a reset, between two device events; the host clock around the same window, ended by a device
synchronise, is reported beside it (for (a) the gap between the two is the enqueue running ahead of the device).  (a) and (b)
alternate window by window after --warmup windows of each.  Reported: the median over --windows windows of the time per update in
microseconds, with the smallest and largest.  Prints one JSON line.  No threshold: nothing passes or fails here but the check
that both routes kept the same frames.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402


def window(fn, reset, updates):
    """(device microseconds, host microseconds) per update of one window."""
    reset()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for k in range(updates):
        fn(k)
    b.record()
    b.synchronize()
    t1 = time.perf_counter()
    return 1e3 * a.elapsed_time(b) / updates, 1e6 * (t1 - t0) / updates


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, cap = a.n, a.capacity
    g = torch.Generator(device=dev).manual_seed(17)
    # a few distinct frames, so that consecutive updates do not read one cached tensor
    devs = [torch.rand((N, 2), device=dev, generator=g) for _ in range(8)]
    poss = [torch.randn((N, 4), device=dev, generator=g) for _ in range(8)]
    box = torch.tensor([[0.0, 0, 0], [50.0, 50, 50], [0.0, 0, 0]], device=dev)
    lo, hi = 0.0, float("inf")

    sel = htf.DeviationSelector(N, cap, lo, hi, policy="first")

    def selector(k):
        sel.update(devs[k % 8], poss[k % 8], box)

    buf = torch.zeros((cap, N, 4), device=dev)
    boxes = torch.zeros((cap, 3, 3), device=dev)
    kept = {"n": 0, "s": []}

    def torch_reset():
        kept["n"], kept["s"] = 0, []

    def torch_ops(k):
        s = devs[k % 8][:, 0].max().item()
        if s != s or s >= hi or s < lo:
            return
        if kept["n"] < cap:
            buf[kept["n"]].copy_(poss[k % 8])
            boxes[kept["n"]].copy_(box)
            kept["s"].append(s)
            kept["n"] += 1

    routes = {"selector": (selector, sel.reset), "torch": (torch_ops, torch_reset)}
    for _ in range(a.warmup):
        for fn, reset in routes.values():
            window(fn, reset, a.updates)
    us = {k: [] for k in routes}
    for _ in range(a.windows):
        for k, (fn, reset) in routes.items():
            us[k].append(window(fn, reset, a.updates))
    # the same frames kept
    f = sel.frames()
    n = min(cap, a.updates)
    if not (len(f["s"]) == kept["n"] == n and np.array_equal(f["s"], np.array(kept["s"], np.float32))
            and np.array_equal(f["positions"], buf[:n].cpu().numpy())):
        raise SystemExit("select_probe: the two routes kept different frames")

    out = {"shape": {"N": N, "capacity": cap}, "updates": a.updates, "windows": a.windows, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "binding": htf._lib.BINDING}
    for k, v in us.items():
        d, h = np.array([x[0] for x in v]), np.array([x[1] for x in v])
        out[k + "_device_us"] = [float(np.median(d)), float(d.min()), float(d.max())]
        out[k + "_host_us"] = [float(np.median(h)), float(h.min()), float(h.max())]
    out["torch_over_selector_host"] = out["torch_host_us"][0] / out["selector_host_us"][0]
    out["note"] = ("(median, min, max) microseconds per update over the windows; device: between two events; host: wall clock "
                   "around the window, ended by a synchronise; the first --capacity updates of a window copy a frame; one run on one device")
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
