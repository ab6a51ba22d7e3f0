#!/usr/bin/env python3
"""Times the force-matching sweep for three hidden layers, DescriptorMLP.deep_loss_gradient (htf_cfw3_loss_grad), at
tools/desc_wide_train_probe.py's box and protocol, beside the two-layer sweep (htf_cfw_loss_grad) at the same H1 x H2.

Usage:  python tools/desc_deep_train_probe.py [--n 131072] [--nn 128] [--samples 15] [--reps 5] [--warmup 3] [--window W] [--json PATH]

N rows x NN slots of a liquid-like list (60 to NN live slots per row, distances 0.8 to 3.2, the slots' particles within
--window rows of their own row), K = 16 channels, one type, tanh, fp32, a random residual table.  For 64^3, 128^3,
160-128-96, 240^3 and 256^3 (the last two on the 16-row tile): the C entry alone, residual and scratch made beforehand, the
two sweeps alternating sample by sample.  A sample is --reps calls between two device events, divided by --reps; medians of
--samples samples after --warmup of each are reported with the smallest and largest.  Also: the share of --peak-tflops (the
fp32 matrix peak, 157.3 on the MI355X) that each sweep's dense FLOPs reach -- per row 8 D H1 + 12 H1 H2 (+ 12 H2 H3): forward
and backward with tangent, and the outer products.  No time is a pass or fail condition.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402
from hoomd_tf_amd import _lib, ops  # noqa: E402
from committee_probe import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=128)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--peak-tflops", type=float, default=157.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, NN, K = a.n, a.nn, 16
    g = torch.Generator(device=dev).manual_seed(31)
    cnt = torch.randint(60, NN + 1, (N, 1), device=dev, generator=g)
    d = torch.randn((N, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=dev)], dim=2).contiguous()
    rows = torch.arange(N, device=dev)[:, None]
    near = ((rows + torch.randint(-a.window, a.window + 1, (N, NN), device=dev, generator=g)) % N).to(torch.int32).contiguous()
    rho = (0.05 * torch.randn((N, 4), device=dev, generator=g)).contiguous()
    stream = ops._stream(x)
    lib = _lib.lib

    out = {"shape": {"N": N, "NN": NN, "K": K, "activation": "tanh"}, "samples": a.samples, "reps": a.reps, "warmup": a.warmup,
           "window": a.window, "device": torch.cuda.get_device_name(0), "peak_tflops": a.peak_tflops, "widths": {}}
    for H1, H2, H3 in ((64, 64, 64), (128, 128, 128), (160, 128, 96), (240, 240, 240), (256, 256, 256)):
        lays = {"deep": htf.DescriptorMLP(K=K, H1=H1, H2=H2, H3=H3, seed=9, conservative=True, dense="mfma"),
                "wide": htf.DescriptorMLP(K=K, H1=H1, H2=H2, seed=9, conservative=True, dense="mfma")}
        floats = {"deep": lib.htf_cfw3_scratch_floats(N, K, 1, H1, H2, H3), "wide": lib.htf_cfw_scratch_floats(N, K, 1, H1, H2)}
        accum = {s: torch.empty(1 + lays[s].P, dtype=torch.float32, device=dev) for s in lays}
        scratch = {s: torch.empty(int(floats[s]), dtype=torch.float32, device=dev) for s in lays}

        def sweep(s):
            lay = lays[s]
            entry, widths = (lib.htf_cfw3_loss_grad, (H1, H2, H3)) if s == "deep" else (lib.htf_cfw_loss_grad, (H1, H2))
            return lambda: _lib.check(entry(x.data_ptr(), _lib.HTF_F32, near.data_ptr(), N, NN, K, 1, *widths, _lib.ACT_TANH,
                                            lay.w.data_ptr(), lay.mu.data_ptr(), float(lay.gap), rho.data_ptr(), accum[s].data_ptr(),
                                            scratch[s].data_ptr(), None, N, 0.0, stream))

        res = {"scratch_mb": {s: 4e-6 * int(floats[s]) for s in lays}}
        res.update(alternate({"sweep_%s_ms" % s: sweep(s) for s in lays}, a.samples, a.reps, a.warmup))
        flops = {"wide": N * (8.0 * K * H1 + 12.0 * H1 * H2)}
        flops["deep"] = flops["wide"] + N * 12.0 * H2 * H3
        res["dense_gflop"] = {s: flops[s] * 1e-9 for s in lays}
        res["share_of_peak"] = {s: flops[s] / (res["sweep_%s_ms" % s][0] * 1e-3) / (a.peak_tflops * 1e12) for s in lays}
        assert all(torch.isfinite(accum[s]).all() for s in lays)
        out["widths"]["%dx%dx%d" % (H1, H2, H3)] = res
    out["note"] = "(median, min, max) in ms per call; one run on one device; wide = the two-layer sweep at the same H1 x H2"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
