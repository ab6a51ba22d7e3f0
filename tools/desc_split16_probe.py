#!/usr/bin/env python3
"""Times the dense stacks of DescriptorMLP(conservative=True) -- dense="lanes" (htf_cf_grad, up to 64 units), dense="mfma"
(htf_cfw_grad) and dense="split16" (htf_cfw16_grad) -- at tools/desc_wide_probe.py's box and protocol, in one run.

Usage:  python tools/desc_split16_probe.py [--n 131072] [--nn 128] [--samples 15] [--reps 10] [--warmup 3] [--window W] [--json PATH]

N rows x NN slots of a liquid-like list (60 to NN live slots per row, distances 0.8 to 3.2, the slots' particles within
--window rows of their own row), K = 16 channels, one type, tanh, fp32.  For the widths 32 x 32, 64 x 64, 128 x 128 and
256 x 256: pass 1 alone and whole total_forces calls of every stack that takes the width.  A sample is --reps calls between two
device events, divided by --reps; the stacks alternate sample by sample after --warmup samples of each; medians of --samples
samples are reported with the smallest and largest.  Also per width: the largest difference of the split16 forces from the mfma
forces over the largest force, and the dense FLOPs -- 4 (D H1 + H1 H2) + 2 H2 per row, forward and backward -- over the
split16 pass-1 time (which also forms the descriptor) as a share of --peak-tflops: the fp16 matrix peak of the MI355X, 2 500,
divided by the three products of a split step.  Prints one JSON line.
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

ENTRY = {"lanes": "htf_cf_grad", "mfma": "htf_cfw_grad", "split16": "htf_cfw16_grad"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=128)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--peak-tflops", type=float, default=2500.0 / 3.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, NN = a.n, a.nn
    g = torch.Generator(device=dev).manual_seed(31)
    cnt = torch.randint(60, NN + 1, (N, 1), device=dev, generator=g)
    d = torch.randn((N, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=dev)], dim=2).contiguous()
    rows = torch.arange(N, device=dev)[:, None]
    near = ((rows + torch.randint(-a.window, a.window + 1, (N, NN), device=dev, generator=g)) % N).to(torch.int32).contiguous()
    stream = ops._stream(x)

    out = {"shape": {"N": N, "NN": NN, "K": 16, "activation": "tanh"}, "samples": a.samples, "reps": a.reps, "warmup": a.warmup,
           "window": a.window, "device": torch.cuda.get_device_name(0), "peak_tflops": a.peak_tflops, "widths": {}}
    for H in (32, 64, 128, 256):
        stacks = ("lanes", "mfma", "split16") if H <= 64 else ("mfma", "split16")
        lays = {s: htf.DescriptorMLP(K=16, H1=H, H2=H, seed=9, conservative=True, dense=s) for s in stacks}
        gbuf = torch.empty((N, 16), dtype=torch.float32, device=dev)
        ebuf = torch.empty((N,), dtype=torch.float32, device=dev)

        def pass1(s):
            lay, entry = lays[s], getattr(_lib.lib, ENTRY[s])
            return lambda: _lib.check(entry(x.data_ptr(), _lib.HTF_F32, N, NN, 16, 1, H, H, _lib.ACT_TANH, lay.w.data_ptr(),
                                            lay.mu.data_ptr(), float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), None, N, 0.0, stream))

        f = {s: lays[s].total_forces(x, near).double() for s in stacks}   # the same answer first
        res = {"split16_vs_mfma_rel": (f["split16"] - f["mfma"]).abs().max().item() / f["mfma"].abs().max().item()}
        res.update(alternate({"pass1_%s_ms" % s: pass1(s) for s in stacks}, a.samples, a.reps, a.warmup))
        res.update(alternate({"total_%s_ms" % s: (lambda lay=lays[s]: lay.total_forces(x, near)) for s in stacks},
                             a.samples, a.reps, a.warmup))
        flops = N * (4.0 * (16 * H + H * H) + 2.0 * H)
        res["dense_gflop"] = flops * 1e-9
        res["split16_share_of_peak"] = flops / (res["pass1_split16_ms"][0] * 1e-3) / (a.peak_tflops * 1e12)
        out["widths"]["%dx%d" % (H, H)] = res
    out["note"] = "(median, min, max) in ms per call; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
