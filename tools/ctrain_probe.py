#!/usr/bin/env python3
"""Times the force-matching sweep on the conservative forces (htf_ct_loss_grad) beside the row sweep (htf_bp_loss_grad).

Usage:  python tools/ctrain_probe.py [--n 131072] [--nn 128] [--block 2048] [--iters 20] [--warmup 5] [--r-cut RC] [--out PATH]

The same tensor for both: N rows x NN slots, K = 32 channels, 64 x 64 tanh, one type -- a block of --block random rows tiled
N / block times.  The index holds, for every slot, a random row of the slot's own tile (the block's index shifted by the
block size per tile: the neighbors of a spatially sorted system sit near their row), and in a second timing a random row of
the whole table (the worst case for the gather: N * 16 bytes of residuals, 2 MB at 131 072 rows).  HIP events around each
call (sweep + reduction), the median of --iters calls after --warmup, all in one process on one device.  Per live slot the
new sweep reads 4 bytes of index and gathers 16 bytes of residual beside the 16 bytes of pair vector both stream.
Prints the times and their ratios; --out also writes them to a file.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402
from hoomd_tf_amd import _lib, ops  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=128)
    ap.add_argument("--block", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--r-cut", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, NN, nb, K, H = a.n, a.nn, a.block, 32, 64
    if N % nb:
        ap.error("--n must be a multiple of --block")
    rep = N // nb
    g = torch.Generator(device=dev).manual_seed(31)
    cnt = torch.randint(NN // 2, NN + 1, (nb, 1), device=dev, generator=g)
    d = torch.randn((nb, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((nb, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((nb, NN, 1), device=dev)], dim=2).repeat(rep, 1, 1).contiguous()
    shift = (nb * torch.arange(rep, dtype=torch.int32, device=dev)).repeat_interleave(nb)[:, None]
    tiled = (torch.randint(0, nb, (nb, NN), device=dev, generator=g).to(torch.int32).repeat(rep, 1) + shift).contiguous()
    whole = torch.randint(0, N, (N, NN), device=dev, generator=g).to(torch.int32).contiguous()
    lay = htf.DescriptorMLP(K=K, H1=H, H2=H, seed=9, trainable="total", **({"r_cut": a.r_cut} if a.r_cut is not None else {}))
    pred = lay.forces(x)
    labels = (pred + 0.05 * torch.randn((N, 4), device=dev, generator=g)).contiguous()
    rho = (pred - labels).contiguous()
    accum = torch.empty(1 + lay.P, dtype=torch.float32, device=dev)
    scratch = torch.empty(int(_lib.lib.htf_bp_scratch_floats(N, K, 1, H, H)), dtype=torch.float32, device=dev)
    rc, stream = float(lay.r_cut or 0.0), ops._stream(x)

    def row_sweep():
        _lib.check(_lib.lib.htf_bp_loss_grad(x.data_ptr(), _lib.HTF_F32, N, NN, K, 1, H, H, _lib.ACT_TANH, lay.w.data_ptr(),
                                             lay.mu.data_ptr(), float(lay.gap), labels.data_ptr(), _lib.HTF_F32, pred.data_ptr(),
                                             accum.data_ptr(), scratch.data_ptr(), None, N, rc, stream))

    def total_sweep(index):
        _lib.check(_lib.lib.htf_ct_loss_grad(x.data_ptr(), _lib.HTF_F32, index.data_ptr(), N, NN, K, 1, H, H, _lib.ACT_TANH,
                                             lay.w.data_ptr(), lay.mu.data_ptr(), float(lay.gap), rho.data_ptr(), accum.data_ptr(),
                                             scratch.data_ptr(), None, N, rc, stream))

    bp = timed(row_sweep, a.iters, a.warmup)
    ct = timed(lambda: total_sweep(tiled), a.iters, a.warmup)
    ctw = timed(lambda: total_sweep(whole), a.iters, a.warmup)
    live = float(mask.mean().item())
    lines = [
        "tools/ctrain_probe.py on %s: N = %d, NN = %d (%.0f%% of the slots live), K = %d, %d x %d tanh, r_cut %s, block %d x %d"
        % (torch.cuda.get_device_name(0), N, NN, 100 * live, K, H, H, a.r_cut, nb, rep),
        "median (min, max) in ms of %d calls after %d, sweep + reduction" % (a.iters, a.warmup),
        "htf_bp_loss_grad                      %.4f (%.4f, %.4f)" % bp,
        "htf_ct_loss_grad, index in its tile   %.4f (%.4f, %.4f)   ratio %.3f" % (ct + (ct[0] / bp[0],)),
        "htf_ct_loss_grad, index anywhere      %.4f (%.4f, %.4f)   ratio %.3f" % (ctw + (ctw[0] / bp[0],)),
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
