#!/usr/bin/env python3
"""Times the force-matching sweep on the angular conservative forces (htf_at_loss_grad) beside the radial one (htf_ct_loss_grad)
and beside total_forces at the same l_max.

Usage:  python tools/atrain_probe.py [--n 131072] [--nn 128] [--block 2048] [--iters 20] [--warmup 5] [--r-cut RC] [--out PATH]

The same tensor for all: N rows x NN slots, K = 16 channels, one type, 32 x 32 tanh, fp32 -- a block of --block random rows tiled
N / block times, the index a random row of the slot's own tile (tools/ctrain_probe.py).  The networks read D = 16, 32 and 48
inputs for l_max = 0, 1 and 2.  HIP events around each call (sweep + reduction; for total_forces its two passes), the median of
--iters calls after --warmup, all in one process on one device.  Beside each angular sweep, htf_ct_loss_grad of an l_max = 0
layer with K = D channels: the same network width, so the same steps 3 to 5, with 2 D wave sums per row.  Prints the times
and the ratios to htf_ct_loss_grad at K = 16; --out also writes them to a file.
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
    N, NN, nb, K, H = a.n, a.nn, a.block, 16, 32
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
    index = (torch.randint(0, nb, (nb, NN), device=dev, generator=g).to(torch.int32).repeat(rep, 1) + shift).contiguous()
    rho = (0.05 * torch.randn((N, 4), device=dev, generator=g)).contiguous()
    cut = {"r_cut": a.r_cut} if a.r_cut is not None else {}
    stream = ops._stream(x)
    lines = [
        "tools/atrain_probe.py on %s: N = %d, NN = %d (%.0f%% of the slots live), K = %d, %d x %d tanh, r_cut %s, block %d x %d"
        % (torch.cuda.get_device_name(0), N, NN, 100 * float(mask.mean().item()), K, H, H, a.r_cut, nb, rep),
        "median (min, max) in ms of %d calls after %d" % (a.iters, a.warmup),
    ]
    base = None
    for l_max in (0, 1, 2):
        lay = htf.DescriptorMLP(K=K, H1=H, H2=H, seed=9, conservative=True, l_max=l_max, **cut)
        accum = torch.empty(1 + lay.P, dtype=torch.float32, device=dev)
        scratch = torch.empty(int(_lib.lib.htf_bp_scratch_floats(N, K, 1 + l_max, H, H)), dtype=torch.float32, device=dev)
        rc = float(lay.r_cut or 0.0)

        def sweep(lay=lay, accum=accum, scratch=scratch, rc=rc, l_max=l_max):
            head = (x.data_ptr(), _lib.HTF_F32, index.data_ptr(), N, NN, K, 1, H, H, _lib.ACT_TANH, lay.w.data_ptr(),
                    lay.mu.data_ptr(), float(lay.gap), rho.data_ptr(), accum.data_ptr(), scratch.data_ptr(), None, N, rc)
            if l_max:
                _lib.check(_lib.lib.htf_at_loss_grad(*(head + (l_max, stream))))
            else:
                _lib.check(_lib.lib.htf_ct_loss_grad(*(head + (stream,))))

        sw = timed(sweep, a.iters, a.warmup)
        tf = timed(lambda lay=lay: lay.total_forces(x, index), a.iters, a.warmup)
        base = sw[0] if base is None else base
        if l_max:   # the radial sweep at the same network width: steps 3 to 5 alike, 2 D wave sums per row against 8 K or 20 K
            wide = htf.DescriptorMLP(K=lay.D, H1=H, H2=H, seed=9, conservative=True, **cut)
            scr = torch.empty(int(_lib.lib.htf_bp_scratch_floats(N, lay.D, 1, H, H)), dtype=torch.float32, device=dev)

            def same_width(wide=wide, accum=accum, scr=scr, rc=rc):
                _lib.check(_lib.lib.htf_ct_loss_grad(x.data_ptr(), _lib.HTF_F32, index.data_ptr(), N, NN, wide.K, 1, H, H,
                                                     _lib.ACT_TANH, wide.w.data_ptr(), wide.mu.data_ptr(), float(wide.gap),
                                                     rho.data_ptr(), accum.data_ptr(), scr.data_ptr(), None, N, rc, stream))

            cw = timed(same_width, a.iters, a.warmup)
        name = "htf_at_loss_grad" if l_max else "htf_ct_loss_grad"
        lines.append("l_max = %d, D = %2d: %s %.4f (%.4f, %.4f)   ratio to l_max = 0 %.3f;   total_forces %.4f (%.4f, %.4f)"
                     % ((l_max, lay.D, name) + sw + (sw[0] / base,) + tf))
        if l_max:
            lines.append("              htf_ct_loss_grad at K = %d (l_max = 0, D = %d) %.4f (%.4f, %.4f)" % ((lay.D, lay.D) + cw))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
