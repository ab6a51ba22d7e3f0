"""Times htf.DescriptorMLP (csrc/bp.hip over desc_row.h) against the same network written with RBFExpansion and Dense on the torch route.

For each shape: a random [N, NN, 4] fp32 pair-vector tensor (60..NN live neighbors per row at 0.8 <= r <= 3.2, zero padding),
the layer with K channels on [0, 3], H1 = H2 hidden units, tanh.  Timed: compute_nlist_forces(nlist, layer(nlist)) (the
kernel), layer.descriptor(nlist) (its first stage), and compute_nlist_forces of the RBFExpansion -> masked sum -> Dense x 3
energy under the same weights (torch ops + autograd, [N, NN, K] intermediates).  Device events around --iters calls per
window, the median of --windows windows (every window is listed too).  A torch route that runs out of device memory is
reported as such.  --r-cut RC gives the layer the cosine cutoff, --species S one network per species with the rows split
evenly (row i is species i mod S); the torch route is written for neither and is then left out, as with --no-torch.
One JSON line.

    python tools/desc_probe.py [--iters 10] [--windows 7] [--r-cut RC] [--species S] [--no-torch]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402

SHAPES = (("c3", 131072, 128, 32, 1, 64, 64), ("small", 4096, 64, 32, 1, 64, 64))


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
    return float(np.median(out)), [round(t, 4) for t in out]


def pair_vectors(N, NN, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    cnt = torch.randint(min(60, NN), NN + 1, (N, 1), device=dev, generator=g)
    d = torch.randn((N, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    return torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=dev)], dim=2).contiguous()


def layers_route(lay):
    """The network as a user writes it with the layers (tests/test_gpu_generic.py's descriptor model, three Dense)."""
    ws = lay.get_weights()
    rbf = htf.RBFExpansion(lay.low, lay.high, lay.K)
    ds = [htf.Dense(lay.H1, activation="tanh"), htf.Dense(lay.H2, activation="tanh"), htf.Dense(1)]
    for d, (k, b) in zip(ds, ((ws[0], ws[1]), (ws[2], ws[3]), (ws[4], ws[5]))):
        d.build(k.shape[0])
        d.set_weights([k, b])

    def run(x):
        nl = htf.Nlist(x)
        r = htf.safe_norm(nl[:, :, :3], axis=2)
        live = (htf.nlist_rinv(nl).tensor() > 0).to(torch.float32)
        g = (rbf(r) * live[..., None]).sum(dim=1)
        return htf.compute_nlist_forces(nl, ds[2](ds[1](ds[0](g)))[:, 0])
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--r-cut", type=float, default=None)
    ap.add_argument("--species", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("desc_probe: needs a GPU")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "windows": a.windows, "r_cut": a.r_cut,
           "species": a.species, "shapes": []}
    extra = {}
    if a.r_cut is not None:
        extra["r_cut"] = a.r_cut
    if a.species != 1:
        extra["n_species"] = a.species
    for name, N, NN, K, T, H1, H2 in SHAPES:
        x = pair_vectors(N, NN, dev, seed=len(res["shapes"]) + 1)
        lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.0, high=3.0, n_types=T, activation="tanh", seed=3, **extra)
        nl = htf.Nlist(x)
        if a.species != 1:
            pos = torch.zeros((N, 4), device=dev)
            pos[:, 3] = (torch.arange(N, device=dev) % a.species).to(torch.float32)
            energy = lambda: lay(nl, pos)   # noqa: E731
        else:
            energy = lambda: lay(nl)        # noqa: E731
        row = {"shape": name, "N": N, "NN": NN, "K": K, "n_types": T, "H1": H1, "H2": H2,
               "pair_tensor_MB": round(x.numel() * 4 / 1e6, 1)}
        fk = htf.compute_nlist_forces(nl, energy())
        med, row["kernel_ms_windows"] = timed(lambda: htf.compute_nlist_forces(nl, energy()), a.iters, a.windows)
        row["kernel_ms"] = round(med, 4)
        row["descriptor_ms"] = round(timed(lambda: lay.descriptor(nl), a.iters, a.windows)[0], 4)
        row["kernel_read_TBps"] = round(x.numel() * 4 / (row["kernel_ms"] * 1e-3) / 1e12, 2)
        if extra or a.no_torch:
            htf.simmodel._trace_log().clear()
            res["shapes"].append(row)
            del x, fk, nl
            torch.cuda.empty_cache()
            continue
        run = layers_route(lay)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        try:
            ft = run(x)
            row["torch_ms"] = round(timed(lambda: run(x), max(1, a.iters // 2), a.windows)[0], 3)
            row["torch_peak_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
            scale = ft[:, :3].abs().max().item()
            row["max_force_diff_rel"] = float((fk[:, :3] - ft[:, :3]).abs().max().item() / scale)
            row["speedup"] = round(row["torch_ms"] / row["kernel_ms"], 1)
            del ft
        except torch.cuda.OutOfMemoryError as e:
            row["torch_ms"] = None
            row["torch_route"] = "out of device memory: %s" % str(e).split("\n")[0][:160]
        htf.simmodel._trace_log().clear()
        res["shapes"].append(row)
        del x, fk, nl
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
