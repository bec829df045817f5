#!/usr/bin/env python
"""Measurement: the two activation-map kernels (ieee_actmap_energy, ieee_actmap_render) at the visualisation tool's size
next to the same arithmetic in torch device ops on the same tensors (permute to NCHW fp32, pow / sum, F.normalize,
F.interpolate(align_corners=False), min-max scaling, a table gather, the image and the overlay).  LABNOTES R11.1.

  python scripts/actmap_probe.py --n 300 --dtype bf16            (device events: ms per call of each path)
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/actmap_probe.py --n 300 --dtype bf16 --iters 5

N images of a [16 x 8 x 2048] trunk map -> figures of 256 x 128.  Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ieee_amd  # noqa: E402,F401


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="kernels only")
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from ieee_amd import _lib
    from ieee_amd.reidtools import IMAGENET_MEAN, IMAGENET_STD, activation_maps, jet_table, render_actmaps
    _lib.require_gpu()
    N, h, w, C, height, width = args.n, 16, 8, 2048, 256, 128
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(1, N, h, w, C, generator=g, device="cuda").clamp_(min=0).to(dt)       # native form, behind a ReLU
    imgs = torch.randn(N, 3, height, width, generator=g, device="cuda")
    lut = torch.from_numpy(jet_table()).cuda()
    mean = torch.tensor(IMAGENET_MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(IMAGENET_STD, device="cuda").view(1, 3, 1, 1)

    def native():
        a = activation_maps(x)[0]
        return a, render_actmaps(imgs, a, width, height)

    def torch_ops():
        out = x[0].permute(0, 3, 1, 2).float()                                  # what return_featuremaps=True hands over
        out = (out ** 2).sum(1)
        a = F.normalize(out.view(N, h * w), p=2, dim=1).view(N, h, w)
        am = F.interpolate(a[:, None], size=(height, width), mode="bilinear", align_corners=False)[:, 0]
        mn, mx = am.amin((1, 2), keepdim=True), am.amax((1, 2), keepdim=True)
        idx = torch.floor(255 * (am - mn) / (mx - mn + 1e-12)).clamp_(0, 255).long()
        col = lut[idx]                                                          # [N, height, width, 3]
        pix = torch.floor((imgs * std + mean).clamp_(0, 1) * 255).permute(0, 2, 3, 1)
        ov = (pix.double() * 0.3 + col.double() * 0.7).clamp_(max=255).to(torch.uint8)
        grid = torch.full((N, height, 3 * width + 20, 3), 255, dtype=torch.uint8, device="cuda")
        grid[:, :, :width] = pix.to(torch.uint8)
        grid[:, :, width + 10:2 * width + 10] = col
        grid[:, :, 2 * width + 20:] = ov
        return a, grid

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    res = {"n": N, "dtype": args.dtype, "iters": args.iters,
           "map_bytes": N * h * w * C * x.element_size(), "figure_bytes": N * height * (3 * width + 20) * 3,
           "image_bytes": N * 3 * height * width * 4}
    # alternate the two paths so that both see the same machine
    ms = {"native": [], "torch": []}
    for _ in range(3):
        ms["native"].append(timed(native))
        if not args.no_torch:
            ms["torch"].append(timed(torch_ops))
    res["native_ms"] = ms["native"]
    res["torch_ms"] = ms["torch"]
    if not args.no_torch:
        a_n, g_n = native()
        a_t, g_t = torch_ops()
        res["max_map_diff"] = float((a_n - a_t).abs().max())
        res["grid_bytes_differing_share"] = float((g_n != g_t).float().mean())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
