#!/usr/bin/env python
"""Train-step time per optimizer: full-size Image3MEngine steps (B = 64 triples, 171 classes, bf16 unless --dtype fp32) over
one resident synthetic batch with build_optimizer(model, optim=..., [staged_lr]), timed with one HIP event pair per step.

  python scripts/optim_probe.py --optim rmsprop --steps 20 --warmup 5 [--staged-lr]
  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/optim_probe.py --optim radam --steps 5 --warmup 2

Prints one JSON line: optimizer class, whether the engine's fused step is taken, launches per optimizer step, and the
median / min / max step time.  Uses only the package's public surface, so the same file times an older tree."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ieee_amd  # noqa: E402,F401  (before torch.cuda is touched: it picks GPU_MAX_HW_QUEUES)

import torch  # noqa: E402

HEADS = ["fc_R", "fc_T", "fc_N", "classifier_R", "classifier_N", "classifier_T"]


class _DM(object):
    num_train_pids = 171
    train_loader = []
    test_loader = {}
    sources = ["synthetic"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--optim", default="sgd", choices=["adam", "amsgrad", "sgd", "rmsprop", "radam"])
    ap.add_argument("--staged-lr", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--momentum", type=float, default=0.9, help="sgd / rmsprop")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    from ieee_amd.engine import Image3MEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    torch.manual_seed(0)
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    model = build_model("ieee3modalPart", num_classes=171, loss="margin", pretrained=False, compute_dtype=dt)
    kw = dict(staged_lr=True, new_layers=HEADS, base_lr_mult=0.1) if args.staged_lr else {}
    opt = build_optimizer(model, optim=args.optim, lr=1e-4, weight_decay=5e-4, momentum=args.momentum, **kw)
    eng = Image3MEngine(_DM(), model, opt, margin=1, weight_m=1, weight_x=1, use_gpu=True, label_smooth=True)
    model.train()
    B = args.batch
    gen = torch.Generator().manual_seed(1)
    imgs = [torch.randn(B, 3, 256, 128, generator=gen).cuda() for _ in range(3)]
    pids = (torch.arange(B) // 4).cuda()
    batch = {"img": imgs, "pid": pids, "camid": pids * 0, "impath": "", "timeid": pids * 0}
    for _ in range(args.warmup):
        eng.forward_backward(batch)
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for e0, e1 in events:
        e0.record()
        s = eng.forward_backward(batch)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in events)
    out = {"tag": args.tag, "optim": args.optim, "staged_lr": args.staged_lr, "class": type(opt).__name__,
           "momentum": args.momentum, "fused_step": bool(eng._fused_ok()), "dtype": args.dtype, "batch": B, "steps": args.steps,
           "ms_median": round(ms[len(ms) // 2], 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
           "loss": float(s["loss"])}
    if hasattr(opt, "launch_ranges"):
        out["launches_per_step"] = len(opt.launch_ranges())
        out["launches_by_part"] = [len(opt.launch_ranges(p)) for p in range(5)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
