#!/usr/bin/env python
"""Measurement: ieee_tsne_affinities and 1 000 iterations of ieee_tsne_run at the sizes the figure is drawn at -- 3 x 836
(RGBNT201 queries) and 3 x 3368 (Market-1501 queries) -- next to the same dense algorithm in torch device ops on the
same matrices, by device events, and the bytes of P the pairwise kernel reads per iteration against the HBM and
Infinity-Cache rates.  LABNOTES R12.1.

  python scripts/tsne_probe.py                       (both sizes)
  python scripts/tsne_probe.py --n 836 --torch-iters 100

The torch loop is timed over --torch-iters iterations and scaled to 1 000 (each iteration costs the same).  Needs the GPU."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ieee_amd  # noqa: E402,F401

HBM_TBS, MALL_TBS = 6.3, 8.6      # achievable HBM stream; Infinity-Cache-resident reads (measured elsewhere on this part)


def torch_affinities(dist, perplexity):
    """sklearn's search with every row stepping at once: 100 fixed steps, rows that have converged stop moving"""
    import torch
    B, n, _ = dist.shape
    eye = torch.eye(n, dtype=torch.bool, device=dist.device)
    d = dist.masked_fill(eye, float('inf'))
    d = d - d.amin(2, keepdim=True)
    beta = torch.ones(B, n, 1, device=dist.device)
    lo = torch.full_like(beta, -float('inf'))
    hi = torch.full_like(beta, float('inf'))
    target = math.log(perplexity)
    for _ in range(100):
        e = torch.exp(-beta * d)
        S = e.sum(2, keepdim=True)
        diff = torch.log(S) + (torch.nan_to_num(beta * d, posinf=0.0) * e).sum(2, keepdim=True) / S - target
        done = diff.abs() <= 1e-5
        up = (diff > 0) & ~done
        down = (diff <= 0) & ~done
        lo = torch.where(up, beta, lo)
        hi = torch.where(down, beta, hi)
        beta = torch.where(up, torch.where(torch.isinf(hi), beta * 2, (beta + hi) / 2), beta)
        beta = torch.where(down, torch.where(torch.isinf(lo), beta / 2, (beta + lo) / 2), beta)
    e = torch.exp(-beta * d)
    cond = e / e.sum(2, keepdim=True)
    return (cond + cond.transpose(1, 2)) / (2 * n)


def torch_run(P, Y, n_iter, exaggeration_iters, early_exaggeration, lr):
    import torch
    upd, gains = torch.zeros_like(Y), torch.ones_like(Y)
    n = P.shape[1]
    eye = torch.eye(n, dtype=torch.bool, device=P.device)
    for it in range(n_iter):
        early = it < exaggeration_iters
        diff = Y[:, :, None, :] - Y[:, None, :, :]
        w = (1.0 / (1.0 + (diff ** 2).sum(3))).masked_fill(eye, 0.0)
        Z = w.sum((1, 2), keepdim=True)
        pw = P * w * (early_exaggeration if early else 1.0)
        g = 4.0 * ((pw[..., None] * diff).sum(2) - ((w * w)[..., None] * diff).sum(2) / Z)
        gains = torch.where(upd * g < 0, gains + 0.2, gains * 0.8).clamp_(min=0.01)
        upd = (0.5 if early else 0.8) * upd - lr * gains * g
        Y = Y + upd
    return Y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[836, 3368])
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--torch-iters", type=int, default=100)
    ap.add_argument("--no-torch", action="store_true", help="kernels only")
    args = ap.parse_args()

    import torch
    from ieee_amd import _lib as L
    from ieee_amd.metrics import compute_distance_matrix
    from ieee_amd.reidtools import _pca_init
    lib = L.require_gpu()

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(reps):
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    for n in args.n:
        B = args.batch
        g = torch.Generator(device="cuda").manual_seed(n)
        ids = max(n // 4, 1)
        # identities of four images whose centres have an 8-dimensional structure (centre scale 2, unit noise): centres
        # drawn independently in all 768 dimensions are all equally far apart, the neighbour graph is then an expander, and
        # the collapsed start is a stable state of the descent in float32 and float64 alike (LABNOTES R12.1)
        centres = 2.0 * torch.randn(B, ids, 8, generator=g, device="cuda") @ torch.randn(B, 8, 768, generator=g, device="cuda") / 8 ** 0.5
        x = centres[:, torch.arange(n, device="cuda") % ids] + torch.randn(B, n, 768, generator=g, device="cuda")
        dist = torch.stack([compute_distance_matrix(x[b], x[b]) for b in range(B)])
        ldp = (n + 3) // 4 * 4
        P = torch.empty(B, n, ldp, device="cuda")
        beta = torch.empty(B, n, device="cuda")
        nbytes = lib.ieee_tsne_workspace_bytes(n, B)
        work = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        Y0 = _pca_init(x).contiguous()                   # tsne_embed's default start
        lr = max(n / 12.0 / 4.0, 50.0)

        def aff():
            L.check(lib.ieee_tsne_affinities(L.ptr(dist), n, n, B, 30.0, L.ptr(P), ldp, L.ptr(beta), L.ptr(work), nbytes,
                                             L.stream()))

        def run(history=None):
            Y, upd, gains = Y0.clone(), torch.zeros_like(Y0), torch.ones_like(Y0)
            L.check(lib.ieee_tsne_run(L.ptr(P), ldp, n, B, L.ptr(Y), L.ptr(upd), L.ptr(gains), 0, args.iters, 250, 12.0, lr,
                                      L.ptr(history), L.ptr(work), nbytes, L.stream()))
            return Y

        hist = torch.empty(B, args.iters, 2, device="cuda")
        res = {"n": n, "batch": B, "iters": args.iters, "p_bytes": B * n * ldp * 4, "workspace_bytes": nbytes}
        # alternate the paths so that both see the same machine
        res["affinities_ms"] = timed(aff, 3)
        res["run_ms"] = timed(run, 3)
        res["run_with_history_ms"] = timed(lambda: run(hist), 3)
        per_iter_s = min(res["run_ms"]) / 1e3 / args.iters
        res["p_read_tb_per_s"] = res["p_bytes"] / per_iter_s / 1e12
        res["p_read_share_of_hbm"] = res["p_read_tb_per_s"] / HBM_TBS
        res["p_read_share_of_infinity_cache"] = res["p_read_tb_per_s"] / MALL_TBS
        res["first_kl"] = [float(v) for v in hist[:, 0, 0]]
        res["final_kl"] = [float(v) for v in hist[:, -1, 0]]
        if not args.no_torch:
            Pt = [None]

            def t_aff():
                Pt[0] = torch_affinities(dist, 30.0)
            res["torch_affinities_ms"] = timed(t_aff, 2)
            res["torch_p_max_rel_diff"] = float(((Pt[0] - P[:, :, :n]).abs() / Pt[0].clamp_min(1e-30)).max())
            t = timed(lambda: torch_run(Pt[0], Y0, args.torch_iters, 250, 12.0, lr), 2)
            res["torch_run_ms_scaled_to_iters"] = [v * args.iters / args.torch_iters for v in t]
            res["affinities_ms_again"] = timed(aff, 2)
            res["run_ms_again"] = timed(run, 2)
        print(json.dumps(res))


if __name__ == "__main__":
    main()
