"""Times query expansion (ieee_amd.expansion) on one MI355X: the driver in both modes, the sum kernel alone, and the same
algorithm in torch device ops (dense similarities, topk, gather) where its N x N matrix fits, with the peak memory of
each.  Device events around every call, the candidates interleaved round by round, medians over the rounds.

    python scripts/expand_probe.py                         # 3368 x 19732 and 10000 x 100000, d = 2304, k = 5
    python scripts/expand_probe.py --sizes 3368,19732 --rounds 7 --out probe.json

One JSON line per (size, mode).  No time or ratio here is a gate."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3368,19732;10000,100000", help="Q,G;Q,G;...")
    ap.add_argument("--dim", type=int, default=2304)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--alpha", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ids", type=int, default=1500)
    ap.add_argument("--dense-share", type=float, default=0.25,
                    help="the torch form runs when its similarity matrix is below this share of the device's memory")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from ieee_amd import _lib
    from ieee_amd.expansion import expand_descriptors, expand_weights, expansion_layout, neighbour_sum, row_rinv
    _lib.require_gpu()
    d, k, alpha = args.dim, args.k, args.alpha

    def timed(fn):
        """-> (milliseconds by device events, peak bytes above what was allocated before)"""
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        del out
        return t0.elapsed_time(t1), torch.cuda.max_memory_allocated() - before

    def torch_form(q, g, mode):
        """the definition in torch device ops: the whole similarity matrix, topk, gather"""
        rows = torch.cat([q, g]) if mode == "both" else q
        cand = F.normalize(rows if mode == "both" else g, p=2, dim=1)
        sim = F.normalize(rows, p=2, dim=1) @ cand.t()
        val, idx = sim.topk(min(k, cand.shape[0]), dim=1)
        w = val.clamp_min(0).pow(alpha) if alpha else torch.ones_like(val)
        y = (w.unsqueeze(2) * cand[idx]).sum(1)
        if mode == "query":
            y = y + F.normalize(rows, p=2, dim=1)
        return F.normalize(y, p=2, dim=1)

    lines = []
    for size in args.sizes.split(";"):
        Q, G = (int(v) for v in size.split(","))
        gen = torch.Generator().manual_seed(0)
        centres = torch.randn(args.ids, d, generator=gen)
        pick = torch.randint(0, args.ids, (Q + G,), generator=gen)
        X = (centres[pick] + 0.5 * torch.randn(Q + G, d, generator=gen)).cuda()
        q, g = X[:Q], X[Q:]
        total = torch.cuda.get_device_properties(0).total_memory
        for mode in ("both", "query"):
            n_rows, n_cand = (Q + G, Q + G) if mode == "both" else (Q, G)
            forms = {"driver": lambda: expand_descriptors(q, g, k, alpha, mode=mode)}
            dense_fits = 4 * n_rows * n_cand < args.dense_share * total
            if dense_fits:
                forms["torch"] = lambda: torch_form(q, g, mode)
            # the sum kernel alone, on the driver's own lists
            _, _, (idx, dist) = expand_descriptors(q, g, k, alpha, mode=mode, return_neighbours=True)
            cand = X if mode == "both" else g
            idx32, w, rinv = idx.to(torch.int32), expand_weights(idx.to(torch.int32), dist, alpha), row_rinv(cand)
            own = dict(self_rows=q, self_rinv=row_rinv(q)) if mode == "query" else {}
            out = torch.empty((n_rows, d), device="cuda")
            forms["sum_kernel"] = lambda: neighbour_sum(cand, idx32, w, rinv=rinv, out=out, **own)
            if dense_fits:       # the two forms agree (other associations: fp32 rounding, and lists that differ at near-ties)
                a, b = expand_descriptors(q, g, k, alpha, mode=mode)[0], torch_form(q, g, mode)[:Q]
                agree = float((a - b).abs().max())
                del a, b
            for fn in forms.values():
                fn()                                             # warm-up of every shape
            ms = {name: [] for name in forms}
            peak = {name: 0 for name in forms}
            for _ in range(args.rounds):
                for name, fn in forms.items():                   # interleaved
                    t, p = timed(fn)
                    ms[name].append(t)
                    peak[name] = max(peak[name], p)
            moved = 4.0 * n_rows * d * (k + 1 + (1 if mode == "query" else 0))      # rows read and written by the sum
            line = {"Q": Q, "G": G, "d": d, "k": k, "alpha": alpha, "mode": mode, "rounds": args.rounds,
                    "ms_median": {n: round(statistics.median(v), 3) for n, v in ms.items()},
                    "ms_min_max": {n: [round(min(v), 3), round(max(v), 3)] for n, v in ms.items()},
                    "peak_MB": {n: round(p / 1e6, 1) for n, p in peak.items()},
                    "layout_MB": round(expansion_layout(Q, G, d, k, mode=mode)["total"] / 1e6, 1),
                    "dense_matrix_MB": round(4 * n_rows * n_cand / 1e6, 1),
                    "sum_kernel_GBps": round(moved / statistics.median(ms["sum_kernel"]) / 1e6, 1),
                    "max_abs_diff_driver_torch": agree if dense_fits else None}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del idx, dist, idx32, w, rinv, out, forms
        del X, q, g
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
