#!/usr/bin/env python
"""Measurement: ieee_rank_cuhk03 (the CUHK03 single-gallery-shot protocol in closed form) at Market-1501 scale --
3 368 x 19 732, 751 identities, 6 cameras, max_rank 50 -- beside ieee_rank_market1501_ws on the same matrix in the same
run, by device events around warm calls on device-resident inputs, the two alternating.  Two matrices: random distances
(every identity has images before every true match: the recurrence runs over all 751 identities) and the same with the
true matches pulled close (what a trained model gives: most identities are no-ops).  LABNOTES R15.1.

  python scripts/cuhk03_probe.py
  python scripts/cuhk03_probe.py --q 3368 --g 19732 --ids 751 --cams 6 --max-rank 50 --reps 10

Needs the GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ieee_amd  # noqa: E402,F401


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--q", type=int, default=3368)
    ap_.add_argument("--g", type=int, default=19732)
    ap_.add_argument("--ids", type=int, default=751)
    ap_.add_argument("--cams", type=int, default=6)
    ap_.add_argument("--max-rank", type=int, default=50)
    ap_.add_argument("--reps", type=int, default=10, help="calls per timed window")
    ap_.add_argument("--windows", type=int, default=5)
    args = ap_.parse_args()

    import numpy as np
    import torch
    from ieee_amd import _lib as L
    from ieee_amd.metrics.rank import fold_keys
    lib = L.require_gpu()
    Q, G, R = args.q, args.g, args.max_rank
    rs = np.random.RandomState(1)
    qp, gp = rs.randint(0, args.ids, Q), rs.randint(0, args.ids, G)
    qc, gc = rs.randint(0, args.cams, Q), rs.randint(0, args.cams, G)
    qk, gk = fold_keys(qc, gc)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    qpd, gpd, qcd, gcd, qkd, gkd = dev(qp), dev(gp), dev(qc), dev(gc), dev(qk), dev(gk)
    gen = torch.Generator(device="cuda").manual_seed(1)
    random = torch.rand(Q, G, generator=gen, device="cuda")
    near = torch.where(qpd[:, None] == gpd[None, :], random * 1e-4, random)

    cmc = torch.empty(Q, R, dtype=torch.float64, device="cuda")
    ap = torch.empty(Q, dtype=torch.float64, device="cuda")
    summary = torch.empty(R + 2, dtype=torch.float64, device="cuda")
    first = torch.empty(Q, dtype=torch.int32, device="cuda")
    m_summary = torch.empty(R + 2, dtype=torch.int64, device="cuda")
    c_bytes, m_bytes = lib.ieee_rank_cuhk03_workspace_bytes(G), lib.ieee_rank_workspace_bytes(G)
    c_work = torch.empty(c_bytes, dtype=torch.uint8, device="cuda")
    m_work = torch.empty(m_bytes, dtype=torch.uint8, device="cuda")

    def cuhk03(d):
        L.check(lib.ieee_rank_cuhk03(L.ptr(d), d.stride(0), Q, G, L.ptr(qpd), L.ptr(gpd), L.ptr(qkd), L.ptr(gkd), R,
                                     L.ptr(cmc), L.ptr(ap), L.ptr(summary), L.ptr(c_work), c_bytes, L.stream()))

    def market(d):
        L.check(lib.ieee_rank_market1501_ws(L.ptr(d), d.stride(0), Q, G, L.ptr(qpd), L.ptr(gpd), L.ptr(qcd), L.ptr(gcd), R,
                                            L.ptr(ap), L.ptr(first), L.ptr(m_summary), L.ptr(m_work), m_bytes, L.stream()))

    def window(fn, d):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn(d)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    for name, d in (("random", random), ("matches_nearest", near)):
        cuhk03(d)
        market(d)
        torch.cuda.synchronize()
        res = {"matrix": name, "q": Q, "g": G, "ids": args.ids, "cams": args.cams, "max_rank": R, "reps": args.reps,
               "cuhk03_ms": [], "market1501_ms": []}
        for _ in range(args.windows):            # alternate the two so that both see the same machine
            res["cuhk03_ms"].append(window(cuhk03, d))
            res["market1501_ms"].append(window(market, d))
        s = summary.cpu().numpy()
        res["num_valid"] = float(s[R])
        res["cuhk03_rank1"] = float(s[0] / s[R])
        res["cuhk03_rank%d" % R] = float(s[R - 1] / s[R])
        res["mAP"] = float(s[R + 1] / s[R])
        print(json.dumps(res))


if __name__ == "__main__":
    main()
