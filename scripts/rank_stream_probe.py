"""Times the streamed CMC / mAP (ieee_amd.metrics.evaluate_rank_streamed) beside the two-step path it replaces
(compute_distance_matrix, then evaluate_rank on the whole [Q, G] matrix).

One mode per process.  Run every invocation under its own `timeout` and chain them with `&&`:

    timeout -k 10 300 python scripts/rank_stream_probe.py --mode compare --labels all && \\
    timeout -k 10 300 python scripts/rank_stream_probe.py --mode compare --labels distractors && \\
    timeout -k 10 300 python scripts/rank_stream_probe.py --mode rank --other-lib <another build of libieee_amd.so>

Every mode prints one JSON line.  Times are device events around whole calls (host planning, uploads and the one
read-back included: every call ends in its read-back), after warm-up, the variants interleaved round by round in one
process.  Peak memory is torch's max_memory_allocated over one call, less what was allocated before it.

  compare  Q x G descriptors of width d on the device.  --labels all: every gallery identity occurs among the queries
           (--ids identities, --cams cameras); --labels distractors: 90 % of the gallery rows carry identities no query
           has.  evaluate_rank_streamed at the default slab and at 2048 rows against compute_distance_matrix +
           evaluate_rank; says whether the results are equal.
  rank     ieee_rank_market1501_ws on a Q x G matrix of random distances with this build and with --other-lib,
           interleaved: has moving the batch core into rank_common.h changed the whole-matrix evaluator?"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from search_probe import descriptors, interleaved, peak_of  # noqa: E402


def label_set(kind, Q, G, ids, cams):
    import numpy as np
    rng = np.random.RandomState(4)
    lab = dict(q_pids=rng.randint(0, ids, Q), g_pids=rng.randint(0, ids, G), q_camids=rng.randint(0, cams, Q),
               g_camids=rng.randint(0, cams, G))
    if kind == "distractors":
        lab["g_pids"][rng.rand(G) < 0.9] += ids
    return lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("compare", "rank"), default="compare")
    ap.add_argument("--labels", choices=("all", "distractors"), default="all")
    ap.add_argument("--q", type=int, default=10000)
    ap.add_argument("--g", type=int, default=100000)
    ap.add_argument("--d", type=int, default=2304)
    ap.add_argument("--ids", type=int, default=751)
    ap.add_argument("--cams", type=int, default=6)
    ap.add_argument("--max-rank", type=int, default=50)
    ap.add_argument("--precision", default=None)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--other-lib", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from ieee_amd import _lib
    from ieee_amd.metrics import (RankAccumulator, compute_distance_matrix, default_slab_rows, evaluate_rank,
                                  evaluate_rank_streamed)
    Q, G, d = args.q, args.g, args.d
    lab = label_set(args.labels, Q, G, args.ids, args.cams)
    line = {"mode": args.mode, "labels": args.labels, "Q": Q, "G": G, "d": d, "ids": args.ids, "cams": args.cams,
            "max_rank": args.max_rank, "precision": args.precision or "fp32", "default_slab": default_slab_rows(Q),
            "device": torch.cuda.get_device_name(0)}

    if args.mode == "rank":
        from ieee_amd.metrics.rank import _i32
        gen = torch.Generator(device="cuda").manual_seed(4)
        dm = torch.rand(Q, G, device="cuda", generator=gen)
        dev = dm.device
        qp, gp = _i32(lab["q_pids"], "q_pids", dev), _i32(lab["g_pids"], "g_pids", dev)
        qc, gc = _i32(lab["q_camids"], "q_camids", dev), _i32(lab["g_camids"], "g_camids", dev)
        apq = torch.empty(Q, dtype=torch.float64, device=dev)
        first = torch.empty(Q, dtype=torch.int32, device=dev)
        summ = torch.empty(args.max_rank + 2, dtype=torch.int64, device=dev)
        work = torch.empty(_lib.require_gpu().ieee_rank_workspace_bytes(G), dtype=torch.uint8, device=dev)

        def entry(lib):
            fn = lib.ieee_rank_market1501_ws
            fn.argtypes, fn.restype = _lib._SIGNATURES["ieee_rank_market1501_ws"], ctypes.c_int
            return lambda: _lib.check(fn(_lib.ptr(dm), G, Q, G, _lib.ptr(qp), _lib.ptr(gp), _lib.ptr(qc), _lib.ptr(gc),
                                         args.max_rank, _lib.ptr(apq), _lib.ptr(first), _lib.ptr(summ), _lib.ptr(work),
                                         work.numel(), _lib.stream()))
        variants = {"this_build": entry(_lib.require_gpu())}
        if args.other_lib:
            variants["other_lib"] = entry(ctypes.CDLL(args.other_lib))
        results = {}
        for name, fn in variants.items():
            fn()
            results[name] = (apq.clone(), first.clone(), summ.clone())
        if args.other_lib:
            line["results_equal"] = bool(all(torch.equal(a, b) for a, b in zip(results["this_build"], results["other_lib"])))
        line["rank_market1501_ws_ms"] = interleaved(variants, args.warmup, max(args.rounds, 15))
        print(json.dumps(line))
        return

    q, g = descriptors(Q, d, 1), descriptors(G, d, 2)
    order = (lab["q_pids"], lab["g_pids"], lab["q_camids"], lab["g_camids"])
    acc = RankAccumulator(lab["q_pids"], lab["q_camids"], lab["g_pids"], lab["g_camids"], args.max_rank)
    line["match_columns"] = int(acc.match_columns.size)
    line["match_keys"], line["removed_keys"] = int(acc.plan.m_off[-1]), int(acc.plan.r_off[-1])
    line["state_bytes"] = int(_lib.require_gpu().ieee_rank_stream_workspace_bytes(Q, line["match_keys"], line["removed_keys"]))
    streamed = lambda slab: evaluate_rank_streamed(q, g, *order, max_rank=args.max_rank, slab=slab, precision=args.precision)
    variants = {"two_step": lambda: evaluate_rank(compute_distance_matrix(q, g, precision=args.precision), *order,
                                                  max_rank=args.max_rank),
                "streamed_default_slab": lambda: streamed(None),
                "streamed_slab_2048": lambda: streamed(2048)}
    line["ms"] = interleaved(variants, args.warmup, args.rounds)
    peaks, outs = {}, {}
    for name, fn in variants.items():
        peaks[name], outs[name] = peak_of(fn)
    line["peak_bytes"] = peaks
    line["mAP"] = outs["two_step"][1]
    line["results_equal"] = {name: bool(np.array_equal(outs[name][0], outs["two_step"][0]) and
                                        outs[name][1] == outs["two_step"][1]) for name in variants if name != "two_step"}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
