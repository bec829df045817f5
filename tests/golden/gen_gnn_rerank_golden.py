"""Generates tests/golden/gnn_rerank_golden.npz by running the REFERENCE's
torchreid/utils/GPU-Re-Ranking/gnn_reranking.py::gnn_reranking, unmodified, on CPU tensors.  The file is loaded by path;
the two CUDA extensions it imports (build_adjacency_matrix, gnn_propagate) are stood in for by torch CPU restatements of
their kernels (a scatter_ of ones; a j-ordered weighted sum of gathered rows), and its `from utils import *` by an
empty module (it uses nothing of it).  Run:
    python tests/golden/gen_gnn_rerank_golden.py

The fixtures are exact and free of boundary ties, because torch.topk breaks ties in no documented order: features are
integers in 0..255 with d <= 64, so every inner product is an integer below 2^24 (exact in fp32 in any order), and the
first seed is taken for which no score row has equal values across the k2 | k2+1 or the k1 | k1+1 boundary."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, ".")
from oracle.ref_import import REF_ROOT  # noqa: E402
from tests.util_gnn_rerank import integer_features  # noqa: E402

CASES = [(60, 400, 32, 40, 26, 7), (100, 900, 32, 60, 26, 7), (40, 300, 16, 25, 10, 3), (30, 90, 16, 8, 6, 2),
         (50, 350, 32, 30, 12, 1)]        # Q, G, d, identities, k1, k2


def _adjacency_forward(initial_rank):
    n = initial_rank.shape[0]
    return torch.zeros((n, n), dtype=torch.float32).scatter_(1, initial_rank.long(), 1.0)


def _propagate_forward(A, initial_rank, S):
    out = torch.zeros_like(A)
    idx = initial_rank.long()
    for j in range(idx.shape[1]):
        out += A[idx[:, j]] * S[:, j:j + 1]
    return out


def load_reference():
    sys.dont_write_bytecode = True
    stand_ins = {"build_adjacency_matrix": types.ModuleType("build_adjacency_matrix"),
                 "gnn_propagate": types.ModuleType("gnn_propagate"), "utils": types.ModuleType("utils")}
    stand_ins["build_adjacency_matrix"].forward = _adjacency_forward
    stand_ins["gnn_propagate"].forward = _propagate_forward
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        path = os.path.join(REF_ROOT, "torchreid", "utils", "GPU-Re-Ranking", "gnn_reranking.py")
        spec = importlib.util.spec_from_file_location("reference_gnn_reranking", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod.gnn_reranking


def boundary_tie(xq, xg, k1, k2):
    X = np.concatenate([xq, xg]).astype(np.float64)
    s = -np.sort(-(X @ X.T), axis=1)
    cuts = [k for k in (k1, k2) if k < s.shape[1]]
    return any(np.any(s[:, k - 1] == s[:, k]) for k in cuts)


def main():
    gnn_reranking = load_reference()
    out = {}
    for c, (Q, G, d, ids, k1, k2) in enumerate(CASES):
        seed = 0
        while True:
            xq, xg = integer_features(seed, Q, G, d, ids)
            if not boundary_tie(xq, xg, k1, k2):
                break
            seed += 1
        L = gnn_reranking(torch.from_numpy(xq.astype(np.float32)), torch.from_numpy(xg.astype(np.float32)), k1, k2)
        assert L.shape == (Q, G) and G < 2 ** 15
        out["xq%d" % c], out["xg%d" % c] = xq, xg
        out["params%d" % c] = np.asarray([k1, k2], dtype=np.int32)
        out["L%d" % c] = L.astype(np.int16)
        print("case %d: Q=%d G=%d d=%d k1=%d k2=%d seed=%d" % (c, Q, G, d, k1, k2, seed))
    out["cases"] = np.asarray(len(CASES))
    np.savez_compressed("tests/golden/gnn_rerank_golden.npz", **out)
    print("wrote tests/golden/gnn_rerank_golden.npz")


if __name__ == "__main__":
    main()
