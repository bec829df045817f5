"""Generates tests/golden/cuhk03_golden.npz by running the REFERENCE's torchreid/metrics/rank.py::eval_cuhk03 (called
directly: its evaluate_py passes 6 of the 8 arguments and cannot reach it) on two synthetic fixtures, 1 000 times each
under np.random.seed(0 ... 999).  The reference returns a 10-draw Monte-Carlo estimate per call; stored are the inputs,
the per-rank mean and standard error of the 1 000 curves, and the mAP (which does not depend on the draw).  The
distances are distinct, because the reference's np.argsort is not stable, and every query sees at least max_rank
identities, because the reference fails otherwise.  eval_regdb (deterministic) is captured on the second fixture with
its debug prints swallowed.  Run:
    python tests/golden/gen_cuhk03_golden.py"""
import contextlib
import io
import sys

import numpy as np

sys.path.insert(0, ".")
from oracle.ref_import import import_reference  # noqa: E402

SEEDS = 1000
FIXTURES = (dict(name="a", Q=12, G=90, ids=15, cams=2, times=2, max_rank=5, seed=31),
            dict(name="b", Q=20, G=300, ids=40, cams=3, times=2, max_rank=10, seed=32))


def make(fx):
    rng = np.random.RandomState(fx["seed"])
    Q, G = fx["Q"], fx["G"]
    out = dict(q_pids=rng.randint(0, fx["ids"], Q), g_pids=rng.randint(0, fx["ids"], G),
               q_camids=rng.randint(0, fx["cams"], Q), g_camids=rng.randint(0, fx["cams"], G),
               q_timeids=rng.randint(0, fx["times"], Q), g_timeids=rng.randint(0, fx["times"], G))
    while True:
        d = rng.rand(Q, G).astype(np.float32)
        if all(len(np.unique(r)) == G for r in d):
            break
    # true matches somewhat nearer than the rest, so that the curve is neither flat nor saturated
    d[out["q_pids"][:, None] == out["g_pids"][None, :]] *= np.float32(0.6)
    assert all(len(np.unique(r)) == G for r in d)
    out["distmat"] = d
    for q in range(Q):      # every query sees at least max_rank identities
        removed = ((out["g_pids"] == out["q_pids"][q]) & (out["g_camids"] == out["q_camids"][q])
                   & (out["g_timeids"] == out["q_timeids"][q]))
        assert len(np.unique(out["g_pids"][~removed])) >= fx["max_rank"]
    return out


def main():
    import_reference()
    if not hasattr(np, "bool"):
        np.bool = bool       # the reference spells the mask's dtype with the alias NumPy 1.24 removed
    from torchreid.metrics import rank as ref_rank
    store = {}
    for fx in FIXTURES:
        data = make(fx)
        args = (data["distmat"], data["q_pids"], data["g_pids"], data["q_camids"], data["g_camids"], data["q_timeids"],
                data["g_timeids"], fx["max_rank"])
        curves, maps = [], []
        for s in range(SEEDS):
            np.random.seed(s)
            cmc, m_ap = ref_rank.eval_cuhk03(*args)
            curves.append(np.asarray(cmc, dtype=np.float64))
            maps.append(float(m_ap))
        curves = np.stack(curves)
        assert curves.shape == (SEEDS, fx["max_rank"]) and len(set(maps)) == 1
        n = fx["name"]
        for k, v in data.items():
            store["%s_%s" % (n, k)] = v.astype(np.float32 if k == "distmat" else np.int32)
        store[n + "_max_rank"] = np.int32(fx["max_rank"])
        store[n + "_cmc_mean"] = curves.mean(0)
        store[n + "_cmc_sem"] = curves.std(0, ddof=1) / np.sqrt(SEEDS)
        store[n + "_mAP"] = np.float64(maps[0])
        print(n, "mean", store[n + "_cmc_mean"], "sem", store[n + "_cmc_sem"], "mAP", maps[0])
    with contextlib.redirect_stdout(io.StringIO()):
        cmc, m_ap = ref_rank.eval_regdb(data["distmat"], data["q_pids"], data["g_pids"], data["q_timeids"],
                                        data["g_timeids"], 20)
    store["b_regdb_cmc"] = np.asarray(cmc, dtype=np.float32)
    store["b_regdb_mAP"] = np.float64(m_ap)
    np.savez_compressed("tests/golden/cuhk03_golden.npz", **store)
    print("wrote tests/golden/cuhk03_golden.npz")


if __name__ == "__main__":
    main()
