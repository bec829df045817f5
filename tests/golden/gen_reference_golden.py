"""Generates tests/golden/reference_golden.npz: what the REFERENCE itself returns for the seeded inputs of three CPU
tests, so that those tests run wherever the repository is checked out.
  - sampler_*: torchreid/data/sampler.py::RandomIdentitySampler (imported from the reference tree) on the 17-identity
    source of tests/test_data_cpu.py::_source, batch 16, 4 instances, under random / numpy seeds 0, 7 and 3.
  - rank_*: the reference's Cython evaluator (oracle/_ref, built by oracle/build_ref.sh) on the seeded 120 x 1500
    problem of tests/test_evaluator_oracle.py.
Run from the repository root after build():
    python tests/golden/gen_reference_golden.py"""
import importlib.util
import os
import random
import sys

import numpy as np

sys.path.insert(0, ".")
from oracle.ref_import import import_reference  # noqa: E402
from tests.test_data_cpu import _source  # noqa: E402
from tests.test_evaluator_oracle import rank_problem  # noqa: E402


def main():
    out = {}
    import_reference()
    from torchreid.data.sampler import RandomIdentitySampler as RefSampler
    data = _source(n_pid=17)
    for seed in (0, 7, 3):
        random.seed(seed); np.random.seed(seed)
        out["sampler_seed%d" % seed] = np.asarray(list(iter(RefSampler(data, 16, 4))), dtype=np.int64)
    out["sampler_len"] = np.asarray(len(RefSampler(data, 16, 4)), dtype=np.int64)

    here = os.path.join("oracle", "_ref")
    so = [f for f in os.listdir(here) if f.startswith("rank_cy") and f.endswith(".so")]
    spec = importlib.util.spec_from_file_location("rank_cy", os.path.join(here, so[0]))
    rank_cy = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rank_cy)
    d, qp, gp, qc, gc = rank_problem()
    cmc, m_ap = rank_cy.evaluate_cy(d, qp, gp, qc, gc, 20, False)
    out["rank_cmc"] = np.asarray(cmc)
    out["rank_mAP"] = np.asarray(float(m_ap), dtype=np.float64)
    np.savez_compressed("tests/golden/reference_golden.npz", **out)
    print("wrote tests/golden/reference_golden.npz")


if __name__ == "__main__":
    main()
