"""Generates tests/golden/optim_golden.npz: the reference's OWN RAdam (torchreid/optim/radam.py:19-130, the class its
build_optimizer constructs for optim='radam', optimizer.py:149-155) run over a seeded tensor.  Runs only where the
reference tree is present (oracle/ref_import.py), like the other gen_*.py:
    python tests/golden/gen_optim_golden.py
Stored per weight decay (0 and 5e-4), betas = (0.9, 0.99), lr = 1e-2, eps = 1e-8, 14 steps over 320 fp32 elements: the
initial parameters, the gradient of every step, the parameters after EVERY step and exp_avg / exp_avg_sq / step at the
end.  With beta2 = 0.99 steps 1-5 take the SGD-like branch (N_sma = 4.96 at step 5) and steps 6-14 the rectified one
(5.94 at step 6), so both branches and the hand-over are in the file.  Gradients are bounded away from zero
(|g| >= 0.5 * scale), so sqrt(exp_avg_sq) + eps is well conditioned.  Only data goes into the file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402

N, STEPS, LR, BETAS, EPS = 320, 14, 1e-2, (0.9, 0.99), 1e-8
DECAYS = (0.0, 5e-4)


def main():
    ref_import.import_reference()
    from torchreid.optim.radam import RAdam
    gen = torch.Generator().manual_seed(1908)
    p0 = torch.randn(N, generator=gen)
    grads = []
    for t in range(STEPS):
        r = torch.randn(N, generator=gen)
        grads.append(torch.sign(r) * (0.5 + r.abs()) * (0.05 + 0.3 * (t % 5)))
    out = {"p0": p0.numpy(), "grads": torch.stack(grads).numpy(), "lr": np.float64(LR), "betas": np.asarray(BETAS, np.float64),
           "eps": np.float64(EPS), "decays": np.asarray(DECAYS, np.float64)}
    for k, wd in enumerate(DECAYS):
        w = torch.nn.Parameter(p0.clone())
        opt = RAdam([w], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
        trace = []
        for g in grads:
            w.grad = g.clone()
            opt.step()
            trace.append(w.detach().clone())
        st = opt.state[w]
        out["params_%d" % k] = torch.stack(trace).numpy()
        out["exp_avg_%d" % k] = st["exp_avg"].numpy()
        out["exp_avg_sq_%d" % k] = st["exp_avg_sq"].numpy()
        out["step_%d" % k] = np.int64(st["step"])
    path = os.path.join(ROOT, "tests", "golden", "optim_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
