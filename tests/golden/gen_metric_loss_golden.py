"""Generates tests/golden/metric_loss_golden.npz: the reference's OWN criteria -- TripletLoss
(torchreid/losses/hard_mine_triplet_loss.py), hetero_loss (hcloss.py, 'l2' / 'l1' / 'cos') and multiModalMarginLossNew
(multi_modal_margin_loss_new.py, 'l2' / 'l1') -- run in fp32 on the CPU over small seeded inputs.  Runs only where the
reference tree is present (oracle/ref_import.py), like the other gen_*.py:
    python tests/golden/gen_metric_loss_golden.py
Stored: the inputs, every loss and the gradient with respect to every input.  Triplet: 12 rows of 4 identities in shuffled
order, D = 24, margin 0.3 (rows ~N(0,1)/sqrt(D) around identity centres, so some hinges are active and some are not).
Centres: 10 rows of 4 identities (torch.chunk pieces of 3, 3, 3, 1), D = 20, margin 1 for the 3M loss.  Only data goes
into the file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402


def triplet_inputs():
    rs = np.random.RandomState(1703)
    pids = np.array([3, 7, 3, 11, 7, 5, 11, 5, 3, 7, 5, 11])
    centres = {p: rs.standard_normal(24) * 0.25 for p in (3, 5, 7, 11)}
    x = np.stack([centres[p] + rs.standard_normal(24) * 0.2 for p in pids]).astype(np.float32)
    return x, pids


def centre_inputs():
    rs = np.random.RandomState(1908)
    pids = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2, 3])
    f = [(rs.standard_normal((10, 20)) * 0.3 + 0.4 * m).astype(np.float32) for m in range(3)]
    return f, pids


def main():
    ref_import.import_reference()
    from torchreid.losses.hard_mine_triplet_loss import TripletLoss
    from torchreid.losses.hcloss import hetero_loss
    from torchreid.losses.multi_modal_margin_loss_new import multiModalMarginLossNew
    out = {}
    x, pids = triplet_inputs()
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    loss = TripletLoss(margin=0.3)(xt, torch.from_numpy(pids))
    loss.backward()
    out.update(t_x=x, t_pids=pids, t_margin=np.float64(0.3), t_loss=np.float32(loss.item()), t_grad=xt.grad.numpy())
    f, cp = centre_inputs()
    out.update(c_f=np.stack(f), c_pids=cp, c_margin=np.float64(1.0))
    for name, make, M in [("h_l2", lambda: hetero_loss(dist_type="l2"), 2), ("h_l1", lambda: hetero_loss(dist_type="l1"), 2),
                          ("h_cos", lambda: hetero_loss(dist_type="cos"), 2),
                          ("m_l2", lambda: multiModalMarginLossNew(margin=1.0, dist_type="l2"), 3),
                          ("m_l1", lambda: multiModalMarginLossNew(margin=1.0, dist_type="l1"), 3)]:
        ft = [torch.from_numpy(v).clone().requires_grad_(True) for v in f[:M]]
        loss = make()(*ft, torch.from_numpy(cp))
        loss.backward()
        out[name + "_loss"] = np.float32(loss.item())
        out[name + "_grad"] = np.stack([t.grad.numpy() if t.grad is not None else np.zeros_like(f[0]) for t in ft])
    path = os.path.join(ROOT, "tests", "golden", "metric_loss_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
