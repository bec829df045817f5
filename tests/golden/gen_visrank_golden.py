"""Generates tests/golden/visrank_golden.npz by running the REFERENCE's torchreid/utils/reidtools.py::
visualize_ranked_results (imported from /root/reference in this container) on a synthetic 3-modal dataset, with its
cv2 swapped for a recorder: every imread path (which gallery images were drawn, in order), every copyMakeBorder
colour (match or miss) and every imwrite name is logged.  The distance matrix is tie-free, because the reference's
np.argsort (:49) is not stable.  Run:
    python tests/golden/gen_visrank_golden.py"""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
from oracle.ref_import import import_reference  # noqa: E402

Q, G, TOPK, WIDTH, HEIGHT = 40, 500, 10, 32, 64
MODALITIES = ("RGB", "NI", "TI")


class Recorder(object):
    """the slice of cv2 that reidtools.py uses for data_type='image'"""
    BORDER_CONSTANT = 0

    def __init__(self):
        self.log = []

    def imread(self, path):
        self.log.append(("imread", path))
        return np.zeros((HEIGHT, WIDTH, 3), dtype=np.uint8)

    def resize(self, img, size):
        return np.zeros((size[1], size[0], 3), dtype=np.uint8)

    def copyMakeBorder(self, img, top, bottom, left, right, kind, value):
        self.log.append(("border", tuple(int(v) for v in value)))
        return np.pad(img, ((top, bottom), (left, right), (0, 0)))

    def imwrite(self, path, img):
        self.log.append(("imwrite", os.path.basename(path), img.shape))
        return True


def paths(prefix, n, pids, camids):
    return [tuple("%s/%04d_%03d_c%d_%s.png" % (prefix, i, pids[i], camids[i], m) for m in MODALITIES) for i in range(n)]


def main():
    import_reference()
    from torchreid.utils import reidtools
    rng = np.random.RandomState(23)
    # one identity pool for both sides, few cameras: same-pid-same-camera entries exist and are skipped
    q_pids, q_camids = rng.randint(0, 30, Q), rng.randint(0, 4, Q)
    g_pids, g_camids = rng.randint(0, 30, G), rng.randint(0, 4, G)
    while True:
        distmat = rng.rand(Q, G).astype(np.float32)
        if all(len(np.unique(r)) == G for r in distmat):
            break
    # most queries see their identity near the top (green tiles); every 7th is nearest to its own same-camera shots,
    # which the figure skips
    for q in range(Q):
        mine = g_pids == q_pids[q]
        same = mine & (g_camids == q_camids[q])
        if q % 7 == 0:
            distmat[q, same] *= np.float32(1e-3)
        elif q % 3:
            distmat[q, mine & ~same] *= np.float32(0.02)
    assert all(len(np.unique(r)) == G for r in distmat)
    qp, gp = paths("query", Q, q_pids, q_camids), paths("gallery", G, g_pids, g_camids)
    query = [(qp[i], int(q_pids[i]), int(q_camids[i]), 0) for i in range(Q)]
    gallery = [(gp[i], int(g_pids[i]), int(g_camids[i]), 0) for i in range(G)]
    rec = Recorder()
    reidtools.cv2 = rec
    with tempfile.TemporaryDirectory() as tmp:
        reidtools.visualize_ranked_results(distmat, (query, gallery), "image", width=WIDTH, height=HEIGHT,
                                           save_dir=tmp, topk=TOPK)
    g_of = {p[0]: i for i, p in enumerate(gp)}
    ranked = -np.ones((Q, TOPK), dtype=np.int32)
    matched = -np.ones((Q, TOPK), dtype=np.int8)
    names, q, r, pending = [], -1, 0, None
    for ev in rec.log:
        if ev[0] == "imread" and ev[1] in g_of:
            pending = g_of[ev[1]]
        elif ev[0] == "imread":
            q, r = q + 1, 0
            assert ev[1] == qp[q][0]
        elif ev[0] == "border" and pending is not None:
            assert ev[1] in (reidtools.GREEN, reidtools.RED)
            ranked[q, r], matched[q, r] = pending, int(ev[1] == reidtools.GREEN)
            r, pending = r + 1, None
        elif ev[0] == "imwrite":
            assert ev[2] == (HEIGHT, (TOPK + 1) * WIDTH + TOPK * 10 + 90, 3)
            names.append(ev[1])
    assert q == Q - 1 and len(names) == Q
    np.savez_compressed("tests/golden/visrank_golden.npz", distmat=distmat, q_pids=q_pids.astype(np.int32),
                        g_pids=g_pids.astype(np.int32), q_camids=q_camids.astype(np.int32),
                        g_camids=g_camids.astype(np.int32), q_paths=np.asarray(qp), g_paths=np.asarray(gp),
                        ranked=ranked, matched=matched, names=np.asarray(names),
                        params=np.asarray([TOPK, WIDTH, HEIGHT], dtype=np.int32))
    print("wrote tests/golden/visrank_golden.npz")


if __name__ == "__main__":
    main()
