"""GPU: ieee_amd.reidtools.visualize_ranked_results against the reference's figures (tests/golden/visrank_golden.npz,
recorded from torchreid/utils/reidtools.py by gen_visrank_golden.py: which gallery images each query's row shows, in
which order, with which border colour, under which file name), and Engine.run(test_only=True, visrank=True)."""
import os

import numpy as np
import pytest
import torch

from tests.util_model import C, id_loader

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V(golden_dir):
    return np.load(os.path.join(golden_dir, "visrank_golden.npz"))


def write_images(root, rel_paths, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for rel in rel_paths:
        p = os.path.join(str(root), rel)
        os.makedirs(os.path.dirname(p), exist_ok=True)
        if not os.path.exists(p):
            # grey-ish tiles: far from the pure green / red of the borders
            Image.fromarray(rng.randint(100, 156, size=(12, 6, 3)).astype(np.uint8)).save(p)
        out.append(p)
    return out


def records(root, paths, pids, cams, seed):
    first = write_images(root, [p[0] for p in paths], seed)          # the figure reads the first modality only
    return [((first[i],) + tuple(os.path.join(str(root), m) for m in paths[i][1:]), int(pids[i]), int(cams[i]), 0)
            for i in range(len(paths))]


def is_green(px):
    r, g, b = (int(v) for v in px)
    return g > 150 and g - max(r, b) > 80


def is_red(px):
    r, g, b = (int(v) for v in px)
    return r > 150 and r - max(g, b) > 80


@pytest.mark.parametrize("as_tensor", [False, True])
def test_figures_match_the_reference(V, tmp_path, as_tensor, capsys):
    from PIL import Image
    from ieee_amd.reidtools import visualize_ranked_results
    topk, width, height = (int(v) for v in V["params"])
    query = records(tmp_path / "img", V["q_paths"], V["q_pids"], V["q_camids"], 1)
    gallery = records(tmp_path / "img", V["g_paths"], V["g_pids"], V["g_camids"], 2)
    out = tmp_path / "out"
    dm = torch.from_numpy(V["distmat"]).cuda() if as_tensor else V["distmat"]
    ranked = visualize_ranked_results(dm, (query, gallery), "image", width=width, height=height, save_dir=str(out),
                                      topk=topk)
    printed = capsys.readouterr().out
    Q, G = V["distmat"].shape
    assert printed.startswith("# query: {}\n# gallery {}\nVisualizing top-{} ranks ...\n".format(Q, G, topk))
    assert 'Done. Images have been saved to "{}" ...'.format(out) in printed
    assert len(ranked) == Q
    for q in range(Q):
        want = [int(g) for g in V["ranked"][q] if g >= 0]
        assert ranked[q] == want, q
    assert sorted(os.listdir(out)) == sorted(str(n) for n in V["names"])
    for q in range(Q):
        img = np.asarray(Image.open(os.path.join(out, str(V["names"][q]))).convert("RGB"))
        assert img.shape == (height, (topk + 1) * width + topk * 10 + 90, 3)
        for r, m in enumerate(V["matched"][q][V["matched"][q] >= 0], start=1):
            start = r * width + r * 10 + 90
            for px in (img[height // 2, start + 1], img[1, start + width // 2], img[height // 2, start + width - 2]):
                assert (is_green if m else is_red)(px), (q, r, m, px)
        assert img[height // 2, width + 45].min() > 240        # the spacing between the query and rank 1 stays white


def test_video_and_bad_topk_refused(V, tmp_path):
    from ieee_amd.reidtools import visualize_ranked_results
    with pytest.raises(NotImplementedError):
        visualize_ranked_results(V["distmat"], ([], []), "video", save_dir=str(tmp_path))
    with pytest.raises(ValueError):
        visualize_ranked_results(V["distmat"][:1, :3], ([(("a",), 0, 0)], [(("b",), 0, 1)] * 3), "image",
                                 save_dir=str(tmp_path), topk=0)


class VisDM(object):
    """a data manager with torchreid's fetch_test_loaders / data_type / width / height"""
    num_train_pids = C
    sources = ["synthetic"]
    data_type = "image"
    width, height = 32, 64

    def __init__(self, root):
        self.train_loader = []
        qp, qc = np.arange(12) % 6, np.zeros(12, dtype=np.int64)
        gp, gc = np.arange(20) % 6, np.ones(20, dtype=np.int64)
        self.test_loader = {"synthetic": {"query": id_loader(12, 1, qp, qc), "gallery": id_loader(20, 2, gp, gc)}}
        mk = lambda side, n: [tuple("%s/%03d_%s.png" % (side, i, m) for m in ("RGB", "NI", "TI")) for i in range(n)]
        self.records = (records(root, mk("q", 12), qp, qc, 4), records(root, mk("g", 20), gp, gc, 5))

    def fetch_test_loaders(self, name):
        assert name == "synthetic"
        return self.records


def report(text):
    return [ln for ln in text.splitlines() if not ln.startswith("Speed:")]


def test_engine_run_visrank(tmp_path, capsys):
    from ieee_amd.engine import MultiModalImageSoftmaxEngine
    from ieee_amd.models import build_model
    from ieee_amd.optim import build_optimizer
    m = build_model("ieee3modalPart", num_classes=C, loss="softmax", pretrained=False, compute_dtype=torch.float32)
    dm = VisDM(tmp_path / "img")
    eng = MultiModalImageSoftmaxEngine(dm, m, build_optimizer(m, optim="sgd", lr=1e-3), use_gpu=True)
    eng.run(test_only=True, save_dir=str(tmp_path / "plain"), ranks=[1, 5])
    plain = report(capsys.readouterr().out)
    eng.run(test_only=True, visrank=True, visrank_topk=5, save_dir=str(tmp_path / "vis"), ranks=[1, 5])
    vis = report(capsys.readouterr().out)
    assert vis[:len(plain)] == plain                    # the report is the same, the figures come after it
    assert any(ln.startswith("mAP:") for ln in plain)
    assert vis[len(plain):][:3] == ["# query: 12", "# gallery 20", "Visualizing top-5 ranks ..."]
    out = tmp_path / "vis" / "visrank_synthetic"
    assert sorted(os.listdir(out)) == sorted("%03d_RGB.jpg" % i for i in range(12))
    # the returned mAP does not depend on visrank
    base = eng.test(ranks=[1])
    assert eng.test(visrank=True, visrank_topk=5, save_dir=str(tmp_path / "vis2"), ranks=[1]) == base
    with pytest.raises(ValueError):
        eng.run(test_only=False, visrank=True)
