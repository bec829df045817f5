"""Generates tests/golden/augment_golden.npz: the reference's train augmentations beyond the flip.  Runs only where the
reference tree is present (oracle/ref_import.py), like gen_transform_golden.py:
    python tests/golden/gen_augment_golden.py
* ce_*    : the reference's OWN Random2DTranslation and RandomErasing (torchreid/data/transforms.py) over seeded uint8
            images: PIL image -> Random2DTranslation -> ToTensor / Normalize (torch, as torchvision's functional
            to_tensor / normalize) -> RandomErasing(mean=norm_mean).  Stored: inputs, seed, outputs, every draw the two
            classes made from `random` (function, arguments, value; recorded by wrapping random.uniform / randint) and
            a digest of random.getstate() after the sequence.
* j_*     : Pillow's ImageEnhance.Brightness / .Contrast (what torchvision's ColorJitter calls for PIL images) for listed
            (first, b, c): factors on both sides of 1, both orders, noise, a constant and a low-contrast image.
* jd_*    : for a seeded torch generator the (flip, permutation, b, c) sequence the restated ColorJitter draw order yields
            (torch.rand(1), torch.randperm(4), uniform_(0.8, 1.2), uniform_(0.85, 1.15) per image) and the state digest.
* chain_* : all four stages on, per image in the reference's Compose order, both generators seeded.
(The seeds of the two 256 x 128 cases are the first under which both images are cropped and one is erased, and under which
the single chain image is flipped, cropped and erased.)
Only data goes into the file."""
import os
import random
import sys

import numpy as np
import torch
from PIL import Image, ImageEnhance

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests.util_augment import digest  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
JITTER = [(0, 0.8, 0.85), (0, 1.2, 1.15), (1, 0.8, 1.15), (1, 1.2, 0.85), (0, 1.0, 1.0), (1, 0.93, 1.07), (0, 1.13, 0.9),
          (1, 1.0, 0.85), (0, 0.8, 1.0)]


def to_tensor_normalize(pil):
    t = torch.from_numpy(np.asarray(pil).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return t.sub_(torch.tensor(MEAN).view(3, 1, 1)).div_(torch.tensor(STD).view(3, 1, 1))


def smooth(h, w, k):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(yy * 255 // (h - 1)), (xx * 255 // (w - 1)), ((yy * (k + 1) + xx * 3) % 256)], -1).astype(np.uint8)


class DrawLog(object):
    """wraps random.uniform / random.randint while active and records (function, a, b, value) of every call"""

    def __enter__(self):
        self.rows = []
        self.saved = (random.uniform, random.randint)

        def uniform(a, b, f=self.saved[0]):
            v = f(a, b)
            self.rows.append((0.0, float(a), float(b), float(v)))
            return v

        def randint(a, b, f=self.saved[1]):
            v = f(a, b)
            self.rows.append((1.0, float(a), float(b), float(v)))
            return v
        random.uniform, random.randint = uniform, randint
        return self

    def __exit__(self, *exc):
        random.uniform, random.randint = self.saved


def jitter_pil(pil, first, b, c):
    for op in ((0, 1) if first == 0 else (1, 0)):
        pil = ImageEnhance.Brightness(pil).enhance(b) if op == 0 else ImageEnhance.Contrast(pil).enhance(c)
    return pil


def main():
    ref_import.import_reference()
    from torchreid.data.transforms import Random2DTranslation, RandomErasing
    out = {"mean": np.asarray(MEAN), "std": np.asarray(STD)}
    rng = np.random.RandomState(416)

    # ---- crop + erase through the reference's classes
    for tag, (H, W), count, seed, noise in (("ce", (64, 32), 10, 11, True), ("ce_big", (256, 128), 2, 4, False)):
        imgs = [rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8) if noise else smooth(H, W, k) for k in range(count)]
        crop, erase = Random2DTranslation(H, W), RandomErasing(mean=MEAN)
        random.seed(seed)
        with DrawLog() as log:
            res = [erase(to_tensor_normalize(crop(Image.fromarray(im, "RGB")))).numpy() for im in imgs]
        out[tag + "_in"], out[tag + "_out"], out[tag + "_seed"] = np.stack(imgs), np.stack(res), np.asarray(seed)
        out[tag + "_draws"] = np.asarray(log.rows, dtype=np.float64)
        out[tag + "_state"] = np.asarray(digest(random.getstate()))

    # ---- jitter through Pillow's ImageEnhance
    H, W = 64, 32
    jin = [rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8), np.full((H, W, 3), 97, dtype=np.uint8),
           rng.randint(120, 131, size=(H, W, 3)).astype(np.uint8)]
    cases, res = [], []
    for k, im in enumerate(jin):
        for (first, b, c) in JITTER:
            b, c = float(np.float32(b)), float(np.float32(c))
            cases.append((k, first, b, c))
            res.append(np.asarray(jitter_pil(Image.fromarray(im, "RGB"), first, b, c)))
    out["j_in"], out["j_cases"], out["j_out"] = np.stack(jin), np.asarray(cases, dtype=np.float64), np.stack(res)
    big = smooth(256, 128, 3)
    out["j_big_in"] = big
    out["j_big_out"] = np.asarray(jitter_pil(Image.fromarray(big, "RGB"), 1, float(np.float32(1.17)), float(np.float32(0.88))))

    # ---- the restated ColorJitter draw order on a seeded torch generator (with the flip's torch.rand(1) before it)
    torch.manual_seed(23)
    rows = []
    for _ in range(16):
        flip = 1 if float(torch.rand(1)) < 0.5 else 0
        perm = torch.randperm(4).tolist()
        b = float(torch.empty(1).uniform_(0.8, 1.2))
        c = float(torch.empty(1).uniform_(0.85, 1.15))
        rows.append([flip] + perm + [b, c])
    out["jd_seed"], out["jd_rows"], out["jd_state"] = np.asarray(23), np.asarray(rows, dtype=np.float64), np.asarray(digest(torch.get_rng_state()))

    # ---- all four stages, the reference's Compose order per image
    for tag, (H, W), sizes, seed in (("chain", (64, 32), [(70, 30), (64, 32), (50, 40), (128, 64), (33, 17), (64, 48)], 7),
                                     ("chain_big", (256, 128), [(256, 128)], 11)):
        imgs = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) if tag == "chain" else smooth(h, w, 5) for h, w in sizes]
        crop, erase = Random2DTranslation(H, W), RandomErasing(mean=MEAN)
        random.seed(seed)
        torch.manual_seed(seed)
        res = []
        for im in imgs:
            pil = Image.fromarray(im, "RGB").resize((W, H), Image.BILINEAR)
            if float(torch.rand(1)) < 0.5:
                pil = pil.transpose(Image.FLIP_LEFT_RIGHT)
            pil = crop(pil)
            perm = torch.randperm(4).tolist()
            b = float(torch.empty(1).uniform_(0.8, 1.2))
            c = float(torch.empty(1).uniform_(0.85, 1.15))
            pil = jitter_pil(pil, 0 if perm.index(0) < perm.index(1) else 1, b, c)
            res.append(erase(to_tensor_normalize(pil)).numpy())
        for k, im in enumerate(imgs):
            out["%s_in%d" % (tag, k)] = im
        out[tag + "_n"], out[tag + "_seed"], out[tag + "_out"] = np.asarray(len(imgs)), np.asarray(seed), np.stack(res)
        out[tag + "_py_state"] = np.asarray(digest(random.getstate()))
        out[tag + "_torch_state"] = np.asarray(digest(torch.get_rng_state()))
    path = os.path.join(ROOT, "tests", "golden", "augment_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
