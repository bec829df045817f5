#!/usr/bin/env python
"""Descriptors of a set of three-modality images: ieee_amd.FeatureExtractor (the reference's
torchreid.utils.FeatureExtractor) from the command line.  The images of one identity shot carry the same file name in the
three directories; every image may have its own size (detector crops).

  python scripts/extract_features.py --images-rgb crops/RGB --images-ni crops/NI --images-ti crops/TI \
      --weights model.pth.tar-60 --save features.pt
  python scripts/extract_features.py --synthetic 100 --save /tmp/features.pt      (generated crops of random sizes)

The resize / ToTensor / Normalize chain runs on the device, one ragged call per modality and chunk; --save writes
{'features': [N, 2304] float32 (CPU), 'names': [N]}."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ieee_amd  # noqa: E402,F401  (before torch.cuda is touched: it picks GPU_MAX_HW_QUEUES)

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')


def make_crops(root, n, seed=0):
    """n crops of random sizes per modality, as lossless PNG, under root/{RGB,NI,TI}"""
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    for mod in ('RGB', 'NI', 'TI'):
        os.makedirs(os.path.join(root, mod), exist_ok=True)
        for i in range(n):
            h, w = int(rng.randint(120, 421)), int(rng.randint(50, 201))
            Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8), 'RGB').save(
                os.path.join(root, mod, 'crop_%05d.png' % i))
    return [os.path.join(root, mod) for mod in ('RGB', 'NI', 'TI')]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--images-rgb', type=str, default='')
    parser.add_argument('--images-ni', type=str, default='')
    parser.add_argument('--images-ti', type=str, default='')
    parser.add_argument('-m', '--model', type=str, default='ieee3modalPart')
    parser.add_argument('--weights', type=str, default='')
    parser.add_argument('--save', type=str, default='')
    parser.add_argument('--height', type=int, default=256)
    parser.add_argument('--width', type=int, default=128)
    parser.add_argument('--batch', type=int, default=64)
    parser.add_argument('--synthetic', type=int, default=0,
                        help='generate this many crops of random sizes per modality instead of --images-*')
    parser.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    args = parser.parse_args()

    import torch
    from ieee_amd import FeatureExtractor

    if args.synthetic:
        with tempfile.TemporaryDirectory(prefix='ieee_crops_') as tmp:
            dirs = make_crops(tmp, args.synthetic)
            names, features = extract(args, dirs, torch, FeatureExtractor)
    else:
        dirs = [args.images_rgb, args.images_ni, args.images_ti]
        if not all(os.path.isdir(d) for d in dirs):
            raise SystemExit('give --images-rgb, --images-ni and --images-ti (directories), or --synthetic N')
        names, features = extract(args, dirs, torch, FeatureExtractor)
    if args.save:
        torch.save({'features': features.cpu(), 'names': names}, args.save)
    print(tuple(features.shape))


def extract(args, dirs, torch, FeatureExtractor):
    names = sorted(f for f in os.listdir(dirs[0]) if f.lower().endswith(EXTENSIONS))
    for d in dirs[1:]:
        missing = [f for f in names if not os.path.isfile(os.path.join(d, f))]
        if missing:
            raise SystemExit('%s lacks %d of the %d images of %s (first: %s)' % (d, len(missing), len(names), dirs[0], missing[0]))
    extractor = FeatureExtractor(model_name=args.model, model_path=args.weights, image_size=(args.height, args.width),
                                 batch_size=args.batch,
                                 compute_dtype=torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    features = extractor([[os.path.join(d, f) for f in names] for d in dirs])
    torch.cuda.synchronize()
    return names, features


if __name__ == '__main__':
    main()
