#!/usr/bin/env python
"""Activation-map figures of a trained checkpoint: the reference's tools/visualize_actmap.py (:157-198) on ieee_amd, with
its arguments.  For every query image, <save-dir>/actmap_vis_<save-name>/<image name>.jpg shows the image, where the
chosen modality's trunk looks, and the two overlaid.

  python scripts/visualize_actmap.py --root /data -d RGBNT201 -m ieee3modalPart --weights model.pth.tar-60 \
      --save-dir log/actmap --save-name run1 --modal TI
  python scripts/visualize_actmap.py --synthetic 8 --save-dir /tmp/actmap --save-name demo      (a generated JPEG tree)

The maps and the figures are computed on the device (ieee_amd.reidtools.visactmap); only the finished bytes are copied
back, once per batch."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ieee_amd  # noqa: E402,F401  (before torch.cuda is touched: it picks GPU_MAX_HW_QUEUES)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--root', type=str, default='', help='directory that holds RGBNT201/')
    parser.add_argument('-d', '--dataset', type=str, default='RGBNT201')
    parser.add_argument('-m', '--model', type=str, default='ieee3modalPart')
    parser.add_argument('--weights', type=str)
    parser.add_argument('--save-dir', type=str, default=os.path.join('log', 'actmap'))
    parser.add_argument('--save-name', type=str, default='actmap')
    parser.add_argument('--modal', type=str, default='RGB')
    parser.add_argument('--height', type=int, default=256)
    parser.add_argument('--width', type=int, default=128)
    parser.add_argument('--synthetic', type=int, default=0,
                        help='generate a JPEG tree with this many identities instead of --root')
    parser.add_argument('--batch', type=int, default=100, help='test batch size (the reference tool uses 100)')
    parser.add_argument('--workers', type=int, default=4)
    parser.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    args = parser.parse_args()

    import torch
    from ieee_amd import data as D
    from ieee_amd.checkpoint import load_pretrained_weights
    from ieee_amd.models import build_model
    from ieee_amd.reidtools import visactmap

    if args.dataset != 'RGBNT201':
        raise SystemExit('only the RGBNT201 layout is registered (ieee_amd.data), got %r' % args.dataset)
    use_gpu = torch.cuda.is_available()
    root = args.root
    if args.synthetic:
        root = os.path.join(tempfile.gettempdir(), 'ieee_example_tree_%d' % args.synthetic)
        if not os.path.isdir(os.path.join(root, 'RGBNT201')):
            sys.path.insert(0, os.path.join(ROOT, 'scripts'))
            import loader_probe
            loader_probe.make_tree(root, n_ids=args.synthetic, per_id=8)
    dataset = D.RGBNT201(root=root)
    _, test_transform = D.build_transforms(args.height, args.width, [])
    query = D.DeviceLoader(dataset.query, test_transform, args.batch, workers=args.workers)     # only query images are drawn
    test_loader = {args.dataset: {'query': query}}

    model = build_model(name=args.model, num_classes=dataset.num_train_pids, pretrained=False, use_gpu=use_gpu,
                        compute_dtype=torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    if use_gpu:
        model = model.cuda()
    if args.weights and os.path.isfile(args.weights):
        load_pretrained_weights(model, args.weights)

    paths = visactmap(model, test_loader, args.save_dir, args.save_name, args.width, args.height, use_gpu=use_gpu,
                      modal=args.modal)
    print('%d figures in %s' % (len(paths), os.path.dirname(paths[0]) if paths else args.save_dir))


if __name__ == '__main__':
    main()
