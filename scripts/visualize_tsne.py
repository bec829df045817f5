#!/usr/bin/env python
"""Feature-space figure of query descriptors: what the reference's evaluator draws under its visrank flag
(torchreid/engine/engine.py:437-439, 463-490), without an evaluation around it.  One exact t-SNE per 768-wide slice of
the [N, 2304] descriptors, all three as one batch on the device, drawn into <save-dir>/<labels>.jpg (star, circle and
triangle for the three slices, one colour per identity).

  python scripts/visualize_tsne.py --synthetic 30 --save-dir /tmp/tsne                  (generated descriptors)
  python scripts/visualize_tsne.py --features qf.pt --save-dir log/tsne --labels 1,2,3  (a torch file with 'features'
                                                                                         [N, 2304] and 'pids' [N])

Inside an evaluation the same figure comes from engine.run(test_only=True, vistsne=True, vistsne_labels=[...])."""
import argparse
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ieee_amd  # noqa: E402,F401  (before torch.cuda is touched: it picks GPU_MAX_HW_QUEUES)


def synthetic(ids, per_id=4, seed=0):
    """ids identities x per_id images: every 768-wide slice is its own clustering (centre scale 2, unit noise)"""
    import torch
    g = torch.Generator().manual_seed(seed)
    pids = torch.arange(ids).repeat_interleave(per_id)
    parts = [2.0 * torch.randn(ids, 768, generator=g)[pids] + torch.randn(ids * per_id, 768, generator=g) for _ in range(3)]
    return torch.cat(parts, 1), pids


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--synthetic', type=int, default=0, help='generate descriptors of this many identities')
    parser.add_argument('--features', type=str, default='', help="torch file: {'features': [N, 2304], 'pids': [N]}")
    parser.add_argument('--save-dir', type=str, default=os.path.join('log', 'tsne'))
    parser.add_argument('--labels', type=str, default='',
                        help='comma-separated relabelled identities to draw; default: six of 1..29 at random')
    parser.add_argument('--perplexity', type=float, default=30.0)
    parser.add_argument('--n-iter', type=int, default=1000)
    args = parser.parse_args()

    import torch
    from ieee_amd.reidtools import show_points_multimodal
    if args.synthetic:
        feats, pids = synthetic(args.synthetic)
    elif args.features:
        blob = torch.load(args.features, map_location='cpu')
        feats, pids = blob['features'], blob['pids']
    else:
        raise SystemExit('give --synthetic N or --features FILE')
    labels = [int(v) for v in args.labels.split(',')] if args.labels else random.sample(range(1, 30), 6)
    path, coords = show_points_multimodal(feats.cuda(), [int(p) for p in pids], labels, args.save_dir,
                                          perplexity=args.perplexity, n_iter=args.n_iter)
    print('%d rows embedded, figure in %s' % (coords.shape[1], path))


if __name__ == '__main__':
    main()
