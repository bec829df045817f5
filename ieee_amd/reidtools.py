"""Ranked-result figures, the reference's torchreid/utils/reidtools.py::visualize_ranked_results (:18-154) with the
same call, layout and printed progress.  The ranking comes from the device (ieee_amd.metrics.rank_topk: k indices per
query, the same-identity same-camera entries already skipped) instead of a host argsort of the whole matrix (:49);
the figures are drawn with PIL."""
from __future__ import absolute_import, print_function

import os
import os.path as osp

import numpy as np

__all__ = ['visualize_ranked_results']

GRID_SPACING = 10
QUERY_EXTRA_SPACING = 90
BW = 5  # border width
GREEN = (0, 255, 0)
RED = (255, 0, 0)    # RGB (the reference's (0, 0, 255) is BGR)
BLACK = (0, 0, 0)


def _first(path):
    return path[0] if isinstance(path, (tuple, list)) else path


def _tile(path, width, height, color):
    """imread -> resize -> constant border -> resize again (reidtools.py:83-90 / :119-131): the border keeps the same
    width on every tile"""
    from PIL import Image, ImageOps
    img = Image.open(path).convert('RGB').resize((width, height), Image.BILINEAR)
    img = ImageOps.expand(img, border=BW, fill=color)
    return np.asarray(img.resize((width, height), Image.BILINEAR))


def visualize_ranked_results(distmat, dataset, data_type='image', width=128, height=256, save_dir='', topk=10):
    """Draws, for every query, its image and its top-k kept gallery images in one row (green border: same identity,
    red: another identity) into <save_dir>/<basename of the query's first image>.jpg.

    distmat: [num_query, num_gallery] distances, a CUDA tensor or a numpy array.  dataset: (query, gallery), each a
    list of (img_paths, pid, camid, ...) records.  Returns the ranked gallery indices drawn for every query."""
    from PIL import Image
    from .metrics.topk import rank_topk
    if data_type != 'image':
        raise NotImplementedError("visualize_ranked_results: data_type=%r; only image re-id is supported" % (data_type,))
    num_q, num_g = distmat.shape
    os.makedirs(save_dir or '.', exist_ok=True)

    print('# query: {}\n# gallery {}'.format(num_q, num_g))
    print('Visualizing top-{} ranks ...'.format(topk))

    query, gallery = dataset
    assert num_q == len(query)
    assert num_g == len(gallery)

    q_pids = np.asarray([r[1] for r in query], dtype=np.int64)
    q_camids = np.asarray([r[2] for r in query], dtype=np.int64)
    g_pids = np.asarray([r[1] for r in gallery], dtype=np.int64)
    g_camids = np.asarray([r[2] for r in gallery], dtype=np.int64)
    indices, _ = rank_topk(distmat, topk, q_pids, g_pids, q_camids, g_camids)
    indices = indices.cpu().numpy()

    ranked = []
    for q_idx in range(num_q):
        qimg_path, qpid = query[q_idx][0], q_pids[q_idx]
        qimg_path_name = _first(qimg_path)
        grid_img = 255 * np.ones((height, (topk + 1) * width + topk * GRID_SPACING + QUERY_EXTRA_SPACING, 3),
                                 dtype=np.uint8)
        grid_img[:, :width, :] = _tile(qimg_path_name, width, height, BLACK)
        row = [int(g) for g in indices[q_idx] if g >= 0]
        for rank_idx, g_idx in enumerate(row, start=1):
            border_color = GREEN if g_pids[g_idx] == qpid else RED
            start = rank_idx * width + rank_idx * GRID_SPACING + QUERY_EXTRA_SPACING
            grid_img[:, start:start + width, :] = _tile(_first(gallery[g_idx][0]), width, height, border_color)
        ranked.append(row)

        imname = osp.basename(osp.splitext(qimg_path_name)[0])
        Image.fromarray(grid_img).save(osp.join(save_dir, imname + '.jpg'), quality=95)   # cv2.imwrite's default

        if (q_idx + 1) % 100 == 0:
            print('- done {}/{}'.format(q_idx + 1, num_q))

    print('Done. Images have been saved to "{}" ...'.format(save_dir))
    return ranked
