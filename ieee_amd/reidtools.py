"""Ranked-result figures, the reference's torchreid/utils/reidtools.py::visualize_ranked_results (:18-154) with the
same call, layout and printed progress.  The ranking comes from the device (ieee_amd.metrics.rank_topk: k indices per
query, the same-identity same-camera entries already skipped) instead of a host argsort of the whole matrix (:49);
the figures are drawn with PIL.

Activation-map figures, the reference's tools/visualize_actmap.py::visactmap (:25-154) with the same call, file layout
and printed progress.  The channel energy of the trunk output and the three-panel figures are computed on the device
(ieee_actmap_energy / ieee_actmap_render); the finished bytes cross to the host once per batch and PIL writes them.

Feature-space figures, the reference's torchreid/engine/engine.py::showPointMultiModal (:453-490): one exact t-SNE per
768-wide descriptor slice, all three as one batch on the device (ieee_tsne_affinities / ieee_tsne_run) where the
reference calls sklearn.manifold.TSNE three times, and one scatter drawn with PIL where it calls matplotlib."""
from __future__ import absolute_import, print_function

import os
import os.path as osp

import numpy as np

__all__ = ['visualize_ranked_results', 'jet_table', 'activation_maps', 'render_actmaps', 'visactmap', 'tsne_embed',
           'relabel', 'draw_points', 'show_points_multimodal']

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


def visualize_ranked_results(distmat, dataset, data_type='image', width=128, height=256, save_dir='', topk=10,
                             indices=None):
    """Draws, for every query, its image and its top-k kept gallery images in one row (green border: same identity,
    red: another identity) into <save_dir>/<basename of the query's first image>.jpg.

    distmat: [num_query, num_gallery] distances, a CUDA tensor or a numpy array.  dataset: (query, gallery), each a
    list of (img_paths, pid, camid, ...) records.  Returns the ranked gallery indices drawn for every query.

    indices (not in the reference): with distmat=None, a ranking that exists already, [num_query, topk] gallery indices
    with -1 for no entry -- what ieee_amd.metrics.search_topk returns without ever forming the matrix.  It is drawn as
    it is (the first topk columns): nothing is ranked or filtered here.  Give exactly one of distmat and indices."""
    from PIL import Image
    if data_type != 'image':
        raise NotImplementedError("visualize_ranked_results: data_type=%r; only image re-id is supported" % (data_type,))
    if (distmat is None) == (indices is None):
        raise ValueError("visualize_ranked_results: give either distmat or indices, not %s" %
                         ("both" if distmat is not None else "neither"))
    if indices is not None:
        indices = np.asarray(indices.detach().cpu().numpy() if hasattr(indices, 'detach') else indices)
        if indices.ndim != 2 or indices.shape[0] != len(dataset[0]) or indices.dtype.kind not in 'iu':
            raise ValueError("visualize_ranked_results: indices must be integers [%d, topk], got %s %s"
                             % (len(dataset[0]), indices.dtype, indices.shape))
        if indices.size and (indices.max() >= len(dataset[1]) or indices.min() < -1):
            raise ValueError("visualize_ranked_results: indices must lie in [-1, %d)" % len(dataset[1]))
        indices = indices[:, :topk]
        num_q, num_g = indices.shape[0], len(dataset[1])
    else:
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
    if indices is None:
        from .metrics.topk import rank_topk
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


# ---- activation maps (tools/visualize_actmap.py) ---------------------------------------------------------------------
IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]
_MODALS = ('RGB', 'NI', 'TI')
_lut_cache = {}


def jet_table():
    """The default colour table of the activation-map figures: the closed-form jet, uint8 [256][3] RGB.  With v = i / 255:
    r = clip(min(4v - 1.5, -4v + 4.5), 0, 1), g = clip(min(4v - 0.5, -4v + 3.5), 0, 1), b = clip(min(4v + 0.5,
    -4v + 2.5), 0, 1), bytes floor(255 c + 0.5), in float64.  (The reference calls cv2.applyColorMap(am, COLORMAP_JET),
    visualize_actmap.py:131; whoever has cv2 can hand its table -- RGB order -- to render_actmaps / visactmap instead.)"""
    v = np.arange(256, dtype=np.float64) / 255.0
    tab = np.empty((256, 3), dtype=np.uint8)
    for c, (lo, hi) in enumerate(((-1.5, 4.5), (-0.5, 3.5), (0.5, 2.5))):
        tab[:, c] = np.floor(255.0 * np.clip(np.minimum(4.0 * v + lo, -4.0 * v + hi), 0.0, 1.0) + 0.5).astype(np.uint8)
    return tab


def _energy(x):
    """x: contiguous channels-last [..., h, w, C] on the device, fp32 or bf16 -> fp32 [..., h, w]"""
    import torch
    from . import _lib
    lib = _lib.require_gpu()
    lead, (h, w, C) = x.shape[:-3], x.shape[-3:]
    n = 1
    for d in lead:
        n *= int(d)
    out = torch.empty(tuple(lead) + (h, w), dtype=torch.float32, device=x.device)
    dt = _lib.IEEE_BF16 if x.dtype == torch.bfloat16 else _lib.IEEE_F32
    _lib.check(lib.ieee_actmap_energy(_lib.ptr(x), dt, n, h * w, C, _lib.ptr(out), _lib.stream()))
    return out


def activation_maps(featuremaps):
    """Activation maps of convolutional feature maps (visualize_actmap.py:84-88): the channel energy sum_c x^2 of every
    position, L2-normalised over each image's positions (F.normalize, eps 1e-12), on the device.

    featuremaps: a 5-D tensor is the native channels-last form [M, B, h, w, C] (`model.trunk_maps`), read in place; a
    4-D tensor is one NCHW map [B, C, h, w] as a torch model returns it (made channels-last with torch first); a list
    or tuple of those gives one more leading axis.  fp32 and bf16 are read as they are, anything else as fp32.
    Returns fp32 [..., h, w] on the device."""
    import torch
    if isinstance(featuremaps, (list, tuple)):
        return torch.stack([activation_maps(f) for f in featuremaps])
    x = featuremaps
    if not torch.is_tensor(x) or x.dim() not in (4, 5):
        raise ValueError('activation_maps: expected [B, C, h, w], the native [M, B, h, w, C], or a list of them; got %s'
                         % (tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
    from . import _lib
    _lib.require_gpu()
    x = x.detach()
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.to(torch.float32)
    x = x.cuda()
    if x.dim() == 4:
        x = x.permute(0, 2, 3, 1)
    return _energy(x.contiguous())


def _lut_on(device, colormap):
    import torch
    if colormap is None:
        key = str(device)
        if key not in _lut_cache:
            _lut_cache[key] = torch.from_numpy(jet_table()).to(device)
        return _lut_cache[key]
    lut = torch.as_tensor(np.ascontiguousarray(colormap.cpu().numpy() if torch.is_tensor(colormap) else colormap))
    if lut.dtype != torch.uint8 or lut.numel() != 768:
        raise ValueError('colormap: expected 256 RGB triples of uint8')
    return lut.reshape(256, 3).contiguous().to(device)


def render_actmaps(imgs, amaps, width, height, img_mean=None, img_std=None, colormap=None, return_index=False):
    """The figures of visualize_actmap.py:119-146 for a batch, on the device.

    imgs: the normalised network input [N, 3, height, width] of the modality shown, or None (then only the colour
    indices are computed); amaps: [N, h, w] from `activation_maps`; colormap: uint8 [256][3] RGB, default `jet_table()`.
    Returns the uint8 grids [N, height, 3 * width + 20, 3] (RGB; left to right: image, coloured map, overlay, two 10-pixel
    white gaps), or (grids, index) with return_index, index = the uint8 [N, height, width] colour index before the table;
    grids is None when imgs is None.  The arithmetic is fixed by include/ieee_amd.h (ieee_actmap_render)."""
    import ctypes
    import torch
    from . import _lib
    lib = _lib.require_gpu()
    if img_mean is None or img_std is None:
        img_mean, img_std = IMAGENET_MEAN, IMAGENET_STD
    amaps = amaps.detach().to(device='cuda', dtype=torch.float32).contiguous()
    if amaps.dim() != 3:
        raise ValueError('render_actmaps: amaps must be [N, h, w], got %s' % (tuple(amaps.shape),))
    N, h, w = amaps.shape
    dev = amaps.device
    grids = index = None
    if imgs is not None:
        if tuple(imgs.shape) != (N, 3, height, width):
            raise ValueError('render_actmaps: imgs must be [%d, 3, %d, %d] (N, 3, height, width), got %s'
                             % (N, height, width, tuple(imgs.shape)))
        imgs = imgs.detach().to(device=dev, dtype=torch.float32).contiguous()
        grids = torch.empty((N, height, 3 * width + 2 * GRID_SPACING, 3), dtype=torch.uint8, device=dev)
    elif not return_index:
        raise ValueError('render_actmaps: without imgs there is only the index to return (return_index=True)')
    if return_index:
        index = torch.empty((N, height, width), dtype=torch.uint8, device=dev)
    mean3 = (ctypes.c_float * 3)(*[float(v) for v in img_mean])
    std3 = (ctypes.c_float * 3)(*[float(v) for v in img_std])
    lut = _lut_on(dev, colormap)
    _lib.check(lib.ieee_actmap_render(_lib.ptr(amaps), h, w, _lib.ptr(imgs), mean3, std3, _lib.ptr(lut), N, height, width,
                                      _lib.ptr(grids), _lib.ptr(index), _lib.stream()))
    return (grids, index) if return_index else grids


def visactmap(model, test_loader, save_dir, save_name, width, height, use_gpu, modal, img_mean=None, img_std=None,
              colormap=None):
    """tools/visualize_actmap.py::visactmap (:25-154): for every query image of every target dataset, the figure [image |
    activation map | overlay] of modality `modal` ('RGB', 'NI' or 'TI') into <save_dir>/actmap_vis_<save_name>/<basename
    of the image>.jpg.  A model with `trunk_maps` (IEEE3modalPart) is read through it, without a copy of the maps; any
    other model is called as the reference calls it, `model(imgs, return_featuremaps=True)`.  Batches may be on the CPU
    or the device and are left as they were (the reference de-normalises the caller's tensors in place, :119-120); every
    image must already have the figure's size (height, width), which the reference's slice assignment (:143) implies.
    The kernels need the device: `use_gpu=False` is an error.  One device-to-host copy per batch.  Returns the paths
    written."""
    import torch
    from PIL import Image
    from .data.loader import DeviceLoader
    if modal not in _MODALS:
        print("Unknow modal!")
        raise RuntimeError("visactmap: modal must be one of %s, got %r" % (list(_MODALS), modal))
    mi = _MODALS.index(modal)
    if img_mean is None or img_std is None:
        # use imagenet mean and std
        img_mean, img_std = IMAGENET_MEAN, IMAGENET_STD
    if not use_gpu:
        from ._lib import IeeeAmdError
        raise IeeeAmdError("visactmap: the activation-map kernels run on the GPU; there is no CPU path (use_gpu=False)")

    model.eval()
    core = getattr(model, 'module', model)
    native = hasattr(core, 'trunk_maps')
    written = []
    with torch.no_grad():
        for target in list(test_loader.keys()):
            data_loader = test_loader[target]['query']  # only process query images
            actmap_dir = osp.join(save_dir, 'actmap_vis_' + save_name)
            os.makedirs(actmap_dir, exist_ok=True)
            print('Visualizing activation maps for {} ...'.format(target))
            # the reference's collate gives impath as [modality][sample] (:98-102); this package's DeviceLoader keeps the
            # records' own [sample][modality]
            by_sample = isinstance(data_loader, DeviceLoader)

            for batch_idx, data in enumerate(data_loader):
                imgs, paths = data['img'], data['impath']
                for i in range(len(imgs)):
                    if tuple(imgs[i].shape[-2:]) != (height, width):
                        raise ValueError('visactmap: images of %s are %d x %d but the figure is height %d x width %d; load '
                                         'them at the size given here' % (_MODALS[i] if i < 3 else i, imgs[i].shape[-2],
                                                                          imgs[i].shape[-1], height, width))
                dev_imgs = [im.cuda() for im in imgs]         # new list: the caller's stays as it is
                if native:
                    amaps = activation_maps(core.trunk_maps(dev_imgs)[mi:mi + 1])[0]
                else:
                    try:
                        outputs = model(dev_imgs, return_featuremaps=True)[mi]
                    except TypeError:
                        raise TypeError('forward() got unexpected keyword argument "return_featuremaps". '
                                        'Please add return_featuremaps as an input argument to forward(). When '
                                        'return_featuremaps=True, return feature maps only.')
                    if outputs.dim() != 4:
                        raise ValueError('The model output is supposed to have shape of (b, c, h, w), i.e. 4 dimensions, '
                                         'but got {} dimensions. Please make sure you set the model output at eval mode '
                                         'to be the last convolutional feature maps'.format(outputs.dim()))
                    amaps = activation_maps(outputs)
                grids = render_actmaps(dev_imgs[mi], amaps, width, height, img_mean, img_std, colormap).cpu().numpy()
                for j in range(grids.shape[0]):
                    path = paths[j][mi] if by_sample else paths[mi][j]
                    imname = osp.basename(osp.splitext(path)[0])
                    out = osp.join(actmap_dir, imname + '.jpg')
                    Image.fromarray(grids[j]).save(out, quality=95)       # cv2.imwrite's default
                    written.append(out)

                if (batch_idx + 1) % 10 == 0:
                    print('- done batch {}/{}'.format(batch_idx + 1, len(data_loader)))
    return written


# ---- descriptor t-SNE (torchreid/engine/engine.py:453-490) -------------------------------------------------------------
# darkorange, limegreen, royalblue, red, darkviolet, black (engine.py:474)
TSNE_COLORS = ((255, 140, 0), (50, 205, 50), (65, 105, 225), (255, 0, 0), (148, 0, 211), (0, 0, 0))
TSNE_ALPHA = 0.4
_FIGURE_MARGIN = 0.1      # the unit square of the coordinates sits inside this share of the canvas on every side


def _pca_init(x):
    """sklearn's init='pca' for x [B, N, d] on the device: the top two principal axes from the eigenvectors of the centred
    covariance in float64, each signed so that its largest-magnitude loading is positive, the projection scaled so that the
    first column has standard deviation 1e-4 (sklearn/manifold/_t_sne.py, _fit)"""
    import torch
    xc = x.to(torch.float64)
    xc = xc - xc.mean(1, keepdim=True)
    _, vecs = torch.linalg.eigh(xc.transpose(1, 2) @ xc)                 # ascending eigenvalues
    v = vecs[:, :, -2:].flip(2)                                          # [B, d, 2], the largest first
    lead = torch.gather(v, 1, v.abs().argmax(1, keepdim=True))           # [B, 1, 2]
    v = v * torch.where(lead < 0, -torch.ones_like(lead), torch.ones_like(lead))
    y = xc @ v
    return (y / y[:, :, :1].std(1, unbiased=False, keepdim=True) * 1e-4).to(torch.float32)


def tsne_embed(features, perplexity=30.0, n_iter=1000, early_exaggeration=12.0, exaggeration_iters=250,
               learning_rate='auto', init='pca', generator=None, return_info=False):
    """Exact t-SNE of descriptors into the plane, on the device: what sklearn.manifold.TSNE(n_components=2,
    method='exact') computes, with sklearn's perplexity search, exaggeration, momentum and gains schedule
    (include/ieee_amd.h: ieee_tsne_affinities, ieee_tsne_run).  All n_iter iterations always run: sklearn's two
    early-stopping rules (min_grad_norm, n_iter_without_progress) would need a host read every 50 iterations.

    features: [N, d], or [B, N, d] for B independent problems in one batch (N <= 12288).  Distances come from
    compute_distance_matrix(x, x).  learning_rate 'auto' = max(N / early_exaggeration / 4, 50).  init: an [N, 2] /
    [B, N, 2] tensor used as given, 'random' (1e-4 * randn from `generator`, a torch.Generator of the device), or 'pca'.
    Returns fp32 [N, 2] / [B, N, 2] on the device of `features` (CPU in, CPU out); with return_info also a dict:
    kl_history and grad_norm_history [B, n_iter] (the KL divergence at each iteration's coordinates before its update,
    the gradient's 2-norm), beta [B, N], kl_divergence [B] (the last history value; without the leading B for [N, d])."""
    import torch
    from . import _lib
    from .metrics.distance import compute_distance_matrix
    if not torch.is_tensor(features) or features.dim() not in (2, 3):
        raise ValueError('tsne_embed: features must be a [N, d] or [B, N, d] tensor, got %s'
                         % (tuple(features.shape) if torch.is_tensor(features) else type(features).__name__))
    single = features.dim() == 2
    B, N, d = (1,) + tuple(features.shape) if single else tuple(features.shape)
    if perplexity >= N:
        raise ValueError('perplexity must be less than n_samples')
    lib = _lib.require_gpu()
    home = features.device
    x = features.detach().to(device='cuda', dtype=torch.float32).reshape(B, N, d).contiguous()
    dev = x.device
    if learning_rate == 'auto':
        learning_rate = max(N / early_exaggeration / 4.0, 50.0)
    if torch.is_tensor(init):
        if tuple(init.shape) != ((N, 2) if single else (B, N, 2)):
            raise ValueError('tsne_embed: init must be %s, got %s' % ((N, 2) if single else (B, N, 2), tuple(init.shape)))
        Y = init.detach().to(device=dev, dtype=torch.float32).reshape(B, N, 2).clone().contiguous()
    elif init == 'random':
        Y = 1e-4 * torch.randn((B, N, 2), dtype=torch.float32, device=dev, generator=generator)
    elif init == 'pca':
        Y = _pca_init(x).contiguous()
    else:
        raise ValueError("tsne_embed: init must be 'pca', 'random' or a tensor, got %r" % (init,))

    ldp = (N + 3) // 4 * 4
    dist = torch.stack([compute_distance_matrix(x[b], x[b]) for b in range(B)])
    P = torch.empty((B, N, ldp), dtype=torch.float32, device=dev)
    beta = torch.empty((B, N), dtype=torch.float32, device=dev)
    nbytes = lib.ieee_tsne_workspace_bytes(N, B)
    if nbytes < 0:
        _lib.check(-1)
    work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.ieee_tsne_affinities(_lib.ptr(dist), N, N, B, float(perplexity), _lib.ptr(P), ldp, _lib.ptr(beta),
                                        _lib.ptr(work), nbytes, _lib.stream()))
    update, gains = torch.zeros_like(Y), torch.ones_like(Y)
    history = torch.empty((B, n_iter, 2), dtype=torch.float32, device=dev) if return_info else None
    _lib.check(lib.ieee_tsne_run(_lib.ptr(P), ldp, N, B, _lib.ptr(Y), _lib.ptr(update), _lib.ptr(gains), 0, int(n_iter),
                                 int(exaggeration_iters), float(early_exaggeration), float(learning_rate),
                                 _lib.ptr(history), _lib.ptr(work), nbytes, _lib.stream()))
    out = (Y[0] if single else Y).to(home)
    if not return_info:
        return out
    pick = (lambda t: t[0]) if single else (lambda t: t)
    info = {'kl_history': pick(history[:, :, 0]).to(home), 'grad_norm_history': pick(history[:, :, 1]).to(home),
            'beta': pick(beta).to(home),
            'kl_divergence': pick(history[:, -1, 0]).to(home) if n_iter > 0 else None}
    return out, info


def relabel(labels):
    """engine.py:453-461: a consecutive index that moves on wherever the label changes from one row to the next"""
    out, index = [], 0
    for i, v in enumerate(labels):
        if i > 0 and v != labels[i - 1]:
            index += 1
        out.append(index)
    return out


def _marker(kind, cx, cy, r):
    """polygon of a star or an upward triangle around (cx, cy); None for the circle"""
    import math
    if kind == 1:
        return None
    if kind == 2:
        return [(cx + r * math.sin(a), cy - r * math.cos(a)) for a in (0.0, 2.0 * math.pi / 3.0, 4.0 * math.pi / 3.0)]
    pts = []
    for k in range(10):
        a, rad = k * math.pi / 5.0, (r if k % 2 == 0 else 0.382 * r)
        pts.append((cx + rad * math.sin(a), cy - rad * math.cos(a)))
    return pts


def draw_points(coords, labels, draw_label, save_path, size=2000):
    """The scatter of engine.py:482-490 with PIL: coords [3, N, 2] in [0, 1] (one slice per marker: star, circle,
    triangle), labels the relabelled identity of every row; only rows whose label is in draw_label are drawn, in colour
    TSNE_COLORS[draw_label.index(label) % 6] at alpha 0.4, onto a white size x size canvas saved as JPEG.  x runs right
    and y up, inside a margin of a tenth of the canvas; marker diameters follow matplotlib's s = 300, 300, 400 points^2
    on a 20-inch figure.  No axes are drawn and no pixel equality with matplotlib is claimed."""
    from PIL import Image, ImageDraw
    coords = np.asarray(coords.detach().cpu().numpy() if hasattr(coords, 'detach') else coords, dtype=np.float64)
    if coords.ndim != 3 or coords.shape[0] != 3 or coords.shape[2] != 2 or coords.shape[1] != len(labels):
        raise ValueError('draw_points: coords must be [3, %d, 2], got %s' % (len(labels), coords.shape))
    draw_label = list(draw_label)
    canvas = Image.new('RGB', (size, size), (255, 255, 255))
    span = size * (1.0 - 2.0 * _FIGURE_MARGIN)
    radius = [0.5 * (s ** 0.5) * size / 1440.0 for s in (300.0, 300.0, 400.0)]      # points -> pixels: size / (20 * 72)
    radius[0] *= 1.3                                                                # a star's tips reach past the circle
    alpha = int(round(255 * TSNE_ALPHA))
    for i, lab in enumerate(labels):
        if lab not in draw_label:
            continue
        color = TSNE_COLORS[draw_label.index(lab) % 6]
        for m in range(3):
            r = radius[m]
            cx = size * _FIGURE_MARGIN + coords[m, i, 0] * span
            cy = size * (1.0 - _FIGURE_MARGIN) - coords[m, i, 1] * span
            x0, y0 = int(cx - r) - 2, int(cy - r) - 2
            box = (max(x0, 0), max(y0, 0), min(x0 + int(2 * r) + 5, size), min(y0 + int(2 * r) + 5, size))
            if box[0] >= box[2] or box[1] >= box[3]:
                continue
            patch = canvas.crop(box).convert('RGBA')
            layer = Image.new('RGBA', patch.size, (0, 0, 0, 0))
            pen = ImageDraw.Draw(layer)
            poly = _marker(m, cx - box[0], cy - box[1], r)
            if poly is None:
                pen.ellipse((cx - box[0] - r, cy - box[1] - r, cx - box[0] + r, cy - box[1] + r), fill=color + (alpha,))
            else:
                pen.polygon(poly, fill=color + (alpha,))
            canvas.paste(Image.alpha_composite(patch, layer).convert('RGB'), box[:2])
    os.makedirs(osp.dirname(save_path) or '.', exist_ok=True)
    canvas.save(save_path, 'JPEG', quality=95)
    return save_path


def modality_slices(features):
    """engine.py:467-469: columns 0:768, 768:1536, 1536:2304, by position -> [3, N, 768]"""
    import torch
    if features.dim() != 2 or features.shape[1] < 2304:
        raise ValueError('expected [N, 2304] descriptors, got %s' % (tuple(features.shape),))
    return torch.stack([features[:, 0:768], features[:, 768:1536], features[:, 1536:2304]])


def minmax_scale(coords):
    """engine.py:476-481: (y - min) / (max - min) per slice and axis, [..., N, 2] -> the same shape in [0, 1]"""
    lo = coords.min(-2, keepdim=True).values
    hi = coords.max(-2, keepdim=True).values
    return (coords - lo) / (hi - lo)


def show_points_multimodal(features, real_label, draw_label, save_path, **tsne_kwargs):
    """engine.py::showPointMultiModal (:463-490): t-SNE of the three 768-wide slices of `features` [N, 2304] (one batched
    tsne_embed call; tsne_kwargs go to it), min-max scaled per slice and axis, the rows whose relabelled identity is in
    draw_label drawn into <save_path>/<str(draw_label)>.jpg.  Returns (path, scaled coordinates [3, N, 2])."""
    draw_label = list(draw_label)
    path = osp.join(save_path, str(draw_label) + '.jpg')
    print('Draw points of features to {}'.format(path))
    labels = relabel([int(v) for v in np.asarray(real_label).reshape(-1)])
    coords = minmax_scale(tsne_embed(modality_slices(features), **tsne_kwargs))
    draw_points(coords, labels, draw_label, path)
    return path, coords
