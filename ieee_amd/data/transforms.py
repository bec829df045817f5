"""Device-side image transforms (reference torchreid/data/transforms.py:233-326 with the live option set of
configs/RGBNT_ieee_part_margin.yaml: Resize, RandomHorizontalFlip, ToTensor, Normalize).  The host only computes
Pillow's per-axis resampling tables (a few hundred integers per distinct source size, cached) and draws the flip
decisions; the pixels are resized, flipped, scaled and normalised by ieee_resize_flip_normalize on the GPU, bit-exactly
what torchvision.transforms does through Pillow on the CPU.
The reference's other train augmentations -- random_crop (Random2DTranslation), color_jitter (torchvision ColorJitter
with brightness 0.2 / contrast 0.15) and random_erase (RandomErasing) -- are drawn on the host into an AugmentPlan
(draw_plan) and applied on the GPU by ieee_augment_normalize ("Train augmentations on the device").
A list of images of MIXED sizes (detector crops, datasets that are not one size) needs no host tables at all: pack_ragged
packs it into one byte buffer and ieee_resize_normalize_ragged resizes the whole batch in one launch, computing Pillow's
coefficients on the device (DeviceTransform.ragged; DESIGN.md, "Ragged batches")."""
import math
import random as _random

import numpy as np
import torch

from .. import _lib

PRECISION_BITS = 32 - 8 - 2       # Pillow's 8-bit resampler keeps 22 fractional bits
IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]


def _axis_tables(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear (triangle) filter over a whole axis:
    bounds int32 [out][2] = (first source index, count), weights int32 [out][ksize] (22-bit fixed point)"""
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size     # the box edges are C floats
    filterscale = scale if scale > 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.float64)
    inv = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        x = np.arange(xmax, dtype=np.float64)
        w = np.abs((x + xmin - center + 0.5) * inv)
        w = np.where(w < 1.0, 1.0 - w, 0.0)
        ww = 0.0
        for v in w:                      # same left-to-right double accumulation as the C loop
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        kk[xx, :xmax] = w
        bounds[xx] = (xmin, xmax)
    fixed = np.trunc(np.where(kk < 0, -0.5, 0.5) + kk * (1 << PRECISION_BITS)).astype(np.int32)
    return bounds, fixed, ksize


_TABLE_CACHE = {}


def resample_tables(hs, ws, ho, wo):
    """everything ieee_resize_flip_normalize needs for an (hs, ws) -> (ho, wo) resize, as Pillow's ImagingResample
    plans it: the horizontal pass runs first and only over the source rows the vertical pass will read"""
    key = (hs, ws, ho, wo)
    if key not in _TABLE_CACHE:
        bh, kh, ksh = _axis_tables(ws, wo)
        bv, kv, ksv = _axis_tables(hs, ho)
        y0 = int(bv[0, 0])
        _TABLE_CACHE[key] = dict(need_h=wo != ws, need_v=ho != hs, bounds_h=bh, kk_h=kh, ksize_h=ksh, bounds_v=bv,
                                 kk_v=kv, ksize_v=ksv, ybox_first=y0, tmp_rows=int(bv[ho - 1, 0] + bv[ho - 1, 1]) - y0)
    return _TABLE_CACHE[key]


RAGGED_ALIGN = 16     # pack_ragged starts every image on a multiple of this many bytes


class _Staging(object):
    """the packed bytes of one ragged batch on their way to the device: one buffer, pinned where there is a GPU and grown by
    doubling; `done` is recorded behind the copy out of it and waited for before the host writes it again.  Owned by ONE
    caller at a time, like the flip and plan rings: a DeviceTransform keeps its own, pack_ragged the module's.  (Not a
    threading.local: a child forked from another thread -- a decode worker started by the prefetch thread -- destroys the
    thread-local objects of every other thread, and freeing pinned memory or an event there takes the child down.)"""

    def __init__(self):
        self.buf = self.done = self.done_on = None

    def room(self, nbytes):
        if self.done is not None:
            self.done.synchronize()
        if self.buf is None or self.buf.numel() < nbytes:
            size = max(1 << 20, 1 << int(nbytes - 1).bit_length())
            self.buf = torch.empty(size, dtype=torch.uint8)
            if torch.cuda.is_available():
                self.buf = self.buf.pin_memory()
        return self.buf


_STAGING = _Staging()       # pack_ragged's own


def _as_rgb_u8(im):
    im = np.asarray(im)
    if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
        raise ValueError("expected uint8 HxWx3 images (PIL 'RGB'), got %s %s" % (im.dtype, im.shape))
    return im


def _pack_ragged(images, staging, tail=0):
    """pack_ragged into `staging`, with `tail` spare bytes behind the images (16-byte aligned):
    -> (the staging tensor, image bytes, offsets, sizes)"""
    arrays = [_as_rgb_u8(im) for im in images]
    n = len(arrays)
    sizes = np.zeros((n, 2), dtype=np.int32)
    offsets = np.zeros(n, dtype=np.int64)
    at = 0
    for i, a in enumerate(arrays):
        sizes[i] = a.shape[:2]
        offsets[i] = at
        at += -(-a.size // RAGGED_ALIGN) * RAGGED_ALIGN
    stage = staging.room(at + tail)
    flat = stage.numpy()
    for a, off in zip(arrays, offsets):
        flat[off:off + a.size].reshape(a.shape)[...] = a           # one pass, strided sources included
    return stage, at, offsets, sizes


def pack_ragged(images):
    """N uint8 HxWx3 images (arrays, PIL 'RGB' images; any strides), each of its own size -> (buffer uint8 [bytes], offsets
    int64 [N], sizes int32 [N, 2] = (H, W)): image i is the tightly packed [H][W][3] block at buffer[offsets[i]:]; every image
    starts on a multiple of 16 bytes.  Host only.  `buffer` is a view of ONE staging buffer (pinned where there is a GPU)
    that the next call overwrites: one caller at a time."""
    stage, nbytes, offsets, sizes = _pack_ragged(images, _STAGING)
    return stage.numpy()[:nbytes], offsets, sizes


PLAN_WORDS = 12       # int32 words per image of the packed plan (ieee_augment_normalize; include/ieee_amd.h)
STAGE_FLIP, STAGE_CROP, STAGE_JITTER, STAGE_ERASE = 1, 2, 4, 8


class AugmentPlan(object):
    """The random decisions of n images, one row per image:
    flip [n] uint8; crop [n][3] int32 = (flag, x1, y1); jitter_first [n] uint8 (0: brightness before contrast, 1: after),
    jitter_b / jitter_c [n] float32 (the two blend factors); erase [n][4] int32 = (r0, c0, h, w), h = 0: no rectangle.
    plan[rows] (a slice or an index array) is the plan of those rows."""
    FIELDS = ('flip', 'crop', 'jitter_first', 'jitter_b', 'jitter_c', 'erase')

    def __init__(self, n):
        self.flip = np.zeros(n, dtype=np.uint8)
        self.crop = np.zeros((n, 3), dtype=np.int32)
        self.jitter_first = np.zeros(n, dtype=np.uint8)
        self.jitter_b = np.ones(n, dtype=np.float32)
        self.jitter_c = np.ones(n, dtype=np.float32)
        self.erase = np.zeros((n, 4), dtype=np.int32)

    def __len__(self):
        return len(self.flip)

    def __getitem__(self, rows):
        if isinstance(rows, (int, np.integer)):
            rows = slice(rows, rows + 1)
        out = AugmentPlan(0)
        for f in self.FIELDS:
            setattr(out, f, np.ascontiguousarray(getattr(self, f)[rows]))
        return out

    def __eq__(self, other):
        return isinstance(other, AugmentPlan) and all(np.array_equal(getattr(self, f), getattr(other, f)) for f in self.FIELDS)

    def pack(self):
        """int32 [n][PLAN_WORDS]: flip, crop flag, x1, y1, jitter_first, bits of b, bits of c, r0, c0, h, w, 0 (the
        device adds each image's sum of L into the last word)"""
        p = np.zeros((len(self), PLAN_WORDS), dtype=np.int32)
        p[:, 0] = self.flip
        p[:, 1:4] = self.crop
        p[:, 4] = self.jitter_first
        p[:, 5] = self.jitter_b.view(np.int32)
        p[:, 6] = self.jitter_c.view(np.int32)
        p[:, 7:11] = self.erase
        return p


class DeviceTransform(object):
    """callable(list of uint8 HxWx3 arrays) -> float32 [N,3,height,width] CUDA tensor.  `train` enables the random
    flip when 'random_flip' is among `transforms`; one torch.rand(1) is drawn per image, in call order, exactly like
    torchvision.transforms.RandomHorizontalFlip inside the reference's per-image Compose.  'random_crop',
    'color_jitter' and 'random_erase' are the reference's stages of those names, in the reference's order
    (flip, crop, jitter, ToTensor, Normalize, erase) whatever the order of the list; they are accepted with augment=True
    (which build_transforms passes) -- without it the constructor takes 'random_flip' alone, as it always has."""

    SUPPORTED = ('random_flip', 'random_crop', 'color_jitter', 'random_erase')
    BRIGHTNESS, CONTRAST = (0.8, 1.2), (0.85, 1.15)      # ColorJitter(brightness=0.2, contrast=0.15, saturation=0, hue=0)

    def __init__(self, height, width, transforms='random_flip', norm_mean=None, norm_std=None, train=True, device=None,
                 augment=False):
        if transforms is None:
            transforms = []
        if isinstance(transforms, str):
            transforms = [transforms]
        if not isinstance(transforms, list):
            raise ValueError('transforms must be a list of strings, but found to be {}'.format(type(transforms)))
        transforms = [t.lower() for t in transforms]
        for t in transforms:
            if t == 'random_patch':
                raise NotImplementedError("transform 'random_patch' is not built: it keeps a pool of up to 50 000 PIL crops "
                                          "across calls and rotates them with Pillow's affine resampler on the host")
            if t != 'random_flip' and t in self.SUPPORTED and not augment:
                # constructed directly, the class keeps the contract it had before these stages existed; build_transforms
                # and build_loaders (the reference's public surface) switch them on
                raise NotImplementedError("transform '%s' is applied on the device only when asked for: construct with "
                                          "augment=True, or go through build_transforms / build_loaders" % t)
            if t not in self.SUPPORTED:
                raise NotImplementedError("transform '%s' is not one of the reference's (%s) and is not built"
                                          % (t, ', '.join(self.SUPPORTED + ('random_patch',))))
        self.height, self.width = int(height), int(width)
        self.flip = train and 'random_flip' in transforms
        self.crop = train and 'random_crop' in transforms
        self.jitter = train and 'color_jitter' in transforms
        self.erase = train and 'random_erase' in transforms
        self.big_height, self.big_width = int(round(self.height * 1.125)), int(round(self.width * 1.125))
        if self.crop and (self.big_height <= self.height or self.big_width <= self.width):
            raise ValueError("random_crop needs a height and width of at least 5 (%dx%d enlarges to %dx%d)"
                             % (self.height, self.width, self.big_height, self.big_width))
        self.augments = self.crop or self.jitter or self.erase      # anything beyond the flip: the plan path
        self.needs_py_rng = self.crop or self.erase                 # stages that draw from python's `random`
        self.last_launches = None                                   # kernel launches of the last augmented call
        self.last_ragged_launches = None                            # kernel launches of the last ragged call
        self.mean = np.asarray(IMAGENET_MEAN if norm_mean is None or norm_std is None else norm_mean, dtype=np.float32)
        self.std = np.asarray(IMAGENET_STD if norm_mean is None or norm_std is None else norm_std, dtype=np.float32)
        self.device = device
        self._dev_tables = {}

    def _tables_on(self, dev, hs, ws):
        key = (str(dev), hs, ws)
        if key not in self._dev_tables:
            t = resample_tables(hs, ws, self.height, self.width)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._dev_tables[key] = (t, up(t["bounds_h"]), up(t["kk_h"]), up(t["bounds_v"]), up(t["kk_v"]))
        return self._dev_tables[key]

    _vector_draw_ok = None     # does torch.rand(n) consume the generator like n x torch.rand(1) on this build?  (checked once)

    def draw_flips(self, n):
        """one torch.rand(1) < 0.5 per image, in call order (torchvision's RandomHorizontalFlip inside the reference's per-image
        Compose).  Drawn as ONE torch.rand(n) when this torch build produces the same numbers that way (checked once on a
        saved generator state): 192 interpreter round trips per batch otherwise, under the lock the train step needs too."""
        if not self.flip:
            return np.zeros(n, dtype=np.uint8)
        cls = DeviceTransform
        if cls._vector_draw_ok is None:
            state = torch.get_rng_state()
            a = torch.rand(37)
            torch.set_rng_state(state)
            b = torch.cat([torch.rand(1) for _ in range(37)])
            torch.set_rng_state(state)
            cls._vector_draw_ok = bool(torch.equal(a, b))
        if cls._vector_draw_ok and n > 0:
            return (torch.rand(n) < 0.5).to(torch.uint8).numpy()
        return np.asarray([1 if float(torch.rand(1)) < 0.5 else 0 for _ in range(n)], dtype=np.uint8)

    @staticmethod
    def _draw_jitter():
        """(first, b, c) of one image: what torchvision's ColorJitter(brightness=0.2, contrast=0.15, saturation=0, hue=0)
        draws per call -- fn_idx = torch.randperm(4), b = float(torch.empty(1).uniform_(0.8, 1.2)),
        c = float(torch.empty(1).uniform_(0.85, 1.15)), nothing for saturation and hue (both collapse to None); the four
        slots are then visited in fn_idx's order, 0 = brightness, 1 = contrast, 2 and 3 nothing, so only whether 0 comes
        before 1 matters (first = 0: brightness first).
        RESTATED from torchvision >= 0.8 (transforms.ColorJitter.get_params / forward): torchvision is not among this
        project's dependencies and the order has not been run against it.  This is the one place that knows the order."""
        order = torch.randperm(4).tolist()
        b = float(torch.empty(1).uniform_(*DeviceTransform.BRIGHTNESS))
        c = float(torch.empty(1).uniform_(*DeviceTransform.CONTRAST))
        return (0 if order.index(0) < order.index(1) else 1), b, c

    def _draw_crop(self, rng):
        """Random2DTranslation(H, W, p=0.5): (flag, x1, y1), x before y, nothing drawn after a miss"""
        if rng.uniform(0, 1) > 0.5:
            return 0, 0, 0
        x1 = int(round(rng.uniform(0, self.big_width - self.width)))
        y1 = int(round(rng.uniform(0, self.big_height - self.height)))
        return 1, x1, y1

    def _draw_erase(self, rng):
        """RandomErasing(probability=0.5, sl=0.02, sh=0.4, r1=0.3): (r0, c0, h, w); h = 0: the image is left alone (a miss,
        or 100 attempts without a rectangle that fits)"""
        if rng.uniform(0, 1) > 0.5:
            return 0, 0, 0, 0
        H, W = self.height, self.width
        for _ in range(100):
            area = rng.uniform(0.02, 0.4) * (H * W)
            ratio = rng.uniform(0.3, 1 / 0.3)
            h = int(round(math.sqrt(area * ratio)))
            w = int(round(math.sqrt(area / ratio)))
            if w < W and h < H:
                r0 = rng.randint(0, H - h)
                c0 = rng.randint(0, W - w)
                return r0, c0, h, w
        return 0, 0, 0, 0

    def draw_plan(self, n, py_rng=None):
        """Every random decision of n images (AugmentPlan), consuming the two generators as the reference's per-image
        Compose does over the same n images: torch's for the flip and the jitter, python's `random` (or `py_rng`, a
        random.Random) for the crop and the erase; per image in stage order flip, crop, jitter, erase.  The two streams are
        independent, so all torch numbers are drawn first and all python numbers after.  With only 'random_flip' enabled
        this is draw_flips(n) (the vectorised draw included) and `random` is not touched."""
        plan = AugmentPlan(n)
        if self.jitter:
            for i in range(n):
                if self.flip:
                    plan.flip[i] = 1 if float(torch.rand(1)) < 0.5 else 0
                plan.jitter_first[i], plan.jitter_b[i], plan.jitter_c[i] = self._draw_jitter()
        else:
            plan.flip = self.draw_flips(n)
        if self.crop or self.erase:
            rng = _random if py_rng is None else py_rng
            for i in range(n):
                if self.crop:
                    plan.crop[i] = self._draw_crop(rng)
                if self.erase:
                    plan.erase[i] = self._draw_erase(rng)
        return plan

    def _check_plan(self, plan, n):
        """a plan the kernels can take: lengths, offsets inside the enlarged image, rectangles inside the output"""
        if len(plan) != n:
            raise ValueError("the plan holds %d images, the batch %d" % (len(plan), n))
        c, e = plan.crop, plan.erase
        if self.crop and np.any((c[:, 0] != 0) & ((c[:, 1] < 0) | (c[:, 1] > self.big_width - self.width) |
                                                  (c[:, 2] < 0) | (c[:, 2] > self.big_height - self.height))):
            raise ValueError("crop offset outside the enlarged image")
        if self.erase and np.any((e[:, 2] > 0) & ((e[:, 0] < 0) | (e[:, 1] < 0) | (e[:, 3] < 0) |
                                                  (e[:, 0] + e[:, 2] > self.height) | (e[:, 1] + e[:, 3] > self.width))):
            raise ValueError("erase rectangle outside the image")

    def _big_tables_on(self, dev):
        """the two fixed enlargement tables (H -> Hbig, W -> Wbig) of the random crop, resident on `dev`"""
        key = (str(dev), "big")
        if key not in self._dev_tables:
            bh, kh, ksh = _axis_tables(self.width, self.big_width)
            bv, kv, ksv = _axis_tables(self.height, self.big_height)
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            self._dev_tables[key] = (up(bh), up(kh), ksh, up(bv), up(kv), ksv)
        return self._dev_tables[key]

    def _plan_to(self, dev, packed):
        """the packed plan through a ring of pinned buffers, like the flip flags in __call__ (a pageable source would make the
        copy synchronous; an event per slot makes rewriting the slot safe whatever the backlog)"""
        n = packed.shape[0]
        ring = self.__dict__.setdefault("_plan_ring", {"at": 0, "bufs": [None] * 8, "done": [None] * 8})
        slot = ring["at"] = (ring["at"] + 1) % 8
        if ring["done"][slot] is not None:
            ring["done"][slot].synchronize()
        if ring["bufs"][slot] is None or ring["bufs"][slot].shape[0] < n:
            ring["bufs"][slot] = torch.empty((max(n, 256), PLAN_WORDS), dtype=torch.int32).pin_memory()
        ring["bufs"][slot][:n].copy_(torch.from_numpy(packed))
        pl = ring["bufs"][slot][:n].to(dev, non_blocking=True)
        if ring["done"][slot] is None:
            ring["done"][slot] = torch.cuda.Event()
        ring["done"][slot].record(torch.cuda.current_stream(dev))
        return pl

    def _augment(self, lib, dev, src, dst, n, hs, ws, pl):
        """one ieee_augment_normalize call: src [n][hs][ws][3] uint8 and the packed plan pl [n][PLAN_WORDS], both on `dev`"""
        t, bh, kh, bv, kv = self._tables_on(dev, hs, ws)
        tmp = torch.empty((n, t["tmp_rows"], self.width, 3), dtype=torch.uint8, device=dev) if t["need_h"] else None
        staged = self.crop or self.jitter
        image = n * self.height * self.width * 3
        work = torch.empty(((1 if staged else 0) + (2 if self.crop else 0)) * image, dtype=torch.uint8, device=dev)
        big = self._big_tables_on(dev) if self.crop else (None, None, 0, None, None, 0)
        stages = ((STAGE_FLIP if self.flip else 0) | (STAGE_CROP if self.crop else 0) | (STAGE_JITTER if self.jitter else 0) |
                  (STAGE_ERASE if self.erase else 0))
        mean = (_lib.ctypes.c_float * 3)(*self.mean.tolist())
        std = (_lib.ctypes.c_float * 3)(*self.std.tolist())
        launches = _lib.c_int(0)
        _lib.check(lib.ieee_augment_normalize(
            _lib.ptr(src), _lib.ptr(dst), _lib.ptr(tmp) if tmp is not None else None, n, hs, ws, self.height,
            self.width, _lib.ptr(bh) if t["need_h"] else None, _lib.ptr(kh) if t["need_h"] else None, t["ksize_h"],
            _lib.ptr(bv) if t["need_v"] else None, _lib.ptr(kv) if t["need_v"] else None, t["ksize_v"],
            t["ybox_first"], t["tmp_rows"], _lib.ptr(pl), stages, _lib.ptr(work) if work.numel() else None, work.numel(),
            self.big_height, self.big_width, _lib.ptr(big[0]), _lib.ptr(big[1]), big[2], _lib.ptr(big[3]), _lib.ptr(big[4]),
            big[5], mean, std, _lib.ctypes.byref(launches), _lib.stream()))
        self.last_launches = int(launches.value)

    def _call_augmented(self, lib, dev, images, out, plan):
        n = len(images)
        if torch.is_tensor(images):
            if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
                raise ValueError("expected a uint8 [N, H, W, 3] batch, got %s %s" % (images.dtype, tuple(images.shape)))
            src = images.to(dev, non_blocking=True)
            self._augment(lib, dev, src, out, n, int(images.shape[1]), int(images.shape[2]), self._plan_to(dev, plan.pack()))
            return out
        groups = {}
        for i, im in enumerate(images):
            im = np.asarray(im)
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                raise ValueError("expected uint8 HxWx3 images (PIL 'RGB'), got %s %s" % (im.dtype, im.shape))
            groups.setdefault(im.shape[:2], []).append(i)
        packed = plan.pack()
        launches = 0
        for (hs, ws), idx in groups.items():
            src = torch.from_numpy(np.stack([np.ascontiguousarray(images[i]) for i in idx])).to(dev, non_blocking=True)
            pl = torch.from_numpy(np.ascontiguousarray(packed[idx])).to(dev)
            dst = out if len(groups) == 1 else torch.empty((len(idx), 3, self.height, self.width), dtype=torch.float32, device=dev)
            self._augment(lib, dev, src, dst, len(idx), hs, ws, pl)
            launches += self.last_launches
            if dst is not out:
                out[torch.as_tensor(idx, device=dev)] = dst
        self.last_launches = launches
        return out

    def ragged(self, images, flips=None):
        """Resize -> flip -> ToTensor -> Normalize of N images of ANY mix of sizes -> float32 [N, 3, height, width] on the
        device: the bits of the one-size path, from one host-to-device copy (the packed pixels with the offset / size / flip
        tables behind them) and one ieee_resize_normalize_ragged call (one launch; Pillow's coefficients are computed on the
        device, nothing is cached per size).  flips: as in __call__ (drawn when None).  The train augmentations beyond the
        flip are not part of this path."""
        lib = _lib.require_gpu()
        dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        n = len(images)
        out = torch.empty((n, 3, self.height, self.width), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        flips = self.draw_flips(n) if flips is None else np.asarray(flips, dtype=np.uint8)
        if len(flips) != n:
            raise ValueError("%d flip decisions for %d images" % (len(flips), n))
        staging = self.__dict__.setdefault("_staging", _Staging())      # this transform's own, like its flip and plan rings
        stage, nbytes, offsets, sizes = _pack_ragged(images, staging, tail=17 * n)
        flat = stage.numpy()
        flat[nbytes:nbytes + 8 * n] = offsets.view(np.uint8)                    # offsets | sizes | flips, behind the pixels
        flat[nbytes + 8 * n:nbytes + 16 * n] = sizes.reshape(-1).view(np.uint8)
        flat[nbytes + 16 * n:nbytes + 17 * n] = flips
        src = stage[:nbytes + 17 * n].to(dev, non_blocking=True)
        if staging.done is None or staging.done_on != dev:        # (room() has waited for the event this one replaces)
            staging.done, staging.done_on = torch.cuda.Event(), dev
        staging.done.record(torch.cuda.current_stream(dev))
        base = src.data_ptr()
        mean = (_lib.ctypes.c_float * 3)(*self.mean.tolist())
        std = (_lib.ctypes.c_float * 3)(*self.std.tolist())
        launches = _lib.c_int(0)
        _lib.check(lib.ieee_resize_normalize_ragged(
            _lib.c_void_p(base), nbytes, _lib.c_void_p(base + nbytes), _lib.c_void_p(base + nbytes + 8 * n),
            _lib.c_void_p(base + nbytes + 16 * n), _lib.c_void_p(offsets.ctypes.data), _lib.c_void_p(sizes.ctypes.data),
            _lib.ptr(out), n, self.height, self.width, mean, std, _lib.ctypes.byref(launches), _lib.stream()))
        self.last_ragged_launches = int(launches.value)
        return out

    def __call__(self, images, flips=None, plan=None):
        """flips: the flip decisions (else drawn); plan: an AugmentPlan with every decision (else drawn by draw_plan).  With
        both, `flips` replaces the plan's flips.  Without augmentations beyond the flip only the flips of a plan are used."""
        lib = _lib.require_gpu()
        dev = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        n = len(images)
        out = torch.empty((n, 3, self.height, self.width), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        if self.augments:
            plan = self.draw_plan(n) if plan is None else plan[:]
            if flips is not None:
                plan.flip = np.asarray(flips, dtype=np.uint8).copy()
            self._check_plan(plan, n)
            return self._call_augmented(lib, dev, images, out, plan)
        if flips is None and plan is not None:
            flips = plan.flip
        flips = self.draw_flips(n) if flips is None else np.asarray(flips, dtype=np.uint8)
        if torch.is_tensor(images):
            # a whole batch of same-size images already stacked [N, H, W, 3] uint8 by the loader's workers (pinned when the
            # DataLoader pins): one asynchronous copy, no per-image work on this thread
            if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
                raise ValueError("expected a uint8 [N, H, W, 3] batch, got %s %s" % (images.dtype, tuple(images.shape)))
            hs, ws = int(images.shape[1]), int(images.shape[2])
            t, bh, kh, bv, kv = self._tables_on(dev, hs, ws)
            src = images.to(dev, non_blocking=True)
            # the flip flags through a small ring of pinned buffers: a pageable source would make this copy synchronous --
            # the prefetch thread would stall until its stream has drained behind the train step's kernels
            # (a slot is rewritten 8 calls later -- under three batches; the copy out of it may still be queued behind other
            # streams' work then, e.g. with one hardware queue per priority in a data-parallel job: an event per slot, recorded
            # behind the copy and waited for before the host writes the slot again, makes the reuse safe whatever the backlog)
            ring = self.__dict__.setdefault("_flip_ring", {"at": 0, "bufs": [None] * 8, "done": [None] * 8})
            slot = ring["at"] = (ring["at"] + 1) % 8
            if ring["done"][slot] is not None:
                ring["done"][slot].synchronize()
            if ring["bufs"][slot] is None or ring["bufs"][slot].numel() < n:
                ring["bufs"][slot] = torch.empty(max(n, 256), dtype=torch.uint8).pin_memory()
            ring["bufs"][slot][:n].copy_(torch.from_numpy(flips))
            fl = ring["bufs"][slot][:n].to(dev, non_blocking=True)
            if ring["done"][slot] is None:
                ring["done"][slot] = torch.cuda.Event()
            ring["done"][slot].record(torch.cuda.current_stream(dev))
            tmp = torch.empty((n, t["tmp_rows"], self.width, 3), dtype=torch.uint8, device=dev) if t["need_h"] else None
            mean = (_lib.ctypes.c_float * 3)(*self.mean.tolist())
            std = (_lib.ctypes.c_float * 3)(*self.std.tolist())
            _lib.check(lib.ieee_resize_flip_normalize(
                _lib.ptr(src), _lib.ptr(out), _lib.ptr(tmp) if tmp is not None else None, n, hs, ws, self.height,
                self.width, _lib.ptr(bh) if t["need_h"] else None, _lib.ptr(kh) if t["need_h"] else None, t["ksize_h"],
                _lib.ptr(bv) if t["need_v"] else None, _lib.ptr(kv) if t["need_v"] else None, t["ksize_v"],
                t["ybox_first"], t["tmp_rows"], _lib.ptr(fl), mean, std, _lib.stream()))
            return out
        groups = {}
        for i, im in enumerate(images):
            im = np.asarray(im)
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                raise ValueError("expected uint8 HxWx3 images (PIL 'RGB'), got %s %s" % (im.dtype, im.shape))
            groups.setdefault(im.shape[:2], []).append(i)
        if len(groups) > 1:
            # mixed sizes: one copy and one launch for the whole list, no table per size (the same bits)
            return self.ragged(images, flips)
        (hs, ws), = groups
        mean = (_lib.ctypes.c_float * 3)(*self.mean.tolist())
        std = (_lib.ctypes.c_float * 3)(*self.std.tolist())
        t, bh, kh, bv, kv = self._tables_on(dev, hs, ws)
        src = torch.from_numpy(np.stack([np.ascontiguousarray(im) for im in images])).to(dev, non_blocking=True)
        fl = torch.from_numpy(flips.copy()).to(dev)
        tmp = torch.empty((n, t["tmp_rows"], self.width, 3), dtype=torch.uint8, device=dev) if t["need_h"] else None
        _lib.check(lib.ieee_resize_flip_normalize(
            _lib.ptr(src), _lib.ptr(out), _lib.ptr(tmp) if tmp is not None else None, n, hs, ws, self.height,
            self.width, _lib.ptr(bh) if t["need_h"] else None, _lib.ptr(kh) if t["need_h"] else None, t["ksize_h"],
            _lib.ptr(bv) if t["need_v"] else None, _lib.ptr(kv) if t["need_v"] else None, t["ksize_v"],
            t["ybox_first"], t["tmp_rows"], _lib.ptr(fl), mean, std, _lib.stream()))
        return out


def build_transforms(height, width, transforms='random_flip', norm_mean=None, norm_std=None, **kwargs):
    """reference transforms.py:233-326: returns (train transform, test transform)"""
    print('Building train transforms ...')
    print('+ resize to {}x{}'.format(height, width))
    tr = DeviceTransform(height, width, transforms, norm_mean, norm_std, train=True, augment=True)
    if tr.flip:
        print('+ random flip')
    if tr.crop:
        print('+ random crop (enlarge to {}x{} and crop {}x{})'.format(tr.big_height, tr.big_width, height, width))
    if tr.jitter:
        print('+ color jitter')
    print('+ to torch tensor of range [0, 1]')
    print('+ normalization (mean={}, std={})'.format(tr.mean.tolist(), tr.std.tolist()))
    if tr.erase:
        print('+ random erase')
    print('Building test transforms ...')
    print('+ resize to {}x{}'.format(height, width))
    print('+ to torch tensor of range [0, 1]')
    print('+ normalization (mean={}, std={})'.format(tr.mean.tolist(), tr.std.tolist()))
    return tr, DeviceTransform(height, width, [], norm_mean, norm_std, train=False)
