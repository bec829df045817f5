"""TEST INFRASTRUCTURE ONLY: numpy restatement of the reference's train transform chain
    Resize -> [flip] -> [random crop] -> [colour jitter] -> ToTensor -> Normalize -> [random erase]
(torchreid/data/transforms.py) applied from an ieee_amd.data.AugmentPlan, i.e. with every random decision given.  The
resize and the tensor conversion are the oracle's (oracle/transforms.py); the jitter restates Pillow's ImageEnhance
(Image.blend in C float against black / a constant grey); tests/golden/augment_golden.npz, made from the reference's own
classes and from Pillow, pins all of it (tests/test_augment_cpu.py)."""
import hashlib

import numpy as np

from oracle.transforms import pil_bilinear_resize_u8, to_tensor_normalize


def digest(obj):
    """a short stable digest of a generator state (random.getstate() / torch.get_rng_state())"""
    if hasattr(obj, "numpy"):
        data = obj.numpy().tobytes()
    else:
        data = repr(obj).encode()
    return hashlib.sha256(data).hexdigest()[:32]


def big_size(height, width):
    return int(round(height * 1.125)), int(round(width * 1.125))


def crop_u8(img, flag, x1, y1):
    """Random2DTranslation with its draws given: enlarge H x W to round(1.125 H) x round(1.125 W), keep the window at (x1, y1)"""
    if not flag:
        return img
    h, w, _ = img.shape
    hb, wb = big_size(h, w)
    return pil_bilinear_resize_u8(img, hb, wb)[y1:y1 + h, x1:x1 + w]


def blend_u8(deg, img, factor):
    """Pillow's ImagingBlend(deg, img, factor) on uint8 arrays: float32 arithmetic, truncation, clipping outside [0, 1]"""
    f = np.float32(factor)
    d = deg.astype(np.int32)
    t = d.astype(np.float32) + f * (img.astype(np.int32) - d).astype(np.float32)
    assert t.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def brightness_u8(img, b):
    return blend_u8(np.zeros_like(img), img, b)


def contrast_u8(img, c):
    x = img.astype(np.int64)
    lum = (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16
    grey = int(float(int(lum.sum())) / lum.size + 0.5)
    return blend_u8(np.full_like(img, grey), img, c)


def jitter_u8(img, first, b, c):
    """ColorJitter(brightness, contrast) with its draws given: first = 0 brightness then contrast, 1 the other way"""
    if first == 0:
        return contrast_u8(brightness_u8(img, b), c)
    return brightness_u8(contrast_u8(img, c), b)


def erase_f32(t, mean, r0, c0, h, w):
    """RandomErasing with its draws given, on the normalised CHW float32 tensor (h = 0: nothing)"""
    if h > 0:
        t = t.copy()
        for ch in range(3):
            t[ch, r0:r0 + h, c0:c0 + w] = np.float32(mean[ch])
    return t


def apply_plan(images, plan, height, width, mean, std, crop=True, jitter=True, erase=True):
    """the whole chain for a list of uint8 HxWx3 images -> float32 [N][3][height][width]; a stage that is off ignores its
    plan columns (the flip column is zero when the flip is off)"""
    out = np.empty((len(images), 3, height, width), dtype=np.float32)
    for i, im in enumerate(images):
        u = pil_bilinear_resize_u8(np.asarray(im), height, width)
        if plan.flip[i]:
            u = np.ascontiguousarray(u[:, ::-1])
        if crop:
            u = crop_u8(u, *[int(v) for v in plan.crop[i]])
        if jitter:
            u = jitter_u8(u, int(plan.jitter_first[i]), plan.jitter_b[i], plan.jitter_c[i])
        t = to_tensor_normalize(u, mean, std, False)
        if erase:
            t = erase_f32(t, mean, *[int(v) for v in plan.erase[i]])
        out[i] = t
    return out
