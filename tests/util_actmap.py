"""numpy restatements of the activation-map arithmetic that include/ieee_amd.h fixes (ieee_actmap_energy,
ieee_actmap_render; reference tools/visualize_actmap.py:84-88, 119-146), and the fixed-seed inputs the CPU and GPU tests
share.  `render_f32` follows the kernel operation for operation in float32 (numpy never fuses a product with a sum), so the
kernel's bytes must equal its bytes; `render_f64` is the same formulas in float64, the yardstick of how far the fp32
pipeline may sit from exact arithmetic (one colour index at a few pixels).  The energy has one restatement, float64: its
fp32 sum order is the kernel's own business and the test's tolerance is the bound of ANY order."""
import math
import zlib

import numpy as np

F = np.float32
GAP = 10
IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]


def jet_table_restated():
    """closed-form jet, written out entry by entry with python floats (float64)"""
    tab = np.zeros((256, 3), dtype=np.uint8)
    for i in range(256):
        v = i / 255.0
        for c, (lo, hi) in enumerate(((-1.5, 4.5), (-0.5, 3.5), (0.5, 2.5))):
            x = min(4.0 * v + lo, -4.0 * v + hi)
            x = 0.0 if x < 0.0 else (1.0 if x > 1.0 else x)
            tab[i, c] = int(math.floor(255.0 * x + 0.5))
    return tab


def energy_f64(x):
    """x [N, P, C] (the dtype-rounded values, any float type) -> float64 [N, P]: E / max(||E||_2, 1e-12)"""
    e = (np.asarray(x, dtype=np.float64) ** 2).sum(-1)
    nrm = np.sqrt((e * e).sum(-1, keepdims=True))
    return e / np.maximum(nrm, 1e-12)


def _coords(n_dst, n_src, T):
    """OpenCV INTER_LINEAR sampling positions in type T: source index, its successor, the successor's weight"""
    ratio = T(n_src) / T(n_dst)
    d = np.arange(n_dst).astype(T)
    s = (d + T(0.5)) * ratio - T(0.5)
    fl = np.floor(s)
    i0 = fl.astype(np.int64)
    f = (s - fl).astype(T)
    lo = i0 < 0
    i0[lo], f[lo] = 0, 0
    hi = i0 >= n_src - 1
    i0[hi], f[hi] = n_src - 1, 0
    return i0, np.minimum(i0 + 1, n_src - 1), f


def resize(m, height, width, T):
    """m [h, w] -> [height, width] in type T: horizontally first, then vertically, each step a + (b - a) * f"""
    m = np.asarray(m).astype(T)
    h, w = m.shape
    y0, y1, fy = _coords(height, h, T)
    x0, x1, fx = _coords(width, w, T)
    a0, b0 = m[y0][:, x0], m[y0][:, x1]
    a1, b1 = m[y1][:, x0], m[y1][:, x1]
    r0 = a0 + (b0 - a0) * fx[None, :]
    r1 = a1 + (b1 - a1) * fx[None, :]
    out = r0 + (r1 - r0) * fy[:, None]
    assert out.dtype == T
    return out


def index_map(m, height, width, T):
    v = resize(m, height, width, T)
    mn, mx = v.min(), v.max()
    den = (mx - mn) + T(F(1e-12))        # the constant is the float 1e-12f in both
    q = np.floor(T(255) * (v - mn) / den)
    assert q.dtype == T
    return np.clip(q, 0, 255).astype(np.uint8)


def render(amap, img, mean, std, lut, height, width, T=F):
    """-> (grid uint8 [N, height, 3 * width + 20, 3] RGB or None, index uint8 [N, height, width])"""
    N = amap.shape[0]
    index = np.stack([index_map(amap[n], height, width, T) for n in range(N)])
    if img is None:
        return None, index
    grid = np.full((N, height, 3 * width + 2 * GAP, 3), 255, dtype=np.uint8)
    x = np.asarray(img).astype(T)
    s = np.asarray(std, dtype=F).astype(T).reshape(1, 3, 1, 1)      # the kernel receives three floats
    m = np.asarray(mean, dtype=F).astype(T).reshape(1, 3, 1, 1)
    u = np.clip(x * s + m, T(0), T(1))
    pix = np.floor(u * T(255)).astype(np.uint8).transpose(0, 2, 3, 1)          # [N, height, width, 3]
    col = np.asarray(lut, dtype=np.uint8).reshape(256, 3)[index]               # [N, height, width, 3]
    ov = np.minimum(pix.astype(np.float64) * 0.3 + col.astype(np.float64) * 0.7, 255.0).astype(np.uint8)
    grid[:, :, :width] = pix
    grid[:, :, width + GAP:2 * width + GAP] = col
    grid[:, :, 2 * width + 2 * GAP:] = ov
    return grid, index


def render_f32(amap, img, mean, std, lut, height, width):
    return render(amap, img, mean, std, lut, height, width, F)


def render_f64(amap, img, mean, std, lut, height, width):
    return render(amap, img, mean, std, lut, height, width, np.float64)


# ---- fixed-seed inputs ------------------------------------------------------------------------------------------------
# (name, N, h, w, height, width, constant map?, with image?)
RENDER_CASES = [
    ("16x8_to_256x128_n5", 5, 16, 8, 256, 128, False, True),
    ("24x8_to_384x128_n1", 1, 24, 8, 384, 128, False, True),
    ("5x3_to_33x20_n5", 5, 5, 3, 33, 20, False, True),          # non-integer ratio
    ("5x3_to_33x21_n5", 5, 5, 3, 33, 21, False, True),          # 249-byte rows: figures start at every alignment
    ("constant_n1", 1, 16, 8, 256, 128, True, True),
    ("index_only_n5", 5, 16, 8, 256, 128, False, False),
]


def render_inputs(name):
    """-> (amap fp32 [N, h, w], img fp32 [N, 3, height, width] or None, height, width): an L2-normalised energy-like map (as
    ieee_actmap_energy writes), an image whose de-normalised values leave [0, 1] on both sides"""
    case = [c for c in RENDER_CASES if c[0] == name][0]
    _, N, h, w, height, width, constant, with_img = case
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0xFFFF)      # the case's own seed, whatever the list's order
    if constant:
        amap = np.full((N, h, w), 0.25, dtype=F)
    else:
        e = rng.rand(N, h * w).astype(np.float64) ** 2 + 1e-3
        amap = (e / np.sqrt((e * e).sum(-1, keepdims=True))).reshape(N, h, w).astype(F)
    img = (rng.randn(N, 3, height, width) * 1.3).astype(F) if with_img else None
    return amap, img, height, width


ENERGY_SHAPES = [(3, 128, 2048), (1, 1, 8), (2, 30, 72), (5, 192, 2048)]


def energy_inputs(shape, seed=0):
    """ReLU-like activations (the trunk output is behind a ReLU): half zeros, the rest |N(0, 1)| * 2"""
    rng = np.random.RandomState(2000 + seed + shape[1])
    x = rng.randn(*shape) * 2.0
    return np.maximum(x, 0.0).astype(F)
