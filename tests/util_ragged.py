"""Shared by the ragged-resize tests: the source sizes, seeded images, and the CPU reference, computed once per target."""
import numpy as np

# every size here resizes identically under oracle.transforms.pil_bilinear_resize_u8 and PIL.Image.resize(BILINEAR), for the
# 256 x 128 and the 64 x 48 target (test_ragged_resize_cpu checks exactly this list): equal, up- and down-scaled axes, one
# pixel, the 4096 limit on either side (65 horizontal taps at 128 columns, 33 vertical taps at 256 rows)
SIZES = [(1, 1), (2, 300), (256, 128), (256, 100), (200, 128), (97, 33), (400, 40), (31, 96), (1025, 517),
         (4096, 128), (4096, 64), (4096, 1), (3, 4096), (40, 4096), (300, 3), (520, 40), (800, 300), (2000, 60)]
# strongly upscaled in width while downscaled in height: Pillow orders its passes differently there and the horizontal-first
# restatement (the existing kernel's behaviour) is one grey level off; the ragged kernel must equal the EXISTING kernel
DEVIATING = [(600, 5), (4096, 33)]
TARGETS = [(256, 128), (64, 48)]
MEAN, STD = [0.5, 0.4, 0.3], [0.2, 0.25, 0.3]

_IMAGES = {}
_WANT = {}


def image(size):
    """the seeded uint8 image of one source size (the same array for every caller; do not write to it)"""
    if size not in _IMAGES:
        rng = np.random.RandomState(size[0] * 4099 + size[1])
        im = rng.randint(0, 256, size=(size[0], size[1], 3)).astype(np.uint8)
        im.setflags(write=False)
        _IMAGES[size] = im
    return _IMAGES[size]


def want(size, target, flip):
    """to_tensor_normalize(pil_bilinear_resize_u8(image)) with MEAN / STD"""
    from oracle import transforms as ot
    key = (size, target, bool(flip))
    if key not in _WANT:
        if (size, target) not in _WANT:
            _WANT[(size, target)] = ot.pil_bilinear_resize_u8(image(size), target[0], target[1])
        _WANT[key] = ot.to_tensor_normalize(_WANT[(size, target)], MEAN, STD, bool(flip))
    return _WANT[key]


def batch37():
    """N = 37 over the 18 sizes: two shuffled passes and one more image, alternating flips"""
    order = np.random.RandomState(37).permutation(len(SIZES)).tolist()
    order = order + order[::-1] + [order[3]]
    sizes = [SIZES[i] for i in order]
    assert len(sizes) == 37 and len(set(sizes)) == 18
    return sizes, [i % 2 for i in range(37)]
