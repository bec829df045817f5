"""CPU: the host side of the ragged-batch resize -- pack_ragged, the soundness of the reference the GPU test compares with,
and the FeatureExtractor's input handling."""
import numpy as np
import pytest

from tests import util_ragged as U


@pytest.mark.parametrize("n", [0, 1, 37])
def test_pack_ragged_round_trips(n):
    from ieee_amd.data import pack_ragged
    sizes = (U.batch37()[0] if n == 37 else U.SIZES[1:2])[:n]
    sizes = [s if s[0] * s[1] <= 200000 else (s[0] // 16 + 1, s[1] // 16 + 1) for s in sizes]     # bytes, not pixels, matter here
    images = [U.image(s) for s in sizes]
    buf, offsets, shapes = pack_ragged(images)
    assert buf.dtype == np.uint8 and buf.ndim == 1
    assert offsets.dtype == np.int64 and offsets.shape == (n,)
    assert shapes.dtype == np.int32 and shapes.shape == (n, 2)
    assert shapes.tolist() == [list(s) for s in sizes]
    end = 0
    for im, off in zip(images, offsets.tolist()):
        assert off >= end and off % 16 == 0                       # in order, no overlap
        end = off + im.size
        assert np.array_equal(buf[off:end].reshape(im.shape), im)
    assert buf.size >= end
    if n == 37:
        assert len(set(sizes)) < n                                # repeated sizes


def test_pack_ragged_takes_strided_arrays_and_pil_images():
    from PIL import Image
    from ieee_amd.data import pack_ragged
    base = U.image((97, 33))
    images = [base[::-1, ::2], np.asfortranarray(base), Image.fromarray(base, "RGB"), base.transpose(1, 0, 2)]
    assert not images[0].flags.c_contiguous and not images[3].flags.c_contiguous
    buf, offsets, shapes = pack_ragged(images)
    assert shapes.tolist() == [[97, 17], [97, 33], [97, 33], [33, 97]]
    for im, off in zip(images, offsets.tolist()):
        im = np.asarray(im)
        assert np.array_equal(buf[off:off + im.size].reshape(im.shape), im)


def test_pack_ragged_reuses_one_staging_buffer():
    from ieee_amd.data import pack_ragged
    a, _, _ = pack_ragged([U.image((97, 33))])
    b, _, _ = pack_ragged([U.image((31, 96))])
    assert a.ctypes.data == b.ctypes.data


@pytest.mark.parametrize("bad", [np.zeros((4, 4, 3), dtype=np.float32), np.zeros((4, 4), dtype=np.uint8),
                                 np.zeros((4, 4, 4), dtype=np.uint8), np.zeros((2, 4, 4, 3), dtype=np.uint8)])
def test_pack_ragged_rejects_what_is_not_uint8_rgb(bad):
    from ieee_amd.data import pack_ragged
    with pytest.raises(ValueError, match="expected uint8 HxWx3 images"):
        pack_ragged([U.image((1, 1)), bad])


@pytest.mark.parametrize("target", U.TARGETS)
def test_the_reference_of_the_gpu_test_equals_pillow(target):
    """for every source size the GPU test uses, the horizontal-first restatement IS Image.resize(BILINEAR)"""
    from PIL import Image
    from oracle import transforms as ot
    for size in U.SIZES:
        im = U.image(size)
        pil = np.asarray(Image.fromarray(im, "RGB").resize((target[1], target[0]), Image.BILINEAR))
        assert np.array_equal(ot.pil_bilinear_resize_u8(im, target[0], target[1]), pil), (size, target)


def _extractor():
    import torch
    from ieee_amd import FeatureExtractor
    return FeatureExtractor(model=torch.nn.Identity(), device="cpu", verbose=False)


def test_feature_extractor_wants_equal_counts():
    fe = _extractor()
    one = U.image((97, 33))
    with pytest.raises(ValueError, match="same number of images"):
        fe([[one, one], [one], [one, one]])
    with pytest.raises(ValueError):
        fe([[one], [one]])


def test_feature_extractor_rejects_other_element_types():
    fe = _extractor()
    one = U.image((97, 33))
    for bad in ([[one], [3], [one]], [[one], [one], 3.5], [[one], [(1, 2)], [one]]):
        with pytest.raises(TypeError, match=r"Type of each element must belong to \[str \| numpy.ndarray\]"):
            fe(bad)


def test_import_keeps_torch_out():
    """`import ieee_amd` must stay free of torch (the package picks the hardware-queue count before the runtime starts);
    FeatureExtractor is resolved on first use"""
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import ieee_amd; assert 'torch' not in sys.modules; "
            "from ieee_amd import FeatureExtractor; assert FeatureExtractor.__name__ == 'FeatureExtractor'; print('ok')" % root)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
