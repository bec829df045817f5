"""CPU: what of the activation-map figures can be held without a device -- the header's declarations, the default colour
table, visactmap's argument checks (raised before the device is touched), and the evidence that the GPU test's bar for the
render kernel (bytes equal to the fp32 restatement of tests/util_actmap.py) is the right one."""
import os
import re

import numpy as np
import pytest
import torch

from tests import util_actmap as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_both_exports():
    txt = open(os.path.join(ROOT, "include", "ieee_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("ieee_actmap_energy", "ieee_actmap_render"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    from ieee_amd import _lib
    assert len(_lib._SIGNATURES["ieee_actmap_energy"]) == 7
    assert len(_lib._SIGNATURES["ieee_actmap_render"]) == 13


def test_jet_table_is_the_closed_form():
    from ieee_amd.reidtools import jet_table
    tab = jet_table()
    assert tab.dtype == np.uint8 and tab.shape == (256, 3)
    assert np.array_equal(tab, U.jet_table_restated())
    assert tuple(tab[0]) == (0, 0, 128) and tuple(tab[255]) == (128, 0, 0)
    assert tuple(tab[32]) == (0, 0, 255)             # 4 * 32 / 255 + 0.5 > 1: the blue plateau


class _NoDevice(torch.nn.Module):
    """a model that must not be reached: any forward fails the test"""

    def forward(self, *a, **k):
        raise AssertionError("visactmap ran the model before checking its arguments")


def _loader(height, width, n=2):
    imgs = [torch.zeros(n, 3, height, width) for _ in range(3)]
    paths = [["/x/%s_%d.jpg" % (m, j) for j in range(n)] for m in ("rgb", "ni", "ti")]
    return {"synthetic": {"query": [{"img": imgs, "impath": paths}]}}


def test_visactmap_rejects_an_unknown_modal(tmp_path, capsys):
    from ieee_amd.reidtools import visactmap
    with pytest.raises(RuntimeError):
        visactmap(_NoDevice(), _loader(32, 16), str(tmp_path), "t", 16, 32, True, "IR")
    assert "Unknow modal!" in capsys.readouterr().out
    assert not os.listdir(str(tmp_path))


def test_visactmap_rejects_images_of_another_size(tmp_path):
    from ieee_amd.reidtools import visactmap
    with pytest.raises(ValueError, match="height 32 x width 16"):
        visactmap(_NoDevice(), _loader(64, 32), str(tmp_path), "t", 16, 32, True, "TI")


@pytest.mark.parametrize("name", [c[0] for c in U.RENDER_CASES])
def test_fp32_and_float64_restatements_differ_by_one_index_at_most(name):
    """The fp32 pipeline (what the kernel runs) against the same formulas in float64, on the GPU test's own inputs: the
    colour index differs by at most 1.  It differs where 255 * (v - min) / ((max - min) + 1e-12) sits within fp32 rounding
    of an integer -- among them every pixel AT the maximum (float64 keeps the 1e-12 and floors to 254, fp32 absorbs it and
    gives 255), a whole plateau where the edge clamp repeats a source value.  Measured shares of differing pixels (the
    test prints them): 16x8 -> 256x128, N = 5: 2.2e-4 (36 of 163 840); 24x8 -> 384x128, N = 1: 2.0e-5 (1 of 49 152);
    5x3 -> 33x20, N = 5: 7.6e-3 (25 of 3 300); 5x3 -> 33x21, N = 5: 2.6e-3 (9 of 3 465); constant map: 0; index only,
    N = 5: 4.3e-4 (70 of 163 840).  So a comparison of the kernel against float64 would need a tolerance of one index on up
    to 8e-3 of the pixels, which could hide a wrong operation order; the kernel follows the fp32 operation order, and
    bytes equal to the fp32 restatement's is the bar of
    tests/test_actmap_gpu.py."""
    amap, img, height, width = U.render_inputs(name)
    _, i32 = U.render_f32(amap, None, None, None, None, height, width)
    _, i64 = U.render_f64(amap, None, None, None, None, height, width)
    diff = np.abs(i32.astype(np.int32) - i64.astype(np.int32))
    print("%s: %d of %d pixels differ (share %.2e), max |diff| %d" % (name, int((diff > 0).sum()), diff.size,
                                                                      float((diff > 0).mean()), int(diff.max())))
    assert diff.max() <= 1
    if "constant" in name:
        assert not i32.any() and not i64.any()
    else:
        # v = max gives fl(255 d) / fl(d + 1e-12f), within two roundings of 255: the floor is 255 or 254
        assert i32.min() == 0 and i32.max() >= 254


def test_restated_figure_layout():
    """the restatement itself: panel positions, white gaps, the overlay's double arithmetic on known bytes"""
    amap, img, height, width = U.render_inputs("5x3_to_33x20_n5")
    lut = U.jet_table_restated()
    grid, index = U.render_f32(amap, img, U.IMAGENET_MEAN, U.IMAGENET_STD, lut, height, width)
    assert grid.shape == (5, 33, 3 * 20 + 20, 3) and index.shape == (5, 33, 20)
    assert (grid[:, :, 20:30] == 255).all() and (grid[:, :, 50:60] == 255).all()
    assert np.array_equal(grid[:, :, 30:50], lut[index])
    pix, col = grid[:, :, :20].astype(np.float64), grid[:, :, 30:50].astype(np.float64)
    assert np.array_equal(grid[:, :, 60:], np.minimum(pix * 0.3 + col * 0.7, 255).astype(np.uint8))
    assert pix.min() == 0 and pix.max() == 255            # the image leaves [0, 1] on both sides before the clamp
