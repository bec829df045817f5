"""Every kernel form of ieee_amd/csrc/conv.hip at the smallest shape that selects it, called through the C ABI the way net.hip calls
it (ieee_conv2d_fwd_ex, ieee_conv2d_fwd_bn_eval, ieee_conv2d_dgrad_ex, ieee_conv2d_wgrad, _wgrad_fold, _wgrad_deferred +
ieee_wgrad_reduce_batch; G = 3 with group strides unless a case says otherwise), every output element against the float64
reference and the derived error budget of tests/util_conv.py.  Each case first asserts through ieee_conv_plan that it selects the
form it names, so a retune that moves a threshold fails here instead of silently testing something else.

The table (util_conv.cases) and what selects each form:
  conv3x3_patch_kernel   maps 8x16 / 16x8 / 32x4 (WLOG 3 / 4 / 5, one tile per image), 32x12 with N = 3 (three tiles per image, 9 row
                         tiles: no multiple of the tile group 4 nor of 8), Ci = 128 (two channel chunks: the zero halo survives the
                         reload), Co = 64 / 192; forward modes 0 / 1 / 3, dgrad (mirrored taps) modes 0 and 2 with the four mask sources
  stem_conv_kernel       border-padded 4-channel image (W = 128, H = 4 / 8, N = 1 / 3), modes 0 / 1 / 3, against the 7x7 / 2 / pad 3 conv
  stem_wgrad_kernel      H = 64 (one slab per image) / 128 (two), N = 1 / 3, immediate and deferred, through ieee_unpad_weight_grad
  conv_gather_kernel     bf16 PIPE 1: plain 1x1 loader (M = 128, 105, 600), im2col (3x3 on 10x6, 3x3 / 2, 1x1 / 2), parity-class rows
                         (3x3 / 2 dgrad on 32x16), compact stride-2 addend (VAR 2), second BatchNorm (VAR 3), Co 64 / 128 / 192;
                         fp32 fast (both tile widths, modes 0 / 3), fp32 slow and bf16 slow (Ci = 3)
  conv_wgrad(_fold)      HALF_M and full tile, in place (nsplit 1), accumulate, vec4 / taps / scalar reductions, one- and two-level fold,
                         xcd_group 2 (nkz = 15) and idle workgroups (nkz = 25 -> 32), npix % 64 != 0, fp32 fast / slow, bf16 slow
  conv3x3_wgrad_patch    WLOG 3 / 4 / 5 x HALF_M x fold, single-k-tile images (8x8, 16x4, 32x2: both halo rows in one tile, and a ragged
                         last split), multi-tile images, Ci = 128, 17 splits (two-level fold)
  128-wide tiles         plan_gather narrows every launch of <= 512 workgroups: the 128x128 gather and patch (STYLE 1) forms run in one
                         child process under IEEE_GATHER_NARROW_WG=0, and once each at a naturally wide shape (516 workgroups)
Not covered (reached by tuning switches only): PIPE 0 / 2-5 for bf16, the 256-wide tile, IEEE_WGRAD_PIPE != 1, IEEE_PATCH_STYLE,
IEEE_PATCH_BN."""
import os
import subprocess
import sys

import pytest

from tests import util_conv as uc

pytestmark = pytest.mark.gpu


def _lib():
    from ieee_amd import _lib
    return _lib, _lib.require_gpu()


@pytest.mark.parametrize("c", uc.cases(False), ids=lambda c: c.name)
def test_form(c):
    L, lib = _lib()
    try:
        fails = uc.run_case(L, lib, c)
    except Exception as e:      # a device fault is sticky: nothing more of this file may run on the card after it
        if any(s in str(e) for s in ("illegal memory access", "hipError", "HIP error", "device-side")):
            pytest.exit("device fault in %s: %s" % (c.name, e), returncode=3)
        raise
    assert not fails, "\n".join(fails)


def test_wide_forms_in_a_child_process():
    """the 128-wide gather and patch instantiations at small shapes: IEEE_GATHER_NARROW_WG is read once per process, so the cases
    of util_conv.cases(True) run in one fresh child (same runners), which also asserts BN = 128 through ieee_conv_plan"""
    env = dict(os.environ, **uc.CHILD_ENV)
    r = subprocess.run([sys.executable, os.path.join(uc.ROOT, "tests", "util_conv.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=uc.ROOT)
    assert r.returncode == 0 and "0 failed comparisons" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])
