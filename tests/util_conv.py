"""The convolution forms of ieee_amd/csrc/conv.hip one at a time: a float64 reference (torch.nn.functional.conv2d on the CPU and
its autograd, on operands already rounded to the stored type), an error budget derived from the reference's own magnitudes,
the table of cases tests/test_conv_forms_gpu.py runs (each names the kernel form it must select under ieee_conv_plan), the
layer grid of the closure test in tests/test_conv_forms_cpu.py, and the runners both the GPU test and its child process share.

Error budget (every bound is computed from the reference, never from a device output):
  accumulation   delta = n * u * A, A = the same convolution / gradient on |x|, |w|, |dy| (sum of |terms|).
                 fp32 kernels: u = 2^-24 (the fp32 MFMA is a k-ordered fmaf chain); bf16 kernels: products are exact, u = 2^-23 per
                 link (how one bf16 MFMA rounds its internal sum is not documented: one ulp, not a half).
                 forward / dgrad: n = R * S * C_in links.  Weight gradient: n = kchunk + nsplit + 2 (the chain inside a split, the
                 slab additions, conversions), kchunk and nsplit from ieee_conv_plan, and never more than the npix terms there are.
  stored output  bf16: delta + 2^-8 (|ref| + delta); fp32: delta + u |ref|.
  addend         the staged epilogue rounds the accumulator to the stored type, adds the addend in fp32 and rounds again: with
                 e1 = the stored-output bound of the conv alone, |err| <= e1 + hu (|ref + a| + e1) + 2^-24 (|ref| + |a|).
  MODE 1 sums    sum y, sum y^2 over the tensor THE KERNEL STORED, per 128-row tile: n = 128 rows + row tiles links of 2^-24.
                 Totals form: the integer image round(partial * 2^24) per tile, summed: half a unit per tile on top.
  MODE 2         g = (dgrad + addend) * mask, stored (mask tensor / bits) or only summed (mask from statistics, none); sum g and
                 sum g*y over the stored tensor as above.  Mask from statistics: an element whose float64 pre-activation
                 y*scale + shift lies within util_bn.KINK of zero may take either sign: its |g| and |g*y| are added to the bound of
                 the sums, and no more than util_bn.KINK_CAP of a case's elements may be such.
  MODE 3         out = relu(acc * scale + shift + residual): e1 * |scale| + 3 * 2^-24 (|y scale| + |shift| + |res|) for the fp32 affine
                 step, then the store rounding hu (|out| + that).
"""
import atexit
import ctypes
import functools
import json
import os
import re
import sys
import types
import zlib

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:      # (run as a script by the child processes)
    sys.path.insert(0, ROOT)
from tests import util_bn as ub  # noqa: E402

F64 = torch.float64
U32 = 2.0 ** -24
DEV = "cuda"
RATIOS = {}      # family -> largest err / bound seen (IEEE_CONV_RATIOS_FILE: written at exit, for the LABNOTES entry)
SENT = 123.0
PADE = 64        # elements between the groups' tensors (group strides = numel + PADE; 16-byte aligned for both types)


# ---- the plan query
def _header_defines():
    txt = open(os.path.join(ROOT, "include", "ieee_amd.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(IEEE_(?:PLAN|CONV_OP)_\w+)\s+(\d+)", txt)}


H = _header_defines()
FIELD = {k[len("IEEE_PLAN_"):]: v for k, v in H.items() if k.startswith("IEEE_PLAN_") and not k.startswith("IEEE_PLAN_F_")
         and k != "IEEE_PLAN_NFIELDS"}
OPS = dict(fwd=H["IEEE_CONV_OP_FWD"], eval=H["IEEE_CONV_OP_FWD_BN_EVAL"], dgrad=H["IEEE_CONV_OP_DGRAD"], wgrad=H["IEEE_CONV_OP_WGRAD"])
FL = dict(sums=H["IEEE_PLAN_F_BN_SUMS"], s2=H["IEEE_PLAN_F_ADDEND_S2"], bn2=H["IEEE_PLAN_F_BN2"], tickets=H["IEEE_PLAN_F_TICKETS"],
          deferred=H["IEEE_PLAN_F_DEFERRED"], accumulate=H["IEEE_PLAN_F_ACCUMULATE"], addend=H["IEEE_PLAN_F_ADDEND"])
GATHER, PATCH, STEM = 0, 1, 2
RED_NONE, RED_VEC4, RED_TAPS, RED_SCALAR = 0, 1, 2, 3
LD_PLAIN, LD_IM2COL, LD_PERM = 0, 1, 2


def plan(lib, op, dtype, G, N, Hi, Wi, Ci, Co, R, stride, pad, flags=0):
    """ieee_conv_plan as a dict NAME -> value; None where the call itself would refuse the combination"""
    n = H["IEEE_PLAN_NFIELDS"]
    buf = (ctypes.c_int64 * n)()
    dt = 1 if dtype in ("bf16", torch.bfloat16) else 0
    rc = lib.ieee_conv_plan(OPS[op], dt, G, N, Hi, Wi, Ci, Co, R, R, stride, pad, flags, buf, n)
    if rc != 0:
        return None
    return {k: int(buf[i]) for k, i in FIELD.items()}


def form_key(op, dtype, p):
    """what distinguishes one instantiation / branch combination from another"""
    if op == "wgrad":
        # (LEAN is read by the LDS-DMA kernels only: PIPE > 0)
        return ("wgrad", dtype, p["FAMILY"], p["SLOW"], p["WLOG"], p["LOADER"], p["LEAN"] if p["PIPE"] > 0 else 0, p["HALF_M"], p["FOLD"],
                (2 if p["N1"] > 1 else 1) if p["FOLD"] else 0, p["XCD_GROUP"], p["DIRECT"], p["REDUCE"])
    return ("gather", dtype, p["FAMILY"], p["SLOW"], p["BN"], p["MODE"], p["VAR"], p["WLOG"], p["STYLE"], p["LOADER"])


# ---- cases
def C(name, op, dtype, G, N, Hh, W, Ci, Co, R, stride, pad, want, **opt):
    c = types.SimpleNamespace(name=name, op=op, dtype=dtype, G=G, N=N, H=Hh, W=W, Ci=Ci, Co=Co, R=R, stride=stride, pad=pad,
                              want=want, sums=False, totals=0, mask="none", addend=False, s2=False, bn2=False, relu=1,
                              wmode="plain", accumulate=0, stem=False, child=False, key=None)
    c.__dict__.update(opt)
    c.Ho, c.Wo = (Hh + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    return c


def plan_dims(c):
    """the dimensions the C ABI sees (the stem: the border-padded 4-channel image under an 8x8 filter without padding)"""
    if c.stem:
        return (c.G, c.N, c.H + 6, c.W + 6, 4, c.Co, 8, 2, 0)
    return (c.G, c.N, c.H, c.W, c.Ci, c.Co, c.R, c.stride, c.pad)


def plan_flags(c):
    f = 0
    if c.sums:
        f |= FL["sums"]
    if c.s2:
        f |= FL["s2"]
    if c.bn2:
        f |= FL["bn2"]
    if c.addend:
        f |= FL["addend"]
    if c.wmode == "fold":
        f |= FL["tickets"]
    if c.wmode == "deferred":
        f |= FL["deferred"]
    if c.accumulate:
        f |= FL["accumulate"]
    return f


def case_plan(lib, c):
    return plan(lib, c.op, c.dtype, *plan_dims(c), flags=plan_flags(c))


def check_plan(lib, c):
    """[] or what of the form the case names the plan does not select"""
    p = case_plan(lib, c)
    if p is None:
        return ["%s: ieee_conv_plan refuses the shape" % c.name]
    bad = ["%s=%d (want %s)" % (k, p[k], v) for k, v in c.want.items()
           if (p[k] not in v if isinstance(v, (tuple, list, set)) else p[k] != v)]
    if c.key is not None and form_key(c.op, c.dtype, p) != tuple(c.key):
        bad.append("form key %s (want %s)" % (form_key(c.op, c.dtype, p), tuple(c.key)))
    return ["%s: %s" % (c.name, ", ".join(bad))] if bad else []


def _patch_cases(child):
    """conv3x3_patch_kernel: WLOG 3 / 4 / 5 one tile per image, 32x12 three tiles per image with N = 3 (9 row tiles), Ci = 128 (two
    channel chunks), Co = 64 / 192, forward modes 0 / 1 / 3, dgrad modes 0 and 2 with the four mask sources.  child: the same
    shapes where Co > 64 under IEEE_GATHER_NARROW_WG=0 (BN = 128, STYLE 1)."""
    out = []
    bn_of = (lambda co: 64) if not child else (lambda co: 128)
    for (W, Hh, N, wl) in ((8, 16, 2, 3), (16, 8, 2, 4), (32, 4, 2, 5), (32, 12, 3, 5)):
        for Ci, Co in ((64, 64), (128, 192)):
            if child and Co == 64:
                continue
            bn = bn_of(Co)
            want = dict(FAMILY=PATCH, WLOG=wl, BN=bn, STYLE=0 if bn == 64 else 1)
            tag = "patch%s-w%dh%d-ci%d-co%d" % ("128" if child else "", W, Hh, Ci, Co)
            out.append(C(tag + "-fwd0", "fwd", "bf16", 3, N, Hh, W, Ci, Co, 3, 1, 1, dict(want, MODE=0), child=child))
            out.append(C(tag + "-fwd1", "fwd", "bf16", 3, N, Hh, W, Ci, Co, 3, 1, 1, dict(want, MODE=1), sums=True, child=child))
            out.append(C(tag + "-eval", "eval", "bf16", 3, N, Hh, W, Ci, Co, 3, 1, 1, dict(want, MODE=3), addend=(W == 32),
                         child=child))
            # dgrad: the GEMM's N is Ci, its K runs over Co
            dbn = 64 if (Ci == 64 or not child) else 128
            dwant = dict(FAMILY=PATCH, WLOG=wl, BN=dbn, STYLE=0 if dbn == 64 else 1)
            out.append(C(tag + "-dgrad0", "dgrad", "bf16", 3, N, Hh, W, Ci, Co, 3, 1, 1, dict(dwant, MODE=0), addend=(W == 16),
                         child=child))
            for i, mk in enumerate(("mask", "bits", "stats", "none")):
                if (Hh != 12 and W != 8) and mk in ("bits", "none"):
                    continue       # all four sources at the 8-wide and the three-tile map; two elsewhere
                for add in (False, True):
                    out.append(C("%s-dgrad2-%s-add%d" % (tag, mk, add), "dgrad", "bf16", 3, N, Hh, W, Ci, Co, 3, 1, 1,
                                 dict(dwant, MODE=2), sums=True, mask=mk, addend=add, child=child))
    if not child:
        out.append(C("patch-w8h16-fwd1-totals1", "fwd", "bf16", 3, 5, 16, 8, 64, 64, 3, 1, 1, dict(FAMILY=PATCH, MODE=1), sums=True,
                     totals=1))
        out.append(C("patch-w8h16-fwd1-totals4", "fwd", "bf16", 3, 5, 16, 8, 64, 64, 3, 1, 1, dict(FAMILY=PATCH, MODE=1), sums=True,
                     totals=4))
        out.append(C("patch-w8h16-dgrad2-totals4", "dgrad", "bf16", 3, 5, 16, 8, 64, 64, 3, 1, 1, dict(FAMILY=PATCH, MODE=2),
                     sums=True, totals=4, mask="stats"))
    return out


def _stem_cases():
    out = []
    for Hh in (4, 8):
        for N in (1, 3):
            base = dict(FAMILY=STEM, BN=64)
            tag = "stem-h%d-n%d" % (Hh, N)
            out.append(C(tag + "-fwd0", "fwd", "bf16", 3, N, Hh, 128, 3, 64, 7, 2, 3, dict(base, MODE=0), stem=True))
            out.append(C(tag + "-fwd1", "fwd", "bf16", 3, N, Hh, 128, 3, 64, 7, 2, 3, dict(base, MODE=1), stem=True, sums=True))
            out.append(C(tag + "-eval", "eval", "bf16", 3, N, Hh, 128, 3, 64, 7, 2, 3, dict(base, MODE=3), stem=True))
    for Hh, N in ((64, 1), (64, 3), (128, 1), (128, 3)):
        for wm in ("plain", "deferred"):
            out.append(C("stem-wgrad-h%d-n%d-%s" % (Hh, N, wm), "wgrad", "bf16", 3, N, Hh, 128, 3, 64, 7, 2, 3,
                         dict(FAMILY=STEM, NSPLIT=N * (Hh // 64), REDUCE=RED_SCALAR), stem=True, wmode=wm))
    return out


def _gather_cases(child):
    out = []
    bn = (lambda n: 64) if not child else (lambda n: 64 if n <= 64 else 128)
    g = dict(FAMILY=GATHER, PIPE=1, SLOW=0)
    # plain 1x1 loader: M = 128 (one full tile), M = 105 = 3 x 5 x 7 (one partial tile), M = 600; Co 64 / 128 / 192
    for (N, Hh, W) in ((1, 16, 8), (3, 5, 7), (5, 12, 10)):
        for Ci, Co in ((64, 64), (128, 128), (64, 192)):
            if child and Co == 64 and Ci == 64:
                continue
            tag = "g1x1%s-m%d-ci%d-co%d" % ("-wide" if child else "", N * Hh * W, Ci, Co)
            w = dict(g, LOADER=LD_PLAIN, BN=bn(Co))
            wd = dict(g, LOADER=LD_PLAIN, BN=bn(Ci))
            out.append(C(tag + "-fwd0", "fwd", "bf16", 3, N, Hh, W, Ci, Co, 1, 1, 0, dict(w, MODE=0), child=child))
            out.append(C(tag + "-fwd1", "fwd", "bf16", 3, N, Hh, W, Ci, Co, 1, 1, 0, dict(w, MODE=1), sums=True, child=child))
            out.append(C(tag + "-eval", "eval", "bf16", 3, N, Hh, W, Ci, Co, 1, 1, 0, dict(w, MODE=3), addend=True, relu=Co != 128,
                         child=child))
            out.append(C(tag + "-dgrad0", "dgrad", "bf16", 3, N, Hh, W, Ci, Co, 1, 1, 0, dict(wd, MODE=0, VAR=0), addend=True,
                         child=child))
            for mk in ("mask", "bits", "stats", "none"):
                out.append(C("%s-dgrad2-%s" % (tag, mk), "dgrad", "bf16", 3, N, Hh, W, Ci, Co, 1, 1, 0, dict(wd, MODE=2, VAR=0),
                             sums=True, mask=mk, addend=mk in ("mask", "stats"), child=child))
            out.append(C(tag + "-dgrad2-bn2", "dgrad", "bf16", 3, N, Hh, W, Ci, Co, 1, 1, 0, dict(wd, MODE=2, VAR=3), sums=True,
                         mask="bits", addend=True, bn2=True, child=child))
    # compact stride-2 addend (power-of-two map)
    for Ci, Co in ((64, 64), (256, 64)):
        if child and Ci == 64:
            continue
        out.append(C("g1x1%s-s2addend-ci%d" % ("-wide" if child else "", Ci), "dgrad", "bf16", 3, 3, 16, 8, Ci, Co, 1, 1, 0,
                     dict(g, LOADER=LD_PLAIN, MODE=2, VAR=2, BN=bn(Ci)), sums=True, mask="bits", addend=True, s2=True, child=child))
    # the same addend under the im2col loader (a 3x3 with a compact addend is kept off the patch form)
    for Ci in (64, 128):
        if child != (Ci == 128):
            continue
        out.append(C("gim%s-s2addend-ci%d" % ("-wide" if child else "", Ci), "dgrad", "bf16", 3, 3, 16, 8, Ci, 64, 3, 1, 1,
                     dict(g, LOADER=LD_IM2COL, MODE=2, VAR=2, BN=bn(Ci)), sums=True, mask="stats", addend=True, s2=True, child=child))
    # im2col loader: 3x3 on a 10x6 map, 3x3 stride 2, 1x1 stride 2
    for (name, Hh, W, R, st, pad) in (("3x3-10x6", 10, 6, 3, 1, 1), ("3x3s2-10x6", 10, 6, 3, 2, 1), ("1x1s2-10x6", 10, 6, 1, 2, 0)):
        for Ci, Co in ((64, 128), (128, 64), (128, 128)):
            if child != (Ci == 128 and Co == 128):
                continue
            tag = "gim%s-%s-ci%d-co%d" % ("-wide" if child else "", name, Ci, Co)
            w = dict(g, LOADER=LD_IM2COL, BN=bn(Co))
            wd = dict(g, LOADER=LD_IM2COL, BN=bn(Ci), VAR=0)
            out.append(C(tag + "-fwd1", "fwd", "bf16", 3, 3, Hh, W, Ci, Co, R, st, pad, dict(w, MODE=1), sums=True, child=child))
            out.append(C(tag + "-eval", "eval", "bf16", 3, 3, Hh, W, Ci, Co, R, st, pad, dict(w, MODE=3), child=child))
            out.append(C(tag + "-dgrad0", "dgrad", "bf16", 3, 3, Hh, W, Ci, Co, R, st, pad, dict(wd, MODE=0), child=child))
            out.append(C(tag + "-dgrad2", "dgrad", "bf16", 3, 3, Hh, W, Ci, Co, R, st, pad, dict(wd, MODE=2), sums=True,
                         mask="stats", addend=True, child=child))
    # permuted stride-2 3x3 dgrad: 32x16 input ((H/2 * W/2) % 128 == 0)
    for Ci, Co in ((64, 64), (128, 128)):
        if child and Ci == 64:
            continue
        tag = "gperm%s-ci%d" % ("-wide" if child else "", Ci)
        w = dict(g, LOADER=LD_PERM, VAR=1, BN=bn(Ci))
        out.append(C(tag + "-dgrad0", "dgrad", "bf16", 3, 2, 32, 16, Ci, Co, 3, 2, 1, dict(w, MODE=0), addend=True, child=child))
        out.append(C(tag + "-dgrad2", "dgrad", "bf16", 3, 2, 32, 16, Ci, Co, 3, 2, 1, dict(w, MODE=2), sums=True, mask="mask",
                     child=child))
        out.append(C(tag + "-dgrad2-stats", "dgrad", "bf16", 3, 2, 32, 16, Ci, Co, 3, 2, 1, dict(w, MODE=2), sums=True, mask="stats",
                     addend=True, child=child))
    if child:
        return out
    # other types: fp32 fast (both tile widths, modes 0 and 3), fp32 slow (Ci = 3, 7x7), bf16 slow
    f = dict(FAMILY=GATHER, PIPE=0)
    for Co, b in ((64, 64), (192, 128)):
        out.append(C("gf32-co%d-fwd0" % Co, "fwd", "f32", 3, 3, 10, 6, 32, Co, 3, 1, 1, dict(f, SLOW=0, BN=b, MODE=0)))
        out.append(C("gf32-co%d-eval" % Co, "eval", "f32", 3, 3, 10, 6, 32, Co, 3, 1, 1, dict(f, SLOW=0, BN=b, MODE=3), addend=True))
        out.append(C("gf32-co%d-1x1-fwd0" % Co, "fwd", "f32", 3, 3, 5, 7, 64, Co, 1, 1, 0, dict(f, SLOW=0, BN=b, MODE=0)))
    out.append(C("gf32-dgrad0", "dgrad", "f32", 3, 3, 10, 6, 64, 32, 3, 2, 1, dict(f, SLOW=0, BN=64, MODE=0), addend=True))
    out.append(C("gf32-dgrad0-wide", "dgrad", "f32", 3, 3, 10, 6, 192, 32, 3, 1, 1, dict(f, SLOW=0, BN=128, MODE=0)))
    out.append(C("gf32-slow-7x7", "fwd", "f32", 3, 2, 12, 10, 3, 64, 7, 2, 3, dict(f, SLOW=1, BN=64, MODE=0)))
    out.append(C("gbf16-slow-7x7", "fwd", "bf16", 3, 2, 12, 10, 3, 64, 7, 2, 3, dict(f, SLOW=1, BN=64, MODE=0)))
    out.append(C("gbf16-slow-co192", "fwd", "bf16", 3, 2, 12, 10, 3, 192, 3, 1, 1, dict(f, SLOW=1, BN=128, MODE=0)))
    out.append(C("gf32-slow-co192", "fwd", "f32", 3, 2, 12, 10, 3, 192, 3, 1, 1, dict(f, SLOW=1, BN=128, MODE=0)))
    return out


def _wgrad_cases():
    out = []
    t = dict(FAMILY=GATHER, SLOW=0)      # family 0 = the TN kernel
    for Co, half in ((64, 1), (128, 0)):
        for wm, fold in (("plain", 0), ("fold", 1)):
            # nsplit 1, written in place (1x1, npix <= 256); the same shape with accumulate: slab + reduction
            if not fold:
                out.append(C("wtn-co%d-direct" % Co, "wgrad", "bf16", 3, 2, 16, 8, 64, Co, 1, 1, 0,
                             dict(t, HALF_M=half, NSPLIT=1, DIRECT=1, REDUCE=RED_NONE, LEAN=1), wmode=wm))
                out.append(C("wtn-co%d-direct-acc" % Co, "wgrad", "bf16", 3, 2, 16, 8, 64, Co, 1, 1, 0,
                             dict(t, HALF_M=half, NSPLIT=1, DIRECT=0, REDUCE=RED_VEC4), wmode=wm, accumulate=1))
            # few splits: vec4 for 1x1, taps for 3x3 (10 images of 16x8: npix 1 280 -> 5 splits; G = 3: nkz = 15, xcd_group 2)
            for acc in (0, 1):
                out.append(C("wtn-co%d-1x1-%s-acc%d" % (Co, wm, acc), "wgrad", "bf16", 3, 10, 16, 8, 128, Co, 1, 1, 0,
                             dict(t, HALF_M=half, FOLD=fold, NSPLIT=5, XCD_GROUP=2, LEAN=1, LOADER=LD_PLAIN,
                                  REDUCE=RED_NONE if fold else RED_VEC4, N1=1 if fold else 0), wmode=wm, accumulate=acc))
            out.append(C("wtn-co%d-3x3s2-%s" % (Co, wm), "wgrad", "bf16", 3, 10, 32, 16, 64, Co, 3, 2, 1,
                         dict(t, HALF_M=half, FOLD=fold, NSPLIT=5, XCD_GROUP=2, LEAN=1, LOADER=LD_IM2COL,
                              REDUCE=RED_NONE if fold else RED_TAPS), wmode=wm))
            # more than 16 splits: scalar reduction / two-level fold (3x3 stride 2, 34 images of 32x16: npix 4 352 -> 17 splits)
            out.append(C("wtn-co%d-17splits-%s" % (Co, wm), "wgrad", "bf16", 3, 34, 32, 16, 64, Co, 3, 2, 1,
                         dict(t, HALF_M=half, FOLD=fold, NSPLIT=17, XCD_GROUP=1, REDUCE=RED_NONE if fold else RED_SCALAR,
                              N1=4 if fold else 0), wmode=wm))
    out.append(C("wtn-3x3s2-deferred", "wgrad", "bf16", 3, 10, 32, 16, 64, 128, 3, 2, 1, dict(t, NSPLIT=5, REDUCE=RED_TAPS),
                 wmode="deferred"))
    out.append(C("wtn-1x1-deferred", "wgrad", "bf16", 3, 10, 16, 8, 128, 128, 1, 1, 0, dict(t, NSPLIT=5, REDUCE=RED_VEC4),
                 wmode="deferred", accumulate=1))
    out.append(C("wtn-17splits-deferred", "wgrad", "bf16", 3, 34, 32, 16, 64, 64, 3, 2, 1, dict(t, NSPLIT=17, REDUCE=RED_SCALAR),
                 wmode="deferred"))
    # nkz = 25 (G = 1): padded to 32, idle workgroups (50 images of 16x8 = 6 400 pixels -> 25 splits of 256)
    out.append(C("wtn-25splits-g1", "wgrad", "bf16", 1, 50, 16, 8, 64, 64, 1, 1, 0,
                 dict(t, NSPLIT=25, XCD_GROUP=1, REDUCE=RED_VEC4), wmode="plain"))
    out.append(C("wtn-25splits-g1-fold", "wgrad", "bf16", 1, 50, 16, 8, 64, 64, 1, 1, 0,
                 dict(t, NSPLIT=25, XCD_GROUP=1, FOLD=1, N1=5), wmode="fold"))
    # npix % 64 != 0: the pointer-form loaders (11 images of 5x7 = 385 pixels; 3x3 and 1x1)
    out.append(C("wtn-ragged-1x1", "wgrad", "bf16", 3, 11, 5, 7, 64, 128, 1, 1, 0, dict(t, LEAN=0, LOADER=LD_PLAIN), wmode="plain"))
    out.append(C("wtn-ragged-3x3", "wgrad", "bf16", 3, 11, 5, 7, 64, 64, 3, 1, 1, dict(t, LEAN=0, LOADER=LD_IM2COL), wmode="plain"))
    out.append(C("wtn-ragged-3x3-fold", "wgrad", "bf16", 3, 11, 5, 7, 64, 64, 3, 1, 1, dict(t, LEAN=0, FOLD=(0, 1)), wmode="fold"))
    # other forms: fp32 fast and slow, bf16 slow
    out.append(C("wf32-3x3", "wgrad", "f32", 3, 3, 10, 6, 32, 64, 3, 1, 1, dict(t, PIPE=0), wmode="plain"))
    out.append(C("wf32-1x1-acc", "wgrad", "f32", 3, 3, 16, 8, 64, 192, 1, 1, 0, dict(t, PIPE=0), wmode="plain", accumulate=1))
    out.append(C("wf32-slow-7x7", "wgrad", "f32", 3, 2, 12, 10, 3, 64, 7, 2, 3, dict(FAMILY=GATHER, SLOW=1), wmode="plain"))
    out.append(C("wbf16-slow-7x7", "wgrad", "bf16", 3, 2, 12, 10, 3, 64, 7, 2, 3, dict(FAMILY=GATHER, SLOW=1), wmode="plain"))
    # 3x3 patch form: WLOG 3 / 4 / 5 x HALF_M x fold; single-k-tile images (8x8, 16x4, 32x2), multi-tile images, ragged last
    # split, 17 splits (34 images of 8x16, G = 1), Ci = 128
    p = dict(FAMILY=PATCH)
    for (W, wl) in ((8, 3), (16, 4), (32, 5)):
        for Co, half in ((64, 1), (128, 0)):
            for wm, fold in (("plain", 0), ("fold", 1)):
                h1 = 64 // W
                out.append(C("wpatch-w%d-co%d-1tile-%s" % (W, Co, wm), "wgrad", "bf16", 3, 9, h1, W, 64, Co, 3, 1, 1,
                             dict(p, WLOG=wl, HALF_M=half, FOLD=fold), wmode=wm))
                out.append(C("wpatch-w%d-co%d-multi-%s" % (W, Co, wm), "wgrad", "bf16", 3, 5, 3 * h1, W, 64 if Co == 64 else 128, Co,
                             3, 1, 1, dict(p, WLOG=wl, HALF_M=half, FOLD=fold), wmode=wm))
    out.append(C("wpatch-17splits", "wgrad", "bf16", 1, 34, 16, 8, 64, 64, 3, 1, 1, dict(p, WLOG=3, NSPLIT=17, REDUCE=RED_SCALAR),
                 wmode="plain"))
    out.append(C("wpatch-17splits-fold", "wgrad", "bf16", 1, 34, 16, 8, 64, 64, 3, 1, 1, dict(p, WLOG=3, NSPLIT=17, FOLD=1, N1=4),
                 wmode="fold"))
    out.append(C("wpatch-deferred", "wgrad", "bf16", 3, 9, 8, 8, 64, 128, 3, 1, 1, dict(p, WLOG=3, FOLD=0), wmode="deferred"))
    return out


# Weight-gradient rows the closure test asked for: the branch combinations (loader x lean x tile height x fold depth x workgroup map x
# in-place x reduction form, both types) that the layer grid reaches and no hand-written row above selects, each at the smallest
# shape a search over small maps found for it.  (dtype, (G, N, H, W, Ci, Co, R, stride, pad), plan flags, the form key it must select)
CLOSURE_ROWS = [
    ('bf16', (1, 17, 12, 10, 64, 128, 1, 1, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1)),
    ('bf16', (1, 1, 8, 4, 64, 128, 1, 1, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 0)),
    ('bf16', (1, 17, 12, 10, 64, 128, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0)),
    ('bf16', (1, 8, 5, 7, 64, 128, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 0, 1, 1, 2, 0, 0)),
    ('bf16', (1, 50, 12, 10, 64, 128, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 0, 1, 2, 1, 0, 0)),
    ('bf16', (1, 17, 12, 10, 64, 64, 1, 1, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 1)),
    ('bf16', (1, 8, 5, 7, 64, 64, 1, 1, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 1, 0, 0, 2, 0, 1)),
    ('bf16', (1, 17, 12, 10, 64, 64, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0)),
    ('bf16', (1, 8, 5, 7, 64, 64, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 0, 1, 1, 1, 2, 0, 0)),
    ('bf16', (1, 5, 12, 32, 64, 128, 1, 1, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1)),
    ('bf16', (1, 5, 12, 32, 64, 128, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0)),
    ('bf16', (1, 3, 64, 32, 64, 128, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 1, 0, 1, 2, 1, 0, 0)),
    ('bf16', (1, 5, 12, 32, 64, 64, 1, 1, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 0, 1, 1, 1, 1, 1, 0, 0)),
    ('bf16', (3, 50, 24, 8, 64, 128, 1, 2, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1)),
    ('bf16', (1, 17, 12, 10, 64, 128, 3, 1, 1), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 2)),
    ('bf16', (1, 24, 5, 7, 64, 128, 1, 2, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 1)),
    ('bf16', (1, 1, 8, 4, 64, 128, 3, 1, 1), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 2)),
    ('bf16', (1, 1, 8, 4, 64, 128, 1, 2, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 0, 0, 2, 1, 0)),
    ('bf16', (1, 17, 12, 10, 64, 128, 3, 1, 1), 8, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 1, 1, 1, 0, 0)),
    ('bf16', (1, 24, 5, 7, 64, 128, 1, 2, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 1, 1, 2, 0, 0)),
    ('bf16', (1, 50, 12, 10, 64, 128, 3, 1, 1), 8, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 0, 1, 2, 1, 0, 0)),
    ('bf16', (1, 17, 12, 10, 64, 64, 3, 1, 1), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 1, 0, 0, 1, 0, 2)),
    ('bf16', (1, 17, 12, 10, 64, 64, 3, 1, 1), 8, ('wgrad', 'bf16', 0, 0, 0, 1, 0, 1, 1, 1, 1, 0, 0)),
    ('bf16', (1, 20, 12, 32, 64, 128, 1, 2, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1)),
    ('bf16', (1, 16, 12, 10, 64, 128, 3, 1, 1), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 2)),
    ('bf16', (1, 10, 16, 8, 64, 128, 1, 2, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 1, 0, 0, 0, 2, 0, 1)),
    ('bf16', (1, 2, 16, 8, 64, 128, 1, 2, 0), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 1, 0, 0, 0, 2, 1, 0)),
    ('bf16', (1, 20, 12, 32, 64, 128, 1, 2, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 1, 1, 0, 1, 1, 1, 0, 0)),
    ('bf16', (1, 16, 12, 10, 64, 64, 3, 1, 1), 0, ('wgrad', 'bf16', 0, 0, 0, 1, 1, 1, 0, 0, 1, 0, 2)),
    ('bf16', (1, 20, 12, 32, 64, 64, 1, 2, 0), 8, ('wgrad', 'bf16', 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0)),
    ('bf16', (1, 34, 16, 8, 64, 128, 3, 1, 1), 0, ('wgrad', 'bf16', 1, 0, 3, 0, 0, 0, 0, 0, 0, 0, 3)),
    ('bf16', (1, 34, 16, 8, 64, 128, 3, 1, 1), 8, ('wgrad', 'bf16', 1, 0, 3, 0, 0, 0, 1, 2, 0, 0, 0)),
    ('bf16', (1, 34, 8, 16, 64, 128, 3, 1, 1), 0, ('wgrad', 'bf16', 1, 0, 4, 0, 0, 0, 0, 0, 0, 0, 3)),
    ('bf16', (1, 34, 8, 16, 64, 128, 3, 1, 1), 8, ('wgrad', 'bf16', 1, 0, 4, 0, 0, 0, 1, 2, 0, 0, 0)),
    ('bf16', (1, 34, 8, 16, 64, 64, 3, 1, 1), 0, ('wgrad', 'bf16', 1, 0, 4, 0, 0, 1, 0, 0, 0, 0, 3)),
    ('bf16', (1, 34, 8, 16, 64, 64, 3, 1, 1), 8, ('wgrad', 'bf16', 1, 0, 4, 0, 0, 1, 1, 2, 0, 0, 0)),
    ('bf16', (1, 34, 4, 32, 64, 64, 3, 1, 1), 0, ('wgrad', 'bf16', 1, 0, 5, 0, 0, 1, 0, 0, 0, 0, 3)),
    ('bf16', (1, 34, 4, 32, 64, 64, 3, 1, 1), 8, ('wgrad', 'bf16', 1, 0, 5, 0, 0, 1, 1, 2, 0, 0, 0)),
    ('f32', (1, 5, 24, 8, 64, 64, 1, 1, 0), 0, ('wgrad', 'f32', 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1)),
    ('f32', (1, 1, 8, 4, 64, 64, 1, 1, 0), 0, ('wgrad', 'f32', 0, 0, 0, 0, 0, 0, 0, 0, 2, 1, 0)),
    ('f32', (1, 10, 12, 32, 64, 64, 1, 2, 0), 0, ('wgrad', 'f32', 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1)),
    ('f32', (1, 5, 24, 8, 64, 64, 3, 1, 1), 0, ('wgrad', 'f32', 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 2)),
    ('f32', (1, 50, 10, 6, 64, 64, 3, 1, 1), 0, ('wgrad', 'f32', 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 3)),
    ('f32', (1, 12, 5, 7, 64, 64, 1, 2, 0), 0, ('wgrad', 'f32', 0, 0, 0, 1, 0, 0, 0, 0, 2, 0, 1)),
    ('f32', (1, 1, 8, 4, 64, 64, 1, 2, 0), 0, ('wgrad', 'f32', 0, 0, 0, 1, 0, 0, 0, 0, 2, 1, 0)),
]


def _closure_cases():
    out = []
    for i, (dtype, d, fl, key) in enumerate(CLOSURE_ROWS):
        wm = "fold" if fl & FL["tickets"] else ("deferred" if fl & FL["deferred"] else "plain")
        out.append(C("wclosure%02d-%s-%s" % (i, dtype, "x".join(str(v) for v in d)), "wgrad", dtype, *d, {}, wmode=wm, key=key))
    return out


def _natural_wide_cases():
    """the unmodified plan reaches the 128-wide instantiations from 513 workgroups on: G = 3, N = 172 images of 8x16 (172 row
    tiles x 3 = 516), Ci = 64, Co = 128.  Forward only: the reference is the cost here."""
    return [C("natural-wide-patch", "fwd", "bf16", 3, 172, 16, 8, 64, 128, 3, 1, 1, dict(FAMILY=PATCH, BN=128, STYLE=1, WLOG=3, MODE=1),
              sums=True),
            C("natural-wide-gather", "fwd", "bf16", 3, 172, 16, 8, 64, 128, 1, 1, 0,
              dict(FAMILY=GATHER, BN=128, PIPE=1, LOADER=LD_PLAIN, MODE=1), sums=True)]


@functools.lru_cache(maxsize=None)
def cases(child=False):
    if child:
        return tuple(_patch_cases(True) + _gather_cases(True))
    return tuple(_patch_cases(False) + _stem_cases() + _gather_cases(False) + _wgrad_cases() + _closure_cases() +
                 _natural_wide_cases())


CHILD_ENV = {"IEEE_GATHER_NARROW_WG": "0"}


# ---- the closure grid: the 22 distinct ResNet-50 / CIM conv shapes at 256x128 (Ci, Co, R, stride, Hin, Win) and the padded stem
LAYERS = [(64, 64, 1, 1, 64, 32), (64, 64, 3, 1, 64, 32), (64, 256, 1, 1, 64, 32), (256, 64, 1, 1, 64, 32),
          (256, 128, 1, 1, 64, 32), (128, 128, 3, 2, 64, 32), (128, 512, 1, 1, 32, 16), (256, 512, 1, 2, 64, 32),
          (512, 128, 1, 1, 32, 16), (128, 128, 3, 1, 32, 16), (512, 256, 1, 1, 32, 16), (256, 256, 3, 2, 32, 16),
          (256, 1024, 1, 1, 16, 8), (512, 1024, 1, 2, 32, 16), (1024, 256, 1, 1, 16, 8), (256, 256, 3, 1, 16, 8),
          (1024, 512, 1, 1, 16, 8), (512, 512, 3, 1, 16, 8), (512, 2048, 1, 1, 16, 8), (1024, 2048, 1, 1, 16, 8),
          (2048, 512, 1, 1, 16, 8), (2048, 2048, 1, 1, 16, 8)]
IMAGE_SIZES = [(256, 128), (128, 64), (384, 128), (192, 96), (160, 80), (224, 224)]
BATCHES = [1, 2, 3, 4, 6, 8, 16, 32, 48, 64, 96, 128]


def grid_calls():
    """(op, dtype, dims, flags) of every conv call net.hip makes over the grid: conv (with and without fused sums), conv_bn_eval
    (with and without residual), dgrad (plain, fused, fused with the compact addend where the ABI allows it), dgrad_compact (the
    1x1 stride-1 dgrad over the output grid of a stride-2 1x1), wgrad_on (immediate, fold, deferred); the padded stem has no dgrad"""
    for (ih, iw) in IMAGE_SIZES:
        for B in BATCHES:
            for dtype in ("bf16", "f32"):
                shapes = [(Ci, Co, R, st, R // 2, Hi * ih // 256, Wi * iw // 128, False) for (Ci, Co, R, st, Hi, Wi) in LAYERS]
                shapes.append((4, 64, 8, 2, 0, ih + 6, iw + 6, True))
                for (Ci, Co, R, st, pad, Hi, Wi, stem) in shapes:
                    if Hi < 1 or Wi < 1:
                        continue
                    d = (3, B, Hi, Wi, Ci, Co, R, st, pad)
                    for fl in (0, FL["sums"]) if dtype == "bf16" else (0,):
                        yield ("fwd", dtype, d, fl)
                    for fl in (0, FL["addend"]):
                        yield ("eval", dtype, d, fl)
                    for fl in (0, FL["tickets"], FL["deferred"]):
                        yield ("wgrad", dtype, d, fl)
                    if stem:
                        continue
                    yield ("dgrad", dtype, d, 0)
                    yield ("dgrad", dtype, d, FL["addend"])
                    if dtype == "bf16":
                        yield ("dgrad", dtype, d, FL["sums"])
                        yield ("dgrad", dtype, d, FL["sums"] | FL["addend"])
                        if st == 1 and Hi > 1 and Wi > 1 and not (Hi & (Hi - 1)) and not (Wi & (Wi - 1)):
                            yield ("dgrad", dtype, d, FL["sums"] | FL["addend"] | FL["s2"])
                    if R == 1 and st == 2:
                        yield ("dgrad", dtype, (3, B, Hi // 2, Wi // 2, Ci, Co, 1, 1, 0), 0)


# ---- reference
def _h(v):
    """a seed that does not change from process to process (str hashes do)"""
    return zlib.crc32(repr(v).encode()) & 0x7FFFFFFF


def _rt(dtype):
    return (lambda t: t.to(torch.bfloat16).to(F64)) if dtype == "bf16" else (lambda t: t.to(torch.float32).to(F64))


class Ref(object):
    """operands [G][N][C][H][W] (float64 values of the stored type) and, on demand, y / dx / dw with their sums of |terms|"""

    def __init__(self, key):
        dtype, G, N, Hh, W, Ci, Co, R, stride, pad = key
        self.key, self.stride, self.pad = key, stride, pad
        g = torch.Generator().manual_seed(_h(key))
        rt = _rt(dtype)
        Ho, Wo = (Hh + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        self.x = rt(torch.randn(G, N, Ci, Hh, W, generator=g))
        self.w = rt(torch.randn(G, Co, Ci, R, R, generator=g) * (2.0 / (Ci * R * R)) ** 0.5)
        self.dy = rt(torch.randn(G, N, Co, Ho, Wo, generator=g))
        self._c = {}

    def _conv(self, x, w):
        return torch.stack([F.conv2d(x[i], w[i], None, self.stride, self.pad) for i in range(x.shape[0])])

    def _grad(self, x, w, dy, wrt):
        outs = []
        for i in range(x.shape[0]):
            xi, wi = x[i].clone().requires_grad_(wrt == "x"), w[i].clone().requires_grad_(wrt == "w")
            y = F.conv2d(xi, wi, None, self.stride, self.pad)
            outs.append(torch.autograd.grad(y, xi if wrt == "x" else wi, dy[i])[0])
        return torch.stack(outs)

    def get(self, what):
        """what in y, dx, dw: (reference, sum of |terms|); y / dx as NHWC [G][N][H][W][C], dw OIHW"""
        if what not in self._c:
            if what == "y":
                r, a = self._conv(self.x, self.w), self._conv(self.x.abs(), self.w.abs())
            else:
                wrt = "x" if what == "dx" else "w"
                r, a = self._grad(self.x, self.w, self.dy, wrt), self._grad(self.x.abs(), self.w.abs(), self.dy.abs(), wrt)
            if what != "dw":
                r, a = r.permute(0, 1, 3, 4, 2).contiguous(), a.permute(0, 1, 3, 4, 2).contiguous()
            self._c[what] = (r, a)
        return self._c[what]


@functools.lru_cache(maxsize=6)
def cached_ref(key):
    return Ref(key)


def ref_of(c):
    return cached_ref((c.dtype, c.G, c.N, c.H, c.W, c.Ci, c.Co, c.R, c.stride, c.pad))


def u_of(dtype):
    return 2.0 ** -23 if dtype == "bf16" else U32


def hu_of(dtype):
    return 2.0 ** -8 if dtype == "bf16" else U32


def store_bound(dtype, ref, delta):
    return delta + hu_of(dtype) * (ref.abs() + delta) if dtype == "bf16" else delta + U32 * ref.abs()


def addend_bound(dtype, ref, e1, a):
    return e1 + hu_of(dtype) * ((ref + a).abs() + e1) + U32 * (ref.abs() + a.abs())


def aux(c, shape, seed, scale=1.0):
    """a further operand of a case (addend, residual, y of the BatchNorm in front, mask source), rounded to the stored type"""
    g = torch.Generator().manual_seed(7919 * seed + _h(c.name) % 100003)
    return _rt(c.dtype)(torch.randn(*shape, generator=g) * scale)


def bn_stats(c, Cn, seed):
    """[G][4][C] fp32 statistics whose scale / shift keep the pre-activations of Gaussian y off the kink: |scale| in [0.5, 1.5],
    every fifth negative, |shift| >= 0.05"""
    g = torch.Generator().manual_seed(104729 * seed + Cn)
    st = torch.randn(c.G, 4, Cn, generator=g)
    sc = torch.rand(c.G, Cn, generator=g) + 0.5
    sc[:, ::5] *= -1
    sh = torch.randn(c.G, Cn, generator=g) * 0.3
    sh = torch.where(sh.abs() < 0.05, torch.full_like(sh, 0.05) * torch.sign(sh + 1e-9), sh)
    st[:, 2], st[:, 3] = sc, sh
    return st.to(torch.float32)


def mode2_reference(c):
    """everything a MODE 2 dgrad case is judged by, from the reference alone: d = dgrad (+ addend), its bound, the mask, the kink set"""
    r = ref_of(c)
    dx, A = r.get("dx")
    delta = c.R * c.R * c.Co * u_of(c.dtype) * A
    e1 = store_bound(c.dtype, dx, delta)
    o = types.SimpleNamespace(y=aux(c, dx.shape, 3), add=None, add_full=None, stats=None, mask_src=None, kink=None)
    d, bound = dx, e1
    if c.addend:
        if c.s2:
            o.add = aux(c, (c.G, c.N, c.H // 2, c.W // 2, c.Ci), 4)
            o.add_full = torch.zeros_like(dx)
            o.add_full[:, :, ::2, ::2] = o.add
        else:
            o.add = o.add_full = aux(c, dx.shape, 4)
        d, bound = dx + o.add_full, addend_bound(c.dtype, dx, e1, o.add_full)
    o.d, o.dbound = d, bound
    if c.mask in ("mask", "bits"):
        o.mask_src = aux(c, dx.shape, 5)           # the activation behind the ReLU: positive = kept
        o.keep = o.mask_src > 0
    elif c.mask == "stats":
        o.stats = bn_stats(c, c.Ci, 6)
        sc, sh = o.stats[:, 2].to(F64)[:, None, None, None, :], o.stats[:, 3].to(F64)[:, None, None, None, :]
        pre, mag = o.y * sc + sh, (o.y * sc).abs() + sh.abs()
        o.keep = pre > 0
        o.kink = ~ub.kink_keep(pre, mag)
    else:
        o.keep = torch.ones_like(dx, dtype=torch.bool)
    o.y2 = aux(c, dx.shape, 8) if c.bn2 else None
    return o


def kink_share(c):
    o = mode2_reference(c)
    return 0.0 if o.kink is None else float(o.kink.double().mean())


# ---- comparison and reporting
def compare(fails, c, family, name, dev, ref, bound):
    dev = dev.detach().to(F64).cpu().reshape(ref.shape)
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    bound = bound.expand_as(ref)
    err = (dev - ref).abs()
    ok = err <= bound                      # NaN fails
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                               torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = family + ":" + name
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    if not bool(ok.all()):
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        fails.append("%s %s: %d of %d beyond the bound; worst at %s: device %.9g reference %.9g bound %.3g (x%.3g)"
                     % (c.name, name, int((~ok).sum()), ok.numel(), idx, float(dev.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                        float(bound.reshape(-1)[i]), worst))


def _dump_ratios():
    path = os.environ.get("IEEE_CONV_RATIOS_FILE")
    if path and RATIOS:
        old = {}
        if os.path.exists(path):
            old = json.load(open(path))
        for k, v in RATIOS.items():
            old[k] = max(old.get(k, 0.0), v)
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)


atexit.register(_dump_ratios)


def family_of(c, p):
    if c.op == "wgrad":
        return "wgrad-" + ("tn", "patch", "stem")[p["FAMILY"]] + ("-fold" if p["FOLD"] else "") + ("-f32" if c.dtype == "f32" else "")
    return ("gather", "patch", "stem")[p["FAMILY"]] + ("-f32" if c.dtype == "f32" else "") + ("-slow" if p["SLOW"] else "")


# ---- device side: the C ABI as net.hip calls it
def _tdt(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _idt(L, c):
    return L.IEEE_BF16 if c.dtype == "bf16" else L.IEEE_F32


def gbuf(c, t, fill=SENT, dtype=None, pad=PADE):
    """[G][...] float64 -> device buffer [G][numel + pad] of the stored type (the group stride is numel + pad); returns
    (buffer, view of the tensors, group stride)"""
    G = t.shape[0]
    n = t[0].numel()
    b = torch.full((G, n + pad), fill, dtype=dtype or _tdt(c))
    b[:, :n] = t.reshape(G, n).to(b.dtype)
    b = b.to(DEV)
    return b, b[:, :n].view(t.shape), n + pad


def pad_untouched(b, n, fill=SENT):
    return bool((b[:, n:].float() == fill).all())


def pack_w(L, lib, c, w, mode):
    """fp32 OIHW [G][Co][Ci][R][S] -> the packed GEMM operand (mode 0 forward, 1 dgrad), groups PADE elements apart"""
    G, Co, Ci, R, S = w.shape
    dt = _idt(L, c)
    ld = lib.ieee_conv_packed_ld(dt, Ci if mode == 0 else Co, R, S)
    rows = Co if mode == 0 else Ci
    wd = w.to(torch.float32).to(DEV).contiguous()
    wp = torch.zeros(G, rows * ld + PADE, device=DEV, dtype=_tdt(c))
    L.check(lib.ieee_pack_conv_weight(L.ptr(wd), L.ptr(wp), dt, mode, G, Co, Ci, R, S, Co * Ci * R * S, rows * ld + PADE, L.stream()))
    return wp, rows * ld + PADE


def stem_operands(L, lib, c, r):
    """the border-padded 4-channel image from ieee_nchw_to_nhwc3 and the 8x8x4 packed weights (ieee_pack_conv_weight_padded)"""
    dt = _idt(L, c)
    G, N, Hh, W = c.G, c.N, c.H, c.W
    assert G == 3
    xs = [r.x[i].to(torch.float32).contiguous().to(DEV) for i in range(3)]
    xp = torch.full((G, N, Hh + 6, W + 6, 4), 7.0, device=DEV, dtype=_tdt(c))
    L.check(lib.ieee_nchw_to_nhwc3(L.ptr(xs[0]), L.ptr(xs[1]), L.ptr(xs[2]), L.ptr(xp), dt, N, 3, Hh, W, 4, 3, L.stream()))
    ld = lib.ieee_conv_packed_ld(dt, 4, 8, 8)
    wp = torch.empty(G, c.Co, ld, device=DEV, dtype=_tdt(c))
    wd = r.w.to(torch.float32).to(DEV).contiguous()
    L.check(lib.ieee_pack_conv_weight_padded(L.ptr(wd), L.ptr(wp), dt, 0, G, c.Co, 3, 7, 7, 4, 8, 8, c.Co * 3 * 49, c.Co * ld, L.stream()))
    return xp, wp, c.Co * ld


def _tile_sums(t, tiles):
    """[G][M][C] float64 -> per 128-row tile sums [G][C][tiles]"""
    G, M, Cn = t.shape
    p = torch.zeros(G, tiles * 128, Cn, dtype=F64)
    p[:, :M] = t
    return p.view(G, tiles, 128, Cn).sum(2).permute(0, 2, 1)


def check_sums(fails, c, fam, part, tot, rep, q1, q2, a1, a2, extra1=None, extra2=None, scale=2.0 ** 24):
    """partials [G][2][C][tiles] (or the fixed-point totals [rep][G][2][C]) against float64 per-tile sums q1 / q2 [G][C][tiles] with
    sums of |terms| a1 / a2; extra: what the kink elements may add to a tile's bound"""
    tiles = q1.shape[-1]
    n = 128 + tiles
    b1, b2 = n * U32 * a1, n * U32 * a2
    if extra1 is not None:
        b1, b2 = b1 + extra1, b2 + extra2
    if tot is None:
        compare(fails, c, fam, "sum1", part[:, 0], q1, b1)
        compare(fails, c, fam, "sum2", part[:, 1], q2, b2)
    else:
        got = tot.sum(0).to(F64).cpu() / scale
        compare(fails, c, fam, "total1", got[:, 0], q1.sum(-1), b1.sum(-1) + tiles * 0.5 / scale)
        compare(fails, c, fam, "total2", got[:, 1], q2.sum(-1), b2.sum(-1) + tiles * 0.5 / scale)
        if rep > 1:      # tile t adds to replica t % rep: every replica against its own tiles
            for r_ in range(rep):
                g_ = tot[r_].to(F64).cpu() / scale
                compare(fails, c, fam, "total1-replica", g_[:, 0], q1[..., r_::rep].sum(-1),
                        b1[..., r_::rep].sum(-1) + tiles * 0.5 / scale)


def perm_rows(c):
    """pixel (n * H * W + h * W + w) of GEMM row m in the parity-class-major order of the stride-2 dgrad (StagedStoreEpi VAR 1):
    class (h & 1, w & 1) outermost, then image, then the class's rows and columns"""
    hw, wc = (c.H // 2) * (c.W // 2), c.W // 2
    m = torch.arange(c.N * c.H * c.W)
    cls, rc = m // (c.N * hw), m % (c.N * hw)
    n, i, j = rc // hw, (rc % hw) // wc, rc % wc
    return n * c.H * c.W + (2 * i + (cls >> 1)) * c.W + 2 * j + (cls & 1)


def _extras(L, tot, gs, rep):
    ex = L.ConvExtras()
    ex.totals, ex.group_stride, ex.replicas, ex.reserved_ = tot.data_ptr(), gs, rep, 0
    ex.overflow = ex.start = ex.stop = None
    return ex


def run_fwd(L, lib, c, p):
    """ieee_conv2d_fwd_ex (MODE 0 / 1, partials or totals) or ieee_conv2d_fwd_bn_eval (MODE 3)"""
    fails, fam = [], family_of(c, p)
    r = ref_of(c)
    dt = _idt(L, c)
    G, N = c.G, c.N
    y, A = r.get("y")
    delta = c.R * c.R * c.Ci * u_of(c.dtype) * A
    if c.stem:
        xd, wp, w_gs = stem_operands(L, lib, c, r)
        x_gs = xd[0].numel()
        dims = (N, c.H + 6, c.W + 6, 4, c.Co, 8, 8, 2, 0)
    else:
        xb, xd, x_gs = gbuf(c, r.x.permute(0, 1, 3, 4, 2).contiguous())
        wp, w_gs = pack_w(L, lib, c, r.w, 0)
        dims = (N, c.H, c.W, c.Ci, c.Co, c.R, c.R, c.stride, c.pad)
    M = N * c.Ho * c.Wo
    ob, od, y_gs = gbuf(c, torch.full_like(y, SENT))
    tiles = (M + 127) // 128
    if c.op == "eval":
        st = bn_stats(c, c.Co, 2)
        std = st.to(DEV)
        res = aux(c, y.shape, 9) if c.addend else None
        rd = gbuf(c, res)[0] if c.addend else None
        L.check(lib.ieee_conv2d_fwd_bn_eval(L.ptr(xd), L.ptr(wp), L.ptr(ob), L.ptr(rd), L.ptr(std), c.relu, dt, G, *dims, x_gs, w_gs,
                                            y_gs, L.stream()))
        torch.cuda.synchronize()
        sc, sh = st[:, 2].to(F64)[:, None, None, None, :], st[:, 3].to(F64)[:, None, None, None, :]
        e1 = store_bound(c.dtype, y, delta) if c.dtype == "bf16" else delta
        pre = y * sc + sh
        mag = (y * sc).abs() + sh.abs()
        if c.addend:
            pre, mag = pre + res, mag + res.abs()
        want = pre.clamp_min(0) if c.relu else pre
        dpre = e1 * sc.abs() + 3 * U32 * mag
        compare(fails, c, fam, "out-mode3", od, want, dpre + hu_of(c.dtype) * (want.abs() + dpre))
    else:
        part = torch.full((G, 2, c.Co, tiles), SENT, device=DEV) if c.sums else None
        tot = torch.zeros(c.totals, G, 2, c.Co, dtype=torch.int64, device=DEV) if c.totals else None
        ex = _extras(L, tot, 2 * c.Co, c.totals) if c.totals else None
        L.check(lib.ieee_conv2d_fwd_ex(L.ptr(xd), L.ptr(wp), L.ptr(ob), dt, G, *dims, x_gs, w_gs, y_gs, L.ptr(part),
                                       ctypes.addressof(ex) if ex is not None else None, L.stream()))
        torch.cuda.synchronize()
        compare(fails, c, fam, "y-mode%d" % (1 if c.sums else 0), od, y, store_bound(c.dtype, y, delta))
        if c.sums:
            s = od.to(F64).cpu().reshape(G, M, c.Co)
            q1, q2, a1 = _tile_sums(s, tiles), _tile_sums(s * s, tiles), _tile_sums(s.abs(), tiles)
            if c.totals:
                # the partial form on the same operands: the totals are its integer image, tile by tile
                part2 = torch.full((G, 2, c.Co, tiles), SENT, device=DEV)
                o2 = torch.empty_like(ob)
                L.check(lib.ieee_conv2d_fwd_ex(L.ptr(xd), L.ptr(wp), L.ptr(o2), dt, G, *dims, x_gs, w_gs, y_gs, L.ptr(part2), None,
                                               L.stream()))
                torch.cuda.synchronize()
                if not torch.equal(tot.sum(0), torch.round(part2.double() * 2.0 ** 24).sum(-1).to(torch.int64)):
                    fails.append("%s: the fixed-point totals are not the integer image of the per-tile partials" % c.name)
                if not bool((part == SENT).all()):
                    fails.append("%s: bn_partial written although totals were given" % c.name)
                check_sums(fails, c, fam, None, tot, c.totals, q1, q2, a1, q2)
            else:
                check_sums(fails, c, fam, part, None, 0, q1, q2, a1, q2)
    if not pad_untouched(ob, y[0].numel()):
        fails.append("%s: the padding behind a group's output was written" % c.name)
    return fails


def run_dgrad(L, lib, c, p):
    """ieee_conv2d_dgrad_ex: MODE 0 (+ addend) or MODE 2 with the mask sources, compact addend, second BatchNorm, totals"""
    fails, fam = [], family_of(c, p)
    r = ref_of(c)
    dt = _idt(L, c)
    G, N = c.G, c.N
    o = mode2_reference(c)
    dyb, dyd, dy_gs = gbuf(c, r.dy.permute(0, 1, 3, 4, 2).contiguous())
    wp, w_gs = pack_w(L, lib, c, r.w, 1)
    M = N * c.H * c.W
    tiles = (M + 127) // 128
    ob, od, dx_gs = gbuf(c, torch.full_like(o.d, SENT))
    addb = None
    if c.addend:
        addb = gbuf(c, o.add, pad=PADE // 4 if c.s2 else PADE)[0]
    part = part2 = yb = y2b = mb = stb = tot = ex = None
    bits = 0
    if c.sums:
        part = torch.full((G, 2, c.Ci, tiles), SENT, device=DEV)
        yb = gbuf(c, o.y)[0]
        if c.mask == "mask":
            mb = gbuf(c, o.mask_src)[0]
        elif c.mask == "bits":
            full = torch.zeros(G, dx_gs, dtype=torch.int32)
            full[:, :o.d[0].numel()] = o.keep.reshape(G, -1).to(torch.int32)
            mb = (full.view(-1, 8) << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8).to(DEV)
            bits = 1
        elif c.mask == "stats":
            stb = o.stats.to(DEV)
        if c.bn2:
            y2b = gbuf(c, o.y2)[0]
            part2 = torch.full((G, 2, c.Ci, tiles), SENT, device=DEV)
        if c.totals:
            tot = torch.zeros(c.totals, G, 2, c.Ci, dtype=torch.int64, device=DEV)
            ex = _extras(L, tot, 2 * c.Ci, c.totals)
    L.check(lib.ieee_conv2d_dgrad_ex(L.ptr(dyd), L.ptr(wp), L.ptr(ob), L.ptr(addb), dt, G, N, c.H, c.W, c.Ci, c.Co, c.R, c.R, c.stride,
                                     c.pad, dy_gs, w_gs, dx_gs, L.ptr(part), L.ptr(yb), L.ptr(mb), L.ptr(stb), bits, 2 if c.s2 else 1,
                                     L.ptr(y2b), L.ptr(part2), ctypes.addressof(ex) if ex is not None else None, L.stream()))
    torch.cuda.synchronize()
    zero = torch.zeros_like(o.d)
    stored_masked = c.sums and c.mask in ("mask", "bits")
    want = torch.where(o.keep, o.d, zero) if stored_masked else o.d
    compare(fails, c, fam, "dx-mode%d" % (2 if c.sums else 0), od, want, torch.where(o.keep, o.dbound, zero) if stored_masked else o.dbound)
    if not pad_untouched(ob, o.d[0].numel()):
        fails.append("%s: the padding behind a group's output was written" % c.name)
    if c.sums:
        s = od.to(F64).cpu()
        g = torch.where(o.keep, s, torch.zeros_like(s))
        rows = perm_rows(c) if p["VAR"] == 1 else None      # a tile's 128 GEMM rows: consecutive pixels, or parity-class order
        flat = lambda t: t.reshape(G, M, c.Ci) if rows is None else t.reshape(G, M, c.Ci)[:, rows]
        q1, q2 = _tile_sums(flat(g), tiles), _tile_sums(flat(g * o.y), tiles)
        a1, a2 = _tile_sums(flat(g.abs()), tiles), _tile_sums(flat((g * o.y).abs()), tiles)
        e1 = e2 = None
        if o.kink is not None:
            if float(o.kink.double().mean()) > ub.KINK_CAP:
                fails.append("%s: more than %g of the elements lie on the ReLU kink" % (c.name, ub.KINK_CAP))
            k = torch.where(o.kink, s.abs(), torch.zeros_like(s))
            e1, e2 = _tile_sums(flat(k), tiles), _tile_sums(flat(k * o.y.abs()), tiles)
        if c.totals:
            check_sums(fails, c, fam, None, tot, c.totals, q1, q2, a1, a2, e1, e2, scale=2.0 ** 40)
            if not bool((part == SENT).all()):
                fails.append("%s: bn_partial written although totals were given" % c.name)
        else:
            check_sums(fails, c, fam, part, None, 0, q1, q2, a1, a2, e1, e2)
        if c.bn2:
            q3, a3 = _tile_sums(flat(g * o.y2), tiles), _tile_sums(flat((g * o.y2).abs()), tiles)
            if not torch.equal(part2[:, 0], part[:, 0]):
                fails.append("%s: the second BatchNorm's sum g differs from the first's" % c.name)
            compare(fails, c, fam, "sum-g-y2", part2[:, 1], q3, (128 + tiles) * U32 * a3)
    return fails


def _reduce_batch(L, lib, descs, G):
    tab = (L.WgradReduceDesc * len(descs))()
    blocks = 0
    for i, d in enumerate(descs):
        ctypes.memmove(ctypes.addressof(tab[i]), ctypes.addressof(d), ctypes.sizeof(d))
        tab[i].block_begin = blocks
        blocks += d.blocks
    raw = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    L.check(lib.ieee_wgrad_reduce_batch(L.ptr(raw), len(descs), blocks, G, L.stream()))


def run_wgrad(L, lib, c, p):
    """ieee_conv2d_wgrad / _wgrad_fold / _wgrad_deferred + ieee_wgrad_reduce_batch; the stem through ieee_unpad_weight_grad"""
    fails, fam = [], family_of(c, p)
    r = ref_of(c)
    dt = _idt(L, c)
    G, N = c.G, c.N
    dw, A = r.get("dw")
    npix = N * c.Ho * c.Wo
    n = min(p["KCHUNK"] + p["NSPLIT"] + 2, npix)
    delta = n * u_of(c.dtype) * A
    dyb, dyd, dy_gs = gbuf(c, r.dy.permute(0, 1, 3, 4, 2).contiguous())
    if c.stem:
        xd = stem_operands(L, lib, c, r)[0]
        x_gs = xd[0].numel()
        dims = (N, c.H + 6, c.W + 6, 4, c.Co, 8, 8, 2, 0)
        wshape = (G, c.Co, 4, 8, 8)
        nbytes = lib.ieee_conv2d_wgrad_workspace_bytes(dt, G, N, c.Ho, c.Wo, 4, c.Co, 8, 8)
    else:
        xb, xd, x_gs = gbuf(c, r.x.permute(0, 1, 3, 4, 2).contiguous())
        dims = (N, c.H, c.W, c.Ci, c.Co, c.R, c.R, c.stride, c.pad)
        wshape = tuple(dw.shape)
        nbytes = lib.ieee_conv2d_wgrad_workspace_bytes(dt, G, N, c.Ho, c.Wo, c.Ci, c.Co, c.R, c.R)
    wn = 1
    for v in wshape[1:]:
        wn *= v
    dw0 = aux(c, wshape, 11).to(torch.float32).to(F64) if c.accumulate else torch.zeros(wshape, dtype=F64)
    tickets = torch.zeros(lib.ieee_conv2d_wgrad_fold_ticket_words(), dtype=torch.int32, device=DEV) if c.wmode == "fold" else None

    def call(acc, base):
        work = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
        ob, od, dw_gs = gbuf(c, base, dtype=torch.float32)
        args = (dt, G, *dims, dy_gs, x_gs, dw_gs, acc)
        if c.wmode == "fold":
            L.check(lib.ieee_conv2d_wgrad_fold(L.ptr(dyd), L.ptr(xd), L.ptr(ob), L.ptr(work), L.ptr(tickets), *args, L.stream()))
        elif c.wmode == "deferred":
            d = L.WgradReduceDesc()
            L.check(lib.ieee_conv2d_wgrad_deferred(L.ptr(dyd), L.ptr(xd), L.ptr(ob), L.ptr(work), *args, ctypes.addressof(d), L.stream()))
            if d.kind != 0:
                _reduce_batch(L, lib, [d], G)
        else:
            L.check(lib.ieee_conv2d_wgrad(L.ptr(dyd), L.ptr(xd), L.ptr(ob), L.ptr(work), *args, L.stream()))
        torch.cuda.synchronize()
        if not pad_untouched(ob, wn):
            fails.append("%s: the padding behind a group's gradient was written" % c.name)
        return od

    got = call(c.accumulate, dw0 if c.accumulate else torch.full(wshape, SENT, dtype=F64))
    if c.stem:
        real = torch.full((G, c.Co, 3, 7, 7), SENT, device=DEV)
        gotc = got.contiguous()
        L.check(lib.ieee_unpad_weight_grad(L.ptr(gotc), L.ptr(real), G, c.Co, 4, 8, 8, 3, 7, 7, wn, c.Co * 147, 0, L.stream()))
        torch.cuda.synchronize()
        # (the zero 4th channel of the image has a zero gradient; the 8th filter row / column sees real pixels and is dropped)
        if float(gotc[:, :, 3].abs().max()) != 0.0:
            fails.append("%s: the gradient of the zero 4th input channel is not zero" % c.name)
        compare(fails, c, fam, "dw", real, dw, delta + U32 * dw.abs())
        return fails
    want = dw0 + dw
    compare(fails, c, fam, "dw-acc" if c.accumulate else "dw", got, want,
            delta + U32 * dw.abs() + (U32 * want.abs() if c.accumulate else 0.0))
    if c.wmode == "fold" and p["FOLD"]:
        again = call(c.accumulate, dw0 if c.accumulate else torch.full(wshape, SENT, dtype=F64))
        if not torch.equal(again, got):
            fails.append("%s: a repeated fold call is not bit-identical" % c.name)
        if not c.accumulate:
            twice = call(1, got.to(F64).cpu())
            if not torch.equal(twice, got + got):
                fails.append("%s: accumulate = 1 on the fold's own result does not double it" % c.name)
        if int(tickets.abs().max()) != 0:
            fails.append("%s: the fold left tickets behind" % c.name)
    return fails


def run_case(L, lib, c):
    """plan assertion first (so the case is known to test what it names), then the run and every comparison"""
    bad = check_plan(lib, c)
    if bad:
        return bad
    p = case_plan(lib, c)
    if c.op in ("fwd", "eval"):
        return run_fwd(L, lib, c, p)
    if c.op == "dgrad":
        return run_dgrad(L, lib, c, p)
    return run_wgrad(L, lib, c, p)


# ---- nested-sum restatement (the reference of the reference): tiny shapes only
def nested(x, w, dy, stride, pad):
    """y, dx, dw of one group by explicit loops over (n, co, ho, wo, ci, r, s) in float64"""
    N, Ci, Hh, W = x.shape
    Co, _, R, S = w.shape
    Ho, Wo = (Hh + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    y, dx, dw = torch.zeros(N, Co, Ho, Wo, dtype=F64), torch.zeros_like(x), torch.zeros_like(w)
    for n in range(N):
        for co in range(Co):
            for ho in range(Ho):
                for wo in range(Wo):
                    for r_ in range(R):
                        for s_ in range(S):
                            hi, wi = ho * stride - pad + r_, wo * stride - pad + s_
                            if 0 <= hi < Hh and 0 <= wi < W:
                                y[n, co, ho, wo] += (x[n, :, hi, wi] * w[co, :, r_, s_]).sum()
                                dx[n, :, hi, wi] += dy[n, co, ho, wo] * w[co, :, r_, s_]
                                dw[co, :, r_, s_] += dy[n, co, ho, wo] * x[n, :, hi, wi]
    return y, dx, dw


# ---- the child process of the 128-wide forms: IEEE_GATHER_NARROW_WG is read once per process
def child_main():
    sys.path.insert(0, ROOT)
    import ieee_amd  # noqa: F401  (before the HIP runtime starts)
    from ieee_amd import _lib as L
    lib = L.require_gpu()
    fails = []
    for c in cases(True):
        fails += run_case(L, lib, c)
    for f in fails:
        print(f)
    print("wide forms: %d cases, %d failed comparisons" % (len(cases(True)), len(fails)))
    return 1 if fails else 0


def child_plan_main():
    """CPU: every child row selects its form under the child's environment"""
    sys.path.insert(0, ROOT)
    from ieee_amd import _lib as L
    lib = L.load()
    bad = []
    for c in cases(True):
        bad += check_plan(lib, c)
    keys = sorted({form_key(c.op, c.dtype, case_plan(lib, c)) for c in cases(True) if case_plan(lib, c) is not None})
    for b in bad:
        print(b)
    print("KEYS " + json.dumps(keys))
    print("wide plans: %d mismatches" % len(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(child_plan_main() if sys.argv[1:] == ["plan"] else child_main())
