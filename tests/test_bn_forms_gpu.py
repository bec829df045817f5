"""Every BatchNorm kernel form of ieee_amd/csrc/bn.hip, called through the C ABI as the executor calls it, against the float64
restatement and the derived error budget of tests/util_bn.py (done_event = NULL throughout).

Geometries (G, M, C) are chosen for what they select:
  bf16 C = 8      cprw = 1                                  fp32 C = 4      cprw = 1
  bf16 C = 24     cprw = 3: the plain kernels' 64-bit modulo branch (the totals entry points must refuse it)
  bf16 C = 64     the network's cprw family; fixed form for MASK = 2
  bf16 C = 2048   cprw = 256; the totals prologue takes 8 rounds; in reduce_channels tx * VEC = 512 exceeds the 256 threads
  fp32 C = 40     cprw = 10, not a power of two             fp32 C = 2048   cprw = 512
  M in {1, 3, 257, 1000}: one row, fewer rows than row lanes (M < ty), more than one row per lane, several row blocks
  G = 3 runs with parameter, buffer and gradient group strides of C + 8
  bf16 G = 1, M = 270 001, C = 64: the plain passes' grid-stride loop (8 192 workgroups) takes a second, ragged trip, the
  totals passes (2 048 workgroups) four trips and a ragged fifth, and the natural reduction reaches 768 row blocks (lpc = 256)
Every option is run at bf16 C = 64, M = 257, G = 3 and once more at each other (type, C), cycling through the row counts.
Longest fp32 addition chain per channel (rows per thread + ty of red_geom) at M = 1 / 3 / 257 / 1000: C = 8, 24 (bf16) and C = 4
(fp32) 257 / 257 / 258 / 260; C = 64 33 / 33 / 35 / 36; C = 40 129 / 129 / 131 / 132; C = 2048 (both types) 5 / 5 / 8 / 8; the large
shape 43.  util_bn.n_chain takes these, one more for the rounding of a product, and never more than M."""
import os
import subprocess
import sys

import pytest
import torch

from tests import util_bn as ub

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float32
GEOMS = [(BF, 8), (BF, 24), (BF, 64), (BF, 2048), (FP, 4), (FP, 40), (FP, 2048)]
TOTALS_GEOMS = [(BF, 8), (BF, 64), (BF, 2048)]
MS = (1, 3, 257, 1000)
LARGE = (BF, 1, 270001, 64)


def _lib():
    from ieee_amd import _lib
    return _lib, _lib.require_gpu()


def _spread(geoms, options):
    """[(dtype, G, M, C, name, options)]: all options at bf16 C = 64, M = 257, G = 3; elsewhere option i at M = MS[i % 4]"""
    out = []
    for dt, C in geoms:
        for i, (name, opt) in enumerate(options):
            if dt == FP and opt.get("bits"):
                opt = dict(opt, bits=False)
            M, G = MS[i % 4], (3 if i % 3 == 0 else 1)
            if (dt, C) == (BF, 64):
                out.append((dt, 3, 257, C, name, opt))
                if M == 257:
                    continue
            out.append((dt, G, M, C, name, opt))
    return sorted(out, key=lambda p: (p[0] == FP, p[3], p[2], p[1]))


def _id(p):
    return "%s-C%d-M%d-G%d-%s" % ("bf16" if p[0] == BF else "fp32", p[3], p[2], p[1], p[4])


def _overflow():
    return torch.full((4,), 7, device="cuda", dtype=torch.int32)


def _report(fails):
    assert not fails, "\n".join(fails)


FWD = _spread(GEOMS, [
    ("train", {}), ("train-norunning", dict(running=False)), ("eval", dict(training=0)), ("noout", dict(out=False)),
    ("res-relu-bits", dict(residual=True, bits=True)), ("res-norelu", dict(residual=True, relu=False)),
    ("relu-bits", dict(bits=True)), ("norelu", dict(relu=False)),
    ("partials1", dict(rb=1)), ("partials129", dict(rb=129)), ("partials300", dict(rb=300)), ("partials1500", dict(rb=1500)),
    ("given", dict(rb=-1, residual=True)), ("eval-noout", dict(training=0, out=False))])


@pytest.mark.parametrize("p", FWD, ids=_id)
def test_fwd(p):
    """ieee_bn2d_fwd: bn_stats_kernel, bn_finalize_kernel (both layouts, lpc 32..256, eval), bn_apply_kernel"""
    L, lib = _lib()
    dt, G, M, C, name, opt = p
    _report(ub.run_fwd(L, lib, ub.cached_case(dt, G, M, C), "fwd[%s]" % _id(p), strided=G == 3, **opt)[0])


BWD = _spread(GEOMS, [("mask%d-gout%d-acc%d" % (m, g, a), dict(mask_kind=m, gout=bool(g), accumulate=a))
                      for m in (0, 1, 2) for g in (1, 0) for a in (0, 1)]
              + [("partials129-mask2", dict(mask_kind=2, rb=129)), ("partials1500-mask0", dict(mask_kind=0, rb=1500, accumulate=1)),
                 ("nodgamma-mask1", dict(mask_kind=1, dgamma=False))])


@pytest.mark.parametrize("p", BWD, ids=_id)
def test_bwd(p):
    """ieee_bn2d_bwd: bn_bwd_reduce_kernel, bn_bwd_finalize_kernel, bn_bwd_apply_kernel; bf16 with the mask from y:
    bn_bwd_apply_fixed_kernel<bf16, 2, GOUT, 1> wherever C / 8 divides 256"""
    L, lib = _lib()
    dt, G, M, C, name, opt = p
    _report(ub.run_bwd(L, lib, ub.cached_case(dt, G, M, C), "bwd[%s]" % _id(p), strided=G == 3, **opt))


FROZEN = _spread(GEOMS, [("mask%d-gout%d" % (m, g), dict(mask_kind=m, gout=bool(g))) for m in (0, 1, 2) for g in (1, 0)])


@pytest.mark.parametrize("p", FROZEN, ids=_id)
def test_bwd_frozen(p):
    """ieee_bn2d_bwd_frozen: dy = scale * g within one rounding of the stored type, coef rows 2 and 3 exactly zero"""
    L, lib = _lib()
    dt, G, M, C, name, opt = p
    _report(ub.run_bwd(L, lib, ub.cached_case(dt, G, M, C), "frozen[%s]" % _id(p), entry="frozen", **opt))


FWD_TOTALS = _spread(TOTALS_GEOMS, [
    ("rep1", dict(totals=1)), ("rep3-res-bits", dict(totals=3, residual=True, bits=True)), ("rep64-res", dict(totals=64, residual=True)),
    ("rep3-bits", dict(totals=3, bits=True)), ("rep3-noout", dict(totals=3, out=False)),
    ("rep1-norunning-norelu", dict(totals=1, running=False, relu=False)), ("rep64-noout-norunning", dict(totals=64, out=False, running=False)),
    ("rep3-res-norelu", dict(totals=3, residual=True, relu=False))])


@pytest.mark.parametrize("p", FWD_TOTALS, ids=_id)
def test_fwd_totals(p):
    """ieee_bn2d_fwd_totals: bn_apply_totals_kernel<bf16, RES, BITS>; the range flags stay untouched on O(1) data"""
    L, lib = _lib()
    dt, G, M, C, name, opt = p
    ov = _overflow()
    fails = ub.run_fwd(L, lib, ub.cached_case(dt, G, M, C), "fwd_totals[%s]" % _id(p), strided=G == 3, overflow=ov, **opt)[0]
    assert bool((ov == 7).all()), ov
    _report(fails)


BWD_TOTALS = _spread(TOTALS_GEOMS, [("rep1-mask%d-gout%d" % (m, g), dict(totals=1, mask_kind=m, gout=bool(g)))
                                    for m in (0, 1, 2) for g in (1, 0)]
                     + [("rep3-mask2", dict(totals=3, mask_kind=2)), ("rep64-mask1", dict(totals=64, mask_kind=1, gout=False)),
                        ("rep3-nodgamma", dict(totals=3, mask_kind=0, dgamma=False))])


@pytest.mark.parametrize("p", BWD_TOTALS, ids=_id)
def test_bwd_totals(p):
    """ieee_bn2d_bwd_totals: bn_bwd_apply_totals_kernel<bf16, MASK, GOUT>"""
    L, lib = _lib()
    dt, G, M, C, name, opt = p
    ov = _overflow()
    fails = ub.run_bwd(L, lib, ub.cached_case(dt, G, M, C), "bwd_totals[%s]" % _id(p), strided=G == 3, entry="totals", overflow=ov,
                       **opt)
    assert bool((ov == 7).all()), ov
    _report(fails)


BWD_DS = _spread(TOTALS_GEOMS, [("rep3-ds1", dict(totals=3, replicas_ds=1)), ("rep1-ds4", dict(totals=1, replicas_ds=4)),
                                ("rep64-ds4", dict(totals=64, replicas_ds=4)), ("rep1-ds1-nodgamma", dict(totals=1, replicas_ds=1,
                                                                                                           dgamma=False))])


@pytest.mark.parametrize("p", BWD_DS, ids=_id)
def test_bwd_totals_ds(p):
    """ieee_bn2d_bwd_totals_ds: bn_bwd_apply_totals_ds_kernel<bf16>; the branch totals start non-zero, word [c] grows by exactly
    the integer total of sum g (again on a second call), word [C + c] by sum g * y_ds in 2^40 fixed point"""
    L, lib = _lib()
    dt, G, M, C, name, opt = p
    ov = _overflow()
    fails = ub.run_bwd(L, lib, ub.cached_case(dt, G, M, C), "bwd_totals_ds[%s]" % _id(p), strided=G == 3, entry="ds", overflow=ov,
                       **opt)
    assert bool((ov == 7).all()), ov
    _report(fails)


@pytest.mark.parametrize("form", ["fwd", "bwd", "fwd_totals", "bwd_totals", "bwd_totals_ds"])
def test_large_shape(form):
    """G = 1, M = 270 001, C = 64 in bf16 (see the module docstring); fwd_totals also shows that the running statistics are
    updated once and not once per workgroup"""
    L, lib = _lib()
    c = ub.cached_case(*LARGE)
    tag = "large[%s]" % form
    ov = _overflow()
    if form == "fwd":
        fails = ub.run_fwd(L, lib, c, tag, residual=True, bits=True)[0]
    elif form == "bwd":
        fails = ub.run_bwd(L, lib, c, tag, mask_kind=2, gout=True)
    elif form == "fwd_totals":
        fails = ub.run_fwd(L, lib, c, tag, residual=True, bits=True, totals=3, overflow=ov)[0]
    elif form == "bwd_totals":
        fails = ub.run_bwd(L, lib, c, tag, mask_kind=2, gout=True, entry="totals", totals=3, overflow=ov)
    else:
        fails = ub.run_bwd(L, lib, c, tag, entry="ds", totals=3, replicas_ds=4, overflow=ov)
    assert bool((ov == 7).all()), ov
    _report(fails)


@pytest.mark.parametrize("M", [20001, 40001])
def test_natural_row_blocks(M):
    """bf16 C = 64 at M = 20 001 / 40 001: the device's own reduction leaves 157 / 313 row blocks, so the finalize kernels walk the
    [rblock][2][C] layout with 64 / 128 lanes per channel (32 at the small shapes, 256 at the large one)"""
    L, lib = _lib()
    c = ub.cached_case(BF, 1, M, 64)
    assert ub.finalize_lpc(ub.red_geom(M, 64, 8).rblocks) == {20001: 64, 40001: 128}[M]
    fails = ub.run_fwd(L, lib, c, "natural_row_blocks[fwd]")[0]
    _report(fails + ub.run_bwd(L, lib, c, "natural_row_blocks[bwd]", mask_kind=2, accumulate=1))


@pytest.mark.parametrize("entry,value,word", [
    ("fwd", (1 << 61), None), ("fwd", (1 << 61) + 1, 2), ("bwd", -(1 << 61), None), ("bwd", -(1 << 61) - 1, 3),
    ("ds", (1 << 61), None), ("ds", (1 << 61) + 1, 3)])
def test_totals_range_flag(entry, value, word):
    """A total beyond +-2^61 sets overflow[2] (forward) / overflow[3] (backward), and only then.  Plain integers built by the
    test in one channel's second total, spread over three replicas; every output still follows the reference of those totals."""
    L, lib = _lib()
    c = ub.cached_case(BF, 1, 3, 64)
    ov = _overflow()
    tag = "range_flag[%s]" % entry
    if entry == "fwd":
        fails = ub.run_fwd(L, lib, c, tag, totals=3, overflow=ov, patch=(1, 5, value))[0]
    else:
        fails = ub.run_bwd(L, lib, c, tag, entry="totals" if entry == "bwd" else "ds", totals=3, replicas_ds=1, overflow=ov,
                           patch=(1, 5, value))
    want = [7, 7, 7, 7]
    if word is not None:
        want[word] = 1
    assert ov.tolist() == want
    _report(fails)


def test_argument_checks():
    """what the entry points must refuse before any launch: each returns non-zero, and L.check raises IeeeAmdError"""
    L, lib = _lib()
    G, M = 1, 3
    dev = "cuda"

    def refused(status):
        assert status != 0
        with pytest.raises(L.IeeeAmdError):
            L.check(status)

    def totals_calls(C, dt, rep, tot_offset=0):
        n = M * 2048
        y, dy, yds = (torch.zeros(n, device=dev, dtype=BF) for _ in range(3))
        gam, bet, dg, db = (torch.ones(2048, device=dev) for _ in range(4))
        stats = torch.ones(4 * 2048, device=dev)
        tot = torch.zeros(66 * 2 * 2048 + 2, device=dev, dtype=torch.int64)[tot_offset:]
        tds = torch.zeros(66 * 2 * 2048, device=dev, dtype=torch.int64)
        yield lib.ieee_bn2d_fwd_totals(L.ptr(y), None, L.ptr(dy), dt, G, M, C, M * C, L.ptr(gam), L.ptr(bet), C, None, None, C,
                                       L.ptr(stats), L.ptr(tot), rep, 0.1, 1e-5, 1, None, None, L.stream())
        yield lib.ieee_bn2d_bwd_totals(L.ptr(y), None, L.ptr(y), L.ptr(dy), None, dt, G, M, C, M * C, L.ptr(gam), C, L.ptr(stats),
                                       L.ptr(dg), L.ptr(db), C, L.ptr(tot), rep, 0, None, None, L.stream())
        yield lib.ieee_bn2d_bwd_totals_ds(L.ptr(y), L.ptr(y), L.ptr(yds), L.ptr(dy), dt, G, M, C, M * C, L.ptr(gam), C,
                                          L.ptr(stats), L.ptr(dg), L.ptr(db), C, L.ptr(tot), rep, L.ptr(tds), max(1, min(rep, 64)),
                                          None, None, L.stream())

    for C, dt, rep, off in ((24, L.IEEE_BF16, 1, 0), (64, L.IEEE_BF16, 0, 0), (64, L.IEEE_BF16, 65, 0), (64, L.IEEE_F32, 1, 0),
                            (64, L.IEEE_BF16, 1, 1)):      # off = 1: a totals pointer that is 8 but not 16 bytes aligned
        for status in totals_calls(C, dt, rep, off):
            refused(status)
    y = torch.zeros(M * 16, device=dev, dtype=BF)
    par = torch.ones(4 * 16, device=dev)
    part = torch.zeros(1024, device=dev)
    refused(lib.ieee_bn2d_fwd(L.ptr(y), None, L.ptr(y.clone()), L.IEEE_BF16, G, M, 12, M * 12, L.ptr(par), L.ptr(par), 12, None,
                              None, 12, L.ptr(par), L.ptr(part), 0.1, 1e-5, 1, 1, 0, None, L.stream()))
    torch.cuda.synchronize()


# measured on an MI355X in two runs: the child takes 7.6 / 9.5 s with unroll = 2 and 3.9 / 4.2 s with unroll = 1 (interpreter
# start, library load, its cases), rounded up here; the limit is five times that
CHILD_SECONDS = {2: 10.0, 1: 5.0}


@pytest.mark.parametrize("unroll", [2, 1])
def test_switched_forms(unroll):
    """IEEE_BN_FIXED = 15 selects bn_apply_fixed_kernel and bn_bwd_apply_fixed_kernel with every mask kind, IEEE_BN_UNROLL = 2
    their two-chunk loops.  Both are read once per process, so ONE fresh child interpreter runs the bf16 forward and backward
    case runner of tests/util_bn.py (switched_shapes: what each shape reaches) and prints one line per failed comparison.
    unroll = 1: the single-chunk instantiations of the forms that are off by default."""
    env = dict(os.environ, IEEE_BN_FIXED="15", IEEE_BN_UNROLL=str(unroll))
    try:
        r = subprocess.run([sys.executable, os.path.join(ub.ROOT, "tests", "util_bn.py"), str(unroll)], cwd=ub.ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=5 * CHILD_SECONDS[unroll])
    except subprocess.TimeoutExpired as e:
        pytest.exit("the switched-forms child did not end within %.0f s; nothing further is started on the GPU\n%s"
                    % (5 * CHILD_SECONDS[unroll], e.output), returncode=1)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit("the switched-forms child ended abnormally (status %d); nothing further is started on the GPU\n%s"
                    % (r.returncode, r.stdout), returncode=1)
    assert r.returncode == 0, r.stdout
