"""The position kernels of ieee_amd/csrc/cim.hip (gpool_sum_others, ca_pool, cim_tail, cim_bwd_datt, cim_bwd_g,
cim_bwd_combine), called through the C ABI, against the float64 restatement and the derived error budget of tests/util_cim.py.
Every output is prefilled with a sentinel and followed by a guard of 64 sentinel elements: every element must be written, the
guard must not.  The argmax, S, and in mode 2 g1 are compared bit for bit.

Map geometries (H, W) with parts = 6, and what each selects at the executor's C = 2048 (four row lanes; 8 channel blocks in
fp32, 4 in bf16):
  (2, 2)    the smallest map; MAXS = 4 with three coinciding bins per row, two row lanes without rows, W below both load batches
  (5, 3)    MAXS = 4, rows per lane 2, 2, 1, 0
  (10, 5)   MAXS = 4 (160 x 80 images); the forward's batch of 4 positions has a tail of 1
  (14, 14)  MAXS = 4 (224 x 224); tails of 2 of 4 and 6 of 8
  (7, 9)    MAXS = 4; one position past the backward kernels' batch of 8
  (3, 3)    MAXS = 2; bins that coincide pairwise
  (12, 6)   MAXS = 2; bins that do not overlap
  (16, 8)   MAXS = 2; the benchmark's map
  (24, 8)   MAXS = 2 (384 x 128); bins that do not overlap
C = 256 at (2, 2), (10, 5), (16, 8): one channel block; four row lanes in fp32, eight in bf16.  fp32 C = 40 (cprw = 10, tx = 2,
128 row lanes, 5 channel blocks) and bf16 C = 24 (cprw = 3, tx = 1, 256 row lanes, 3 channel blocks) at (5, 3) and (16, 8).
Every form runs at (14, 14) and (16, 8) with C = 2048; every other cell runs the tail forward and bwd_g in mode 0 and two of
the other forms (util_cim.spread; tests/test_cim_forms_cpu.py proves which kernel instantiations the list reaches)."""
import pytest
import torch

from tests import util_cim as uc

pytestmark = pytest.mark.gpu

BF, FP = uc.BF, uc.FP


def _lib():
    from ieee_amd import _lib
    return _lib, _lib.require_gpu()


def _report(fails):
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("p,form", uc.spread(), ids=lambda v: uc.cell_id(v) if isinstance(v, tuple) else v)
def test_form(p, form):
    L, lib = _lib()
    _report(uc.run_form(L, lib, p, form))


def test_combine_second_ragged_trip():
    """fp32, C = 2048, 16 x 8, B = 9: 589 824 chunks against the launch's 2048 x 256 threads"""
    L, lib = _lib()
    _report(uc.run_form(L, lib, (FP, 9, 16, 8, 2048, 2), "combine-m0"))


@pytest.mark.parametrize("dtype,C", [(FP, 2048), (BF, 2048), (FP, 40), (BF, 24)], ids=["fp32-C2048", "bf16-C2048", "fp32-C40", "bf16-C24"])
def test_refusals(dtype, C):
    """a one-row map puts all six bins on one row lane: the three row-block launchers must refuse it; cim_tail_fwd also refuses
    parts = 9 and a statistics pointer that is not 16-byte aligned.  Nothing may be written."""
    L, lib = _lib()
    B, W = 2, 4
    dt = L.IEEE_BF16 if dtype == BF else L.IEEE_F32

    def refused(status):
        assert status != 0
        with pytest.raises(L.IeeeAmdError):
            L.check(status)

    def outs(H, parts=uc.PARTS):
        return [uc.Out((3, B, parts, C), FP), uc.Out((3, B, C), FP), uc.Out((3, B, H * W, C), dtype), uc.Out((3, B, H * W, C), dtype),
                uc.Out((3, 2, C, B), FP), uc.Out((3, 2, C, B), FP)]

    def ins(H, parts=uc.PARTS):
        y = torch.ones(3, B, H * W, C, device="cuda", dtype=dtype)
        st = torch.ones(3 * 4 * C + 4, device="cuda")
        vec = torch.ones(3, 2 * B, C, device="cuda")
        am = torch.zeros(3, B, C, device="cuda", dtype=torch.int32)
        return y, st, vec, am, torch.ones(3, B, parts, C, device="cuda")

    def untouched(os_):
        torch.cuda.synchronize()
        fails = []
        for i, o in enumerate(os_):
            o.check(fails, "refusals", "output %d" % i, written=False)
        _report(fails)

    y, st, vec, am, dP = ins(1)
    Pp, datt, g1, g2, b1, b2 = o = outs(1)
    refused(lib.ieee_cim_tail_fwd(L.ptr(y), L.ptr(y), L.ptr(st), L.ptr(st), L.ptr(vec), L.ptr(Pp.t), dt, B, 1, W, C, uc.PARTS, 0,
                                  L.stream()))
    refused(lib.ieee_cim_tail_bwd_datt(L.ptr(dP), L.ptr(y), L.ptr(st), L.ptr(datt.t), dt, B, 1, W, C, uc.PARTS, L.stream()))
    refused(lib.ieee_cim_tail_bwd_g(L.ptr(dP), L.ptr(y), L.ptr(y), L.ptr(st), L.ptr(st), L.ptr(vec), L.ptr(vec),
                                    uc._off(L, vec, B * C), 2 * B * C, L.ptr(am), L.ptr(g1.t), L.ptr(g2.t), dt, B, 1, W, C, uc.PARTS,
                                    0, L.ptr(b1.t), L.ptr(b2.t), L.stream()))
    untouched(o)
    y, st, vec, am, dP = ins(16, 9)
    o = outs(16, 9)
    refused(lib.ieee_cim_tail_fwd(L.ptr(y), L.ptr(y), L.ptr(st), L.ptr(st), L.ptr(vec), L.ptr(o[0].t), dt, B, 16, W, C, 9, 0,
                                  L.stream()))
    y, st, vec, am, dP = ins(16)
    o += outs(16)
    refused(lib.ieee_cim_tail_fwd(L.ptr(y), L.ptr(y), L.ptr(st), uc._off(L, st, 1), L.ptr(vec), L.ptr(o[6].t), dt, B, 16, W, C,
                                  uc.PARTS, 0, L.stream()))
    untouched(o)
