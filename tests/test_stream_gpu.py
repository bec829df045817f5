"""GPU: the device side of what the retrieval drivers share (ieee_amd/metrics/_stream.py).  SlabDistances against
compute_distance_matrix on the same rows, bit for bit, with the life of its one buffer; device_matrix on every layout it
tells apart; TopKAccumulator.merge / state against add / result."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, D, WIDTHS = 3, 10, (5, 8, 3, 13)            # d = 10 is padded to 16; the slabs are one gallery of 29 rows


def bits(t):
    return t.contiguous().view(torch.int32)


def descriptors(dtype):
    gen = torch.Generator().manual_seed(5)
    return torch.randn(Q, D, generator=gen).to(dtype), torch.randn(sum(WIDTHS), D, generator=gen).to(dtype)


def stage_of(q, metric, precision):
    from ieee_amd import _lib
    from ieee_amd.metrics import _stream as S
    from ieee_amd.metrics import distance
    prec, cdt = distance._resolve(precision, q.dtype)
    return S.SlabDistances(_lib.require_gpu(), q, S.check_metric(metric), cdt, prec, torch.device("cuda"))


@pytest.mark.parametrize("metric,precision,dtype", [("euclidean", "fp32", torch.float32), ("cosine", "fp32", torch.float32),
                                                    ("euclidean", "f16x2", torch.float32),
                                                    ("euclidean", None, torch.bfloat16), ("cosine", None, torch.bfloat16)])
def test_slab_distances(metric, precision, dtype):
    from ieee_amd.metrics import compute_distance_matrix
    q, g = descriptors(dtype)
    qd = q.cuda()
    ref = [compute_distance_matrix(qd, rows.cuda(), metric, precision) for rows in torch.split(g, WIDTHS)]
    for resident in ("host", "device"):
        stage, ptrs, kept = stage_of(q if resident == "host" else qd, metric, precision), [], []
        assert stage.q.shape == (Q, 16) and stage.q.is_cuda
        for rows, want in zip(torch.split(g if resident == "host" else g.cuda(), WIDTHS), ref):
            buf, ldd, n = stage.stage(rows)
            assert n == rows.shape[0] and ldd % 4 == 0 and ldd >= n and buf.shape == (Q, ldd) and buf.stride() == (ldd, 1)
            assert buf.dtype == torch.float32 and buf.is_cuda
            assert torch.equal(bits(buf[:, :n]), bits(want)), (resident, n)
            ptrs.append(buf.data_ptr())
            kept.append(buf)        # while the test holds a replaced buffer, its successor cannot come to the same address
            del buf
        assert [b.shape[1] for b in kept] == [8, 8, 8, 16]
        assert ptrs[0] == ptrs[1] == ptrs[2] and kept[1] is kept[2]              # width 8, then 3: the buffer stays
        assert ptrs[3] != ptrs[2]                                                # width 13: a wider one takes its place


def test_device_matrix():
    from ieee_amd.metrics._stream import device_matrix
    gen = torch.Generator().manual_seed(6)
    base = torch.randn(6, 12, generator=gen).cuda()
    dev = torch.device("cuda")

    def check(x, cols, copied, want):
        with warnings.catch_warnings():
            warnings.simplefilter("error")                   # a read-only numpy array reaches from_numpy as a copy
            d, ldd = device_matrix(x, dev, cols)
            d2, ldd2 = device_matrix(x)
        for m, ld in ((d, ldd), (d2, ldd2)):
            assert m.is_cuda and m.dtype == torch.float32 and m.shape == want.shape
            assert m.stride(1) == 1 and ld >= cols and ld == max(m.stride(0), cols)
            assert torch.equal(bits(m), bits(want))
            if isinstance(x, torch.Tensor):
                assert (m.data_ptr() != x.data_ptr()) == copied
            if copied:
                assert ld == cols and m.is_contiguous()
        return ldd

    assert check(base, 12, False, base) == 12                                    # contiguous: as it is
    assert check(base[:, 2:7], 5, False, base[:, 2:7]) == 12                     # a row-strided slice: read in place
    assert check(base[1:5, 4:], 8, False, base[1:5, 4:]) == 12
    check(base[:, ::2], 6, True, base[:, ::2])                                   # a column stride: copied
    check(base.t(), 6, True, base.t())
    check(base[0:1].expand(4, 12), 12, True, base[0:1].expand(4, 12))            # rows that overlap: copied
    a = np.random.RandomState(7).rand(5, 9).astype(np.float32)
    a.setflags(write=False)
    check(a, 9, True, torch.from_numpy(a.copy()).cuda())                         # read-only numpy: copied first
    check(a.astype(np.float64)[:, ::3], 3, True, torch.from_numpy(a.astype(np.float64)[:, ::3].astype(np.float32)).cuda())
    check(base.double().cpu(), 12, True, base.double().float())                  # other types, the host: converted
    check(base.half(), 12, True, base.half().float())
    d, ldd = device_matrix(base[:, :0], dev, 0)                                  # an empty slab
    assert d.shape == (6, 0) and ldd >= 0


@pytest.mark.parametrize("filtered", [False, True])
def test_merge_and_state_against_add_and_result(filtered):
    from ieee_amd.metrics import TopKAccumulator
    from ieee_amd.metrics._stream import host_labels, on_device
    rng = np.random.RandomState(8)
    d = (rng.rand(4, 50) * 10).astype(np.float32)
    d[:, 7] = d[:, 31]                                                           # ties go to the lower index
    qp, qc, gp, gc = rng.randint(0, 3, 4), rng.randint(0, 2, 4), rng.randint(0, 3, 50), rng.randint(0, 2, 50)
    q_labels = (qp, qc) if filtered else ()
    k = 6
    by_add = TopKAccumulator(4, k, *q_labels)
    by_add.add(d, *((gp, gc) if filtered else ()))
    by_merge = TopKAccumulator(4, k, *q_labels)
    idx0, dist0 = by_merge.state()
    assert idx0.dtype == torch.int32 and dist0.dtype == torch.float32 and idx0.shape == dist0.shape == (4, k)
    assert (idx0 == -1).all() and torch.isinf(dist0).all()
    wide = torch.zeros(4, 52, device="cuda")                                     # already in form: row stride 52 >= 50
    wide[:, :50] = torch.from_numpy(d)
    dev = wide.device
    g_labels = tuple(on_device(host_labels(x, "g", 50, "test"), dev) for x in (gp, gc)) if filtered else ()
    by_merge.merge(wide, 52, 50, *g_labels)
    assert by_merge.num_seen == by_add.num_seen == 50
    idx1, dist1 = by_merge.state()
    assert idx1 is idx0 and dist1 is dist0                                       # the live lists, not copies
    ri, rd = by_add.result()
    mi, md = by_merge.result()
    assert mi.dtype == torch.int64 and torch.equal(mi, ri) and torch.equal(bits(md), bits(rd))
    assert torch.equal(idx1.long(), ri) and torch.equal(bits(dist1), bits(rd))
    assert (ri[:, 0] >= 0).all() and mi.data_ptr() != idx1.data_ptr() and md.data_ptr() != dist1.data_ptr()
    by_merge.merge(None, 0, 0)                                                   # an empty slab: nothing is launched
    assert by_merge.num_seen == 50 and torch.equal(by_merge.result()[0], ri)
