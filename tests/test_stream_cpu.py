"""CPU: the pieces the retrieval drivers share (ieee_amd/metrics/_stream.py) that need no device -- every validator
accepts and refuses what its copies in search.py, rank_stream.py, topk.py and rerank.py did, with the caller's name in
the message, and walk() cuts a tensor, a list and a generator into the right slabs, checking a piece when it is reached."""
import numpy as np
import pytest
import torch

from ieee_amd.metrics import _stream as S

WHO = "some_caller"


@pytest.mark.parametrize("k", [0, -3, 1025, 2.5, True, False])
def test_check_k_refuses(k):
    with pytest.raises(ValueError, match=r"some_caller: k must be an integer in \[1, 1024\]"):
        S.check_k(k, WHO)


def test_check_k_accepts():
    for k in (1, 10, 1024, 7.0, np.int64(5)):
        out = S.check_k(k, WHO)
        assert type(out) is int and out == k
    assert S.TOPK_MAX == 1024


@pytest.mark.parametrize("slab", [0, -5, 2.5, True, False])
def test_check_slab_refuses(slab):
    with pytest.raises(ValueError, match="some_caller: slab must be a positive integer"):
        S.check_slab(slab, 10, WHO)
    with pytest.raises(ValueError, match="gnn re-ranking: slab_rows must be a positive integer"):
        S.check_slab(slab, 10, "gnn re-ranking", "slab_rows")


def test_check_slab_accepts_and_defaults():
    for slab in (1, 3, 2048, 4.0, np.int32(9), 10 ** 9):
        out = S.check_slab(slab, 10, WHO)
        assert type(out) is int and out == slab
    for num_q in (0, 1, 100, 10000, 10 ** 7):
        assert S.check_slab(None, num_q, WHO) == S.default_slab_rows(num_q)


def test_default_slab_rows():
    assert S.TOPK_CHUNK == 2048
    for num_q in (0, 1, 7, 256, 10000, 16384, 16385, 10 ** 6, 10 ** 9):
        rows = S.default_slab_rows(num_q)
        assert rows % S.TOPK_CHUNK == 0 and rows >= S.TOPK_CHUNK
        assert rows == S.TOPK_CHUNK or max(num_q, 1) * rows * 4 <= S.SLAB_BUDGET_BYTES


def test_moved_names_are_still_exported():
    from ieee_amd import metrics
    from ieee_amd.metrics import rank, search, topk
    assert metrics.default_slab_rows is search.default_slab_rows is S.default_slab_rows
    assert search.TOPK_CHUNK == S.TOPK_CHUNK and search.SLAB_BUDGET_BYTES == S.SLAB_BUDGET_BYTES
    assert topk.TOPK_MAX == S.TOPK_MAX and callable(rank._i32)


def test_labels_all_or_none():
    z = np.zeros(3)
    assert S.check_labels_all_or_none(None, None, None, None, WHO) is False
    assert S.check_labels_all_or_none(z, z, z, z, WHO) is True
    for mask in range(1, 15):                                     # one, two or three of the four
        args = [z if mask >> i & 1 else None for i in range(4)]
        with pytest.raises(ValueError, match=r"some_caller: give all four of q_pids, g_pids, q_camids, g_camids, or none "
                                             r"\(got %d\)" % bin(mask).count("1")):
            S.check_labels_all_or_none(*args, WHO)


def test_metric_precision_query_piece_device():
    assert S.check_metric("euclidean") == 0 and S.check_metric("cosine") == 1
    for bad in ("manhattan", None, 0):
        with pytest.raises(ValueError, match="Unknown distance metric"):
            S.check_metric(bad)
    for ok in (None, "fp32", "bf16x3", "f16x2", "bf16x2", "bf16"):
        S.check_precision(ok)
    with pytest.raises(ValueError, match="Unknown distmat precision: fp8"):
        S.check_precision("fp8")
    assert tuple(S.check_query(torch.zeros(4, 10), WHO)) == (4, 10)
    assert tuple(S.check_query(torch.zeros(0, 8), WHO)) == (0, 8)
    for bad, got in ((torch.zeros(8), r"\(8,\)"), (torch.zeros(2, 3, 4), r"\(2, 3, 4\)"), (np.zeros((4, 8)), "ndarray")):
        with pytest.raises(ValueError, match=r"some_caller: query must be a \[Q, d\] tensor, got " + got):
            S.check_query(bad, WHO)
    S.check_piece(torch.zeros(5, 8), 8, WHO)
    S.check_piece(torch.zeros(0, 8), 8, WHO)
    for bad in (torch.zeros(5, 7), torch.zeros(8), np.zeros((5, 8)), None):
        with pytest.raises(ValueError, match=r"some_caller: the gallery and every piece of it must be a \[g, 8\] tensor"):
            S.check_piece(bad, 8, WHO)
    assert S.check_device(None, WHO) == torch.device("cuda") and S.check_device("cuda:1", WHO).index == 1
    with pytest.raises(ValueError, match="some_caller: device must be a CUDA device, got cpu"):
        S.check_device("cpu", WHO)


def test_host_labels():
    big = np.iinfo(np.int32).max
    for x in ([3, -1, big, -big - 1], np.array([3.0, 4.0]), torch.tensor([[1], [2]]), np.zeros(0)):
        a = S.host_labels(x, "g_pids", None, WHO)
        assert a.dtype == np.int32 and a.ndim == 1 and a.flags.c_contiguous
        assert a.tolist() == np.asarray(x).reshape(-1).tolist()
    assert S.host_labels(np.arange(10)[::3], "q_pids", 4, WHO).tolist() == [0, 3, 6, 9]
    for bad in ([0, big + 1], [-big - 2], np.array([2.0 ** 40]), torch.tensor([1 << 31])):
        with pytest.raises(ValueError, match="some_caller: g_camids does not fit int32"):
            S.host_labels(bad, "g_camids", None, WHO)
    with pytest.raises(ValueError, match="some_caller: q_pids has 3 entries, expected 4"):
        S.host_labels(np.zeros(3), "q_pids", 4, WHO)
    with pytest.raises(ValueError, match="some_caller: q_pids has 5 entries, expected 4"):
        S.host_labels(np.zeros(5), "q_pids", 4, WHO)
    with pytest.raises(ValueError, match="^q_pids does not fit int32$"):        # rank._i32's message: no caller
        S.host_labels([1 << 31], "q_pids", None, None)
    t = S.on_device(S.host_labels([1, 2, 3], "q_pids", 3, WHO), "cpu")
    assert t.dtype == torch.int32 and t.tolist() == [1, 2, 3]


# ---- walk ------------------------------------------------------------------------------------------------------------
def gallery(lengths, dim=4):
    """pieces whose rows carry their gallery index"""
    total = sum(lengths)
    whole = torch.arange(total, dtype=torch.float32).reshape(-1, 1).repeat(1, dim)
    return whole, list(torch.split(whole, lengths))


def walked(pieces, slab, dim=4):
    out = []
    for base, rows in S.walk(pieces, slab, dim, WHO):
        assert rows.dim() == 2 and rows.shape[1] == dim and 1 <= rows.shape[0] <= slab
        assert rows[:, 0].tolist() == list(range(base, base + rows.shape[0]))      # base is the first row's gallery index
        out.append((base, rows.shape[0]))
    return out


def expected(lengths, slab):
    out, base = [], 0
    for g in lengths:
        out += [(base + lo, min(slab, g - lo)) for lo in range(0, g, slab)]
        base += g
    return out


@pytest.mark.parametrize("lengths", [[7], [5, 0, 4], [0, 6, 1, 0], [1, 1, 1]])
def test_walk_cuts(lengths):
    whole, pieces = gallery(lengths)
    total = sum(lengths)
    for slab in sorted({1, 2, 3, max(lengths) - 1, max(lengths), total, total + 1, 10 ** 9} - {0}):
        want = expected(lengths, slab)
        assert walked(pieces, slab) == walked(tuple(pieces), slab) == walked((p for p in pieces), slab) == want
        assert sum(n for _, n in want) == total and [b for b, _ in want] == list(np.cumsum([0] + [n for _, n in want])[:-1])
        if len(lengths) == 1:
            assert walked(whole, slab) == want                                     # a tensor is one piece
    assert walked(pieces, total + 1) == [(b, g) for b, g in zip(np.cumsum([0] + lengths[:-1]), lengths) if g]


def test_walk_on_a_tensor():
    whole, _ = gallery([7])
    assert walked(whole, 1) == [(i, 1) for i in range(7)]
    assert walked(whole, 6) == [(0, 6), (6, 1)]
    assert walked(whole, 8) == [(0, 7)]
    assert walked(whole[:0], 3) == []
    rows = next(S.walk(whole, 4, 4, WHO))[1]
    assert rows.data_ptr() == whole.data_ptr()                                     # a view, not a copy


def test_walk_checks_a_piece_when_it_is_reached():
    _, pieces = gallery([5, 4])
    reached = []

    def source():
        for piece in pieces + [torch.zeros(3, 5), torch.zeros(2, 4)]:
            reached.append(tuple(piece.shape))
            yield piece
    it = S.walk(source(), 3, 4, WHO)
    assert reached == []                                                          # nothing is consumed ahead of its turn
    assert [next(it)[0] for _ in range(4)] == [0, 3, 5, 8]
    assert reached == [(5, 4), (4, 4)]
    with pytest.raises(ValueError, match=r"some_caller: the gallery and every piece of it must be a \[g, 4\] tensor, got "
                                         r"\(3, 5\)"):
        next(it)
    assert reached == [(5, 4), (4, 4), (3, 5)]                                    # ... and the piece after it never is
    for bad in ([pieces[0], np.zeros((2, 4))], [torch.zeros(4)]):
        it = S.walk(bad, 3, 4, WHO)
        with pytest.raises(ValueError, match="every piece of it must be"):
            list(it)
    for bad in ("gallery", b"gallery", 5, None):
        with pytest.raises(ValueError, match="some_caller: gallery must be a .* tensor or an iterable"):
            list(S.walk(bad, 3, 4, WHO))


def test_walk_tells_of_every_piece_after_its_check():
    _, pieces = gallery([5, 0, 4])
    seen = []
    out = list(S.walk(iter(pieces), 4, 4, WHO, lambda base, piece: seen.append((base, piece.shape[0]))))
    assert seen == [(0, 5), (5, 0), (5, 4)] and [b for b, _ in out] == [0, 4, 5]

    def stop(base, piece):
        if base:
            raise ValueError("stop at %d" % base)
    it = S.walk(iter(pieces), 4, 4, WHO, stop)
    assert [next(it)[0], next(it)[0]] == [0, 4]
    with pytest.raises(ValueError, match="stop at 5"):                             # before a slab of that piece is cut
        next(it)


def test_count_rows():
    _, pieces = gallery([5, 0, 4])
    assert S.count_rows(pieces, 4, WHO) == 9 and S.count_rows((), 4, WHO) == 0
    with pytest.raises(ValueError, match=r"must be a \[g, 4\] tensor"):
        S.count_rows(pieces + [torch.zeros(2, 3)], 4, WHO)
