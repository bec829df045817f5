"""Query expansion without a device: the argument checks of ieee_amd.expansion and of the engine's query_expansion
keyword (each before a device is needed), the signatures, the C ABI's argument errors, the float64 restatement against
the dense float64 implementation, and the bounds: the kernel's arithmetic emulated on the host stays inside them and
deliberately wrong references leave them."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import util_expansion as ux


def defaults(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def test_signatures():
    from ieee_amd.engine import Engine
    from ieee_amd.expansion import expand_descriptors, expansion_layout, neighbour_sum
    E = inspect.Parameter.empty
    assert defaults(expand_descriptors) == [("query", E), ("gallery", E), ("k", 5), ("alpha", 3), ("times", 1),
                                            ("mode", "both"), ("slab", None), ("block", None), ("precision", None),
                                            ("return_neighbours", False)]
    assert defaults(neighbour_sum)[:7] == [("src", E), ("idx", E), ("weights", E), ("rinv", None), ("self_rows", None),
                                           ("self_rinv", None), ("normalize", True)]
    assert defaults(expansion_layout) == [("Q", E), ("G", E), ("d", E), ("k", E), ("slab", None), ("block", None),
                                          ("mode", "both")]
    for fn in (Engine.run, Engine.test, Engine._evaluate):
        assert dict(defaults(fn))["query_expansion"] is None


def test_expand_descriptors_argument_checks(monkeypatch):
    from ieee_amd import _lib
    from ieee_amd import expansion as X
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a check came after the device was asked for"))
    q, g = torch.zeros(3, 8), torch.zeros(7, 8)
    for kw, msg in ((dict(k=0), "k must be"), (dict(k=1025), "k must be"), (dict(k=True), "k must be"),
                    (dict(k=2.5), "k must be"), (dict(alpha=2.5), "alpha must be"), (dict(alpha=True), "alpha must be"),
                    (dict(alpha=-1), "alpha must be"), (dict(alpha=65), "alpha must be"), (dict(alpha="3"), "alpha must be"),
                    (dict(times=0), "times must be"), (dict(times=1.5), "times must be"), (dict(times=True), "times must be"),
                    (dict(mode="gallery"), "mode must be"), (dict(slab=0), "slab must be"), (dict(block=0), "block must be"),
                    (dict(block=True), "block must be"), (dict(precision="fp8"), "precision")):
        with pytest.raises(ValueError, match=msg):
            X.expand_descriptors(q, g, **kw)
    with pytest.raises(ValueError, match=r"query must be a \[Q, d\] tensor"):
        X.expand_descriptors(torch.zeros(3), g)
    with pytest.raises(ValueError, match="the gallery and every piece"):
        X.expand_descriptors(q, torch.zeros(7, 9))
    with pytest.raises(ValueError, match="the gallery and every piece"):
        X.expand_descriptors(q, [g])                            # 'both' takes tensors
    with pytest.raises(ValueError, match="the gallery and every piece"):
        X.expand_descriptors(q, [g, torch.zeros(2, 9)], mode="query")
    with pytest.raises(ValueError, match="one-shot"):
        X.expand_descriptors(q, (p for p in [g]), mode="query")
    with pytest.raises(ValueError, match="one-shot"):
        X.expand_descriptors(q, iter([g]), mode="query")
    with pytest.raises(ValueError, match="gallery must be"):
        X.expand_descriptors(q, 5, mode="query")
    # 3.0 is an integer; with every argument in order the next thing asked for is the device
    monkeypatch.setattr(_lib, "require_gpu", lambda: (_ for _ in ()).throw(_lib.IeeeAmdError("device")))
    with pytest.raises(_lib.IeeeAmdError, match="device"):
        X.expand_descriptors(q, g, k=3.0, alpha=3.0, times=1.0)
    with pytest.raises(_lib.IeeeAmdError, match="device"):
        X.expand_descriptors(q, [g, torch.zeros(0, 8)], mode="query")


def test_neighbour_sum_and_layout_argument_checks(monkeypatch):
    from ieee_amd import _lib
    from ieee_amd import expansion as X
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("a check came after the device was asked for"))
    src, idx, w = torch.zeros(7, 8), torch.zeros(3, 5, dtype=torch.int32), torch.zeros(3, 5)
    for args, kw, msg in (((src[0], idx, w), {}, "src must be a 2-D"), ((src, idx[0], w), {}, "idx must be a 2-D"),
                          ((src, idx, w[:, :4]), {}, "weights .* do not match"),
                          ((src, idx.float(), w), {}, "idx must be an integer"),
                          ((src, torch.zeros(3, 1025, dtype=torch.int32), torch.zeros(3, 1025)), {}, "k must be"),
                          ((torch.zeros(7, 0), idx, w), {}, "at least one column"),
                          ((src, idx, w), dict(rinv=torch.zeros(6)), "rinv must be"),
                          ((src, idx, w), dict(self_rinv=torch.zeros(3)), "self_rinv without self_rows"),
                          ((src, idx, w), dict(self_rows=torch.zeros(3, 7)), "self_rows must be"),
                          ((src, idx, w), dict(self_rows=torch.zeros(3, 8), self_rinv=torch.zeros(4)), "self_rinv must be")):
        with pytest.raises(ValueError, match=msg):
            X.neighbour_sum(*args, **kw)
    for args, kw, msg in (((3, 7, 8, 0), {}, "k must be"), ((3, 7, 8, 1025), {}, "k must be"), ((-1, 7, 8, 5), {}, "Q must be"),
                          ((3, 7.5, 8, 5), {}, "G must be"), ((3, 7, 0, 5), {}, "d must be"),
                          ((3, 7, 8, 5), dict(mode="x"), "mode must be"), ((3, 7, 8, 5), dict(slab=0), "slab must be"),
                          ((3, 7, 8, 5), dict(block=-2), "block must be")):
        with pytest.raises(ValueError, match=msg):
            X.expansion_layout(*args, **kw)


def test_layout_counts():
    from ieee_amd.expansion import BLOCK_ROWS, expansion_layout
    from ieee_amd.metrics._stream import SLAB_BUDGET_BYTES
    lay = expansion_layout(3368, 19732, 2304, 5)
    N = 3368 + 19732
    assert lay["rows"] == lay["out"] == N * 2304 * 4 and lay["distances"] == BLOCK_ROWS * N * 4 <= SLAB_BUDGET_BYTES
    assert lay["total"] == sum(v for key, v in lay.items() if key != "total")
    # no term grows like N^2: ten times the rows, at most ten times (and a rounding) the bytes
    big = expansion_layout(33680, 197320, 2304, 5)
    assert big["total"] <= 10 * lay["total"] + 4096
    # the memory picture of the GPU test: a fifth of the N x N matrix is not reached
    assert expansion_layout(5000, 15000, 64, 5)["total"] < 20000 * 20000 * 4 // 5
    # an explicit blocking is what is counted; 'query' mode holds a table, never the gallery
    assert expansion_layout(10, 90, 8, 5, slab=7, block=3)["distances"] == 512        # 3 x 8 floats, rounded up
    lq = expansion_layout(100, 10 ** 6, 2304, 5, slab=16384, mode="query")
    assert lq["table"] >= 500 * 2304 * 4 and lq["staged"] == 16384 * 2304 * 4 and lq["total"] < 10 ** 6 * 2304 * 4 // 20


class DM(object):
    num_train_pids = 3
    sources = ["synthetic"]
    train_loader = []
    test_loader = {"synthetic": {"query": "query", "gallery": "gallery"}}


def test_engine_keyword_checks(monkeypatch):
    from ieee_amd import dist as ddp
    from ieee_amd.engine import Engine
    eng = Engine(DM(), use_gpu=False)
    seen = []
    eng._descriptors = lambda loader, clock: seen.append(loader)
    eng.set_model_mode = lambda *a, **k: seen.append("mode")
    bad = ("yes", 3, dict(k1=3), dict(k=0), dict(k=True), dict(alpha=2.5), dict(alpha=True), dict(alpha=65),
           dict(times=0), dict(times=1.5), dict(mode="gallery"), [("k", 3)])
    for qe in bad:
        for call in (lambda: eng.run(test_only=True, query_expansion=qe), lambda: eng.test(query_expansion=qe),
                     lambda: eng._evaluate(dataset_name="x", query_expansion=qe)):
            with pytest.raises(ValueError, match="query_expansion"):
                call()
    assert seen == []
    monkeypatch.setattr(ddp, "world_size", lambda: 2)
    for qe in (True, dict(k=3)):
        for call in (lambda: eng.run(test_only=True, query_expansion=qe), lambda: eng.test(query_expansion=qe),
                     lambda: eng._evaluate(dataset_name="x", query_expansion=qe)):
            with pytest.raises(ValueError, match="query_expansion runs on one rank"):
                call()
    assert seen == []


def test_engine_keyword_settings():
    from ieee_amd.engine import _check_query_expansion
    assert _check_query_expansion(None) is None and _check_query_expansion(False) is None
    assert _check_query_expansion(True) == dict(k=5, alpha=3, times=1, mode="both")
    assert _check_query_expansion(dict(k=3, alpha=3.0)) == dict(k=3, alpha=3, times=1, mode="both")
    assert _check_query_expansion(dict(mode="query", times=2)) == dict(k=5, alpha=3, times=2, mode="query")


def test_c_abi_argument_checks():
    from ieee_amd import _lib
    lib = _lib.load()
    null, one, two = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)   # never dereferenced

    def nsum(src=one, ld_src=8, n_src=7, rinv=null, idx=one, w=one, ld_list=5, n=3, k=5, self_rows=null, self_rinv=null,
             ld_self=0, d=8, normalize=1, out=two, ld_out=8):
        return lib.ieee_neighbour_sum(src, ld_src, n_src, rinv, idx, w, ld_list, n, k, self_rows, self_rinv, ld_self, d,
                                      normalize, out, ld_out, null)
    for kw, msg in ((dict(k=0), b"k 0 out of range"), (dict(k=1025, ld_list=1025), b"k 1025 out of range"),
                    (dict(d=0), b"d 0 out of range"), (dict(n=-1), b"rows n -1"), (dict(n_src=1 << 31), b"n_src"),
                    (dict(ld_list=4), b"stride below the row"), (dict(ld_src=7), b"stride below the row"),
                    (dict(ld_out=7), b"stride below the row"), (dict(self_rinv=one), b"self_rinv without self rows"),
                    (dict(self_rows=one, ld_self=7), b"stride below the row (self"),
                    (dict(idx=null), b"null pointer"), (dict(w=null), b"null pointer"), (dict(out=null), b"null pointer"),
                    (dict(src=null), b"null pointer"),
                    (dict(out=one), b"out overlaps src"),
                    (dict(out=ctypes.c_void_p((1 << 20) + 6 * 8 * 4 + 7 * 4)), b"out overlaps src"),     # src's last float
                    (dict(src=ctypes.c_void_p((1 << 30) + 2 * 8 * 4 + 7 * 4)), b"out overlaps src"),     # out's last float
                    (dict(self_rows=two, ld_self=8), b"out overlaps the self rows")):
        assert nsum(**kw) == -1, kw
        assert b"neighbour_sum" in lib.ieee_last_error() and msg in lib.ieee_last_error(), (kw, lib.ieee_last_error())
    assert nsum(n=0) == 0 and nsum(n=0, out=one) == 0                    # nothing to do: no launch
    assert lib.ieee_expand_weights(one, one, 10, 65, one, null) == -1 and b"expand_weights: alpha" in lib.ieee_last_error()
    assert lib.ieee_expand_weights(one, one, 10, -1, one, null) == -1 and b"expand_weights: alpha" in lib.ieee_last_error()
    assert lib.ieee_expand_weights(one, one, -1, 3, one, null) == -1 and b"expand_weights: count" in lib.ieee_last_error()
    assert lib.ieee_expand_weights(null, one, 10, 3, one, null) == -1 and b"null pointer" in lib.ieee_last_error()
    assert lib.ieee_expand_weights(null, null, 0, 3, null, null) == 0
    assert lib.ieee_row_rinv(one, 3, 6, one, null) == -1 and b"row_rinv: rows 3, feature dim 6" in lib.ieee_last_error()
    assert lib.ieee_row_rinv(one, -1, 8, one, null) == -1 and b"row_rinv" in lib.ieee_last_error()
    assert lib.ieee_row_rinv(null, 3, 8, one, null) == -1 and b"null pointer" in lib.ieee_last_error()
    assert lib.ieee_row_rinv(ctypes.c_void_p(68), 3, 8, one, null) == -1 and b"16-byte" in lib.ieee_last_error()
    assert lib.ieee_row_rinv(null, 0, 8, null, null) == 0


# ---------------------------------------------------------------- the float64 definitions and the bounds
SMALL = ux.FIXTURES[:2]


@pytest.fixture(scope="module")
def cases():
    return {shape: ux.make_fixture(*shape) for shape in SMALL}


@pytest.mark.parametrize("shape", SMALL, ids=str)
@pytest.mark.parametrize("mode", ("both", "query"))
def test_restatement_equals_the_dense_definition(cases, shape, mode):
    q, g = cases[shape]
    for k, alpha in ((1, 0), (5, 3), (5, 0), (4, 1), (sum(shape[:2]) + 3, 3)):
        rows = np.concatenate([q, g]) if mode == "both" else q
        cand = rows if mode == "both" else g
        idx, dist = ux.dense_lists(rows, cand, k)
        w = np.where(idx < 0, 0.0, np.ones_like(dist) if alpha == 0 else np.maximum(1 - dist, 0) ** alpha)
        val, mag, bound = ux.restate_round(cand, idx, w, self_rows=q if mode == "query" else None)
        dq, dg = ux.dense_expand(q, g, k, alpha, 1, mode)
        want = np.concatenate([dq, dg]) if mode == "both" else dq
        assert np.abs(val - want).max() < 1e-12
        assert np.all(mag >= np.abs(val * 0)) and np.all(bound > 0)
    # two rounds chain
    a = ux.dense_expand(*ux.dense_expand(q, g, 3, 3, 1, mode), 3, 3, 1, mode)
    b = ux.dense_expand(q, g, 3, 3, 2, mode)
    assert np.abs(a[0] - b[0]).max() < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-12


@pytest.mark.parametrize("shape", ux.FIXTURES, ids=str)
def test_every_row_is_its_own_nearest_neighbour(shape):
    q, g = ux.make_fixture(*shape)
    X = np.concatenate([q, g])
    idx, dist = ux.dense_lists(X, X, 2)
    assert np.array_equal(idx[:, 0], np.arange(len(X))) and dist[:, 0].max() < 1e-12
    assert dist[:, 1].min() > 1e-3          # far beyond what fp32 distances can confuse


def test_weight_chain_emulation():
    dist = np.array([0, -1e-7, 0.25, 1, 1 + 1e-7, 2, np.inf, np.nan], np.float32)
    for idx in (np.zeros(8, np.int32), np.full(8, -1, np.int32)):
        assert np.array_equal(ux.weights_fp32(idx, dist, 0), np.where(idx < 0, 0, 1).astype(np.float32))
        w3 = ux.weights_fp32(idx, dist, 3)
        s = np.float32(1) - np.float32(-1e-7)
        want = [1, np.float32(np.float32(s * s) * s), np.float32(0.421875), 0, 0, 0, 0, 0]
        assert np.array_equal(w3, np.where(idx < 0, 0, np.array(want, np.float32)).astype(np.float32))


def _emulated(q, g, k, alpha, mode):
    """the kernels' arithmetic on the host for one round, from fp32 lists -> (emulation, lists, weights)"""
    rows = np.concatenate([q, g]) if mode == "both" else q
    cand = rows if mode == "both" else g
    idx, dist = ux.dense_lists(rows, cand, k)
    w = ux.weights_fp32(idx, dist.astype(np.float32), alpha)
    rinv = ux.rinv64(cand).astype(np.float32)
    kw = dict(self_rows=q, self_rinv=ux.rinv64(q).astype(np.float32)) if mode == "query" else {}
    return ux.chain_fp32(cand, idx, w, rinv, **kw), cand, idx, w


@pytest.mark.parametrize("shape", SMALL, ids=str)
@pytest.mark.parametrize("mode", ("both", "query"))
def test_bounds_hold_the_emulation_and_reject_wrong_references(cases, shape, mode):
    q, g = cases[shape]
    k, alpha = 5, 3
    got, cand, idx, w = _emulated(q, g, k, alpha, mode)
    self_rows = q if mode == "query" else None
    val, _, bound = ux.restate_round(cand, idx, w, self_rows=self_rows)
    share = (np.abs(got - val) / bound).max()
    print("%s %s: the fp32 emulation uses %.1f %% of the bound" % (shape, mode, 100 * share))
    assert share < 1.0              # not vacuous either: measured shares are a few per cent
    dist = ux.dense_lists(np.concatenate([q, g]) if mode == "both" else q, cand, k)[1].astype(np.float32)
    wrong = {
        "alpha + 1": (idx, ux.weights_fp32(idx, dist, alpha + 1)),
        "alpha = 0": (idx, ux.weights_fp32(idx, dist, 0)),
        "last neighbour dropped": (np.where(np.arange(k) == k - 1, -1, idx), w),
        "weights paired with the wrong neighbours": (idx, w[:, ::-1]),
        "second neighbour twice": (np.concatenate([idx[:, :2], idx[:, 1:2], idx[:, 3:]], 1), w),
    }
    for name, (wi, ww) in wrong.items():
        bad = ux.restate_round(cand, wi, ww, self_rows=self_rows)[0]
        excess = (np.abs(bad - val) / bound).max()
        print("   %s: %.3g times the bound" % (name, excess))
        assert excess > 100, name
