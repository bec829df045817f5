"""tests/util_bn.py on its own: the float64 restatement of BatchNorm2d against float64 autograd, the builders for partial
sums and fixed-point totals, the ReLU-kink filter, and the teeth of the error budget (pure CPU)."""
import pytest
import torch
import torch.nn.functional as F

from tests import util_bn as ub

BF, FP = torch.bfloat16, torch.float32
F64 = torch.float64
# (dtype, G, M, C): every channel count of test_bn_forms_gpu.py, the row counts with M > 1 where autograd is defined
CASES = [(BF, 3, 3, 8), (BF, 1, 257, 8), (BF, 1, 257, 24), (BF, 3, 257, 64), (BF, 1, 1000, 64), (BF, 1, 3, 2048),
         (BF, 1, 257, 2048), (FP, 3, 257, 4), (FP, 1, 1000, 4), (FP, 3, 3, 40), (FP, 1, 257, 40), (FP, 1, 257, 2048)]
ALL_CASES = CASES + [(BF, 3, 1, 64), (FP, 1, 1, 4), (BF, 1, 1, 2048)]


def _id(p):
    return "%s-G%d-M%d-C%d" % ("bf16" if p[0] == BF else "fp32", p[1], p[2], p[3])


def _exact_stats(c):
    s1, s2 = c.y.sum(1), (c.y * c.y).sum(1)
    z = torch.zeros_like(s1)
    r = ub.fwd_ref(c, sums=(s1, s2, z, z), relu=False)
    return torch.stack([r[k][0] for k in ("mean", "invstd", "scale", "shift")], 1)


@pytest.mark.parametrize("p", CASES, ids=_id)
@pytest.mark.parametrize("mask_kind", [0, 1, 2])
def test_restatement_equals_float64_autograd(p, mask_kind):
    c = ub.make_case(*p)
    residual, relu = mask_kind == 1, mask_kind != 0
    ref = ub.fwd_ref(c, residual=residual, relu=relu)
    back = ub.bwd_ref(c, _exact_stats(c), mask_kind, sums="exact")
    y = c.y.clone().requires_grad_(True)
    gamma, beta = c.gamma.clone().requires_grad_(True), c.beta.clone().requires_grad_(True)
    rm, rv = c.rm.clone(), c.rv.clone()
    outs = []
    for i in range(c.G):
        o = F.batch_norm(y[i], rm[i], rv[i], gamma[i], beta[i], True, ub.MOMENTUM, ub.EPS)
        if residual:
            o = o + c.res[i]
        outs.append(F.relu(o) if relu else o)
    out = torch.stack(outs)
    out.backward(back["dout"])
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["out"][0], out.detach(), **tol)
    torch.testing.assert_close(ref["rm"][0], rm, **tol)
    torch.testing.assert_close(ref["rv"][0], rv, **tol)
    torch.testing.assert_close(back["dy"][0], y.grad, **tol)
    torch.testing.assert_close(back["dgamma"][0], gamma.grad, **tol)
    torch.testing.assert_close(back["dbeta"][0], beta.grad, **tol)
    torch.testing.assert_close(back["g"][0], back["dout"] * (out.detach() > 0) if relu else back["dout"], rtol=0, atol=0)


def test_eval_and_frozen_forms():
    c = ub.make_case(FP, 3, 257, 40)
    ref = ub.fwd_ref(c, form="eval", training=False, residual=True, relu=True)
    want = torch.stack([F.relu(F.batch_norm(c.y[i], c.rm[i], c.rv[i], c.gamma[i], c.beta[i], False, ub.MOMENTUM, ub.EPS)
                               + c.res[i]) for i in range(c.G)])
    torch.testing.assert_close(ref["out"][0], want, rtol=1e-12, atol=1e-12)
    st = torch.stack([ref[k][0] for k in ("mean", "invstd", "scale", "shift")], 1)
    y = c.y.clone().requires_grad_(True)
    out = torch.stack([F.relu(F.batch_norm(y[i], c.rm[i], c.rv[i], c.gamma[i], c.beta[i], False, ub.MOMENTUM, ub.EPS))
                       for i in range(c.G)])
    back = ub.bwd_ref(c, st, 2, frozen=True)
    out.backward(back["dout"])
    torch.testing.assert_close(back["dy"][0], y.grad, rtol=1e-12, atol=1e-12)
    assert not back["k2"][0].any() and not back["k3"][0].any()


@pytest.mark.parametrize("p", [(BF, 3, 257, 64), (FP, 1, 3, 40), (BF, 1, 1, 8)], ids=_id)
def test_builders_add_back_up(p):
    c = ub.make_case(*p)
    s1, s2 = c.y.sum(1), (c.y * c.y).sum(1)
    for rb in (1, 129, 300, 1500):
        part, q1, q2 = ub.build_partials(c.y, c.y * c.y, rb)
        assert part.shape == (c.G, 2, c.C, rb) and part.dtype == torch.float32
        # each of the (at most M non-empty) partials was rounded once
        n = min(rb, c.M)
        assert bool(((q1 - s1).abs() <= n * ub.U * c.y.abs().sum(1)).all())
        assert bool(((q2 - s2).abs() <= n * ub.U * s2).all())
        assert torch.equal(part.to(F64).sum(3)[:, 0], q1)
    for fix in (ub.FWD_FIX, ub.BWD_FIX):
        for rep in (1, 3, 64):
            tot, q1, q2 = ub.build_totals(s1, s2, fix, rep)
            assert tot.shape == (rep, c.G, 2, c.C) and tot.dtype == torch.int64
            assert torch.equal(tot.sum(0)[:, 0], torch.round(s1 * fix).to(torch.int64))
            assert torch.equal(tot.sum(0)[:, 1], torch.round(s2 * fix).to(torch.int64))
            assert bool(((q1 - s1).abs() <= 0.5 / fix + 1e-15 * s1.abs()).all())
            assert rep == 1 or bool((tot < 0).any())


@pytest.mark.parametrize("p", ALL_CASES, ids=_id)
def test_kink_filter_stays_under_its_cap(p):
    c = ub.make_case(*p)
    st = ub.stats32(c)
    for mask_kind in (1, 2):
        kept = ub.bwd_ref(c, st, mask_kind, frozen=True)["kept"]
        assert (~kept).double().mean().item() <= ub.KINK_CAP


def _exceeds(a, b):
    """does the wrong reference a[name] leave the bound of the right one b[name] anywhere"""
    return any(bool(((a[k][0] - b[k][0]).abs() > b[k][1]).any()) for k in b if isinstance(b[k], tuple))


@pytest.mark.parametrize("mutate", ["unbiased", "swap_mom", "neighbour_chunk", "mask_y", "no_k3"])
def test_the_checker_has_teeth(mutate):
    hit = []
    for p in CASES:
        c = ub.make_case(*p)
        if mutate in ("unbiased", "swap_mom", "neighbour_chunk"):
            hit.append(_exceeds(ub.fwd_ref(c, mutate=mutate), ub.fwd_ref(c)))
        else:
            st = ub.stats32(c)
            hit.append(_exceeds(ub.bwd_ref(c, st, 2, mutate=mutate), ub.bwd_ref(c, st, 2)))
    assert any(hit)
    # ... and not by a hair: on most cases
    assert sum(hit) > len(hit) // 2


# the shapes of test_bn2d_fwd_bwd itself in both types, and every bf16 case of this file.  The fp32 tolerances of that test are
# absolute ones chosen at M >= 384: a worst-case bound cannot stay below them at fp32 with M <= 3 (a channel whose three
# samples lie close together has |y * scale| ~ 1e3, and 4 u of that is 2.8e-4 against 1e-4) nor for d(gamma) at fp32 C = 4,
# M = 1000 (a 261-link chain: 8.7e-3 against 5e-3 + 1e-3 |d(gamma)|), so those are not asserted here.
TODAY = [(t, G, M, C) for t in (FP, BF) for G, M, C in ((3, 1000, 64), (1, 515, 256), (3, 384, 2048), (2, 4096, 512))]


@pytest.mark.parametrize("p", TODAY + [p for p in ALL_CASES if p[0] == BF and p not in TODAY], ids=_id)
def test_bounds_are_no_looser_than_test_bn2d_fwd_bwd(p):
    """the tolerances of tests/test_kernels_gpu.py::test_bn2d_fwd_bwd, as atol + rtol * |reference|"""
    c = ub.make_case(*p)
    bf = c.dtype == BF
    fwd = ub.fwd_ref(c, residual=True, relu=True)
    bwd = ub.bwd_ref(c, ub.stats32(c), 1)
    today = {"out": (2e-2, 3e-2) if bf else (1e-4, 1e-4), "rm": (1e-4, 1e-5), "rv": (1e-4, 1e-5),
             "dy": (3e-2, 3e-2) if bf else (2e-4, 2e-4), "dgamma": (3e-2, 0.5) if bf else (1e-3, 5e-3),
             "dbeta": (3e-2, 0.5) if bf else (1e-3, 5e-3), "g": (1e-2, 1e-2) if bf else (1e-6, 1e-6)}
    loose = []
    for k, (rtol, atol) in today.items():
        ref, bound = (fwd if k in fwd else bwd)[k]
        if not bool((bound <= atol + rtol * ref.abs()).all()):
            loose.append("%s: bound up to %.3g against %.3g" % (k, float(bound.max()), float((atol + rtol * ref.abs()).min())))
    assert not loose, loose


def test_geometry_restatement():
    """the shapes of test_bn_forms_gpu.py select what its comments say they select"""
    g = ub.red_geom(270001, 64, 8)
    assert (g.rblocks, ub.finalize_lpc(g.rblocks)) == (768, 256)
    assert [ub.finalize_lpc(r) for r in (1, 129, 300, 1500)] == [32, 64, 128, 256]
    assert [ub.red_geom(M, 64, 8).rblocks for M in (20001, 40001)] == [157, 313]
    assert ub.ew_blocks(270001 * 8) == 8192 and 8192 * 256 < 270001 * 8 < 2 * 8192 * 256      # a second, ragged trip
    assert ub.tot_blocks(270001 * 8, 1) == 2048 and 4 * 2048 * 256 < 270001 * 8 < 5 * 2048 * 256
    assert max(ub.chain_length(M, C, v) for M in (1, 3, 257, 1000) for C, v in ((8, 8), (24, 8), (64, 8), (2048, 8), (4, 4),
                                                                                (40, 4), (2048, 4))) <= 267
    assert ub.chain_length(270001, 64, 8) == 43
    assert ub.red_geom(1000, 2048, 8).tx * 8 == 512
    ub.switched_shapes(2)
