"""tests/util_cim.py on its own: the float64 restatement of the cross-modality interaction tail against float64 autograd
through torch's adaptive pools (torch's own bins are the authority for the bin formula, which the restatement shares with the
kernels), the restated launch geometry and what each case of tests/test_cim_forms_gpu.py selects, the builder's guarantees,
and the teeth of the error budget (pure CPU)."""
import pytest
import torch
import torch.nn.functional as F

from tests import util_cim as uc

BF, FP, F64 = uc.BF, uc.FP, uc.F64
TOL = dict(rtol=1e-12, atol=1e-12)
SMALL = [p for p in uc.cells() if p[4] <= 256]


def _nchw(c, t):
    return t.reshape(c.B, c.H, c.W, c.C).permute(0, 3, 1, 2)


def _flat(c, t):
    return t.permute(0, 2, 3, 1).reshape(c.B, c.P, c.C)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("hw", list(uc.MAPS), ids=lambda hw: "%dx%d" % hw)
def test_restatement_equals_float64_autograd(hw, mode):
    data = uc.make_data(FP, 2, hw[0], hw[1], 8, seed=mode)
    c = uc.types.SimpleNamespace(**dict(vars(data), mode=mode))
    parts, _ = uc.fwd_ref(c)
    pool = uc.pool_ref(c)
    g = uc.g_ref(c)
    datt, _ = uc.datt_ref(c)
    for z in range(3):
        y1, y2 = c.y1[z].clone().requires_grad_(True), c.y2[z].clone().requires_grad_(True)
        att = c.att[z].clone().requires_grad_(True)
        per_c = lambda v: v[z][None, :, None, None]
        pre1 = _nchw(c, y1) * per_c(c.sc1) + per_c(c.sh1)
        pre2 = _nchw(c, y2) * per_c(c.sc2) + per_c(c.sh2)
        pre1.retain_grad()
        pre2.retain_grad()
        one, rest = F.relu(pre1), F.relu(pre2)
        avg = F.adaptive_avg_pool2d(rest, 1)[..., 0, 0]
        mx, idx = F.adaptive_max_pool2d(rest, 1, return_indices=True)
        if mode == 0:
            out = one + rest * (1 + att[:, :, None, None])
        elif mode == 1:
            out = one + rest
        else:
            out = _nchw(c, y1)
        got = F.adaptive_avg_pool2d(out, (uc.PARTS, 1))[..., 0].permute(0, 2, 1)
        loss = (got * c.dP[z]).sum()
        if mode == 0:
            loss = loss + (avg * c.davg[z]).sum() + (mx[..., 0, 0] * c.dmax[z]).sum()
        loss.backward()
        torch.testing.assert_close(parts[z], got.detach(), **TOL)
        torch.testing.assert_close(pool.avg[0][z], avg.detach(), **TOL)
        torch.testing.assert_close(pool.max[0][z], mx.detach()[..., 0, 0], **TOL)
        # where the maximum is unique torch's index is the argmax; where it is shared the rule is ours (checked below)
        unique = (pool.rest[z] == pool.max[0][z][:, None, :]).sum(1) == 1
        assert torch.equal(pool.argmax[z][unique].long(), idx[..., 0, 0][unique])
        if mode == 2:
            torch.testing.assert_close(g.g1[0][z], y1.grad, **TOL)
            assert g.g2 is None and g.bn1 is None
            # the fp32 evaluation of d_out stands within its own budget of the float64 one
            assert bool(((g.g1_bits.to(F64) - g.g1[0]).abs() <= g.g1[1]).all())
            continue
        torch.testing.assert_close(g.g1[0][z], _flat(c, pre1.grad), **TOL)
        torch.testing.assert_close(g.g2[0][z], _flat(c, pre2.grad), **TOL)
        if mode == 0:
            torch.testing.assert_close(datt[z], att.grad, **TOL)
    if mode != 2:     # fp32 case: the stored gradient is the fp32 rounding of g; the sums lie [3][2][C][B]
        for (s, b), (gg, _), y in ((g.bn1, g.g1, c.y1), (g.bn2, g.g2, c.y2)):
            st = gg.to(FP).to(F64)
            torch.testing.assert_close(s[:, 0], st.sum(2).permute(0, 2, 1), **TOL)
            torch.testing.assert_close(s[:, 1], (st * y).sum(2).permute(0, 2, 1), **TOL)
            assert s.shape == (3, 2, c.C, c.B) and bool((b >= 0).all())


def test_argmax_rule_and_special_channels():
    """first occurrence where the maximum is shared; argmax 0 and no gradient where rest is zero everywhere"""
    for dt, C in ((FP, 8), (BF, 16), (FP, 2048)):
        c = uc.make_case(dt, 2, 5, 3, C, 0)
        pool, g = uc.pool_ref(c), uc.g_ref(c)
        cz, ct = uc.special_channels(C)
        pA, pB = uc.tie_positions(dt, 5, 3, C)
        assert bool((pool.argmax[..., ct] == pA).all()) and bool((uc.pool_ref(c, "last_argmax").argmax[..., ct] == pB).all())
        assert bool((pool.argmax[..., cz] == 0).all()) and bool((pool.max[0][..., cz] == 0).all())
        assert bool((g.g2[0][..., cz] == 0).all()) and bool((g.g2[1][..., cz] == 0).all())
        assert bool((g.bn2[0][:, :, cz] == 0).all()) and bool((g.bn2[1][:, :, cz] == 0).all())


@pytest.mark.parametrize("hw", [(2, 2), (7, 9), (16, 8)], ids=lambda hw: "%dx%d" % hw)
def test_gpool_and_combine_equal_float64_autograd(hw):
    for mode in (0, 2):
        c = uc.make_case(BF, 2, hw[0], hw[1], 16, mode)
        Fm = c.y1.clone().requires_grad_(True)
        S = torch.stack([Fm[(m + 1) % 3] + Fm[(m + 2) % 3] for m in range(3)])
        G = torch.stack([_nchw(c, Fm[m]).mean((2, 3)) for m in range(3)])
        loss = (G * c.dG).sum() + (Fm * c.y1).sum()        # D1 = y1, DS = y2
        if mode == 0:
            loss = loss + (S * c.y2).sum()
        loss.backward()
        (Gr, _), S_bits, S64 = uc.gpool_ref(c)
        torch.testing.assert_close(Gr, G.detach(), **TOL)
        torch.testing.assert_close(S64, S.detach(), **TOL)
        assert torch.equal(S_bits, S.detach().to(BF))      # bf16 + bf16 is exact in float64: one rounding
        torch.testing.assert_close(uc.combine_ref(c)[0], Fm.grad, **TOL)


def test_geometry_restatement():
    """pos_geom, row_block and row_block_bins restated: every claim the GPU file's case table makes"""
    geom = lambda dt, C: (lambda g: (g.cprw, g.tx, g.ty, g.cblocks))(uc.pos_geom(C, uc.vec_of(dt)))
    assert geom(FP, 2048) == (512, 64, 4, 8) and geom(BF, 2048) == (256, 64, 4, 4)
    assert geom(FP, 256) == (64, 64, 4, 1) and geom(BF, 256) == (32, 32, 8, 1)
    assert geom(FP, 40) == (10, 2, 128, 5) and geom(BF, 24) == (3, 1, 256, 3)
    # four row lanes: three bins (MAXS = 4) / two bins (MAXS = 2) at these map heights; one row: all six, refused
    assert all(uc.row_block_bins(4, H) == 3 for H in (2, 5, 7, 10, 11, 13, 14, 15, 17))
    assert all(uc.row_block_bins(4, H) == 2 for H in (3, 4, 6, 8, 9, 12, 16, 20, 24))
    assert uc.row_block_bins(4, 1) == 6 and all(uc.maxs_of(dt, 1, C) is None for dt, C in ((FP, 2048), (BF, 2048), (FP, 40), (BF, 24)))
    for (H, W), m in uc.MAPS.items():
        assert uc.maxs_of(FP, H, 2048) == m and uc.maxs_of(BF, H, 2048) == m
    for p in uc.cells():
        assert uc.maxs_of(p[0], p[2], p[4]) == p[5], uc.cell_id(p)
    rows = lambda H: [r1 - r0 for r0, r1, _ in (uc.row_block(t, 4, H) for t in range(4))]
    assert rows(2) == [1, 1, 0, 0] and rows(5) == [2, 2, 1, 0]
    bins = lambda H: [(uc.bin_start(i, H), uc.bin_end(i, H)) for i in range(6)]
    assert bins(2) == [(0, 1)] * 3 + [(1, 2)] * 3                                       # three coinciding bins per row
    assert bins(3) == [(0, 1), (0, 1), (1, 2), (1, 2), (2, 3), (2, 3)]                  # coinciding pairwise
    assert all(bins(H) == [(i * H // 6, (i + 1) * H // 6) for i in range(6)] for H in (12, 24))   # no overlap
    # load batches: 4 positions in the forward, 8 in the two backward kernels
    assert (5 % 4, 14 % 4, 14 % 8, 9 % 8) == (1, 2, 6, 1) and 2 < 4 and 3 < 4
    # the combine launch runs 2048 workgroups of 256 threads: B = 9 at 16 x 8, fp32 C = 2048 leaves a second, ragged trip
    chunks = 9 * 128 * 2048 // 4
    assert chunks == 589824 and 2048 * 256 < chunks < 2 * 2048 * 256
    # eight row lanes at a two-row map: six of them have no rows
    assert sum(1 for t in range(8) if uc.row_block(t, 8, 2)[0] == uc.row_block(t, 8, 2)[1]) == 6


def test_the_cases_reach_every_instantiation():
    """cim_tail_kernel, cim_bwd_datt_kernel and cim_bwd_g_kernel (all three modes) with T in {float, bf16} and MAXS in {2, 4}"""
    seen = set()
    for p, form in uc.spread():
        runner, mode, _ = uc.FORMS[form]
        seen.add((runner.__name__, mode, p[0], uc.maxs_of(p[0], p[2], p[4])))
    for dt in (FP, BF):
        for m in (2, 4):
            assert ("run_datt", 0, dt, m) in seen
            for mode in (0, 1, 2):
                assert ("run_tail_fwd", mode, dt, m) in seen and ("run_bwd_g", mode, dt, m) in seen
    cellforms = {}
    for p, form in uc.spread():
        cellforms.setdefault(p, set()).add(form)
    assert set(cellforms) == set(uc.cells())
    for p, forms in cellforms.items():
        assert set(uc.EVERYWHERE) <= forms
        if (p[2], p[3]) in uc.FULL_MAPS and p[4] == 2048:
            assert forms == set(uc.FORMS)
    for form in uc.FORMS:       # and every form away from the two full maps as well
        assert any(f == form and (p[2], p[3]) not in uc.FULL_MAPS for p, f in uc.spread()), form


@pytest.mark.parametrize("p", uc.cells() + [(FP, 9, 16, 8, 2048, 2)], ids=uc.cell_id)
def test_builder_guarantees(p):
    f = uc.builder_facts(uc.cached_data(*p[:5]))
    assert f.kink == 0 and f.near == 0
    assert f.zero_channel and f.tie_channel
    assert f.exact


def _beyond(a, ref):
    return bool(((a - ref[0]).abs() > ref[1]).any())


@pytest.mark.parametrize("mutate", ["floor_end", "bin_div", "no_att", "last_argmax", "unrounded_sums", "cb_shift"])
def test_the_checker_has_teeth(mutate):
    hit = []
    for p in SMALL:
        c = uc.make_case(p[0], p[1], p[2], p[3], p[4], 0)
        if mutate in ("floor_end", "bin_div", "cb_shift"):
            hit.append(_beyond(uc.fwd_ref(c, mutate)[0], uc.fwd_ref(c)))
        elif mutate == "last_argmax":
            hit.append(not torch.equal(uc.pool_ref(c, mutate).argmax, uc.pool_ref(c).argmax))
        elif mutate == "no_att":
            hit.append(_beyond(uc.g_ref(c, mutate).g2[0], uc.g_ref(c).g2))
        elif p[0] == BF:
            a, b = uc.g_ref(c, mutate), uc.g_ref(c)
            hit.append(_beyond(a.bn1[0], b.bn1) or _beyond(a.bn2[0], b.bn2))
    assert any(hit)
    if mutate not in ("floor_end", "bin_div", "cb_shift"):     # (bins that do not overlap and a single channel block hide those)
        assert all(hit)
