"""The cross-modality interaction tail restated in float64, with an error budget for every quantity the position kernels of
ieee_amd/csrc/cim.hip produce (gpool_sum_others, ca_pool, cim_tail, cim_bwd_datt, cim_bwd_g, cim_bwd_combine), the case
builder, and the runners that tests/test_cim_forms_gpu.py calls.

The formulas are those of the kernels' header comments.  All maps are [3][B][P][C] (modality, sample, position h * W + w,
channel); scale / shift are fp32 values handed to the kernels as rows 2 and 3 of a [3][4][C] block (rows 0 and 1 are NaN:
nothing here runs a BatchNorm kernel).  Every backward kernel gets inputs built from the reference (att, argmax, d_avg,
d_max, dP), so a failure names one kernel.

Error budget (u = 2^-24; every bound is computed from the reference's own magnitudes, never from a device output):
  reductions   |err| <= n * u * sum|terms|.  n is the longest fp32 chain the geometry gives, from the restatement of
               pos_geom / row_block below -- positions per row + rows per lane + row lanes for the row-block kernels
               (chain_rows), positions per lane + row lanes for the strided pools (chain_pos), never more than the number of
               terms -- plus the roundings behind one term (N_* below, counted at each use).
  stored g     half an ulp of the stored type on the reference value + EW u on the sum of the absolute terms.
  BN sums      sums of the STORED gradient.  The fp32 value behind an element lies within delta = EW u sum|terms| of the
               reference g, and rounding is monotone, so the stored element lies in [round(g - delta), round(g + delta)]: where
               both ends equal round(g) the stored element is known exactly, elsewhere it may sit one step away.  The sums
               inherit these per-element bounds and add their own chain.
  exact        argmax; S = one fp32 add, one rounding; mode 2: g1 = the fp32 d_out, rounded once.
The ReLU pre-activations of every case are off the kink (|y * scale + shift| > 2^-18 (|y * scale| + |shift|)), so both sides
take the same mask decisions and no element is excluded anywhere; and a channel's maximum is either clear of every other value
by more than the rounding of the pre-activation or shared by bit-identical inputs, so the argmax is defined."""
import atexit
import functools
import json
import os
import types

import torch

U = 2.0 ** -24
KINK = 2.0 ** -18
F64 = torch.float64
BF, FP = torch.bfloat16, torch.float32
PARTS = 6
MAXS_MAX = 4
SENT = 123.0      # representable in bf16; no output of these cases comes near it
ISENT = -7
GUARD = 64
EW = 8            # roundings behind g2 = (sum of <= 3 (dP * inv)) * (1 + att) + davg * (1 / P) + dmax: 4 + 2 + 1 + 1
N_TERM = 9        # forward term: two pre-activations (2 each), 1 + att, the product, the add; 1 / count and its product
N_DATT = 7        # d (4), the pre-activation (2), d * row
N_POOL = 4        # the pre-activation (2), the division by P, one to spare for s / P formed as a product
TIE_TOL = 8 * U   # two pre-activations (2 u of their magnitude each) cannot be told apart within this

RATIOS = {}       # "kernel:quantity" -> largest err / bound seen (IEEE_CIM_RATIOS_FILE: written at exit)


def half_ulp(dtype):
    return 2.0 ** -8 if dtype == BF else U


def vec_of(dtype):
    return 8 if dtype == BF else 4


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the launch geometry of cim.hip, restated
def pos_geom(C, vec):
    cprw = C // vec
    tx = 1
    while tx * 2 <= 64 and cprw % (tx * 2) == 0:
        tx *= 2
    return types.SimpleNamespace(cprw=cprw, tx=tx, ty=256 // tx, cblocks=cprw // tx)


def bin_start(i, H, parts=PARTS):
    return (i * H) // parts


def bin_end(i, H, parts=PARTS):
    return ((i + 1) * H + parts - 1) // parts


def row_block(ty, tyn, H, parts=PARTS):
    """(r0, r1, first): the rows of row lane ty and the first bin that ends behind r0"""
    rpt = cdiv(H, tyn)
    r0 = min(ty * rpt, H)
    r1 = min(r0 + rpt, H)
    first = 0
    while first < parts and bin_end(first, H, parts) <= r0:
        first += 1
    return r0, r1, first


def row_block_bins(tyn, H, parts=PARTS):
    """the largest number of bins any row lane's rows meet"""
    worst = 0
    for ty in range(tyn):
        r0, r1, first = row_block(ty, tyn, H, parts)
        last = first - 1
        for i in range(first, parts):
            if bin_start(i, H, parts) < r1 and bin_end(i, H, parts) > r0:
                last = i
        if r1 > r0:
            worst = max(worst, last - first + 1)
    return worst


def maxs_of(dtype, H, C, parts=PARTS):
    """the MAXS the launchers pick (None: they refuse)"""
    n = row_block_bins(pos_geom(C, vec_of(dtype)).ty, H, parts)
    return None if n > MAXS_MAX else (2 if n <= 2 else 4)


def chain_rows(c):
    """row-block kernels: positions of a row, rows of a lane, row lanes"""
    ty = pos_geom(c.C, vec_of(c.dtype)).ty
    return c.W + cdiv(c.H, ty) + ty


def chain_pos(c):
    """strided pools: positions of a lane, row lanes"""
    ty = pos_geom(c.C, vec_of(c.dtype)).ty
    return cdiv(c.P, ty) + ty


def chain_bn(c):
    """BN sums of cim_bwd_g: all positions of a lane's rows in one chain, then the row lanes"""
    ty = pos_geom(c.C, vec_of(c.dtype)).ty
    return cdiv(c.H, ty) * c.W + ty


# ---- the cases of tests/test_cim_forms_gpu.py (shared with the CPU file, which checks the claims made here)
# map -> the MAXS the executor's geometry (C = 2048, four row lanes) selects
MAPS = {(2, 2): 4, (5, 3): 4, (10, 5): 4, (14, 14): 4, (7, 9): 4, (3, 3): 2, (12, 6): 2, (16, 8): 2, (24, 8): 2}
FULL_MAPS = ((14, 14), (16, 8))


def cells():
    """[(dtype, B, H, W, C, expected MAXS)]"""
    out = []
    for (H, W), m in MAPS.items():
        for dt in (FP, BF):
            out.append((dt, 3, H, W, 2048, m))
    for dt in (FP, BF):
        out.append((dt, 1, 2, 2, 2048, 4))
    # C = 256: four row lanes in fp32, eight in bf16 (two rows a lane at 10 and 16 rows: never more than two bins)
    for (H, W), m32, m16 in (((2, 2), 4, 4), ((10, 5), 4, 2), ((16, 8), 2, 2)):
        out.append((FP, 3, H, W, 256, m32))
        out.append((BF, 3, H, W, 256, m16))
    # beyond the executor: 128 / 256 row lanes, one row each at most, 5 / 3 channel blocks
    for H, W in ((5, 3), (16, 8)):
        out.append((FP, 3, H, W, 40, 2))
        out.append((BF, 3, H, W, 24, 2))
    return out


def cell_id(p):
    return "%s-C%d-%dx%d-B%d" % ("bf16" if p[0] == BF else "fp32", p[4], p[2], p[3], p[1])


# ---- cases
def _round_to(t, dtype):
    return t.to(dtype).to(F64)


def _off_kink(y, sc, sh, dtype):
    """nudge every y whose pre-activation lies on the ReLU kink one ulp of its type at a time, away from the kink"""
    scb, shb = sc[:, None, None, :], sh[:, None, None, :]
    ys = y * scb
    bad = (ys + shb).abs() <= KINK * (ys.abs() + shb.abs())
    idx = bad.reshape(-1).nonzero()[:, 0]
    if idx.numel() == 0:
        return y
    C = y.shape[3]
    z, ch = idx // (y.numel() // 3), idx % C
    s, h = sc[z, ch], sh[z, ch]
    v = y.reshape(-1)[idx].to(dtype)
    it = torch.int16 if dtype == BF else torch.int32
    for _ in range(256):
        v64 = v.to(F64)
        pre = v64 * s + h
        bad = pre.abs() <= KINK * ((v64 * s).abs() + h.abs())
        if not bool(bad.any()):
            break
        assert bool((v64[bad] != 0).all())
        up = torch.sign(pre) * torch.sign(s) >= 0         # the direction of y in which |pre| grows
        step = torch.where(up == (v64 > 0), 1, -1).to(it)   # one ulp: the magnitude's bit pattern + / - 1
        v = torch.where(bad, (v.view(it) + step).view(dtype), v)
    y = y.clone()
    y.reshape(-1)[idx] = v.to(F64)
    return y


def _acts(y, sc, sh):
    ys = y * sc[:, None, None, :]
    pre = ys + sh[:, None, None, :]
    return pre, ys.abs() + sh[:, None, None, :].abs()


def tie_positions(dtype, H, W, C):
    """(pA, pB), pA < pB, in different row lanes of ca_pool (lane = p mod ty); where the map has more positions than lanes the
    later position sits in lane 0, which the combine over the lanes visits first"""
    ty, P = pos_geom(C, vec_of(dtype)).ty, H * W
    return (1, ty) if ty < P else (1, P - 1)


def special_channels(C):
    """(zero channel, tie channel): in the last and in the first channel block"""
    return C - 2, 1


def _params(g, C, lo=0.05):
    sc = torch.rand(3, C, generator=g) + 0.5
    sc[:, ::5] *= -1
    sh = torch.randn(3, C, generator=g) * 0.3
    sh = torch.where(sh.abs() < lo, torch.full_like(sh, lo) * torch.sign(sh + 1e-9), sh)
    return sc.to(F64), sh.to(F64)


def near_ties(y2, sc2, sh2):
    """positions whose rest is within TIE_TOL of their channel's maximum without bit-identical input; and the inputs there"""
    pre, mag = _acts(y2, sc2, sh2)
    rest = pre.clamp_min(0)
    mx, am = rest.max(2, keepdim=True)
    ymax = torch.gather(y2, 2, am)
    near = (rest > 0) & (mx - rest <= TIE_TOL * mag.max(2, keepdim=True)[0]) & (y2 != ymax)
    return near, ymax


def make_data(dtype, B, H, W, C, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * C + 131 * H + W + 17 * B + (5 if dtype == BF else 0))
    rt = lambda t: _round_to(t, dtype)
    P = H * W
    c = types.SimpleNamespace(dtype=dtype, B=B, H=H, W=W, C=C, P=P, seed=seed, dev={})
    y1 = rt(torch.randn(3, B, P, C, generator=g) * 1.5 + 0.25)
    y2 = rt(torch.randn(3, B, P, C, generator=g) * 1.5 - 0.25)
    c.sc1, c.sh1 = _params(g, C)
    c.sc2, c.sh2 = _params(g, C)
    c.att = torch.rand(3, B, C, generator=g).to(F64)
    c.dP = torch.randn(3, B, PARTS, C, generator=g).to(F64)
    c.davg = torch.randn(3, B, C, generator=g).to(F64)
    c.dmax = torch.randn(3, B, C, generator=g).to(F64)
    c.dG = torch.randn(3, B, C, generator=g).to(F64)
    cz, ct = special_channels(C)
    pA, pB = tie_positions(dtype, H, W, C)
    # rest = 0 everywhere: scale 1, shift -1/4, y2 <= -1
    c.sc2[:, cz], c.sh2[:, cz] = 1.0, -0.25
    y2[:, :, :, cz] = rt(-y2[:, :, :, cz].abs() - 1.0)
    # the maximum at pA and at pB: scale 1, one value clear of all the others
    c.sc2[:, ct], c.sh2[:, ct] = 1.0, 0.125
    top = rt(y2[:, :, :, ct].max(2)[0] + 1.0)
    y2[:, :, pA, ct] = top
    y2[:, :, pB, ct] = top
    y1 = _off_kink(y1, c.sc1, c.sh1, dtype)
    y2 = _off_kink(y2, c.sc2, c.sh2, dtype)
    near, ymax = near_ties(y2, c.sc2, c.sh2)
    c.y1, c.y2 = y1, torch.where(near, ymax, y2)
    return c


@functools.lru_cache(maxsize=2)
def cached_data(dtype, B, H, W, C, seed=0):
    return make_data(dtype, B, H, W, C, seed)


def make_case(dtype, B, H, W, C, mode, seed=0):
    """the data do not depend on the mode (one set is shared by every form run at a cell); the mode selects the formulas"""
    c = cached_data(dtype, B, H, W, C, seed)
    return types.SimpleNamespace(**dict(vars(c), mode=mode))


def builder_facts(c):
    """what the builder guarantees, measured (the CPU file asserts it at every cell)"""
    pre1, mag1 = _acts(c.y1, c.sc1, c.sh1)
    pre2, mag2 = _acts(c.y2, c.sc2, c.sh2)
    cz, ct = special_channels(c.C)
    pA, pB = tie_positions(c.dtype, c.H, c.W, c.C)
    rest = pre2.clamp_min(0)
    ty = pos_geom(c.C, vec_of(c.dtype)).ty
    maps = [c.y1, c.y2]
    return types.SimpleNamespace(
        kink=int((pre1.abs() <= KINK * mag1).sum() + (pre2.abs() <= KINK * mag2).sum()),
        near=int(near_ties(c.y2, c.sc2, c.sh2)[0].sum()),
        zero_channel=bool((rest[..., cz] == 0).all()),
        tie_channel=bool((rest[:, :, pA, ct] == rest[..., ct].max(2)[0]).all() and (rest[:, :, pB, ct] == rest[:, :, pA, ct]).all()
                         and pA < pB and pA % ty != pB % ty and bool((rest[:, :, pA, ct] > 0).all())),
        exact=all(torch.equal(_round_to(t, c.dtype), t) for t in maps)
        and all(torch.equal(t.to(FP).to(F64), t) for t in (c.sc1, c.sh1, c.sc2, c.sh2, c.att, c.dP, c.davg, c.dmax, c.dG)))


# ---- the reference
def row_weights(c, mutate=None):
    """[parts][H]: 1 / (rows of bin i * W) where row h lies in bin i = [floor(i H / parts), ceil((i + 1) H / parts))"""
    wt = torch.zeros(PARTS, c.H, dtype=F64)
    for i in range(PARTS):
        s, e = bin_start(i, c.H), bin_end(i, c.H)
        if mutate == "floor_end":
            e = ((i + 1) * c.H) // PARTS
        if e > s:
            wt[i, s:e] = 1.0 / (c.H / PARTS * c.W) if mutate == "bin_div" else 1.0 / ((e - s) * c.W)
    return wt


def _rows(c, t):
    return t.reshape(3, c.B, c.H, c.W, c.C).sum(3)


def _per_pos(c, t):
    """[3][B][H][C] -> [3][B][P][C]: a row's value at each of its positions"""
    return t[:, :, :, None, :].expand(3, c.B, c.H, c.W, c.C).reshape(3, c.B, c.P, c.C)


def fwd_ref(c, mutate=None):
    """(parts [3][B][6][C], bound)"""
    if c.mode == 2:
        out, tmag = c.y1, c.y1.abs()
    else:
        pre1, mag1 = _acts(c.y1, c.sc1, c.sh1)
        pre2, mag2 = _acts(c.y2, c.sc2, c.sh2)
        a = 1.0 + c.att[:, :, None, :] if c.mode == 0 else 1.0
        out = pre1.clamp_min(0) + pre2.clamp_min(0) * a
        tmag = mag1 * (pre1 > 0) + mag2 * (pre2 > 0) * a
    parts = torch.einsum("ih,zbhc->zbic", row_weights(c, mutate), _rows(c, out))
    n = torch.tensor([min(chain_rows(c), (bin_end(i, c.H) - bin_start(i, c.H)) * c.W) + N_TERM for i in range(PARTS)], dtype=F64)
    bound = torch.einsum("ih,zbhc->zbic", row_weights(c), _rows(c, tmag)) * n[None, None, :, None] * U
    if mutate == "cb_shift":      # channel block cb written to slot cb + 1
        parts = torch.roll(parts, pos_geom(c.C, vec_of(c.dtype)).tx * vec_of(c.dtype), 3)
    return parts, bound


def pool_ref(c, mutate=None):
    """avg, max (value, bound) [3][B][C] and the first-occurrence argmax of rest = relu(y2 * scale2 + shift2)"""
    pre, mag = _acts(c.y2, c.sc2, c.sh2)
    rest = pre.clamp_min(0)
    n = min(chain_pos(c), c.P) + N_POOL
    avg = rest.sum(2) / c.P
    davg = n * U * (mag * (pre > 0)).sum(2) / c.P
    mx = rest.max(2)[0]
    dmx = 2 * U * mag.max(2)[0]       # every candidate carries the two roundings of its pre-activation
    pos = torch.arange(c.P)[None, None, :, None]
    hit = rest == mx[:, :, None, :]
    if mutate == "last_argmax":
        am = torch.where(hit, pos, torch.full_like(pos, -1)).max(2)[0]
    else:
        am = torch.where(hit, pos, torch.full_like(pos, c.P)).min(2)[0]
    return types.SimpleNamespace(avg=(avg, davg), max=(mx, dmx), argmax=am.to(torch.int32), rest=rest, mag=mag, on=pre > 0)


def dout_ref(c):
    """d_out of a row [3][B][H][C], the sum of its absolute terms, and the fp32 evaluation the kernels make of it (terms dP *
    (1 / count) in bin order, each product and each addition rounded once)"""
    wt = row_weights(c)
    d = torch.einsum("ih,zbic->zbhc", wt, c.dP)
    dabs = torch.einsum("ih,zbic->zbhc", wt, c.dP.abs())
    d32 = torch.zeros(3, c.B, c.H, c.C, dtype=FP)
    dP32 = c.dP.to(FP)
    for i in range(PARTS):
        s, e = bin_start(i, c.H), bin_end(i, c.H)
        inv = torch.tensor(1.0, dtype=FP) / torch.tensor(float((e - s) * c.W), dtype=FP)
        d32[:, :, s:e] = d32[:, :, s:e] + (dP32[:, :, i] * inv)[:, :, None, :]
    return d, dabs, d32


def datt_ref(c):
    """d_att [3][B][C] = sum over positions of d_out * rest"""
    p = pool_ref(c)
    d, dabs, _ = dout_ref(c)
    n = min(chain_rows(c), c.P) + N_DATT
    return (_per_pos(c, d) * p.rest).sum(2), n * U * (_per_pos(c, dabs) * p.mag * p.on).sum(2)


def _stored(c, g, delta):
    """the stored gradient as far as the reference knows it: round(g), and how far the device's element may sit from it"""
    s = _round_to(g, c.dtype)
    lo, hi = _round_to(g - delta, c.dtype), _round_to(g + delta, c.dtype)
    return s, torch.maximum(hi - s, s - lo)


def _bn_sums(c, g, delta, y, mutate):
    s, eb = (g, torch.zeros_like(g)) if mutate == "unrounded_sums" else _stored(c, g, delta)
    n = min(chain_bn(c), c.P)
    mag = s.abs() + eb
    s1, b1 = s.sum(2), eb.sum(2) + n * U * mag.sum(2)
    s2, b2 = (s * y).sum(2), (eb * y.abs()).sum(2) + (n + 1) * U * (mag * y.abs()).sum(2)
    # [3][2][C][B]: the sample index innermost
    return torch.stack([s1, s2], 1).permute(0, 1, 3, 2).contiguous(), torch.stack([b1, b2], 1).permute(0, 1, 3, 2).contiguous()


def g_ref(c, mutate=None):
    """g1, g2 (value, bound) [3][B][P][C], bn1, bn2 (value, bound) [3][2][C][B], and in mode 2 g1_bits: the exact stored g1"""
    hu = half_ulp(c.dtype)
    d, dabs, d32 = dout_ref(c)
    d, dabs = _per_pos(c, d), _per_pos(c, dabs)
    r = types.SimpleNamespace(g2=None, bn1=None, bn2=None, g1_bits=None)
    if c.mode == 2:
        delta = 4 * U * dabs
        r.g1 = (d, hu * (d.abs() + delta) + delta)
        r.g1_bits = _per_pos(c, d32).to(c.dtype)
        return r
    pre1, _ = _acts(c.y1, c.sc1, c.sh1)
    pre2, _ = _acts(c.y2, c.sc2, c.sh2)
    g1 = torch.where(pre1 > 0, d, torch.zeros_like(d))
    t1 = dabs * (pre1 > 0)
    if c.mode == 0:
        a = 1.0 + c.att[:, :, None, :]
        hit = torch.arange(c.P)[None, None, :, None] == pool_ref(c).argmax[:, :, None, :]
        tv = (d if mutate == "no_att" else d * a) + c.davg[:, :, None, :] / c.P + hit * c.dmax[:, :, None, :]
        terms = dabs * a + c.davg[:, :, None, :].abs() / c.P + hit * c.dmax[:, :, None, :].abs()
    else:
        tv, terms = d, dabs
    g2 = torch.where(pre2 > 0, tv, torch.zeros_like(tv))
    t2 = terms * (pre2 > 0)
    for name, g, t, y in (("1", g1, t1, c.y1), ("2", g2, t2, c.y2)):
        delta = EW * U * t
        setattr(r, "g" + name, (g, hu * (g.abs() + delta) + delta))
        setattr(r, "bn" + name, _bn_sums(c, g, delta, y, mutate))
    return r


def gpool_ref(c):
    """G_m = mean over positions of F_m (value, bound) [3][B][C]; S_m = F_a + F_b as the kernel forms it: one fp32 add, one
    rounding to the stored type"""
    Fm = c.y1
    n = min(chain_pos(c), c.P) + 2
    F32 = Fm.to(FP)
    S = torch.stack([(F32[(m + 1) % 3] + F32[(m + 2) % 3]).to(c.dtype) for m in range(3)])
    return (Fm.sum(2) / c.P, n * U * Fm.abs().sum(2) / c.P), S, torch.stack([Fm[(m + 1) % 3] + Fm[(m + 2) % 3] for m in range(3)])


def combine_ref(c):
    """dF_m = D1_m + dG_m / P (+ DS_a + DS_b unless mode 2) (value, bound) [3][B][P][C]; D1 = y1, DS = y2 of the case"""
    D1, DS = c.y1, c.y2
    x = D1 + c.dG[:, :, None, :] / c.P
    terms = D1.abs() + c.dG[:, :, None, :].abs() / c.P
    if c.mode != 2:
        x = x + torch.stack([DS[(m + 1) % 3] + DS[(m + 2) % 3] for m in range(3)])
        terms = terms + torch.stack([DS[(m + 1) % 3].abs() + DS[(m + 2) % 3].abs() for m in range(3)])
    delta = 6 * U * terms      # 1 / P, its product, three additions, one to spare
    return x, half_ulp(c.dtype) * (x.abs() + delta) + delta


# ---- comparison
def compare(fails, tag, name, dev, ref, bound):
    dev = dev.detach().to(F64).cpu().reshape(ref.shape)
    bound = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    bound = bound.expand_as(ref)
    err = (dev - ref).abs()
    ok = err <= bound                      # NaN fails
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                               torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = tag.split("[")[0] + ":" + name
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    if not bool(ok.all()):
        i = int(ratio.reshape(-1).argmax())
        fails.append("%s %s: %d of %d beyond the bound; worst at flat index %d: device %.9g reference %.9g bound %.3g (x%.3g)"
                     % (tag, name, int((~ok).sum()), ok.numel(), i, float(dev.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                        float(bound.reshape(-1)[i]), worst))


def exact(fails, tag, name, dev, want):
    dev = dev.detach().cpu().reshape(want.shape)
    if not torch.equal(dev, want):
        bad = (dev != want).reshape(-1)
        i = int(bad.to(torch.int32).argmax())
        fails.append("%s %s: %d of %d differ; first at flat index %d: device %s, wanted %s"
                     % (tag, name, int(bad.sum()), bad.numel(), i, dev.reshape(-1)[i].item(), want.reshape(-1)[i].item()))


def _dump_ratios():
    path = os.environ.get("IEEE_CIM_RATIOS_FILE")
    if path and RATIOS:
        old = {}
        if os.path.exists(path):
            old = json.load(open(path))
        for k, v in RATIOS.items():
            old[k] = max(old.get(k, 0.0), v)
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)


atexit.register(_dump_ratios)


# ---- device side: the C ABI as the executor calls it
DEV = "cuda"


class Out(object):
    """an output prefilled with a sentinel, with a guard of GUARD sentinel elements behind it"""

    def __init__(self, shape, dtype, sent=SENT):
        self.shape, self.sent = tuple(shape), sent
        self.n = 1
        for s in self.shape:
            self.n *= s
        self.flat = torch.full((self.n + GUARD,), sent, dtype=dtype, device=DEV)

    @property
    def t(self):
        return self.flat[:self.n].view(self.shape)

    def check(self, fails, tag, name, written=True):
        if not bool((self.flat[self.n:] == self.sent).all()):
            fails.append("%s %s: the guard behind the output was written" % (tag, name))
        left = int((self.flat[:self.n] == self.sent).sum())
        if written and left:
            fails.append("%s %s: %d of %d elements were not written" % (tag, name, left, self.n))
        if not written and left != self.n:
            fails.append("%s %s: %d elements written although the call must leave it alone" % (tag, name, self.n - left))


def tdt(L, c):
    return L.IEEE_BF16 if c.dtype == BF else L.IEEE_F32


def stats_block(sc, sh):
    """[3][4][C] fp32 with NaN in the rows the kernels must not read"""
    st = torch.full((3, 4, sc.shape[1]), float("nan"), dtype=FP)
    st[:, 2], st[:, 3] = sc.to(FP), sh.to(FP)
    return st


def _d(c, name):
    """the device copy of an input (kept with the cached data)"""
    if name not in c.dev:
        if name in ("y1", "y2"):
            t = getattr(c, name).to(c.dtype)
        elif name == "st1":
            t = stats_block(c.sc1, c.sh1)
        elif name == "st2":
            t = stats_block(c.sc2, c.sh2)
        elif name == "argmax":
            t = pool_ref(c).argmax
        elif name == "davgmax":      # [3][2B][C]: d_avg in front of d_max, as the executor keeps them
            t = torch.cat([c.davg, c.dmax], 1).to(FP)
        else:
            t = getattr(c, name).to(FP)
        c.dev[name] = t.contiguous().to(DEV)
    return c.dev[name]


def _off(L, t, elems):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def run_tail_fwd(L, lib, c, tag):
    fails = []
    ref, bound = fwd_ref(c)
    Pp = Out((3, c.B, PARTS, c.C), FP)
    L.check(lib.ieee_cim_tail_fwd(L.ptr(_d(c, "y1")), L.ptr(_d(c, "y2")), L.ptr(_d(c, "st1")), L.ptr(_d(c, "st2")),
                                  L.ptr(_d(c, "att")), L.ptr(Pp.t), tdt(L, c), c.B, c.H, c.W, c.C, PARTS, c.mode, L.stream()))
    torch.cuda.synchronize()
    Pp.check(fails, tag, "parts")
    compare(fails, tag, "parts", Pp.t, ref, bound)
    return fails


def run_ca_pool(L, lib, c, tag):
    fails = []
    r = pool_ref(c)
    B, C = c.B, c.C
    am = Out((3, B, C), torch.int32, ISENT)
    avgmax = Out((3, 2 * B, C), FP)
    L.check(lib.ieee_ca_pool(L.ptr(_d(c, "y2")), L.ptr(_d(c, "st2")), L.ptr(avgmax.t), _off(L, avgmax.t, B * C), 2 * B * C,
                             L.ptr(am.t), tdt(L, c), B, c.H, c.W, C, L.stream()))
    torch.cuda.synchronize()
    am.check(fails, tag, "argmax")
    avgmax.check(fails, tag, "avg / max")
    compare(fails, tag, "avg", avgmax.t[:, :B], *r.avg)
    compare(fails, tag, "max", avgmax.t[:, B:], *r.max)
    exact(fails, tag, "argmax", am.t, r.argmax)
    return fails


def run_datt(L, lib, c, tag):
    fails = []
    ref, bound = datt_ref(c)
    datt = Out((3, c.B, c.C), FP)
    L.check(lib.ieee_cim_tail_bwd_datt(L.ptr(_d(c, "dP")), L.ptr(_d(c, "y2")), L.ptr(_d(c, "st2")), L.ptr(datt.t), tdt(L, c),
                                       c.B, c.H, c.W, c.C, PARTS, L.stream()))
    torch.cuda.synchronize()
    datt.check(fails, tag, "datt")
    compare(fails, tag, "datt", datt.t, ref, bound)
    return fails


def run_bwd_g(L, lib, c, tag, partials=True):
    fails = []
    r = g_ref(c)
    B, C = c.B, c.C
    g1, g2 = Out((3, B, c.P, C), c.dtype), Out((3, B, c.P, C), c.dtype)
    bp1, bp2 = Out((3, 2, C, B), FP), Out((3, 2, C, B), FP)
    dam = _d(c, "davgmax")
    L.check(lib.ieee_cim_tail_bwd_g(L.ptr(_d(c, "dP")), L.ptr(_d(c, "y1")), L.ptr(_d(c, "y2")), L.ptr(_d(c, "st1")),
                                    L.ptr(_d(c, "st2")), L.ptr(_d(c, "att")), L.ptr(dam), _off(L, dam, B * C), 2 * B * C,
                                    L.ptr(_d(c, "argmax")), L.ptr(g1.t), L.ptr(g2.t), tdt(L, c), B, c.H, c.W, C, PARTS, c.mode,
                                    L.ptr(bp1.t) if partials else None, L.ptr(bp2.t) if partials else None, L.stream()))
    torch.cuda.synchronize()
    g1.check(fails, tag, "g1")
    g2.check(fails, tag, "g2", written=c.mode != 2)
    sums = partials and c.mode != 2
    bp1.check(fails, tag, "bn1", written=sums)
    bp2.check(fails, tag, "bn2", written=sums)
    compare(fails, tag, "g1", g1.t, *r.g1)
    if c.mode == 2:
        exact(fails, tag, "g1 = rounded d_out", g1.t, r.g1_bits)
    else:
        compare(fails, tag, "g2", g2.t, *r.g2)
    if sums:
        for k, bp, ref in (("1", bp1, r.bn1), ("2", bp2, r.bn2)):
            compare(fails, tag, "bn%s_sum_g" % k, bp.t[:, 0], ref[0][:, 0], ref[1][:, 0])
            compare(fails, tag, "bn%s_sum_gy" % k, bp.t[:, 1], ref[0][:, 1], ref[1][:, 1])
    return fails


def run_gpool(L, lib, c, tag, write_s=True):
    fails = []
    (G, dG), S, _ = gpool_ref(c)
    Sd = Out((3, c.B, c.P, c.C), c.dtype)
    Gp = Out((3, c.B, c.C), FP)
    L.check(lib.ieee_gpool_sum_others(L.ptr(_d(c, "y1")), L.ptr(Sd.t) if write_s else None, L.ptr(Gp.t), tdt(L, c), c.B, c.H, c.W,
                                      c.C, L.stream()))
    torch.cuda.synchronize()
    Gp.check(fails, tag, "G")
    Sd.check(fails, tag, "S", written=write_s)
    compare(fails, tag, "G", Gp.t, G, dG)
    if write_s:
        exact(fails, tag, "S", Sd.t, S)
    return fails


def run_combine(L, lib, c, tag):
    fails = []
    ref, bound = combine_ref(c)
    dF = Out((3, c.B, c.P, c.C), c.dtype)
    L.check(lib.ieee_cim_bwd_combine(L.ptr(_d(c, "y1")), L.ptr(_d(c, "y2")), L.ptr(_d(c, "dG")), L.ptr(dF.t), tdt(L, c), c.B, c.H,
                                     c.W, c.C, c.mode, L.stream()))
    torch.cuda.synchronize()
    dF.check(fails, tag, "dF")
    compare(fails, tag, "dF", dF.t, ref, bound)
    return fails


# form name -> (runner, mode, options)
FORMS = {
    "fwd-m0": (run_tail_fwd, 0, {}), "fwd-m1": (run_tail_fwd, 1, {}), "fwd-m2": (run_tail_fwd, 2, {}),
    "datt": (run_datt, 0, {}),
    "g-m0-bn": (run_bwd_g, 0, dict(partials=True)), "g-m0-nobn": (run_bwd_g, 0, dict(partials=False)),
    "g-m1-bn": (run_bwd_g, 1, dict(partials=True)), "g-m1-nobn": (run_bwd_g, 1, dict(partials=False)),
    "g-m2-bn": (run_bwd_g, 2, dict(partials=True)), "g-m2-nobn": (run_bwd_g, 2, dict(partials=False)),
    "ca_pool": (run_ca_pool, 0, {}),
    "gpool-s": (run_gpool, 0, dict(write_s=True)), "gpool-nos": (run_gpool, 0, dict(write_s=False)),
    "combine-m0": (run_combine, 0, {}), "combine-m2": (run_combine, 2, {}),
}
EVERYWHERE = ("fwd-m0", "g-m0-bn")


def spread():
    """[(cell, form)]: every form at FULL_MAPS with C = 2048; elsewhere the tail forward and bwd_g in mode 0 and two of the
    other forms, cycling through them"""
    rest = [f for f in FORMS if f not in EVERYWHERE]
    out, j = [], 0
    for p in cells():
        if (p[2], p[3]) in FULL_MAPS and p[4] == 2048:
            out += [(p, f) for f in FORMS]
            continue
        out += [(p, f) for f in EVERYWHERE]
        out += [(p, rest[(2 * j) % len(rest)]), (p, rest[(2 * j + 1) % len(rest)])]
        j += 1
    return out


def run_form(L, lib, p, form):
    runner, mode, opt = FORMS[form]
    c = make_case(p[0], p[1], p[2], p[3], p[4], mode)
    tag = "%s.%s[%s-%s]" % (runner.__name__[4:], "bf16" if p[0] == BF else "fp32", cell_id(p), form)
    return runner(L, lib, c, tag, **opt)
