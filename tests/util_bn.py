"""BatchNorm2d (+ReLU, +residual) forward and backward restated in float64, with an error budget for every quantity the
device forms of ieee_amd/csrc/bn.hip produce, the builders for what those forms take as input (transposed partial sums,
fixed-point totals), and the case runners that tests/test_bn_forms_gpu.py and its child process share.

The formulas are those of the header comment of bn.hip (torch.nn.BatchNorm2d defaults: biased variance for the
normalisation, unbiased for the running estimate) and nothing here calls torch.nn.functional.batch_norm, so M = 1 is defined.

Error budget (u = 2^-24; every bound is computed from the reference's own magnitudes, never from a device output):
  reductions      |err| <= n * u * sum|terms| for an fp32 addition chain of n links.  The longest chain that feeds a channel
                  is rows-per-thread + ty of red_geom (chain_length() below: 260 at bf16 C = 8, M = 1000; 43 at the large
                  shape; never more than 267 < 512 at the shapes of these tests), plus the rounding of the product, and a
                  chain cannot be longer than the M - 1 additions of its M terms: n = min(chain_length + 1, M).
  totals forms    the sums are exact integers; the conversions to fp32 and rsqrtf (4 ulp) remain.
  elementwise     half an ulp of the stored type on the reference value + 4 u * sum|terms| + the first-order propagation of
                  the coefficient bounds.  The device forms shift = beta - mean * scale from its OWN scale, so an error of
                  scale reaches out = (y - mean) * scale + beta through |y - mean|, not through |y| + |mean|; the same holds
                  for k2 * y + k3 = -A * invstd * c2 * (y - mean) - A * c1 in the backward.
  invstd          var -> 1 / sqrt(var + eps) is monotone: the bound is the larger half of the interval [var - dvar,
                  var + dvar] (clamped at 0) mapped through it, which stays valid where dvar is not small beside var + eps.
"""
import functools
import json
import os
import sys
import types

import numpy as np
import torch

U = 2.0 ** -24
N_CHAIN = 512
MOMENTUM = float(np.float32(0.1))
EPS = float(np.float32(1e-5))
KINK = 2.0 ** -18
KINK_CAP = 0.005
FWD_FIX = 2.0 ** 24
BWD_FIX = 2.0 ** 40
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RATIOS = {}   # tag -> largest err / bound seen (IEEE_BN_RATIOS_FILE: written at exit, for the LABNOTES entry)


def half_ulp(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else U


def vec_of(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def n_chain(c):
    """links of the longest fp32 chain behind a channel's sum over the M rows of case c: the additions of one thread's rows and of
    the ty row lanes (chain_length) and the rounding of the product -- and never more than M - 1 additions and that product"""
    n = min(chain_length(c.M, c.C, vec_of(c.dtype)) + 1, c.M)
    assert n <= N_CHAIN
    return n


# ---- the launch geometry of bn.hip, restated (what selects a form; used for comments, grid.x of the _ds bound, the child's shapes)
def cdiv(a, b):
    return (a + b - 1) // b


def red_geom(M, C, vec, red_max_blocks=768):
    cprw = C // vec
    tx = 1
    while tx * 2 <= min(cprw, 64) and cprw % (tx * 2) == 0:
        tx *= 2
    ty = 256 // tx
    cblocks = cdiv(cprw, tx)
    rb = max(1, red_max_blocks // cblocks)
    rb = max(1, min(rb, cdiv(M, ty * 4)))
    rows_per_block = cdiv(cdiv(M, rb), ty) * ty
    return types.SimpleNamespace(cprw=cprw, tx=tx, ty=ty, cblocks=cblocks, rows_per_block=rows_per_block,
                                 rblocks=cdiv(M, rows_per_block))


def chain_length(M, C, vec):
    g = red_geom(M, C, vec)
    return g.rows_per_block // g.ty + g.ty


def finalize_lpc(rblocks):
    lpc = 32
    while lpc < 256 and lpc * 4 < rblocks:
        lpc *= 2
    return lpc


def ew_blocks(chunks, cap=8192):
    return max(1, min(cdiv(chunks, 256), cap))


def tot_blocks(chunks, groups):
    return max(1, min(cdiv(chunks, 256), max(256, 2048 // max(groups, 1))))


# ---- cases
def make_case(dtype, G, M, C, seed=0):
    """Gaussian data as test_bn2d_fwd_bwd draws it, already rounded to the stored type; every fifth gamma negative."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * C + M + (17 if dtype == torch.bfloat16 else 0))
    rt = (lambda t: t.to(torch.bfloat16)) if dtype == torch.bfloat16 else (lambda t: t)
    c = types.SimpleNamespace(dtype=dtype, G=G, M=M, C=C)
    c.y = rt(torch.randn(G, M, C, generator=g) * 2 + 0.5).to(F64)
    c.res = rt(torch.randn(G, M, C, generator=g)).to(F64)
    c.dout = rt(torch.randn(G, M, C, generator=g)).to(F64)
    c.yds = rt(torch.randn(G, M, C, generator=g) * 1.5 - 0.25).to(F64)
    gamma = torch.rand(G, C, generator=g) + 0.5
    gamma[:, ::5] *= -1
    c.gamma = gamma.to(F64)
    beta = torch.randn(G, C, generator=g) * 0.3
    # |beta| >= 0.05: at M = 1 the pre-activation IS beta (y = mean) beside |y * scale| ~ 1e3, and a beta within 2^-18 of that
    # would put the whole channel on the kink
    c.beta = torch.where(beta.abs() < 0.05, torch.full_like(beta, 0.05) * torch.sign(beta + 1e-9), beta).to(F64)
    c.rm = (torch.randn(G, C, generator=g) * 0.1).to(F64)
    c.rv = (torch.rand(G, C, generator=g) + 0.5).to(F64)
    c.dg0 = torch.randn(G, C, generator=g).to(F64)    # prior d(gamma) / d(beta) for accumulate = 1
    c.db0 = torch.randn(G, C, generator=g).to(F64)
    return c


@functools.lru_cache(maxsize=4)
def cached_case(dtype, G, M, C):
    return make_case(dtype, G, M, C)


def f32(t):
    """round to fp32, back in float64"""
    return t.to(torch.float32).to(F64)


def _b(t):
    return t[:, None, :]


# ---- forward
def natural_sums(c):
    """(s1, s2, ds1, ds2): per-channel sum y, sum y^2 and what an fp32 chain of n links may lose of them"""
    n = n_chain(c)
    s1, s2 = c.y.sum(1), (c.y * c.y).sum(1)
    return s1, s2, n * U * c.y.abs().sum(1), n * U * s2


def fwd_ref(c, sums=None, form="finalize", residual=False, relu=True, training=True, given=None, momentum=MOMENTUM,
            eps=EPS, mutate=None):
    """name -> (reference, bound) for mean, invstd, scale, shift, rm, rv, out; plus "pre" and "mag" (see kink_keep).
    form: "finalize" (double 1/sqrt, one rounding), "totals" (fp32 variance, rsqrtf), "eval" (running statistics, fp32
    1/sqrtf), "given" (stats [G][4][C] supplied: nothing is finalized)."""
    M, hu = c.M, half_ulp(c.dtype)
    r = {}
    if form == "given":
        mean, invstd, scale, shift = (given[:, i] for i in range(4))
        zero = torch.zeros_like(mean)
        dmean = dinv = dscale = zero
        dshift = zero
        rm, rv, drm, drv = c.rm, c.rv, zero, zero
    else:
        if training:
            s1, s2, ds1, ds2 = sums if sums is not None else natural_sums(c)
            mean = s1 / M
            var = (s2 / M - mean * mean).clamp_min(0)
            dmean_in = ds1 / M
            dvar = ds2 / M + 2 * mean.abs() * dmean_in
            if form == "totals":     # var -> fp32, + eps in fp32
                dvar = dvar + U * var + U * (var + eps)
            nvar = var * (M / (M - 1.0)) if (mutate == "unbiased" and M > 1) else var
            invstd = (nvar + eps).rsqrt()
            lo = ((var + dvar) + eps).rsqrt()
            hi = ((var - dvar).clamp_min(0) + eps).rsqrt()
            dinv = torch.maximum(hi - (var + eps).rsqrt(), (var + eps).rsqrt() - lo) + (8 * U if form == "totals" else U) * invstd
            dmean = dmean_in + U * mean.abs()
            unbiased = var * (M / (M - 1.0)) if M > 1 else var
            m1, m2 = (momentum, 1 - momentum) if mutate == "swap_mom" else (1 - momentum, momentum)
            rm = m1 * c.rm + m2 * mean
            rv = m1 * c.rv + m2 * unbiased
            kub = M / (M - 1.0) if M > 1 else 1.0
            drm = momentum * dmean + 4 * U * ((1 - momentum) * c.rm.abs() + momentum * mean.abs())
            drv = momentum * kub * dvar + 4 * U * ((1 - momentum) * c.rv.abs() + momentum * unbiased)
        else:
            mean, dmean = c.rm, torch.zeros_like(c.rm)
            invstd = (c.rv + eps).rsqrt()
            dinv = 4 * U * invstd      # fp32 add, sqrtf, divide: three roundings, the first halved by the square root
            rm, rv, drm, drv = c.rm, c.rv, torch.zeros_like(c.rm), torch.zeros_like(c.rm)
        scale = c.gamma * invstd
        dscale = c.gamma.abs() * dinv + U * scale.abs()
        shift = c.beta - mean * scale
        dshift = scale.abs() * dmean + mean.abs() * dscale + 2 * U * (c.beta.abs() + (mean * scale).abs())
    if mutate == "neighbour_chunk":
        v = vec_of(c.dtype)
        scale, shift = torch.roll(scale, v, 1), torch.roll(shift, v, 1)
    r.update(mean=(mean, dmean), invstd=(invstd, dinv), scale=(scale, dscale), shift=(shift, dshift), rm=(rm, drm),
             rv=(rv, drv))
    ys = c.y * _b(scale)
    pre = ys + _b(shift)
    mag = ys.abs() + _b(shift).abs()
    if residual:
        pre = pre + c.res
        mag = mag + c.res.abs()
    out = pre.clamp_min(0) if relu else pre
    dpre = (c.y - _b(mean)).abs() * _b(dscale) + _b(scale.abs() * dmean) + 4 * U * (mag + _b((mean * scale).abs() + c.beta.abs()))
    if form == "given":
        dpre = 4 * U * mag
    r["out"] = (out, dpre + hu * (out.abs() + dpre))
    r["pre"], r["mag"] = pre, mag
    return r


def kink_keep(pre, mag):
    """False where a mask decision is within rounding distance of the ReLU kink (the device recomputes the pre-activation
    in fp32, possibly with an fma): the tests zero dout there"""
    return pre.abs() > KINK * mag


def stats32(c):
    """[G][4][C] fp32 statistics (mean, invstd, scale, shift) for the backward forms, from the exact sums"""
    if getattr(c, "st32", None) is None:
        c.st32 = _stats32(c)
    return c.st32


def _stats32(c):
    s1, s2 = c.y.sum(1), (c.y * c.y).sum(1)
    z = torch.zeros_like(s1)
    r = fwd_ref(c, sums=(s1, s2, z, z), relu=False)
    return torch.stack([r[k][0] for k in ("mean", "invstd", "scale", "shift")], 1).to(torch.float32)


# ---- backward
def bwd_ref(c, st, mask_kind, sums="natural", accumulate=False, frozen=False, mutate=None):
    """name -> (reference, bound) for dy, g, dgamma, dbeta, k1, k2, k3, from the fp32 statistics `st` [G][4][C] the device is
    handed.  mask_kind 0: g = dout; 1: g = dout * [a > 0] with a = relu(y*scale + shift + res) (returned as "a"); 2: g = dout *
    [y*scale + shift > 0].  dout is zeroed at the kink first ("dout", "kept").  sums: "natural" (fp32 chains), "exact" (the caller
    quantises "s1" / "s2" itself and passes them back as a pair)."""
    M, hu = c.M, half_ulp(c.dtype)
    st = st.to(F64)
    mean, invstd, scale, shift = (st[:, i] for i in range(4))
    ys = c.y * _b(scale)
    pre2 = ys + _b(shift)
    mag2 = ys.abs() + _b(shift).abs()
    r = {}
    if mask_kind == 1:
        pre, mag = pre2 + c.res, mag2 + c.res.abs()
        r["a"] = pre.clamp_min(0)
    else:
        pre, mag = pre2, mag2
    # the kink matters where the DEVICE recomputes the pre-activation (kind 2); kind 1 reads its decisions from the tensor a
    keep = kink_keep(pre, mag) if mask_kind == 2 else torch.ones_like(pre, dtype=torch.bool)
    if mask_kind == 0:
        g = c.dout
    else:
        mask = (c.y > 0) if mutate == "mask_y" else (pre > 0)
        g = torch.where(mask & keep, c.dout, torch.zeros_like(c.dout))
    r["dout"], r["kept"] = torch.where(keep, c.dout, torch.zeros_like(c.dout)), keep
    r["g"] = (g, torch.zeros_like(g))
    if frozen:
        z = torch.zeros_like(scale)
        r.update(k1=(scale, z), k2=(z, z), k3=(z, z))
        dy = _b(scale) * g
        r["dy"] = (dy, hu * dy.abs())      # one product, one rounding of the stored type (fp32: the product's own)
        return r
    gy = g * c.y
    if isinstance(sums, tuple):
        s1, s2 = sums
        ds1 = ds2 = torch.zeros_like(s1)
    else:
        s1, s2 = g.sum(1), gy.sum(1)
        if sums == "natural":
            n = n_chain(c)
            ds1, ds2 = n * U * g.abs().sum(1), n * U * gy.abs().sum(1)
        else:
            ds1 = ds2 = torch.zeros_like(s1)
    r["s1"], r["s2"] = s1, s2
    sgx = invstd * (s2 - mean * s1)
    dsgx = invstd * (ds2 + mean.abs() * ds1)
    dgam, dbet = sgx, s1
    ddg, ddb = dsgx + U * sgx.abs(), ds1 + U * s1.abs()
    if accumulate:
        dgam, dbet = c.dg0 + sgx, c.db0 + s1
        ddg, ddb = ddg + U * dgam.abs(), ddb + U * dbet.abs()
    r["dgamma"], r["dbeta"] = (dgam, ddg), (dbet, ddb)
    A = c.gamma * invstd
    c1, c2 = s1 / M, sgx / M
    k1 = A
    k2 = -A * invstd * c2
    k3 = -A * c1 + A * invstd * c2 * mean
    dk1 = U * k1.abs()
    dk2 = (A * invstd).abs() * dsgx / M + U * k2.abs()
    dk3 = A.abs() * ds1 / M + (A * invstd * mean).abs() * dsgx / M + U * k3.abs()
    r.update(k1=(k1, dk1), k2=(k2, dk2), k3=(k3, dk3))
    t1, t2 = _b(k1) * g, _b(k2) * c.y
    dy = t1 + t2 + (0 if mutate == "no_k3" else _b(k3))
    terms = t1.abs() + t2.abs() + _b(k3).abs()
    ddy = (_b((A * invstd).abs() * dsgx / M) * (c.y - _b(mean)).abs() + _b(A.abs() * ds1 / M)
           + U * terms + 4 * U * terms)      # coefficient sums; their three roundings to fp32; the evaluation in fp32
    r["dy"] = (dy, ddy + hu * (dy.abs() + ddy))
    return r


def ds_sums(g, yds):
    """the downsample branch's backward sums: sum g, sum g * y_ds (and sum |g * y_ds| for the bound)"""
    p = g * yds
    return g.sum(1), p.sum(1), p.abs().sum(1)


# ---- builders for what the device forms take as input
def build_partials(terms1, terms2, rb):
    """transposed partials [G][2][C][rb] (fp32): the rows split over rb blocks (empty ones where rb > M), each block's float64
    sum rounded to fp32; also the float64 sums of the ROUNDED partials, which is what the device adds up (in double)"""
    G, M, C = terms1.shape
    edges = np.linspace(0, M, rb + 1).astype(np.int64)
    out = torch.zeros(G, 2, C, rb, dtype=torch.float32)
    # cumulative sums in float64: block sum = cs[e1] - cs[e0] would cancel, so the blocks are summed directly where they are few
    for q, t in enumerate((terms1, terms2)):
        if rb <= 64:
            for b in range(rb):
                out[:, q, :, b] = t[:, edges[b]:edges[b + 1]].sum(1).to(torch.float32)
        else:   # one segment reduction: rows sorted by block already
            idx = torch.from_numpy(np.searchsorted(edges[1:], np.arange(M), side="right"))
            acc = torch.zeros(G, rb, C, dtype=F64)
            acc.index_add_(1, idx, t)
            out[:, q] = acc.permute(0, 2, 1).to(torch.float32)
    s = out.to(F64).sum(3)
    return out.contiguous(), s[:, 0], s[:, 1]


def build_totals(s1, s2, fix, rep, seed=0, patch=None):
    """int64 totals [REP][G][2][C] whose replicas (arbitrary parts, some negative) add up to round(sum * fix); also the sums
    the totals stand for, total / fix, as the device converts them (int64 -> double).  patch = (quantity, channel, integer):
    that total is replaced by the given integer in every group (the range-flag cases)."""
    total = torch.stack([torch.round(s1 * fix), torch.round(s2 * fix)], 1).to(torch.int64)      # [G][2][C]
    if patch is not None:
        total[:, patch[0], patch[1]] = patch[2]
    g = torch.Generator().manual_seed(4242 + seed + rep)
    parts = torch.randint(-(1 << 44), 1 << 44, (rep,) + tuple(total.shape), generator=g, dtype=torch.int64)
    parts[rep - 1] = total - parts[:rep - 1].sum(0)
    q = total.to(F64) / fix
    return parts.contiguous(), q[:, 0], q[:, 1]


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


def _dump_ratios():
    path = os.environ.get("IEEE_BN_RATIOS_FILE")
    if path and RATIOS:
        old = {}
        if os.path.exists(path):
            old = json.load(open(path))
        for k, v in RATIOS.items():
            old[k] = max(old.get(k, 0.0), v)
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)


import atexit  # noqa: E402
atexit.register(_dump_ratios)


# ---- device side: the C ABI as the executor calls it (done_event = NULL throughout)
DEV = "cuda"


def _tdt(L, c):
    return L.IEEE_BF16 if c.dtype == torch.bfloat16 else L.IEEE_F32


def _strided(t, gs, fill):
    """[G][C] float64 -> fp32 device tensor [G][gs] with `fill` in the padding behind each group's C values"""
    G, C = t.shape
    o = torch.full((G, gs), fill, dtype=torch.float32)
    o[:, :C] = t.to(torch.float32)
    return o.to(DEV)


def _act(c, t):
    return t.to(c.dtype).to(DEV).contiguous()


def want_bits(out):
    """bit e of byte k = [stored out[8k + e] > 0]"""
    return ((out.reshape(-1, 8) > 0).to(torch.int32) << torch.arange(8, device=out.device, dtype=torch.int32)).sum(1)


SENT = 123.0


def run_fwd(L, lib, c, tag, training=1, running=True, out=True, residual=False, relu=True, bits=False, rb=0, strided=False,
            totals=0, overflow=None, patch=None):
    """One forward call and every comparison it allows.  rb: 0 the device's own reduction, > 0 test-built transposed partials,
    < 0 test-supplied statistics.  totals = REP > 0: ieee_bn2d_fwd_totals.  Returns (failures, device stats)."""
    fails = []
    G, M, C = c.G, c.M, c.C
    ps = C + 8 if strided else C
    yd = _act(c, c.y)
    resd = _act(c, c.res) if residual else None
    od = torch.full_like(yd, SENT)
    gd, bd = _strided(c.gamma, ps, float("nan")), _strided(c.beta, ps, float("nan"))
    rmd, rvd = _strided(c.rm, ps, SENT), _strided(c.rv, ps, SENT)
    bitsd = torch.zeros(G * M * C // 8, device=DEV, dtype=torch.uint8) if bits else None
    dt = _tdt(L, c)
    given = None
    z = torch.zeros(G, C, dtype=F64)
    tot = None
    if totals:
        s1, s2 = c.y.sum(1), (c.y * c.y).sum(1)
        tot, q1, q2 = build_totals(s1, s2, FWD_FIX, totals, patch=patch)
        ref = fwd_ref(c, sums=(q1, q2, z, z), form="totals", residual=residual, relu=relu)
        stats = torch.full((G, 4, C), SENT, device=DEV)
        totd = tot.to(DEV)
        L.check(lib.ieee_bn2d_fwd_totals(L.ptr(yd), L.ptr(resd), L.ptr(od) if out else None, dt, G, M, C, M * C, L.ptr(gd),
                                         L.ptr(bd), ps, L.ptr(rmd) if running else None, L.ptr(rvd) if running else None, ps,
                                         L.ptr(stats), L.ptr(totd), totals, MOMENTUM, EPS, int(relu), L.ptr(bitsd),
                                         L.ptr(overflow), L.stream()))
    else:
        part = torch.empty(G * lib.ieee_bn_partial_floats(dt, M, C) + 64, device=DEV)
        if rb > 0:
            p, q1, q2 = build_partials(c.y, c.y * c.y, rb)
            part = p.to(DEV)
            ref = fwd_ref(c, sums=(q1, q2, z, z), residual=residual, relu=relu)
        elif rb < 0:
            # statistics that are NOT those of y: out must follow what is supplied, not a recomputation
            s = stats32(c).to(F64)
            given = torch.stack([s[:, 0], s[:, 1], f32(s[:, 2] * 1.25), f32(s[:, 3] + 0.125)], 1)
            ref = fwd_ref(c, form="given", given=given, residual=residual, relu=relu)
        elif training:
            ref = fwd_ref(c, residual=residual, relu=relu)
        else:
            ref = fwd_ref(c, form="eval", training=False, residual=residual, relu=relu)
        stats = given.to(torch.float32).to(DEV) if given is not None else torch.full((G, 4, C), SENT, device=DEV)
        stats0 = stats.clone()
        L.check(lib.ieee_bn2d_fwd(L.ptr(yd), L.ptr(resd), L.ptr(od) if out else None, dt, G, M, C, M * C, L.ptr(gd), L.ptr(bd),
                                  ps, L.ptr(rmd) if running else None, L.ptr(rvd) if running else None, ps, L.ptr(stats),
                                  L.ptr(part), MOMENTUM, EPS, training, int(relu), rb, L.ptr(bitsd), L.stream()))
        if rb < 0 and not torch.equal(stats, stats0):
            fails.append("%s stats: supplied statistics were rewritten" % tag)
    torch.cuda.synchronize()
    if rb >= 0:
        for i, k in enumerate(("mean", "invstd", "scale", "shift")):
            compare(fails, tag, k, stats[:, i], *ref[k])
    updated = running and training and rb >= 0
    for k, d, src in (("rm", rmd, c.rm), ("rv", rvd, c.rv)):
        if updated:
            compare(fails, tag, k, d[:, :C], *ref[k])
        elif not torch.equal(d[:, :C].cpu(), src.to(torch.float32)):
            fails.append("%s %s: running statistic changed although it must not" % (tag, k))
        if strided and not bool((d[:, C:] == SENT).all()):
            fails.append("%s %s: padding behind the group's channels was written" % (tag, k))
    if out:
        compare(fails, tag, "out", od, *ref["out"])
        if bits and not torch.equal(bitsd.to(torch.int32), want_bits(od)):
            fails.append("%s relu_bits differ from the stored out" % tag)
    elif not bool((od == SENT).all()):
        fails.append("%s out: written although out = NULL" % tag)
    return fails, stats


def run_bwd(L, lib, c, tag, mask_kind=0, gout=True, accumulate=0, rb=0, strided=False, entry="bwd", totals=0, replicas_ds=0,
            dgamma=True, overflow=None, patch=None):
    """One backward call (entry: "bwd", "frozen", "totals", "ds") and every comparison it allows."""
    fails = []
    G, M, C = c.G, c.M, c.C
    ps = C + 8 if strided else C
    dt = _tdt(L, c)
    gout = gout and entry != "ds"      # the _ds form has no g output
    st32 = stats32(c)
    z = torch.zeros(G, C, dtype=F64)
    if entry == "frozen":
        ref = bwd_ref(c, st32, mask_kind, frozen=True)
    elif entry in ("totals", "ds") or rb > 0:
        ref = bwd_ref(c, st32, mask_kind, sums="exact")
        g = ref["g"][0]
        if rb > 0:
            p, q1, q2 = build_partials(g, g * c.y, rb)
        else:
            tot, q1, q2 = build_totals(ref["s1"], ref["s2"], BWD_FIX, totals, patch=patch)
        ref = bwd_ref(c, st32, mask_kind, sums=(q1, q2), accumulate=bool(accumulate))
    else:
        ref = bwd_ref(c, st32, mask_kind, accumulate=bool(accumulate))
    if (~ref["kept"]).double().mean().item() > KINK_CAP:
        fails.append("%s: more than %g of the elements lie on the ReLU kink" % (tag, KINK_CAP))
    yd = _act(c, c.y)
    dd = _act(c, ref["dout"] if entry != "ds" else ref["g"][0])
    ad = _act(c, ref["a"]) if mask_kind == 1 else None
    dyd = torch.full_like(yd, SENT)
    god = torch.full_like(yd, SENT) if gout else None
    gd = _strided(c.gamma, ps, float("nan"))
    statsd = st32.to(DEV)
    dgd = _strided(c.dg0, ps, SENT) if dgamma else None
    dbd = _strided(c.db0, ps, SENT) if dgamma else None
    coef = torch.full((G, 3, C), SENT, device=DEV)
    mfy = 1 if mask_kind == 2 else 0
    if entry == "bwd":
        part = p.to(DEV) if rb > 0 else torch.empty(G * lib.ieee_bn_partial_floats(dt, M, C) + 64, device=DEV)
        L.check(lib.ieee_bn2d_bwd(L.ptr(dd), L.ptr(ad), L.ptr(yd), L.ptr(dyd), L.ptr(god), dt, G, M, C, M * C, L.ptr(gd), ps,
                                  L.ptr(statsd), L.ptr(dgd), L.ptr(dbd), ps, L.ptr(part), L.ptr(coef), accumulate, mfy, rb,
                                  L.stream()))
    elif entry == "frozen":
        L.check(lib.ieee_bn2d_bwd_frozen(L.ptr(dd), L.ptr(ad), L.ptr(yd), L.ptr(dyd), L.ptr(god), dt, G, M, C, M * C,
                                         L.ptr(statsd), L.ptr(coef), mfy, None, L.stream()))
    elif entry == "totals":
        totd = tot.to(DEV)
        L.check(lib.ieee_bn2d_bwd_totals(L.ptr(dd), L.ptr(ad), L.ptr(yd), L.ptr(dyd), L.ptr(god), dt, G, M, C, M * C, L.ptr(gd),
                                         ps, L.ptr(statsd), L.ptr(dgd), L.ptr(dbd), ps, L.ptr(totd), totals, mfy,
                                         L.ptr(overflow), None, L.stream()))
    else:
        totd = tot.to(DEV)
        ydsd = _act(c, c.yds)
        gen = torch.Generator().manual_seed(99 + replicas_ds)
        t0 = torch.randint(-(1 << 40), 1 << 40, (replicas_ds, G, 2, C), generator=gen, dtype=torch.int64)
        tds = t0.to(DEV)
        d1 = None
        for call in range(2):     # a second identical call adds the same integer to word [c] again
            L.check(lib.ieee_bn2d_bwd_totals_ds(L.ptr(dd), L.ptr(yd), L.ptr(ydsd), L.ptr(dyd), dt, G, M, C, M * C, L.ptr(gd), ps,
                                                L.ptr(statsd), L.ptr(dgd), L.ptr(dbd), ps, L.ptr(totd), totals, L.ptr(tds),
                                                replicas_ds, L.ptr(overflow), None, L.stream()))
            torch.cuda.synchronize()
            grown = (tds.cpu() - t0).sum(0)           # [G][2][C], summed over the replicas
            t1 = tot.sum(0)[:, 0]
            if call == 0:
                d1 = grown
                if not torch.equal(grown[:, 0], t1):
                    fails.append("%s totals_ds[c]: grew by something else than the integer total of sum g" % tag)
                _, sgy, sabs = ds_sums(ref["g"][0], c.yds)
                grid = tot_blocks(M * C // 8, G)
                # fp32 chain per workgroup share (a thread's trips + the 256 / cprw row lanes of the workgroup: never longer than the
                # reduction kernels' chain at the same shape), one rounding to fixed point per workgroup (half a unit each)
                compare(fails, tag, "ds_sum_gy", grown[:, 1].to(F64), sgy * BWD_FIX,
                        n_chain(c) * U * sabs * BWD_FIX + grid)
            elif not torch.equal(grown[:, 0], 2 * t1):
                fails.append("%s totals_ds[c]: the second call did not add the same integer again" % tag)
    torch.cuda.synchronize()
    compare(fails, tag, "dy", dyd, *ref["dy"])
    if gout:
        compare(fails, tag, "g_out", god, *ref["g"])
    if entry in ("bwd", "frozen"):
        for i, k in enumerate(("k1", "k2", "k3")):
            compare(fails, tag, k, coef[:, i], *ref[k])
        if entry == "frozen" and not bool((coef[:, 1:] == 0).all()):
            fails.append("%s coef rows 2 and 3 are not exactly zero" % tag)
    if entry != "frozen" and dgamma:
        compare(fails, tag, "dgamma", dgd[:, :C], *ref["dgamma"])
        compare(fails, tag, "dbeta", dbd[:, :C], *ref["dbeta"])
        if strided and not bool((dgd[:, C:] == SENT).all() and (dbd[:, C:] == SENT).all()):
            fails.append("%s dgamma / dbeta: padding behind the group's channels was written" % tag)
    return fails


# ---- the child process of test_switched_forms: IEEE_BN_FIXED / IEEE_BN_UNROLL are read once per process
def switched_shapes(unroll):
    """C in {8, 64, 2048} x M in {3, 257}; C = 64, M = 70 000; and, with two chunks in flight, C = 64, M = 262 145.
    ew_blocks: a pass over M * C / 8 chunks runs min(ceil(chunks / 256), 8192) workgroups, so its stride is at least the
    number of chunks until the cap binds: at M = 70 000 (560 000 chunks, 2 188 workgroups, stride 560 128) the two-chunk loop
    makes no trip and only the single-chunk tail runs.  The cap binds from 8192 * 256 = 2 097 152 chunks on, i.e. M > 262 144 at
    C = 64: M = 262 145 is the smallest size at which threads 0..7 run the two-chunk loop and all the others its tail."""
    shapes = [(C, M) for C in (8, 64, 2048) for M in (3, 257)] + [(64, 70000)]
    if unroll == 2:
        assert ew_blocks(70000 * 8) * 256 >= 70000 * 8 and ew_blocks(262145 * 8) * 256 < 262145 * 8 <= ew_blocks(262144 * 8) * 256 + 8
        shapes.append((64, 262145))
    return shapes


def child_main(unroll):
    sys.path.insert(0, ROOT)
    import ieee_amd  # noqa: F401  (before the HIP runtime starts)
    from ieee_amd import _lib as L
    lib = L.require_gpu()
    fails = []
    for C, M in switched_shapes(unroll):
        c = make_case(torch.bfloat16, 1 if M > 1000 else 3, M, C)
        big = M > 1000       # the long shapes are there for the loop structure: one forward and three backward forms
        for residual in (False, True):
            for bits in (False, True):
                if big and not (residual and bits):
                    continue
                tag = "switched-fwd[C%d-M%d-res%d-bits%d]" % (C, M, residual, bits)
                fails += run_fwd(L, lib, c, tag, residual=residual, bits=bits, strided=M == 257)[0]
        for mask_kind in (0, 1, 2):
            for gout in (False, True):
                if big and gout != (mask_kind != 1):
                    continue
                tag = "switched-bwd[C%d-M%d-mask%d-gout%d]" % (C, M, mask_kind, gout)
                fails += run_bwd(L, lib, c, tag, mask_kind=mask_kind, gout=gout)
    for f in fails:
        print(f)
    print("switched forms: %d failed comparisons" % len(fails))
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(child_main(int(sys.argv[1])))
