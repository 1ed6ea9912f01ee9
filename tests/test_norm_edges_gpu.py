"""Float64 edge-case gate of the norm kernels (csrc/sdv_norm.hip): sdv_groupnorm_stats, sdv_groupnorm_finalize, sdv_groupnorm_apply
(bf16 and e4m3), sdv_layernorm_bf16 (generic MAXC 1 / 2 / 4 and the 320-family kernels) and sdv_rowstats_finalize - chosen `splits`
with a short, an empty and a beyond-HW last range, the 4-way unrolled tails, the pix_per_block tail of the apply pass, groups that
straddle a chunk or the concat seam, the chunk loop (C > 2048), rows < rows-per-block, the nchunk boundaries 64 / 65 and 128 / 129.

Every case compares EVERY partial / output element with float64 on the operands the kernel sees.  acc_eps = 1e-5 is the project's
fp32 accumulation allowance (helpers._half_ulp_ratio), eps the fp32 value the kernel is handed:

    partials     per (image, split, group), against float64 sums over exactly that split's pixel (stats) or block (finalize) range:
                 |S - S64| <= acc_eps sum |x|,  |Q - Q64| <= acc_eps Q64;  an empty range gives (0, 0) exactly
    statistics   entitlement of the documented one-pass algorithm: dmean = acc_eps mean64 |x|, dvar = 3 acc_eps E64[x^2] (one share
                 for Q, two for mean^2), rstd in [rsqrt(var64 + dvar + eps), rsqrt(max(var64 - dvar, 0) + eps)] widened by 4 fp32 ulp
                 (= [rstd_lo, rstd_hi]); drstd the larger distance from rstd64 to either end
    GroupNorm    v = (x - mean64) rstd64 gamma + beta,  mag = (|x| + |mean64|) rstd_hi |gamma| + |beta|,
                 allow = acc_eps mag + |gamma| (rstd_hi dmean + |x - mean64| drstd):
                 |out - act(v)| <= 0.5 ulp_bf16 (1 + 1e-3) + L allow + acc_eps |act(v)|,   L = 1.1 with SiLU (|silu'| <= 1.0999), else 1
                 (the last term pays for __expf and the division).  Apply driven by hand-made partials: mean64, E64[x^2] and
                 mean64 |x| (= sum_i |s_i| / cnt) are those of the partials, in float64
    e4m3         the same with everything times q_scale, the half ulp that of e4m3 (3 mantissa bits, subnormal step 2^-9) and the
                 reference clamped to +-448: |v q| >= 448 must store exactly +-448; no byte 0x7F / 0xFF.  The saturation counter lies
                 between the float64 counts of |act(v) q| > 448 + a and > 448 - a, a = q (L allow + acc_eps |act(v)|) per element
    LayerNorm    two-pass: |out - ref64| <= 0.5 ulp_bf16 (1 + 1e-3) + acc_eps ((|x| + |mean64|) rstd64 |gamma| + |beta|)
    rowstats     the panel gate's entitlement from the float64 sums of the GIVEN partials: |mean - mean64| <= acc_eps mean64 |y|
                 (sum_i |s_i| / C), dvar = acc_eps E64[y^2], the rstd bracket widened by 4 fp32 ulp.  Integer partials: the mean
                 EQUALS fl(s fl(1 / C)), s the exact sum - the kernel multiplies by the inv_c it is handed, two roundings, so
                 "the fp32 rounding of the exact quotient" is one ulp off for a share of the sums of a correct kernel
                 (test_rowstats_integer_mean_is_two_roundings counts them on the CPU)

Two input families per GroupNorm shape.  "random": per (image, group) a common mode N(0, 3) and sigma in exp(U(-3.4, 0.7)), the mode
clamped so that the regular groups keep |mean| <= 10 sigma (asserted on the float64 statistics: then dvar / var <= 3.03e-3, the
rstd bracket reaches 0.16 % to either side at the most and the half ulp dominates the bound); where a shape has 8 groups or more, image 0's first
seven are the constants 0, 1, -7.5, 100, 3e-3, a group with a single non-zero element and a group at mean 50, sigma 0.5;
gamma = 1 + 0.3 N, beta = 0.5 N.  Every random case runs twice and must agree bit for bit.  "integer": x integer in [-8, 8] - every
fp32 sum is exact, so the partials of stats / finalize must EQUAL the float64 sums; apply gets hand-made partials that give group g the
integer mean g - groups / 2 and variance 1 (s = m cnt_i, q = (m^2 + 1) cnt_i per split), gamma = 1, beta = 0: a wrong group index at a
chunk or seam boundary is off by 1 at the least.  LayerNorm: rows like test_ffn_gpu._rows (|mean| / sigma up to some hundred), from
8 rows on the first seven the same constants / single element / (50, 0.5).

Memory discipline of every launch: `out`, `partials`, the rowstats output are NaN (e4m3: the byte 171) before the launch and windows
of larger allocations with GUARD rows in front and behind that must be bit-unchanged; X, X2, hand-made partials and rowstats partials
are windows with NaN rows around them; P of finalize has NaN in the columns >= C of ld and NaN blocks in front and behind: a pixel,
row, block or column beyond the tensor that is USED shows as NaN.  Every launch stays inside the preconditions of sdv_hip.h.

Worst element as a fraction of its bound, measured on MI355X (one line per test in the parity report conftest.report appends to):
    stats (10 shapes, both families)      worst partial 0.067; the integer family equal to the float64 sums everywhere; empty and
                                          beyond-HW splits (0, 0)
    apply on kernel partials (11 shapes)  0.989 without and with SiLU - the ONE rounding of the output (half a bf16 ulp is 1 / 1.001 of
                                          the bound); on hand-made integer partials 0.003 without, 0.947 with SiLU
    wrapper (3 gn_splits regimes)         0.991
    finalize (13 shapes x 3 splits)       worst partial 0.025, integer family equal; the apply that follows 0.987, and bit-identical to
                                          apply after the statistics pass where the sums are exact
    e4m3                                  0.998 calibrated and tight (the one e4m3 rounding); counter 0 calibrated (float64 count
                                          0 .. 1), 1280 tight (float64 count 1265 .. 1315 without, 1270 .. 1290 with SiLU): 1 % of 128 000
    LayerNorm                             0.996 generic (40 cases), 0.996 320 family (18 cases), 0.996 with gamma / beta misaligned
    rowstats_finalize (48 cases)          mean at 0.015 of its bound, every rstd inside its entitlement, integer means equal
Reported, not asserted - worst relative error of the rstd the apply pass derives from the GPU's partials (finalised in fp32 as the kernel
documents it, that last step in CPU arithmetic), per group class: regular groups (|mean| <= 10 sigma) 9.7e-6 from stats / 8.3e-6 from
finalize, the group at mean 50, sigma 0.5 8.6e-4 / 7.4e-4 (E[x^2] - mean^2 leaves 4 digits: what a ResBlock receives for a group with
|mean| / sigma = 100; allowed dvar / var = 0.3), constant groups 1.5e-7 (their sums are exact here, the 100s included), the single element
5.0e-8.  sdv_rowstats_finalize's emitted rstd: random rows 6.8e-6, random rows with |mean| > 10 sigma 2.9e-3, the (50, 0.5) row 6.6e-4,
constant rows 5.5e-8, integer rows 8.9e-8.  No case failed: the kernels honour their contract at every edge listed here - no pixel,
row, block or column beyond the tensor used, nothing written outside a window, rows independent, the counter exact.  Every test
function takes well under a second on the GPU.

Planted errors (test_checker_rejects_planted_errors) were exercised on the CPU stand-in only - one pixel missing from the statistics,
the last split skipped, the count off by one pixel, the group index taken from the chunk's first channel, the seam off by one chunk,
eps omitted, SiLU omitted on the tail pixels, a missed e4m3 clamp, a LayerNorm tail row unwritten, a write into a guard row, a
finalize block range off by one - none of them was run on the GPU.
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from conftest import bf16_round, report
from helpers import _half_ulp_ratio
from test_ffn_gpu import _rows
from test_igemm_edges_gpu import GUARD, OutBuf, _bits, _window

gpu = pytest.mark.gpu          # (not a module-wide pytestmark: the checker's own tests below run in the CPU tier)

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FP8 = torch.float8_e4m3fn
NAN = float("nan")
EPS = float(torch.tensor(1e-5, dtype=F32))      # the eps the kernels see
ACC_EPS = 1e-5
HARD = (0.0, 1.0, -7.5, 100.0, 3e-3)            # constant groups / rows; then a single non-zero element; then mean 50, sigma 0.5
NHARD = len(HARD) + 2
FAMILIES = ("random", "integer")

# (nimg, HW, C1, C2, groups, splits) - 1. stats with chosen splits.                    per  PT  apply: ppb  blocks (last)
STATS_SHAPES = ((2, 200, 320, 0, 32, 3),        # last range 66, cpg 10 (not the chunk)   67   6          52   4 (44)
                (2, 67, 64, 0, 32, 1),          # the unroll taken by 3 lanes only        67  32         256   1 (67)
                (1, 130, 640, 320, 32, 2),      # cpg 30, [630, 660) straddles the seam   65   2          18   8 (4)
                (2, 37, 128, 0, 32, 4),         #                                         10  16         128   1 (37)
                (1, 9, 64, 0, 32, 4),           # split 3 is empty                         3  32         256   1 (9)
                (1, 5, 64, 0, 32, 4),           # split 3 starts beyond HW                 2  32         256   1 (5)
                (2, 16, 1280, 1280, 32, 1),     # nchunk 320 > 256: the chunk loop        16   1           7   3 (2)
                (1, 16, 1920, 0, 32, 2),        #                                          8   1           9   2 (7)
                (1, 64, 8, 0, 1, 1),            # one chunk, one group                    64 256        2048   1 (64)
                (1, 40, 512, 0, 64, 1))         # groups = 64                             40   4          32   2 (8)
APPLY_SHAPES = STATS_SHAPES + ((1, 600, 32, 0, 32, 3),)      # cpg 1                     200  64         512   2 (88)
WRAPPER_SHAPES = ((1, 64, 32), (1, 1024, 32), (1, 4096, 32), (2, 1024, 64))              # (nimg, HW, C): gn_splits 1, 8, 16, 8
FP8_SHAPE = (2, 200, 320, 0, 32, 3)
# 4. finalize: (nimg, C1, ld1, bpi1, nrep1, C2, ld2, bpi2, nrep2, groups); every splits of FIN_SPLITS
FIN_SHAPES = tuple((2, 64, 72, bpi, nrep, 0, 0, 0, 0, 32) for bpi in (1, 3, 4, 5, 7, 17) for nrep in (1, 4)) + ((2, 40, 48, 8, 1, 24, 40, 2, 4, 4),)
FIN_SPLITS = (1, 2, 4)
LN_GENERIC = tuple((C, rows) for C in (8, 64, 512, 520, 768, 1024, 1032, 2048) for rows in (1, 3, 4, 5, 37))
LN_RPB = {320: 32, 640: 16, 1280: 8}
LN_320 = tuple((C, rows) for C, rpb in LN_RPB.items() for rows in (1, 3, rpb - 1, rpb, rpb + 1, 2 * rpb + 5))
ROWSTATS = tuple((rows, slots, C) for rows in (1, 255, 256, 257) for slots in (1, 2, 5) for C in (320, 1280))


# ------------------------------------------------------------------------------------------------
# geometry, as sdv_norm.hip documents it
# ------------------------------------------------------------------------------------------------
def split_range(n, splits, sp):
    """the pixel / block range of split sp: per = ceil(n / splits), clamped to n (empty when it starts at or beyond n)"""
    per = -(-n // splits)
    a = min(sp * per, n)
    return a, min(a + per, n)


def thread_geometry(C):
    """(CT, PT): a block's 256 threads as CT channel chunks x PT pixel lanes; chunks beyond 256 are looped"""
    ct = min(C // 8, 256)
    return ct, 256 // ct


def apply_geometry(nimg, HW, C):
    """(pix_per_block, blocks per image) of the apply pass"""
    elems = min(max(nimg * HW * C // 4096, 16384), 131072)
    ppb = max(-(-elems // C), 1)
    return ppb, -(-HW // ppb)


def _ulp32(v):
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


def silu64(v):
    return v * torch.sigmoid(v)


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def _hard_fill(x2d, i, g):
    """x2d [n, width] becomes hard group / row i"""
    if i < len(HARD):
        x2d[:] = float(torch.tensor(HARD[i]).to(BF16))
    elif i == len(HARD):
        x2d[:] = 0.0
        x2d[x2d.shape[0] // 2, x2d.shape[1] // 3] = 3.0
    else:
        x2d[:] = bf16_round(50.0 + 0.5 * torch.randn(x2d.shape, generator=g))


def group_stats64(x, groups):
    """x [nimg, HW, C] -> float64 mean, E[x^2], mean |x| per (image, group)"""
    nimg, HW, C = x.shape
    xg = x.double().reshape(nimg, HW, groups, C // groups)
    return xg.mean((1, 3)), (xg * xg).mean((1, 3)), xg.abs().mean((1, 3))


@functools.lru_cache(maxsize=None)
def gn_case(shape, family):
    """The operands of one GroupNorm case on the CPU (x fp32 holding bf16 values, [nimg, HW, C1 + C2]) and its float64 statistics."""
    nimg, HW, C1, C2, groups, splits = shape
    C = C1 + C2
    cpg = C // groups
    g = torch.Generator().manual_seed(7000 + 13 * HW + C + 5 * splits + (family == "integer"))
    c = SimpleNamespace(shape=shape, family=family, nimg=nimg, HW=HW, C1=C1, C2=C2, C=C, groups=groups, splits=splits, cpg=cpg,
                        gidx=torch.arange(C) // cpg, cls=[["regular"] * groups for _ in range(nimg)])
    if family == "integer":
        c.x = torch.randint(-8, 9, (nimg, HW, C), generator=g).float()
        c.gamma, c.beta = torch.ones(C), torch.zeros(C)
        c.cls = [["integer"] * groups for _ in range(nimg)]
    else:
        mode = torch.randn(nimg, groups, generator=g) * 3.0
        sigma = torch.exp(torch.empty(nimg, groups).uniform_(-3.4, 0.7, generator=g))
        z = torch.randn(nimg, HW, groups, cpg, generator=g)
        cap = 8.0 * sigma * z.std((1, 3), unbiased=False)
        mode = torch.minimum(torch.maximum(mode, -cap), cap)
        x = bf16_round(mode[:, None, :, None] + sigma[:, None, :, None] * z)
        if groups >= NHARD + 1:
            for i in range(NHARD):
                _hard_fill(x[0, :, i], i, g)                         # (a view [HW, cpg] of x)
                c.cls[0][i] = "constant" if i < len(HARD) else ("single element" if i == len(HARD) else "mean 50, sigma 0.5")
        c.x = x.reshape(nimg, HW, C).contiguous()
        c.gamma, c.beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    c.mean64, c.e2, c.absmean = group_stats64(c.x, groups)
    xg = c.x.double().reshape(nimg, HW, groups, cpg)
    S, A, Q = (torch.zeros(nimg, splits, groups, dtype=F64) for _ in range(3))
    for sp in range(splits):
        a, b = split_range(HW, splits, sp)
        S[:, sp], A[:, sp], Q[:, sp] = xg[:, a:b].sum((1, 3)), xg[:, a:b].abs().sum((1, 3)), (xg[:, a:b] ** 2).sum((1, 3))
    c.S64, c.A64, c.Q64 = S, A, Q
    return c


def regular_groups_within_cap(c):
    """the condition of the random family: |mean64| <= 10 sigma64 in every regular group"""
    var = (c.e2 - c.mean64 ** 2).clamp_min(0.0)
    reg = torch.tensor([[k == "regular" for k in row] for row in c.cls])
    return bool((c.mean64.abs() <= 10.0 * var.sqrt())[reg].all())


def handmade_partials(c):
    """integer family: partials fp32 [nimg, splits, groups, 2] that give group g mean g - groups / 2 and variance 1, exactly"""
    m = (torch.arange(c.groups) - c.groups // 2).double()
    cnt = torch.tensor([(b - a) * c.cpg for a, b in (split_range(c.HW, c.splits, sp) for sp in range(c.splits))], dtype=F64)
    p = torch.stack([m[None] * cnt[:, None], (m * m + 1.0)[None] * cnt[:, None]], -1)         # [splits, groups, 2]
    assert float(p.abs().max()) < 2 ** 24
    return p[None].expand(c.nimg, -1, -1, -1).contiguous().float()


def stats_of_partials(parts64, cnt):
    """float64 (mean, E[x^2], mean |x|) per (image, group) of given partials [nimg, splits, groups, 2]"""
    return parts64[..., 0].sum(1) / cnt, parts64[..., 1].sum(1) / cnt, parts64[..., 0].abs().sum(1) / cnt


def entitlement(mean64, e2, absmean, shares=3.0):
    """the statistics entitlement of the module docstring (shares = 3: GroupNorm; 1: the panel gate's, rowstats)"""
    var64 = (e2 - mean64 * mean64).clamp_min(0.0)
    dvar = shares * ACC_EPS * e2
    lo, hi = torch.rsqrt(var64 + dvar + EPS), torch.rsqrt((var64 - dvar).clamp_min(0.0) + EPS)
    lo, hi = lo - 4 * _ulp32(lo), hi + 4 * _ulp32(hi)
    rstd64 = torch.rsqrt(var64 + EPS)
    return SimpleNamespace(mean=mean64, var=var64, rstd=rstd64, dmean=ACC_EPS * absmean, lo=lo, hi=hi,
                           drstd=torch.maximum(rstd64 - lo, hi - rstd64))


@functools.lru_cache(maxsize=None)
def gn_reference(shape, family, silu, handmade):
    """-> (ref64 [nimg, HW, C], extra = L allow + acc_eps |ref|) of apply; cached per case"""
    c = gn_case(shape, family)
    if handmade:
        ent = entitlement(*stats_of_partials(handmade_partials(c).double(), float(c.HW * c.cpg)))
    else:
        ent = entitlement(c.mean64, c.e2, c.absmean)
    x, gm, bt = c.x.double(), c.gamma.double()[None, None], c.beta.double()[None, None]
    m, r, hi = (t[:, c.gidx][:, None, :] for t in (ent.mean, ent.rstd, ent.hi))
    dmean, drstd = ent.dmean[:, c.gidx][:, None, :], ent.drstd[:, c.gidx][:, None, :]
    v = (x - m) * r * gm + bt
    mag = (x.abs() + m.abs()) * hi * gm.abs() + bt.abs()
    allow = ACC_EPS * mag + gm.abs() * (hi * dmean + (x - m).abs() * drstd)
    ref = silu64(v) if silu else v
    return ref, (1.1 if silu else 1.0) * allow + ACC_EPS * ref.abs()


@functools.lru_cache(maxsize=None)
def ln_case(C, rows):
    x = _rows(rows, "cpu", 300 + C + rows, K=C)[0].float()
    g = torch.Generator().manual_seed(31 * C + rows)
    cls = ["random"] * rows
    if rows >= NHARD + 1:
        for i in range(NHARD):
            _hard_fill(x[i:i + 1].T, i, g)
            cls[i] = "constant" if i < len(HARD) else ("single element" if i == len(HARD) else "mean 50, sigma 0.5")
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    rstd = torch.rsqrt(x64.var(1, unbiased=False, keepdim=True) + EPS)
    ref = (x64 - mean) * rstd * gamma.double()[None] + beta.double()[None]
    mag = (x64.abs() + mean.abs()) * rstd * gamma.double().abs()[None] + beta.double().abs()[None]
    return SimpleNamespace(C=C, rows=rows, x=x, gamma=gamma, beta=beta, ref=ref, mag=mag, cls=cls)


@functools.lru_cache(maxsize=None)
def rowstats_case(rows, slots, C, family):
    """partials fp32 [rows, slots, 2]: (sum, sumsq) of `slots` column ranges of y [rows, C]"""
    if family == "integer":
        y = torch.randint(-8, 9, (rows, C), generator=torch.Generator().manual_seed(rows + slots + C)).double()
        cls = ["integer"] * rows
    else:
        lc = ln_case_rows(rows, C)
        y, cls = lc.x.double(), lc.cls
    cuts = [C * i // slots for i in range(slots + 1)]
    part = torch.stack([torch.stack([y[:, a:b].sum(1), (y[:, a:b] ** 2).sum(1)], 1) for a, b in zip(cuts, cuts[1:])], 1).float()
    return SimpleNamespace(rows=rows, slots=slots, C=C, part=part, cls=cls, family=family)


def ln_case_rows(rows, C):
    return ln_case(C, rows)


@functools.lru_cache(maxsize=None)
def fin_case(shape, family):
    """finalize on synthetic P: a tensor x [nimg, HW, C1 + C2] with HW = 32 bpi nrep; block k of repetition r of image i holds the
    (sum, sumsq) per channel of the pixels [(r bpi + k) 32, + 32) of image i (float64 sums rounded to fp32: exact in the integer family)"""
    nimg, C1, ld1, bpi1, nrep1, C2, ld2, bpi2, nrep2, groups = shape
    HW = 32 * bpi1 * nrep1
    assert C2 == 0 or HW == 32 * bpi2 * nrep2
    c = gn_case((nimg, HW, C1, C2, groups, 1), family)
    f = SimpleNamespace(shape=shape, family=family, gn=c, HW=HW, srcs=[])
    for c0, Cs, ld, bpi, nrep in ((0, C1, ld1, bpi1, nrep1), (C1, C2, ld2, bpi2, nrep2)):
        if Cs == 0:
            continue
        xb = c.x[:, :, c0:c0 + Cs].double().reshape(nimg, nrep, bpi, 32, Cs)
        blocks = torch.stack([xb.sum(3), (xb * xb).sum(3)], 3).permute(1, 0, 2, 3, 4)          # [nrep, nimg, bpi, 2, Cs]
        P = torch.full((nrep * nimg * bpi, 2, ld), NAN)
        P[:, :, :Cs] = blocks.reshape(-1, 2, Cs).float()
        f.srcs.append(SimpleNamespace(c0=c0, C=Cs, ld=ld, bpi=bpi, nrep=nrep, rep_stride=nimg * bpi, P=P))
    return f


def fin_reference(f, splits):
    """float64 (S, sum |P_s|, Q) [nimg, splits, groups] over exactly the block range of every (source, split)"""
    c = f.gn
    S, A, Q = (torch.zeros(c.nimg, splits, c.C, dtype=F64) for _ in range(3))
    for s in f.srcs:
        P = s.P[:, :, :s.C].double().reshape(s.nrep, c.nimg, s.bpi, 2, s.C)
        for sp in range(splits):
            a, b = split_range(s.bpi, splits, sp)
            S[:, sp, s.c0:s.c0 + s.C] = P[:, :, a:b, 0].sum((0, 2))
            A[:, sp, s.c0:s.c0 + s.C] = P[:, :, a:b, 0].abs().sum((0, 2))
            Q[:, sp, s.c0:s.c0 + s.C] = P[:, :, a:b, 1].sum((0, 2))
    return tuple(t.reshape(c.nimg, splits, c.groups, c.cpg).sum(3) for t in (S, A, Q))


# ------------------------------------------------------------------------------------------------
# THE checkers (CPU, float64; what the GPU tier and the stand-in tier both go through)
# ------------------------------------------------------------------------------------------------
def check_partials(parts, clean, S64, A64, Q64, exact, label=None):
    """parts float64 [nimg, splits, groups, 2] of the fp32 the kernel wrote -> the worst ratio to the bound"""
    assert parts.shape == S64.shape + (2,)
    assert clean, "the kernel wrote outside the partials window"
    assert bool(torch.isfinite(parts).all()), "non-finite partial: left unwritten, or a pixel / block / column beyond the tensor was used"
    S, Q = parts[..., 0], parts[..., 1]
    empty = A64 == 0
    assert bool((S[empty] == 0).all()) and bool((Q[Q64 == 0] == 0).all()), "an empty range (or an all-zero group) must give (0, 0) exactly"
    if exact:
        assert torch.equal(S, S64) and torch.equal(Q, Q64), "integer family: the partials must equal the float64 sums"
        return 0.0
    rs = ((S - S64).abs() / (ACC_EPS * A64).clamp_min(1e-300))[~empty]
    rq = ((Q - Q64).abs() / (ACC_EPS * Q64).clamp_min(1e-300))[Q64 != 0]
    worst = max(float(rs.max()) if rs.numel() else 0.0, float(rq.max()) if rq.numel() else 0.0)
    if label is not None:
        report(f"norm-edges {label}: worst partial at {worst:.3f} of the bound")
    assert worst <= 1.0, f"worst partial at {worst:.3f} of the bound"
    return worst


def check_output(win, clean, ref, extra, label=None, what="output"):
    """bf16 output against the half-ulp bound of the module docstring (extra = everything but the half ulp) -> worst ratio"""
    assert win.shape == ref.shape
    finite = bool(torch.isfinite(win).all())
    worst = float(_half_ulp_ratio(win, ref, extra / ACC_EPS, acc_eps=ACC_EPS).max()) if finite else float("inf")
    if label is not None:
        report(f"norm-edges {label}: worst {what} element at {worst:.3f} of the bound")
    assert clean, "the kernel wrote outside its output window (guard rows)"
    assert finite, "non-finite output element: left unwritten, or NaN memory (a pixel / row beyond the tensor, a foreign partial) was used"
    if worst > 1.0:
        bad = (_half_ulp_ratio(win, ref, extra / ACC_EPS, acc_eps=ACC_EPS) > 1.0).nonzero()
        raise AssertionError(f"worst {what} element at {worst:.3f} of the bound; {len(bad)} beyond it, first at {tuple(int(i) for i in bad[0])}")
    return worst


def fp8_decode(b):
    """e4m3fn bytes (as float64 or uint8) -> float64 values; 0x7F / 0xFF (NaN) stay NaN"""
    return b.to(torch.uint8).view(FP8).double()


def check_fp8(bytes64, clean, ref, extra, q, counter=None, label=None):
    """e4m3 bytes [nimg, HW, C] (float64 of the uint8) against the module docstring's fp8 bound; counter: the saturation counter read
    after the launch (None: not registered).  -> (worst ratio, float64 clamp share, band share)"""
    assert bytes64.shape == ref.shape
    assert clean, "the kernel wrote outside its output window (guard rows)"
    b = bytes64.to(torch.uint8)
    assert not bool(((b & 0x7F) == 0x7F).any()), "a NaN byte (0x7F / 0xFF): e4m3fn has no infinity - a clamp was missed, or NaN memory was used"
    out = fp8_decode(b)
    vq = ref * q
    refq = vq.clamp(-448.0, 448.0)
    sat = vq.abs() >= 448.0
    assert torch.equal(out[sat], torch.sign(vq[sat]) * 448.0), "an element with |v q| >= 448 is not exactly +-448"
    e = torch.floor(torch.log2(torch.maximum(refq.abs(), out.abs()).clamp_min(1e-30))).clamp_min(-6.0)
    ratio = (out - refq).abs() / (0.5 * torch.exp2(e - 3) * (1 + 1e-3) + q * extra)
    worst = float(ratio.max())
    a = q * extra
    lo_n, hi_n = int((vq.abs() > 448.0 + a).sum()), int((vq.abs() > 448.0 - a).sum())
    if label is not None:
        report(f"norm-edges {label}: worst e4m3 element at {worst:.3f} of the bound; counter {counter}, float64 count in [{lo_n}, {hi_n}]")
    if worst > 1.0:
        bad = (ratio > 1.0).nonzero()
        raise AssertionError(f"worst e4m3 element at {worst:.3f} of the bound; {len(bad)} beyond it, first at {tuple(int(i) for i in bad[0])}")
    if counter is not None:
        assert lo_n <= counter <= hi_n, f"saturation counter {counter} outside the float64 counts [{lo_n}, {hi_n}]"
    return worst, float(sat.double().mean()), (hi_n - lo_n) / vq.numel()


def check_rowstats(rc, stats, clean, label=None):
    """stats float64 [rows, 2] against the entitlement from the float64 sums of the given partials -> (worst mean ratio, per class
    the worst relative rstd error)"""
    assert stats.shape == (rc.rows, 2)
    assert clean, "the kernel wrote outside the statistics window"
    assert bool(torch.isfinite(stats).all()), "non-finite statistic: a row left unwritten, or a row / slot beyond the partials was used"
    p = rc.part.double()
    ent = entitlement(p[:, :, 0].sum(1) / rc.C, p[:, :, 1].sum(1) / rc.C, p[:, :, 0].abs().sum(1) / rc.C, shares=1.0)
    dm = (stats[:, 0] - ent.mean).abs()
    if rc.family == "integer":       # the sum s is exact: the mean EQUALS fl(s fl(1 / C)) (test_rowstats_integer_mean_is_two_roundings)
        s32 = p[:, :, 0].sum(1).float()
        want = (s32 * (torch.tensor(1.0, dtype=F32) / rc.C)).double()
        assert torch.equal(stats[:, 0], want), "integer partials: the mean is fl(s fl(1 / C)), s the exact sum"
        assert bool(((want - (s32.double() / rc.C).float().double()).abs() <= _ulp32(want.abs().clamp_min(1e-30))).all())
    bad = (dm > ent.dmean).nonzero()
    assert len(bad) == 0, f"mean of row {int(bad[0])}: {float(stats[bad[0], 0])} vs {float(ent.mean[bad[0]])}"
    bad = ((stats[:, 1] < ent.lo) | (stats[:, 1] > ent.hi)).nonzero()
    assert len(bad) == 0, f"rstd of row {int(bad[0])} ({rc.cls[int(bad[0])]}): {float(stats[bad[0], 1])} outside [{float(ent.lo[bad[0]])}, {float(ent.hi[bad[0]])}]"
    rel = ((stats[:, 1] - ent.rstd) / ent.rstd).abs()
    per = {}
    for i, k in enumerate(rc.cls):
        if k == "random" and float(ent.mean[i].abs()) > 10.0 * math.sqrt(float(ent.var[i])):
            k = "random, |mean| > 10 sigma"
        per[k] = max(per.get(k, 0.0), float(rel[i]))
    worst = float((dm / ent.dmean.clamp_min(1e-300))[ent.dmean > 0].max()) if bool((ent.dmean > 0).any()) else 0.0
    if label is not None:
        report(f"norm-edges {label}: mean at {worst:.3f} of its bound")
    return worst, per


def finalise_fp32(parts, cnt, eps=EPS):
    """the first lines of the apply pass in fp32 (CPU arithmetic): partials fp32 [nimg, splits, groups, 2] -> (mean, rstd) fp32"""
    s, q = torch.zeros_like(parts[:, 0, :, 0]), torch.zeros_like(parts[:, 0, :, 0])
    for sp in range(parts.shape[1]):
        s, q = s + parts[:, sp, :, 0], q + parts[:, sp, :, 1]
    cnt = torch.tensor(cnt, dtype=F32)
    mean = s / cnt
    return mean, torch.rsqrt((q / cnt - mean * mean).clamp_min(0.0) + torch.tensor(eps, dtype=F32))


def rstd_error_per_class(c, parts64):
    """REPORTED, not asserted: relative error of the rstd the apply pass derives from these partials (finalised in fp32 as the kernel
    documents it, on the CPU) against rstd64 of the tensor, worst per group class"""
    _, rstd = finalise_fp32(parts64.float(), float(c.HW) * float(c.cpg))
    ent = entitlement(c.mean64, c.e2, c.absmean)
    rel = ((rstd.double() - ent.rstd) / ent.rstd).abs()
    inside = bool(((rstd.double() >= ent.lo) & (rstd.double() <= ent.hi)).all())
    per = {}
    for i in range(c.nimg):
        for j in range(c.groups):
            per[c.cls[i][j]] = max(per.get(c.cls[i][j], 0.0), float(rel[i, j]))
    return per, inside


def _merge(dst, src):
    for k, v in src.items():
        dst[k] = max(dst.get(k, 0.0), v)


def _fmt(per):
    return ", ".join(f"{k}: {v:.1e}" for k, v in sorted(per.items()))


# ------------------------------------------------------------------------------------------------
# launching (GPU tier): the C entry points through hip.load(), as the wrappers call them
# ------------------------------------------------------------------------------------------------
_DEVICE = {}          # case key -> device operands (the lru caches above hold no GPU memory)


def gn_operands(c, dev):
    d = _DEVICE.setdefault(("gn", c.shape, c.family), {})
    if not d:
        x = c.x.reshape(c.nimg * c.HW, c.C)
        d["x"] = _window(x[:, :c.C1], c.C1, 0, 4, 4, BF16, dev)
        d["x2"] = _window(x[:, c.C1:], c.C2, 0, 4, 4, BF16, dev) if c.C2 else None
        d["gamma"], d["beta"] = c.gamma.to(dev), c.beta.to(dev)
    return d


def _p(t):
    return t.data_ptr() if t is not None else None


def launch_stats(hip, dev, c, splits=None):
    """-> (partials float64 [nimg, splits, groups, 2], clean, the OutBuf holding them)"""
    d, splits = gn_operands(c, dev), splits or c.splits
    pb = OutBuf(c.nimg * splits * c.groups, 2, 2, 0, F32, dev)
    hip._check(hip.load().sdv_groupnorm_stats(_p(d["x"]), _p(d["x2"]), c.C1, c.C2, c.nimg, c.HW, c.groups, splits, _p(pb.arg), hip._stream()),
               "sdv_groupnorm_stats")
    torch.cuda.synchronize()
    win, clean = pb.take()
    return win.reshape(c.nimg, splits, c.groups, 2), clean, pb


def launch_apply(hip, dev, c, parts, splits, silu, q=None):
    """parts: a device fp32 tensor (window).  -> (output float64 [nimg, HW, C] - e4m3: the bytes -, clean)"""
    d = gn_operands(c, dev)
    ob = OutBuf(c.nimg * c.HW, c.C, c.C, 0, torch.uint8 if q else BF16, dev)
    lib = hip.load()
    if q:
        rc = lib.sdv_groupnorm_apply_fp8(_p(d["x"]), _p(d["x2"]), c.C1, c.C2, c.nimg, c.HW, c.groups, splits, _p(parts), _p(d["gamma"]),
                                         _p(d["beta"]), EPS, int(silu), _p(ob.arg), q, hip._stream())
    else:
        rc = lib.sdv_groupnorm_apply(_p(d["x"]), _p(d["x2"]), c.C1, c.C2, c.nimg, c.HW, c.groups, splits, _p(parts), _p(d["gamma"]),
                                     _p(d["beta"]), EPS, int(silu), _p(ob.arg), hip._stream())
    hip._check(rc, "sdv_groupnorm_apply")
    torch.cuda.synchronize()
    win, clean = ob.take()
    return win.reshape(c.nimg, c.HW, c.C), clean


def parts_window(parts, dev):
    return _window(parts.reshape(-1, 2), 2, 0, GUARD, GUARD, F32, dev)


def launch_finalize(hip, dev, f, splits):
    c = f.gn
    d = _DEVICE.setdefault(("fin", f.shape, f.family), {})
    if not d:
        for i, s in enumerate(f.srcs):       # NaN blocks in front of and behind the blocks in use
            d[i] = torch.cat([torch.full((3, 2, s.ld), NAN), s.P, torch.full((3, 2, s.ld), NAN)]).to(dev)[3:3 + s.P.shape[0]]
    a = f.srcs[0]
    b = f.srcs[1] if len(f.srcs) > 1 else SimpleNamespace(C=0, ld=0, bpi=0, nrep=0, rep_stride=0)
    pb = OutBuf(c.nimg * splits * c.groups, 2, 2, 0, F32, dev)
    hip._check(hip.load().sdv_groupnorm_finalize(_p(d[0]), a.C, a.ld, a.bpi, a.nrep, a.rep_stride, _p(d.get(1)), b.C, b.ld, b.bpi, b.nrep,
                                                 b.rep_stride, c.nimg, c.groups, splits, _p(pb.arg), hip._stream()), "sdv_groupnorm_finalize")
    torch.cuda.synchronize()
    win, clean = pb.take()
    return win.reshape(c.nimg, splits, c.groups, 2), clean, pb


def launch_layernorm(hip, dev, lc, x=None, misaligned=False):
    x = lc.x if x is None else x
    xw = _window(x, lc.C, 0, 4, 4, BF16, dev)
    if misaligned:       # views 4 bytes into a larger buffer: not 16-byte aligned
        gm, bt = torch.cat([torch.full((1,), NAN), lc.gamma]).to(dev)[1:], torch.cat([torch.full((1,), NAN), lc.beta]).to(dev)[1:]
        assert gm.data_ptr() % 16 == 4 and bt.data_ptr() % 16 == 4
    else:
        gm, bt = lc.gamma.to(dev), lc.beta.to(dev)
        assert gm.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0
    ob = OutBuf(lc.rows, lc.C, lc.C, 0, BF16, dev)
    hip.layernorm(xw, gm, bt, EPS, out=ob.flat[ob.base:ob.base + lc.rows * lc.C].view(lc.rows, lc.C))
    torch.cuda.synchronize()
    return ob.take()


class launch_kinds:
    """with launch_kinds(hip) as kinds: the kinds of the launches that went through hip._launch; the hook is restored on the way out"""

    def __init__(self, hip):
        self.hip, self.kinds = hip, []

    def __enter__(self):
        self.prev = self.hip.LAUNCH_HOOK
        self.hip.LAUNCH_HOOK = lambda kind, info, fn: (self.kinds.append(kind), fn())
        return self.kinds

    def __exit__(self, *exc):
        self.hip.LAUNCH_HOOK = self.prev


# ------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------
def _fail(row, e):
    raise AssertionError(f"{row}: {e}") from None


@gpu
def test_stats_with_chosen_splits(hip, dev):
    """1. sdv_groupnorm_stats at every shape of STATS_SHAPES: uneven, empty and beyond-HW last ranges, the 4-way unroll tails, the
    chunk loop, groups across chunks and the seam.  Random: the bound, twice bit for bit; integer: equal to the float64 sums.  The
    rstd these partials lead to is reported per group class."""
    worst, per = 0.0, {}
    for shape in STATS_SHAPES:
        for family in FAMILIES:
            c = gn_case(shape, family)
            try:
                assert family == "integer" or regular_groups_within_cap(c), "input condition: a regular group beyond |mean| = 10 sigma"
                parts, clean, _ = launch_stats(hip, dev, c)
                worst = max(worst, check_partials(parts, clean, c.S64, c.A64, c.Q64, family == "integer"))
                if family == "random":
                    again, _, _ = launch_stats(hip, dev, c)
                    assert torch.equal(parts, again), "a repeated launch changed bits"
                    p, inside = rstd_error_per_class(c, parts)
                    assert inside, "the rstd these partials lead to leaves its entitlement"
                    _merge(per, p)
            except AssertionError as e:
                _fail((shape, family), e)
    report(f"norm-edges stats: {len(STATS_SHAPES)} shapes x 2 families, worst partial at {worst:.3f} of the bound; "
           f"worst relative rstd error (reported) {_fmt(per)}")


@gpu
@pytest.mark.parametrize("silu", (0, 1))
def test_apply_on_handmade_and_kernel_partials(hip, dev, silu):
    """2. sdv_groupnorm_apply at APPLY_SHAPES (the pix_per_block tail at every one): integer family on hand-made partials (group g at
    mean g - groups / 2), random family on the partials sdv_groupnorm_stats just wrote, twice bit for bit."""
    worst = {f: 0.0 for f in FAMILIES}
    for shape in APPLY_SHAPES:
        for family in FAMILIES:
            c = gn_case(shape, family)
            try:
                if family == "integer":
                    parts = parts_window(handmade_partials(c), dev)
                else:
                    assert regular_groups_within_cap(c), "input condition: a regular group beyond |mean| = 10 sigma"
                    p64, clean, pb = launch_stats(hip, dev, c)
                    check_partials(p64, clean, c.S64, c.A64, c.Q64, False)
                    parts = pb.arg
                ref, extra = gn_reference(shape, family, silu, family == "integer")
                win, clean = launch_apply(hip, dev, c, parts, c.splits, silu)
                worst[family] = max(worst[family], check_output(win, clean, ref, extra))
                if family == "random":
                    again, _ = launch_apply(hip, dev, c, parts, c.splits, silu)
                    assert torch.equal(win, again), "a repeated launch changed bits"
            except AssertionError as e:
                _fail((shape, family, silu), e)
    report(f"norm-edges apply silu={silu}: {len(APPLY_SHAPES)} shapes, worst element at {worst['random']:.3f} (random, kernel partials) / "
           f"{worst['integer']:.3f} (integer, hand-made partials) of the bound")


@gpu
def test_wrapper_path(hip, dev):
    """3. hip.groupnorm at the three gn_splits regimes: one gn_stats and one gn_apply launch, the output within the bound"""
    worst = 0.0
    for nimg, HW, C in WRAPPER_SHAPES:
        shape = (nimg, HW, C, 0, 32, hip.gn_splits(HW))
        for silu in (0, 1):
            c = gn_case(shape, "random")
            assert regular_groups_within_cap(c)
            d = gn_operands(c, dev)
            ob = OutBuf(nimg * HW, C, C, 0, BF16, dev)
            with launch_kinds(hip) as kinds:
                hip.groupnorm(d["x"], d["gamma"], d["beta"], nimg=nimg, HW=HW, groups=32, eps=EPS, silu=bool(silu),
                              out=ob.flat[ob.base:ob.base + nimg * HW * C].view(nimg * HW, C))
            torch.cuda.synchronize()
            assert kinds == ["gn_stats", "gn_apply"], kinds
            win, clean = ob.take()
            try:
                worst = max(worst, check_output(win.reshape(nimg, HW, C), clean, *gn_reference(shape, "random", silu, False)))
            except AssertionError as e:
                _fail((shape, silu), e)
    assert [hip.gn_splits(HW) for _, HW, _ in WRAPPER_SHAPES] == [1, 8, 16, 8]
    report(f"norm-edges wrapper: {len(WRAPPER_SHAPES)} shapes, worst element at {worst:.3f} of the bound")


@gpu
def test_finalize_on_synthetic_blocks(hip, dev):
    """4. sdv_groupnorm_finalize: the `k + 3 < k1` unroll tail (bpi 1 .. 17), bpi < splits (empty block ranges), ld > C with NaN
    columns, nrep = 4, two sources with a group across the seam; then apply with the same splits on the tensor the blocks came from."""
    worst_p, worst_o, per = 0.0, 0.0, {}
    for shape in FIN_SHAPES:
        for family in FAMILIES:
            f = fin_case(shape, family)
            c = f.gn
            for splits in FIN_SPLITS:
                try:
                    parts, clean, pb = launch_finalize(hip, dev, f, splits)
                    worst_p = max(worst_p, check_partials(parts, clean, *fin_reference(f, splits), family == "integer"))
                    if family == "random":
                        again, _, _ = launch_finalize(hip, dev, f, splits)
                        assert torch.equal(parts, again), "a repeated launch changed bits"
                        _merge(per, rstd_error_per_class(c, parts)[0])
                    if splits == FIN_SPLITS[-1] or shape == FIN_SHAPES[-1]:
                        ref, extra = gn_reference(c.shape, family, 1, False)
                        win, clean = launch_apply(hip, dev, c, pb.arg, splits, 1)
                        worst_o = max(worst_o, check_output(win, clean, ref, extra))
                        sp64, sclean, spb = launch_stats(hip, dev, c)                  # the same tensor through the statistics pass
                        check_partials(sp64, sclean, c.S64, c.A64, c.Q64, family == "integer")
                        win2, clean2 = launch_apply(hip, dev, c, spb.arg, c.splits, 1)
                        check_output(win2, clean2, ref, extra)
                        if family == "integer":
                            assert torch.equal(win, win2), "exact partials: apply after finalize and after stats must agree bit for bit"
                except AssertionError as e:
                    _fail((shape, family, splits), e)
    report(f"norm-edges finalize: {len(FIN_SHAPES)} shapes x {len(FIN_SPLITS)} splits x 2 families, worst partial at {worst_p:.3f}, worst "
           f"element of the apply that follows at {worst_o:.3f} of the bound; worst relative rstd error (reported) {_fmt(per)}")


def fp8_scales(ref):
    """(calibrated, tight) q_scale for a float64 result: 448 / max |y|, and 448 / the 99th percentile of |y| (1 % clamped)"""
    a = ref.abs().flatten()
    return 448.0 / float(a.max()), 448.0 / float(torch.quantile(a, 0.99))


def _q32(q):
    return float(torch.tensor(q, dtype=F32))       # the q_scale the kernel sees


@gpu
@pytest.mark.parametrize("silu", (0, 1))
def test_fp8_apply_clamp_and_counter(hip, dev, silu):
    """5. sdv_groupnorm_apply_fp8: calibrated (nothing clamped but the band) and tight (1 % clamped): bytes, clamp, counter; the bf16
    apply leaves the counter alone.  The counter is unset on the way out - the pointer is process-global."""
    c = gn_case(FP8_SHAPE, "random")
    ref, extra = gn_reference(FP8_SHAPE, "random", silu, False)
    p64, clean, pb = launch_stats(hip, dev, c)
    check_partials(p64, clean, c.S64, c.A64, c.Q64, False)
    cal, tight = (_q32(q) for q in fp8_scales(ref))
    cbuf = torch.zeros(3, dtype=torch.int32, device=dev)
    try:
        hip.set_fp8_saturation_counter(cbuf[1:2])
        win, clean = launch_apply(hip, dev, c, pb.arg, c.splits, silu, q=cal)
        n_cal = int(cbuf[1])
        w0, share0, band0 = check_fp8(win, clean, ref, extra, cal, counter=n_cal, label=f"fp8 calibrated silu={silu}")
        assert share0 <= 1.0 / ref.numel() * 4 and band0 <= 1e-3
        cbuf.zero_()
        win, clean = launch_apply(hip, dev, c, pb.arg, c.splits, silu, q=tight)
        n_tight = int(cbuf[1])
        w1, share1, band1 = check_fp8(win, clean, ref, extra, tight, counter=n_tight, label=f"fp8 tight silu={silu}")
        assert 0.005 <= share1 <= 0.02 and band1 <= 1e-3, f"input condition: clamp share {share1}, band share {band1}"
        again, _ = launch_apply(hip, dev, c, pb.arg, c.splits, silu, q=tight)
        assert torch.equal(win, again) and int(cbuf[1]) == 2 * n_tight, "a repeated launch changed bytes or counted differently"
        before = cbuf.clone()
        out, clean = launch_apply(hip, dev, c, pb.arg, c.splits, silu)
        check_output(out, clean, ref, extra)
        assert torch.equal(cbuf, before), "the bf16 apply touched the saturation counter"
        assert int(cbuf[0]) == 0 and int(cbuf[2]) == 0, "a neighbour of the counter was written"
    finally:
        hip.set_fp8_saturation_counter(None)
    cbuf.zero_()
    launch_apply(hip, dev, c, pb.arg, c.splits, silu, q=tight)
    assert int(cbuf.abs().sum()) == 0, "the counter was written after it was unset"


@gpu
def test_layernorm_generic_kernels(hip, dev):
    """6a. layernorm_kernel<1 / 2 / 4> on both sides of nchunk = 64 | 65 and 128 | 129, CLIP's 768 and 1024, rows below, at and
    beyond a block's four rows; twice bit for bit"""
    worst = 0.0
    for C, rows in LN_GENERIC:
        lc = ln_case(C, rows)
        try:
            with launch_kinds(hip) as kinds:
                win, clean = launch_layernorm(hip, dev, lc)
            assert kinds == ["layernorm"]
            worst = max(worst, check_output(win, clean, lc.ref, ACC_EPS * lc.mag))
            assert torch.equal(win, launch_layernorm(hip, dev, lc)[0]), "a repeated launch changed bits"
        except AssertionError as e:
            _fail((C, rows), e)
    report(f"norm-edges layernorm generic: {len(LN_GENERIC)} cases, worst element at {worst:.3f} of the bound")


@gpu
def test_layernorm_320_family_and_misaligned_affine(hip, dev):
    """6b. layernorm320_kernel<8 / 16 / 32> at rows around its rows per block (32, 16, 8); the same cases with gamma / beta 4 bytes
    off a 16-byte boundary (the generic kernel takes them) meet the same bound"""
    worst = {False: 0.0, True: 0.0}
    for C, rows in LN_320:
        lc = ln_case(C, rows)
        for mis in (False, True):
            try:
                with launch_kinds(hip) as kinds:
                    win, clean = launch_layernorm(hip, dev, lc, misaligned=mis)
                assert kinds == ["layernorm"]
                worst[mis] = max(worst[mis], check_output(win, clean, lc.ref, ACC_EPS * lc.mag))
                assert torch.equal(win, launch_layernorm(hip, dev, lc, misaligned=mis)[0]), "a repeated launch changed bits"
            except AssertionError as e:
                _fail((C, rows, mis), e)
    report(f"norm-edges layernorm 320 family: {len(LN_320)} cases, worst element at {worst[False]:.3f} of the bound; gamma / beta "
           f"misaligned (generic kernel) {worst[True]:.3f}")


@gpu
@pytest.mark.parametrize("C", (320, 640, 1280, 520, 1032))
def test_layernorm_rows_are_independent(hip, dev, C):
    """6c. one row of NaN leaves every other output row bit-identical (rows share a wave in the 320 family)"""
    rows = 2 * LN_RPB.get(C, 16) + 5
    lc = ln_case(C, rows)
    base, clean = launch_layernorm(hip, dev, lc)
    check_output(base, clean, lc.ref, ACC_EPS * lc.mag)
    for r in (0, 1, rows // 2, rows - 2, rows - 1):
        x = lc.x.clone()
        x[r] = NAN
        win, clean = launch_layernorm(hip, dev, lc, x=x)
        keep = torch.arange(rows) != r
        assert clean and torch.equal(win[keep], base[keep]), f"C = {C}: NaN in row {r} changed another row"
        assert bool(win[r].isnan().all())


@gpu
def test_rowstats_finalize(hip, dev):
    """7. sdv_rowstats_finalize around its 256 rows per block, 1 / 2 / 5 slots: the panel gate's entitlement on random partials,
    the rounded exact quotient on integer ones; the relative rstd error per row class is reported"""
    worst, per = 0.0, {}
    for rows, slots, C in ROWSTATS:
        for family in FAMILIES:
            rc = rowstats_case(rows, slots, C, family)
            pw = _window(rc.part.reshape(rows, 2 * slots), 2 * slots, 0, 4, 4, F32, dev)
            outs = []
            for _ in range(2):
                ob = OutBuf(rows, 2, 2, 0, F32, dev)
                hip._check(hip.load().sdv_rowstats_finalize(_p(pw), rows, slots, C, EPS, _p(ob.arg), hip._stream()), "sdv_rowstats_finalize")
                torch.cuda.synchronize()
                outs.append(ob.take())
            try:
                w, p = check_rowstats(rc, *outs[0])
                assert torch.equal(outs[0][0], outs[1][0]), "a repeated launch changed bits"
            except AssertionError as e:
                _fail((rows, slots, C, family), e)
            worst = max(worst, w)
            _merge(per, p)
    report(f"norm-edges rowstats_finalize: {2 * len(ROWSTATS)} cases, mean at {worst:.3f} of its bound; worst relative rstd error (reported) {_fmt(per)}")


@gpu
def test_argument_errors(hip, dev):
    """8. what the ABI refuses, before any launch: every output stays NaN.  sdv_groupnorm_apply refuses splits, nimg, HW <= 0 like stats."""
    lib, st = hip.load(), hip._stream()
    x = torch.full((4, 8200), NAN, dtype=BF16, device=dev)
    parts = torch.full((4, 64, 64, 2), NAN, device=dev)
    gm, bt = torch.ones(8200, device=dev), torch.zeros(8200, device=dev)
    y = torch.full((4, 8200), NAN, dtype=BF16, device=dev)
    y8 = torch.full((4, 8200), 171, dtype=torch.uint8, device=dev)
    X, Pp, G, B, Y, Y8 = (_p(t) for t in (x, parts, gm, bt, y, y8))

    def stats(C1, C2, nimg, HW, groups, splits, x2=X):
        return lib.sdv_groupnorm_stats(X, x2, C1, C2, nimg, HW, groups, splits, Pp, st)

    def apply(C1, C2, nimg, HW, groups, splits, x2=X):
        return lib.sdv_groupnorm_apply(X, x2, C1, C2, nimg, HW, groups, splits, Pp, G, B, EPS, 1, Y, st)

    def apply8(C1, C2, nimg, HW, groups, splits, x2=X, q=1.0):
        return lib.sdv_groupnorm_apply_fp8(X, x2, C1, C2, nimg, HW, groups, splits, Pp, G, B, EPS, 1, Y8, q, st)

    bad = dict(c_mod_8=(12, 0, 1, 4, 2, 1), c2_mod_8=(16, 12, 1, 4, 2, 1), groups_65=(520, 0, 1, 4, 65, 1), c_mod_groups=(64, 0, 1, 4, 3, 1),
               splits_0=(64, 0, 1, 4, 32, 0), splits_neg=(64, 0, 1, 4, 32, -1), nimg_0=(64, 0, 0, 4, 32, 1), hw_0=(64, 0, 1, 0, 32, 1),
               hw_neg=(64, 0, 1, -4, 32, 1))
    for name, a in bad.items():
        for fn in (stats, apply, apply8):
            with pytest.raises(hip.SdvHipError):
                hip._check(fn(*a), f"{fn.__name__} {name}")
    for fn in (stats, apply, apply8):
        with pytest.raises(hip.SdvHipError):
            hip._check(fn(32, 32, 1, 4, 32, 1, x2=None), f"{fn.__name__}: C2 > 0 without X2")
    with pytest.raises(hip.SdvHipError):
        hip._check(stats(8200, 0, 1, 1, 8, 1), "stats: C = 8200 needs 65600 bytes of LDS")
    for q in (0.0, -1.0):
        with pytest.raises(hip.SdvHipError):
            hip._check(apply8(64, 0, 1, 4, 32, 1, q=q), "apply_fp8: q_scale <= 0")
    for C in (2056, 12):
        with pytest.raises(hip.SdvHipError):
            hip._check(lib.sdv_layernorm_bf16(X, G, B, EPS, 4, C, Y, st), f"layernorm C = {C}")
    with pytest.raises(hip.SdvHipError):
        hip._check(lib.sdv_groupnorm_finalize(Pp, 64, 64, 4, 1, 4, None, 0, 0, 0, 0, 0, 1, 32, 65, Pp, st), "finalize splits = 65")
    torch.cuda.synchronize()
    assert bool(y.isnan().all()) and bool(parts.isnan().all()) and bool((y8 == 171).all())


# ------------------------------------------------------------------------------------------------
# the checker's own tests (CPU tier): an fp32 stand-in of the documented summation order, and planted errors
# ------------------------------------------------------------------------------------------------
def emulate_stats(c, drop_pixel=False, skip_last_split=False, seam_off=False):
    """CPU stand-in of sdv_groupnorm_stats (never a reference): thread (pixel lane tp, channel) adds its pixels p_begin + tp,
    + PT, ... in order; one thread per group folds [lane][channel of the group] in order.  fp32 [nimg, splits, groups, 2]"""
    x = c.x
    if seam_off:             # the chunk behind the seam read from the first source
        x = x.clone()
        x[..., c.C1:c.C1 + 8] = x[..., c.C1 - 8:c.C1]
    _, PT = thread_geometry(c.C)
    out = torch.zeros(c.nimg, c.splits, c.groups, 2)
    ch = torch.arange(c.groups) * c.cpg
    for sp in range(c.splits - 1 if skip_last_split else c.splits):
        a, b = split_range(c.HW, c.splits, sp)
        lanes = []
        for tp in range(PT):
            s, q = torch.zeros(c.nimg, c.C), torch.zeros(c.nimg, c.C)
            for p in range(a + tp, b, PT):
                if drop_pixel and sp == 0 and p == a + (b - a) // 2:
                    continue
                f = x[:, p]
                s, q = s + f, q + f * f
            lanes.append((s, q))
        fs, fq = torch.zeros(c.nimg, c.groups), torch.zeros(c.nimg, c.groups)
        for s, q in lanes:
            for k in range(c.cpg):
                fs, fq = fs + s[:, ch + k], fq + q[:, ch + k]
        out[:, sp, :, 0], out[:, sp, :, 1] = fs, fq
    return out


def tail_pixels(c):
    """the pixels an apply block handles in its `for (; p < p_end; p += PT)` loop, after the 4-way unrolled one"""
    ppb, nblk = apply_geometry(c.nimg, c.HW, c.C)
    _, PT = thread_geometry(c.C)
    tail = torch.zeros(c.HW, dtype=torch.bool)
    for blk in range(nblk):
        a, b = blk * ppb, min(blk * ppb + ppb, c.HW)
        for tp in range(PT):
            ps = list(range(a + tp, b, PT))
            tail[ps[len(ps) // 4 * 4:]] = True
    return tail


def emulate_apply(c, parts, silu, q=None, count_off=False, group_from_chunk=False, seam_off=False, no_eps=False, no_silu_tail=False,
                  no_clamp=False):
    """CPU stand-in of sdv_groupnorm_apply(_fp8) in fp32, ONE rounding at the end.  -> float64 [nimg, HW, C] (e4m3: the bytes)"""
    x = c.x
    if seam_off:
        x = x.clone()
        x[..., c.C1:c.C1 + 8] = x[..., c.C1 - 8:c.C1]
    mean, rstd = finalise_fp32(parts, float(c.HW - 1 if count_off else c.HW) * float(c.cpg), 0.0 if no_eps else EPS)
    gidx = (torch.arange(c.C) // 8 * 8) // c.cpg if group_from_chunk else c.gidx
    sc = rstd[:, gidx] * c.gamma[None]
    sh = c.beta[None] - mean[:, gidx] * sc
    v = x * sc[:, None] + sh[:, None]
    if silu:
        act = v / (1.0 + torch.exp(-v))
        if no_silu_tail:
            t = tail_pixels(c)
            act[:, t] = v[:, t]
        v = act
    if q is None:
        return v.to(BF16).double()
    t = v * torch.tensor(q, dtype=F32)
    b = _bits(t.clamp(-448.0, 448.0).to(FP8)).clone()
    if no_clamp:
        b[t.abs() > 448.0] = 0x7F
    return b.double()


def emulate_finalize(f, splits, first_block_off=False):
    """CPU stand-in of sdv_groupnorm_finalize: thread = channel, repetitions then blocks in order; one thread per group folds"""
    c = f.gn
    ch = torch.zeros(c.nimg, splits, c.C, 2)
    for s in f.srcs:
        P = s.P[:, :, :s.C].reshape(s.nrep, c.nimg, s.bpi, 2, s.C)
        for sp in range(splits):
            a, b = split_range(s.bpi, splits, sp)
            acc = torch.zeros(c.nimg, 2, s.C)
            for r in range(s.nrep):
                for k in range(a + 1 if first_block_off and b - a > 1 else a, b):
                    acc = acc + P[r, :, k]
            ch[:, sp, s.c0:s.c0 + s.C] = acc.transpose(1, 2)
    out = torch.zeros(c.nimg, splits, c.groups, 2)
    for k in range(c.cpg):
        out = out + ch[:, :, torch.arange(c.groups) * c.cpg + k]
    return out


def emulate_layernorm(lc):
    """two-pass fp32, one rounding at the end"""
    x = lc.x
    mean = x.sum(1, keepdim=True) / lc.C
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) / lc.C + torch.tensor(EPS))
    return (d * rstd * lc.gamma[None] + lc.beta[None]).to(BF16).double()


def emulate_rowstats(rc):
    s, q = torch.zeros(rc.rows), torch.zeros(rc.rows)
    for i in range(rc.slots):
        s, q = s + rc.part[:, i, 0], q + rc.part[:, i, 1]
    inv = torch.tensor(1.0, dtype=F32) / rc.C
    mean = s * inv
    return torch.stack([mean, torch.rsqrt((q * inv - mean * mean).clamp_min(0.0) + torch.tensor(EPS))], 1).double()


def _buffered(t2d, dtype, poke=None):
    """t2d through a CPU OutBuf, as the launch helpers hand it to the checkers: (window float64, clean)"""
    rows, cols = t2d.shape
    ob = OutBuf(rows, cols, cols, 0, dtype, "cpu")
    ob.flat[ob.idx] = t2d.to(dtype)
    if poke is not None:
        ob.flat[poke(ob)] = 0
    return ob.take()


CHECKED_GN = ((2, 200, 320, 0, 32, 3), (1, 130, 640, 320, 32, 2))
CHECKED_LN = ((320, 37), (1032, 37))


def test_input_conditions_hold():
    """the conditions the bounds rest on, for the seeds used: regular groups within |mean| <= 10 sigma (then dvar / var <= 3.03e-3);
    the e4m3 tight scale clamps 0.5 - 2 % and the calibrated one only the maximum; the excluded band holds 0.1 % at the most"""
    from stable_diffusion_videos_amd import hip
    shapes = (APPLY_SHAPES + tuple((n, HW, C, 0, 32, hip.gn_splits(HW)) for n, HW, C in WRAPPER_SHAPES) +
              tuple(fin_case(s, "random").gn.shape for s in FIN_SHAPES))
    nreg = 0
    for shape in shapes:
        c = gn_case(shape, "random")
        assert regular_groups_within_cap(c), shape
        ent = entitlement(c.mean64, c.e2, c.absmean)
        reg = torch.tensor([[k == "regular" for k in row] for row in c.cls])
        nreg += int(reg.sum())
        if bool(reg.any()):
            assert float((3 * ACC_EPS * c.e2 / ent.var)[reg].max()) <= 3.03e-3 + 1e-9
            assert float(((ent.hi - ent.lo) / ent.rstd)[reg].max()) <= 3.1e-3
    assert nreg > 500
    c = gn_case(FP8_SHAPE, "random")
    for silu in (0, 1):
        ref, extra = gn_reference(FP8_SHAPE, "random", silu, False)
        cal, tight = (_q32(q) for q in fp8_scales(ref))
        for q, lo, hi in ((cal, 0.0, 4.0 / ref.numel()), (tight, 0.005, 0.02)):
            vq, a = ref * q, q * extra
            share = float((vq.abs() >= 448.0).double().mean())
            band = float(((vq.abs() > 448.0 - a) & ~(vq.abs() > 448.0 + a)).double().mean())
            assert lo <= share <= hi and band <= 1e-3, (silu, q, share, band)


def test_apply_shapes_reach_the_block_tail():
    """the geometry comments of the shape table: per, PT, pix_per_block and a short last apply block at every shape"""
    want = {(2, 200, 320, 0, 32, 3): (67, 6, 52, 4), (2, 67, 64, 0, 32, 1): (67, 32, 256, 1), (1, 130, 640, 320, 32, 2): (65, 2, 18, 8),
            (2, 37, 128, 0, 32, 4): (10, 16, 128, 1), (1, 9, 64, 0, 32, 4): (3, 32, 256, 1), (1, 5, 64, 0, 32, 4): (2, 32, 256, 1),
            (2, 16, 1280, 1280, 32, 1): (16, 1, 7, 3), (1, 16, 1920, 0, 32, 2): (8, 1, 9, 2), (1, 64, 8, 0, 1, 1): (64, 256, 2048, 1),
            (1, 40, 512, 0, 64, 1): (40, 4, 32, 2), (1, 600, 32, 0, 32, 3): (200, 64, 512, 2)}
    assert set(want) == set(APPLY_SHAPES)
    for shape, (per, PT, ppb, nblk) in want.items():
        nimg, HW, C1, C2, groups, splits = shape
        assert -(-HW // splits) == per and thread_geometry(C1 + C2)[1] == PT and apply_geometry(nimg, HW, C1 + C2) == (ppb, nblk), shape
        assert HW % ppb != 0, shape
        assert thread_geometry(C1 + C2)[1] * (C1 + C2) * 8 <= 65536          # the statistics pass's LDS
    assert split_range(9, 4, 3) == (9, 9) and split_range(5, 4, 3) == (5, 5) and split_range(5, 4, 2) == (4, 5) and split_range(200, 3, 2) == (134, 200)
    assert {C // 8 for C, _ in LN_GENERIC} >= {64, 65, 128, 129, 256, 1}


def test_rowstats_integer_mean_is_two_roundings():
    """sdv_rowstats_finalize is handed inv_c = fl(1 / C) and multiplies: mean = fl(s fl(1 / C)), TWO roundings.  "The fp32 rounding of
    the exact quotient" is therefore no entitlement of a correct kernel: over the integers |s| <= 8 C of the integer family a share of
    them (counted here) lands one fp32 ulp beside fl(s / C), never further (|fl(s fl(1 / C)) - s / C| <= (2^-24 + 2^-24 + 2^-48)
    |s / C|).  check_rowstats holds the kernel to the corrected, equally sharp entitlement: EQUAL to fl(s fl(1 / C)), s the exact sum."""
    for C in (320, 1280):
        s = torch.arange(-8 * C, 8 * C + 1, dtype=F32)
        two, one = (s * (torch.tensor(1.0, dtype=F32) / C)).double(), (s.double() / C).float().double()
        off = two != one
        assert 0.05 < float(off.double().mean()) < 0.6
        assert bool(((two - one).abs() <= _ulp32(one.abs().clamp_min(1e-30))).all())


def test_checker_accepts_the_stand_in():
    """every checker on the stand-in's output: two GroupNorm shapes (both families, both activations, e4m3), finalize, two
    LayerNorm shapes, rowstats"""
    for shape in CHECKED_GN:
        for family in FAMILIES:
            c = gn_case(shape, family)
            parts = emulate_stats(c)
            pw, clean = _buffered(parts.reshape(-1, 2), F32)
            w = check_partials(pw.reshape(parts.shape), clean, c.S64, c.A64, c.Q64, family == "integer")
            assert w <= 0.5, w
            for silu in (0, 1):
                hand = family == "integer"
                src = handmade_partials(c) if hand else parts
                ref, extra = gn_reference(shape, family, silu, hand)
                out = emulate_apply(c, src, silu)
                check_output(*_buffered(out.reshape(-1, c.C), BF16), ref.reshape(-1, c.C), extra.reshape(-1, c.C))
            per, inside = rstd_error_per_class(c, parts.double())
            assert inside
    c = gn_case(FP8_SHAPE, "random")
    ref, extra = gn_reference(FP8_SHAPE, "random", 1, False)
    for q in fp8_scales(ref):
        q = _q32(q)
        b = emulate_apply(c, emulate_stats(c), 1, q=q)
        win, clean = _buffered(b.reshape(-1, c.C), torch.uint8)
        check_fp8(win.reshape(ref.shape), clean, ref, extra, q)
    for shape in (FIN_SHAPES[5], FIN_SHAPES[-1]):
        for family in FAMILIES:
            f = fin_case(shape, family)
            for splits in FIN_SPLITS:
                parts = emulate_finalize(f, splits)
                check_partials(parts.double(), True, *fin_reference(f, splits), family == "integer")
                if family == "integer":          # the blocks add up to the tensor's sums
                    assert torch.equal(parts.sum(1).double(), torch.stack([f.gn.S64.sum(1), f.gn.Q64.sum(1)], -1))
    for C, rows in CHECKED_LN:
        lc = ln_case(C, rows)
        assert check_output(*_buffered(emulate_layernorm(lc), BF16), lc.ref, ACC_EPS * lc.mag) <= 1.0
    for family in FAMILIES:
        rc = rowstats_case(257, 5, 320, family)
        check_rowstats(rc, *_buffered(emulate_rowstats(rc), F32))


def test_checker_rejects_planted_errors():
    """the checkers refuse the stand-in's output with each edge error planted (CPU stand-in only: none of these ran on the GPU)"""
    def refused(fn, *a, **k):
        with pytest.raises(AssertionError):
            fn(*a, **k)

    for shape in CHECKED_GN:
        for family in FAMILIES:
            c = gn_case(shape, family)
            exact = family == "integer"
            good = emulate_stats(c)
            # the partials: one pixel missing, the last split skipped, the seam off by one chunk, a guard written, one left NaN
            mutants = [emulate_stats(c, drop_pixel=True), emulate_stats(c, skip_last_split=True)] + ([emulate_stats(c, seam_off=True)] if c.C2 else [])
            for parts in mutants:
                refused(check_partials, parts.double(), True, c.S64, c.A64, c.Q64, exact)
            if not exact:
                w = ((emulate_stats(c, drop_pixel=True).double()[..., 0] - c.S64).abs() / (ACC_EPS * c.A64).clamp_min(1e-300))[c.A64 > 0].max()
                assert float(w) > 100.0          # far beyond the bound, not just over it
            pw, clean = _buffered(good.reshape(-1, 2), F32, poke=lambda ob: ob.base - 1)
            refused(check_partials, pw.reshape(good.shape), clean, c.S64, c.A64, c.Q64, exact)
            nan = good.clone()
            nan[-1, -1, -1, 1] = NAN
            refused(check_partials, nan.double(), True, c.S64, c.A64, c.Q64, exact)
            # the output
            src = handmade_partials(c) if exact else good
            for silu in (0, 1):
                ref, extra = gn_reference(shape, family, silu, exact)
                ref2, extra2 = ref.reshape(-1, c.C), extra.reshape(-1, c.C)

                def out_refused(out, poke=None):
                    refused(check_output, *_buffered(out.reshape(-1, c.C), BF16, poke), ref2, extra2)

                muts = dict(count_off=True, group_from_chunk=True, no_eps=True)
                if c.C2:
                    muts["seam_off"] = True
                if silu:
                    muts["no_silu_tail"] = True
                for k in muts:
                    if exact and k in ("no_eps",):          # hand-made partials have variance 1: eps is 1e-5 of it, below half an ulp
                        continue
                    out_refused(emulate_apply(c, src, silu, **{k: True}))
                if not exact:                               # statistics with an edge error, then a correct apply
                    out_refused(emulate_apply(c, emulate_stats(c, drop_pixel=True), silu))
                    out_refused(emulate_apply(c, emulate_stats(c, skip_last_split=True), silu))
                good_out = emulate_apply(c, src, silu)
                out_refused(good_out, poke=lambda ob: int(ob.idx[-1, -1]) + 1)          # the first element behind the window
                out_refused(good_out, poke=lambda ob: ob.base - 1)
                left = good_out.clone()
                left[-1, -1, -8:] = NAN                     # the last chunk of the last pixel left unwritten
                out_refused(left)
    c = gn_case(FP8_SHAPE, "random")
    ref, extra = gn_reference(FP8_SHAPE, "random", 1, False)
    tight = _q32(fp8_scales(ref)[1])
    parts = emulate_stats(c)
    refused(check_fp8, emulate_apply(c, parts, 1, q=tight, no_clamp=True), True, ref, extra, tight)          # a missed clamp: NaN bytes
    good = emulate_apply(c, parts, 1, q=tight)
    sat = (ref * tight).abs() >= 448.0
    low = good.clone()
    low[sat.nonzero()[0].unbind()] = 0x76                   # 416: one step below the clamp value
    refused(check_fp8, low, True, ref, extra, tight)
    n64 = int(((ref * tight).abs() > 448.0).sum())
    check_fp8(good, True, ref, extra, tight, counter=n64)
    refused(check_fp8, good, True, ref, extra, tight, counter=0)
    refused(check_fp8, good, True, ref, extra, tight, counter=2 * n64)
    refused(check_fp8, good, False, ref, extra, tight)
    for family in FAMILIES:
        f = fin_case(FIN_SHAPES[-1], family)
        refused(check_partials, emulate_finalize(f, 2, first_block_off=True).double(), True, *fin_reference(f, 2), family == "integer")
    for C, rows in CHECKED_LN:
        lc = ln_case(C, rows)
        out = emulate_layernorm(lc)

        def ln_refused(o, poke=None):
            refused(check_output, *_buffered(o, BF16, poke), lc.ref, ACC_EPS * lc.mag)

        left = out.clone()
        left[-1] = NAN                                      # a tail row left unwritten
        ln_refused(left)
        swapped = out.clone()
        swapped[[9, 10]] = out[[10, 9]]
        ln_refused(swapped)
        ln_refused(out, poke=lambda ob: int(ob.idx[-1, -1]) + 1)          # a row past the tensor written
        x = lc.x
        noeps = ((x - x.mean(1, keepdim=True)) * torch.rsqrt(x.var(1, unbiased=False, keepdim=True)) * lc.gamma[None] + lc.beta[None]).to(BF16).double()
        ln_refused(noeps)
    rc = rowstats_case(257, 5, 320, "random")
    st = emulate_rowstats(rc)
    bad = st.clone()
    bad[256] = st[255]                                      # the first row of the second block taken from its neighbour
    refused(check_rowstats, rc, bad, True)
    bad = st.clone()
    bad[100, 0] += 1e-4 * rc.part[100, :, 0].abs().sum().double() / rc.C
    refused(check_rowstats, rc, bad, True)
    refused(check_rowstats, rc, *_buffered(st, F32, poke=lambda ob: int(ob.idx[-1, -1]) + 1))
    rci = rowstats_case(257, 5, 320, "integer")
    sti = emulate_rowstats(rci)
    sti[7, 0] = torch.nextafter(sti[7, 0].float(), torch.tensor(1e9)).double()
    refused(check_rowstats, rci, sti, True)
