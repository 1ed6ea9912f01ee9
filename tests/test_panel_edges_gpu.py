"""Float64 edge-case gate of the one-wave-per-SIMD panel kernels (csrc/sdv_ffn.hip): sdv_ffn_geglu_bf16, sdv_linear320_bf16 and
sdv_linear640_bf16 - M tails, the panel walk, the store paths (row-major through a buffer descriptor, the per-lane `live` flag of the
feed-forward, the transposed V^T epilogue), the emitted LayerNorm statistics and the independence of rows.

Every case compares EVERY output element with a float64 evaluation of the formulas of sdv_hip.h on the operands the kernel sees:

    linears       |out - ref64| <= 0.5 ulp_bf16 (1 + 1e-3) + 2e-5 mag,          mag = alpha (rstd (sum |x||w| + |mean||s|) + |t|) (+ |r|)
    feed-forward  |out - ref64| <= 0.5 ulp_bf16 (1 + 1e-3) + 1e-5 mag2 + flip,  mag2 = |x| + sum |hid||w2| + |b2|,
                  flip = 4 max_j ulp_bf16(hid_j) max_j |w2_nj|   (hidden activations that round the other way: test_ffn_gpu.py)

(helpers._half_ulp_ratio; the bounds test_ffn_gpu.py already holds these kernels to).  Two launches of every random case must agree
bit for bit.  Emitted statistics (stats_out, N = K) against the float64 statistics of the STORED rows with the entitlement of the
documented one-pass fp32 algorithm, acc_eps = 1e-5 being the project's fp32 accumulation allowance:

    |mean - mean64| <= acc_eps mean64(|y|),     dvar = acc_eps E64[y^2],
    rsqrt(var64 + dvar + eps) - 4 ulp_fp32 <= rstd <= rsqrt(max(var64 - dvar, 0) + eps) + 4 ulp_fp32

(4 ulps: the roundings between the sums and the result plus the hardware rsq's one).  The relative rstd error per row class is
reported, not asserted: it is what a consumer's LayerNorm fold receives for rows with a high |mean| / sigma.

Two input families per shape.  "random": rows like test_ffn_gpu._rows (a common mode of several sigma, sigma in exp(U(-3.4, 0.7))),
the first six rows - when M >= 8 - overwritten with the constants 0, 1, -7.5, 100, 3e-3 and a row with a single non-zero element,
ln_stats the true fp32 statistics of the bf16 rows, weights of test_ffn_gpu._weights / _lin_forms.  "selector": integers in [-8, 8],
channels 0 .. 2 carrying the row code (1, row // 16 + 1, row % 16 + 1), one-hot weights built through the real helpers
(geglu_interleave, ln_fold, ffn_fold_columns, ffn_w2_permute), s = t = 0, alpha none or powers of two: the output must EQUAL
(torch.equal) the selected input - x[pi_b(n)] alpha_b (+ r) for the linears, x[n] + b2[n] + sum_{j = n mod 320} x[sigma(j)] for the
feed-forward (gate rows zero with b1 = 16: gelu(16) = 16 exactly in float64 and in gelu_erf_fast_f, W2 = 1 / 16).

Memory discipline of every launch: `out` is NaN before the launch and a window of a larger NaN allocation - 8 guard rows in front
and behind, in the "slice" layout ldo = N + 16 with the window 8 columns in, in the "contig" layout ldo = N - that must be
bit-unchanged outside the window; x is a window with ldx = K + 24, 8 columns in, NaN rows around it; the residual a window with
ldr = 344 != ldo; ln_stats M rows inside a NaN-padded buffer; stats_out M rows inside a NaN-guarded buffer that must stay NaN
outside; V^T store[1:-1, :, :hw] of a [nimg + 2, 320, hw + pad] NaN allocation.  A row or statistic beyond M that is USED shows as
NaN.  Every launch stays inside the preconditions of sdv_hip.h.

The panel walk - a workgroup handing over from one 128-row panel to the next - is reached with sdv_gemm_set_grid_limit (1, 2 or 3
workgroups for 2 .. 6 panels) and must leave the bits of the unlimited launch.

Worst element, as a fraction of the bound, measured on MI355X (one line per family in the parity report that conftest.report
appends to; the selector family is exact everywhere): tails 0.994 (feed-forward), 0.993 / 0.993 / 0.992 / 0.990 (linear320 bias /
+ residual / q2 / qkv), 0.991 / 0.991 / 0.993 (linear640 bias / q2 / qkv); panel walk the same figures to 0.001 and every walked
launch bit-identical to the unlimited one; V^T 0.990, bit-identical to the row-major launch at every (hw, nimg, pad, limit).  These
are the ONE rounding of the output - half a bf16 ulp is 1 / 1.001 of the bound.  Emitted statistics: the mean at 0.006 - 0.009 of
its bound, every rstd inside its entitlement; worst relative rstd error per row class (reported, W = I): constant rows 7.5e-1
(the row of 100s, the only one whose E[y^2] = 1e4 is large enough: E[y^2] - mean^2 leaves about 1.5e-4 where the variance is 0,
against eps = 1e-5 - rstd comes back near 80 instead of 316; allowed: dvar = 0.1), random rows with |mean| > 10 sigma 4.5e-4 (C = 320) / 7.6e-4 (C = 640), other
random rows 4.8e-6 / 2.9e-5, the single-element row 1e-7; with a residual added (no constant rows left) 7.2e-6.  No case failed:
the kernels honour their contract at every edge listed here - no store past M or beside the window with ldo > N, no row or
statistic beyond M used, rows independent.  Not measured on the GPU: the 2^-22 of test_fold_kstep_carries_24_bits and the planted
errors (CPU stand-in).
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import bf16_round, report
from helpers import _half_ulp_ratio
from stable_diffusion_videos_amd import weights
from test_ffn_gpu import _deinterleave, _lin_forms, _rows, _weights
from test_igemm_edges_gpu import GUARD, OutBuf, _bits, _window

gpu = pytest.mark.gpu          # (not a module-wide pytestmark: the checker's own tests below run in the CPU tier)

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
C = 320
EPS = float(torch.tensor(1e-5, dtype=F32))      # the eps the kernel sees
ACC_EPS = 1e-5
HARD = (0.0, 1.0, -7.5, 100.0, 3e-3)            # constant rows; row len(HARD) holds a single non-zero element
POW2 = (2.0, 0.5, 4.0, 0.25, 8.0, 0.125)        # the selector family's alpha per 320-column block

# form -> kernel ("ffn" / "lin"), K, N, weights of test_ffn_gpu._lin_forms (src), residual, emitted statistics
FORMS = {"ffn": dict(kind="ffn", K=320, N=320, src=None, res=False, stats=False),
         "l320 bias": dict(kind="lin", K=320, N=320, src="bias", res=False, stats=True),
         "l320 bias+res": dict(kind="lin", K=320, N=320, src="bias", res=True, stats=True),
         "l320 q2": dict(kind="lin", K=320, N=320, src="q2", res=False, stats=False),
         "l320 qkv": dict(kind="lin", K=320, N=960, src="qkv", res=False, stats=False),
         "l640 bias": dict(kind="lin", K=640, N=640, src="bias", res=False, stats=True),
         "l640 q2": dict(kind="lin", K=640, N=640, src="q2", res=False, stats=False),
         "l640 qkv": dict(kind="lin", K=640, N=1920, src="qkv", res=False, stats=False),
         # W = I, t = 0: the stored rows ARE the x rows (4. emitted statistics)
         "l320 ident": dict(kind="lin", K=320, N=320, src="ident", res=False, stats=True),
         "l320 ident+res": dict(kind="lin", K=320, N=320, src="ident", res=True, stats=True),
         "l640 ident": dict(kind="lin", K=640, N=640, src="ident", res=False, stats=True)}
KERNEL_FORMS = tuple(f for f, d in FORMS.items() if d["src"] != "ident")
IDENT_FORMS = tuple(f for f, d in FORMS.items() if d["src"] == "ident")
FAMILIES = ("random", "selector")
LAYOUTS = ("slice", "contig")


# ------------------------------------------------------------------------------------------------
# the operations, from the formulas of sdv_hip.h (float64)
# ------------------------------------------------------------------------------------------------
def linear_ref64(x, w, s, t, mean=None, rstd=None, alpha=None, r=None):
    """out[m][n] = alpha[n / 320] rstd_m (x_m . w_n - mean_m s_n + t_n / rstd_m), or x_m . w_n + t_n + r[m][n]; and the magnitudes"""
    M, N = x.shape[0], w.shape[0]
    acc, accmag = x @ w.T, x.abs() @ w.abs().T
    if r is not None:
        return acc + t[None] + r, accmag + t.abs()[None] + r.abs()
    m = torch.zeros((M, 1), dtype=torch.float64) if mean is None else mean.reshape(M, 1)
    rs = torch.ones((M, 1), dtype=torch.float64) if rstd is None else rstd.reshape(M, 1)
    al = torch.ones(N, dtype=torch.float64) if alpha is None else alpha.repeat_interleave(C)
    return (rs * (acc - m * s[None]) + t[None]) * al[None], (rs * (accmag + m.abs() * s.abs()[None]) + t.abs()[None]) * al.abs()[None]


def ffn_ref64(x, mean, rstd, w1, s1, t1, w2, b2, round_hidden=True):
    """out = x + b2 + W2 . (v gelu(g)), [v | g] = rstd (x W1'^T - mean s) + t de-interleaved; the hidden activations rounded to bf16
    once, as the kernel hands them to ff.net.2 (round_hidden=False: the plain formula).  -> ref, mag2, hid"""
    pre = (x @ w1.T - mean.reshape(-1, 1) * s1[None]) * rstd.reshape(-1, 1) + t1[None]
    v, gt = _deinterleave(pre)
    hid = v * F.gelu(gt)
    if round_hidden:
        hid = hid.to(BF16).double()
    return x + hid @ w2.T + b2[None], x.abs() + hid.abs() @ w2.abs().T + b2.abs()[None], hid


def row_stats64(y):
    mean = y.mean(1)
    e2 = (y * y).mean(1)
    return mean, e2, (e2 - mean * mean).clamp_min(0.0), y.abs().mean(1)


def _ulp32(v):
    return torch.exp2(torch.floor(torch.log2(v)) - 23)


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def sel_channel(b, j, K):
    """selector linears: output column 320 b + j copies this input channel - the row code for j < 3, else a walk over K that differs
    per block and touches every 8-channel chunk"""
    return j if j < 3 else (37 * j + 101 * b + 5) % K


def sel_sigma(j):
    """selector feed-forward: hidden channel j copies this x channel"""
    return (37 * j + 11 * (j // C)) % C


@functools.lru_cache(maxsize=None)
def _lin_weights(K):
    from stable_diffusion_videos_amd import hip
    return _lin_forms(hip, "cpu", K)


@functools.lru_cache(maxsize=None)
def _ffn_weights():
    return _weights("cpu")


def _true_stats(x):
    """what the producer's epilogue emits (test_ffn_gpu._rows): fp32 (mean, rstd) of the bf16 rows"""
    return torch.stack([x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-5)], 1).contiguous()


def random_rows(M, K, seed):
    """-> x [M, K] fp32 (bf16 values), its fp32 statistics, the class of every row"""
    x = _rows(M, "cpu", seed, K=K)[0].float()
    cls = ["random"] * M
    if M >= 8:
        for i, c in enumerate(HARD):
            x[i] = float(torch.tensor(c).to(BF16))
            cls[i] = "constant"
        x[len(HARD)] = 0.0
        x[len(HARD), 77] = 3.0
        cls[len(HARD)] = "single element"
    return x, _true_stats(x), cls


def selector_rows(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (M, K), generator=g).float()
    rows = torch.arange(M)
    x[:, :3] = torch.stack([torch.ones(M), rows // 16 + 1.0, rows % 16 + 1.0], 1)
    return x


@functools.lru_cache(maxsize=256)
def make_case(form, M, family):
    """The operands (on the CPU, exactly what the kernel is handed) and the float64 reference of one case."""
    fd = FORMS[form]
    K, N, src = fd["K"], fd["N"], fd["src"]
    seed = 1000 + 7 * M + K + 3 * N + sorted(FORMS).index(form)
    sel = family == "selector"
    c = SimpleNamespace(form=form, M=M, K=K, N=N, family=family, kind=fd["kind"], stats=fd["stats"], st=None, alpha=None, r=None,
                        exact=sel or form in ("l320 ident", "l640 ident"), acc_eps=1e-5 if fd["kind"] == "ffn" else 2e-5)
    if sel:
        c.x, c.cls = selector_rows(M, K, seed), ["selector"] * M
    else:
        c.x, st, c.cls = random_rows(M, K, seed)
    x64 = c.x.double()
    gi = torch.Generator().manual_seed(seed + 1)
    if fd["kind"] == "ffn":
        if sel:
            w1 = torch.zeros((8 * C, C))
            w1[torch.arange(4 * C), torch.tensor([sel_sigma(j) for j in range(4 * C)])] = 1.0
            b1 = torch.cat([torch.zeros(4 * C), torch.full((4 * C,), 16.0)])
            w2 = torch.zeros((C, 4 * C))
            w2[torch.arange(4 * C) % C, torch.arange(4 * C)] = 1.0 / 16.0
            w1p, s1, t1 = weights.ln_fold(weights.geglu_interleave(w1), torch.ones(C), torch.zeros(C), weights.geglu_interleave(b1), "cpu")
            P = dict(w1p=w1p, s1=s1, t1=t1, w1x=weights.ffn_fold_columns(s1, t1), w2=w2.to(BF16), w2p=weights.ffn_w2_permute(w2.to(BF16)),
                     b2=torch.randint(-8, 9, (C,), generator=gi).float())
            c.st = torch.stack([torch.zeros(M), torch.ones(M)], 1)
        else:
            P, c.st = _ffn_weights(), st
        c.P = P
        c.ref, mag2, hid = ffn_ref64(x64, c.st[:, 0].double(), c.st[:, 1].double(), P["w1p"].double(), P["s1"].double(), P["t1"].double(),
                                     P["w2"].double(), P["b2"].double())
        hid_ulp = torch.exp2(torch.floor(torch.log2(hid.abs().clamp_min(1e-30))) - 7)
        flip = 4.0 * hid_ulp.max(1, keepdim=True).values * P["w2"].double().abs().max(1).values[None]
        c.mag = mag2 + flip / c.acc_eps          # (_half_ulp_ratio: 0.5 ulp (1 + 1e-3) + acc_eps mag = ... + 1e-5 mag2 + flip)
        return c
    if sel or src == "ident":
        c.w = torch.zeros((N, K))
        cols = torch.arange(N) if src == "ident" else torch.tensor([sel_channel(n // C, n % C, K) for n in range(N)])
        c.w[torch.arange(N), cols] = 1.0
        c.s, c.t = torch.zeros(N), torch.zeros(N)
        c.wx = weights.ffn_fold_columns(c.s, c.t)
        if sel and src in ("q2", "qkv"):
            c.alpha = torch.tensor(POW2[:N // C])
    else:
        f = _lin_weights(K)[src]
        c.w, c.s, c.t, c.wx = f["w"].float(), f["s"], f["t"], f["wx"]
        c.alpha = f["alpha"]
        if src != "bias":
            c.st = st
    if fd["res"]:
        c.r = torch.randint(-8, 9, (M, C), generator=gi).float() if sel else bf16_round(torch.randn((M, C), generator=gi) * 2.0)
    c.ref, c.mag = linear_ref64(x64, c.w.double(), c.s.double(), c.t.double(), None if c.st is None else c.st[:, 0].double(),
                                None if c.st is None else c.st[:, 1].double(), None if c.alpha is None else c.alpha.double(),
                                None if c.r is None else c.r.double())
    return c


# ------------------------------------------------------------------------------------------------
# THE checker
# ------------------------------------------------------------------------------------------------
def check_stats(case, win, stats):
    """stats [M, 2] (float64 of the fp32 the kernel wrote) against the entitlement of the module docstring; -> the worst ratio of a
    mean error to its bound and, per row class, the worst relative rstd error"""
    assert stats.shape == (case.M, 2)
    assert bool(torch.isfinite(stats).all()), "non-finite statistic: a row left unwritten, or a row beyond M was used"
    mean64, e2, var64, absmean = row_stats64(win)
    dvar = ACC_EPS * e2
    lo, hi = torch.rsqrt(var64 + dvar + EPS), torch.rsqrt((var64 - dvar).clamp_min(0.0) + EPS)
    lo, hi = lo - 4 * _ulp32(lo), hi + 4 * _ulp32(hi)
    dm = (stats[:, 0] - mean64).abs()
    bad = (dm > ACC_EPS * absmean).nonzero()
    assert len(bad) == 0, f"emitted mean of row {int(bad[0])}: {float(stats[bad[0], 0])} vs {float(mean64[bad[0]])} (mean |y| {float(absmean[bad[0]])})"
    bad = ((stats[:, 1] < lo) | (stats[:, 1] > hi)).nonzero()
    assert len(bad) == 0, (f"emitted rstd of row {int(bad[0])} ({case.cls[int(bad[0])]}): {float(stats[bad[0], 1])} outside "
                           f"[{float(lo[bad[0]])}, {float(hi[bad[0]])}]")
    rel = ((stats[:, 1] - torch.rsqrt(var64 + EPS)) * torch.sqrt(var64 + EPS)).abs()
    per_class = {}
    for i, k in enumerate(case.cls):
        if k == "random" and float(mean64[i].abs()) > 10.0 * math.sqrt(float(var64[i])):
            k = "random, |mean| > 10 sigma"
        per_class[k] = max(per_class.get(k, 0.0), float(rel[i]))
    return float((dm / (ACC_EPS * absmean).clamp_min(1e-300)).max()), per_class


def check_against_float64(case, win, guards_clean, stats=None, label=None):
    """THE check of this file: the guards bit-unchanged, every element finite and - exact cases - equal to the float64 value, or
    within the bound of the module docstring; emitted statistics within their entitlement.  Returns the worst ratio to the bound."""
    assert win.shape == case.ref.shape
    finite = bool(torch.isfinite(win).all())
    if case.exact:
        worst = 0.0 if torch.equal(win, case.ref) else float("inf")
    else:
        worst = float(_half_ulp_ratio(win, case.ref, case.mag, acc_eps=case.acc_eps).max()) if finite else float("inf")
    if label is not None:
        report(f"panel-edges {label}: worst element at {worst:.3f} of the bound")
    assert guards_clean, "the kernel wrote outside a window (rows past M, guard rows / columns, stats_out rows past M, V^T guards / pad)"
    assert finite, "non-finite output element: an element left unwritten, or NaN memory (a row or statistic beyond M) was used"
    if case.exact:
        bad = (win != case.ref).nonzero()
        assert worst == 0.0, f"exact case: {len(bad)} elements differ from the selected input, first at {tuple(int(i) for i in bad[0])}"
    assert worst <= 1.0, f"worst element at {worst:.3f} of the bound"
    if case.stats:
        assert stats is not None, "the form emits statistics"
        check_stats(case, win, stats)
    return worst


# ------------------------------------------------------------------------------------------------
# launching a case
# ------------------------------------------------------------------------------------------------
def layout_of(layout, ncols):
    """(c0, ldo) - ldr = 344 differs from both"""
    return (8, ncols + 16) if layout == "slice" else (0, ncols)


LDR = C + 24
_DEVICE_OPERANDS = {}          # id(case) -> its device tensors (make_case's cache holds no GPU memory)


def _stats_window(st, dev):
    buf = torch.full((4 + st.shape[0] + 4, 2), NAN)
    buf[4:4 + st.shape[0]] = st
    return buf.to(dev)[4:4 + st.shape[0]]


def operands(case, dev, poison=None):
    """x, ln_stats, residual as windows of NaN-padded allocations, the weights; cached per case unless a row is poisoned"""
    d = {} if poison is not None else _DEVICE_OPERANDS.setdefault(id(case), {})
    if not d:
        d["case"] = case
        x, st, r = case.x, case.st, case.r
        if poison is not None:
            x = x.clone()
            x[poison] = NAN
            if st is not None:
                st = st.clone()
                st[poison] = NAN
            if r is not None:
                r = r.clone()
                r[poison] = NAN
        d["x"] = _window(x, case.K + 24, 8, 4, 4, BF16, dev)
        d["st"] = _stats_window(st, dev) if st is not None else None
        d["r"] = _window(r, LDR, 8, GUARD, GUARD, BF16, dev) if r is not None else None
        if case.kind == "ffn":
            d.update({k: case.P[k].to(dev) for k in ("w1p", "w1x", "w2p", "b2")})
        else:
            d["w"], d["wx"] = case.w.to(dev, BF16), case.wx.to(dev)
            d["alpha"] = case.alpha.to(dev, F32) if case.alpha is not None else None
    return d


def _view(ob, rows, ncols):
    return ob.flat.as_strided((rows, ncols), (ob.ld, 1), ob.base)


def run_case(hip, dev, case, layout="slice", vt=None, poison=None, label=None, check=True):
    """One launch of `case` into fresh NaN outputs.  vt = (hw, pad): the N = 960 form with the transposed V^T output.
    -> (window float64 [M, N] - V^T moved back behind [Q | K] -, stats float64 or None, worst ratio)"""
    d = operands(case, dev, poison)
    M = case.M
    ncols = 2 * C if vt else case.N
    c0, ldo = layout_of(layout, ncols)
    ob = OutBuf(M, ncols, ldo, c0, BF16, dev)
    out = _view(ob, M, ncols)
    sb = OutBuf(M, 2, 2, 0, F32, dev) if case.stats else None
    if case.kind == "ffn":
        hip.ffn_geglu(d["x"], d["st"], d["w1p"], d["w1x"], d["w2p"], d["b2"], out=out)
    else:
        kw = {}
        if vt:
            hw, pad = vt
            store = torch.full((M // hw + 2, C, hw + pad), NAN, dtype=BF16, device=dev)
            kw = dict(vt=store[1:-1, :, :hw], hw=hw)
        hip.linear320(d["x"], d["w"], d["wx"], ln_stats=d["st"], alpha=d["alpha"], residual=d["r"], out=out, want_stats=case.stats,
                      stats_out=_view(sb, M, 2) if sb is not None else None, **kw)
    torch.cuda.synchronize()
    win, clean = ob.take()
    if vt:
        s = store.cpu()
        win = torch.cat([win, s[1:-1, :, :hw].transpose(1, 2).reshape(M, C).double()], 1)
        s[1:-1, :, :hw] = NAN
        clean = clean and bool((_bits(s) == _bits(torch.full((1,), NAN, dtype=BF16))[0]).all())
    stats = None
    if sb is not None:
        stats, sclean = sb.take()
        clean = clean and sclean
    worst = check_against_float64(case, win, clean, stats, label) if check else None
    return win, stats, worst


class grid_limit:
    """with grid_limit(hip, n): at most n workgroups per persistent launch; the previous limit is restored on the way out"""

    def __init__(self, hip, n):
        self.lib, self.n = hip.load(), n

    def __enter__(self):
        self.prev = self.lib.sdv_gemm_set_grid_limit(self.n)

    def __exit__(self, *exc):
        self.lib.sdv_gemm_set_grid_limit(self.prev)


# ------------------------------------------------------------------------------------------------
# the case tables (walked by test_case_tables_cover_every_form on the CPU tier)
# ------------------------------------------------------------------------------------------------
TAIL_M = (1, 31, 32, 33, 96, 97, 127, 128, 129, 257)
WALKS = ((1, 128 * 2), (1, 128 * 3 + 1), (1, 128 * 4 + 97), (2, 128 * 3), (2, 128 * 5 + 33), (3, 128 * 4 + 127))      # (grid limit, M)
WALK_RANDOM = ((1, 128 * 3 + 1), (2, 128 * 5 + 33), (3, 128 * 4 + 127))
VT_SHAPES = ((128, 1), (128, 3), (256, 2), (384, 1))           # (hw, nimg)
VT_PADS = (8, 64)
VT_LIMITS = (0, 1, 2)
STATS_M = (33, 129)
POISON_M, POISON_ROWS = 129, (0, 31, 32, 127, 128)


def tail_rows(form):
    return [("tails", form, family, layout, M, 0) for M in TAIL_M for family in FAMILIES for layout in LAYOUTS]


def walk_rows(form):
    return [("walk", form, "selector", "slice", M, limit) for limit, M in WALKS] + [("walk", form, "random", "slice", M, limit) for limit, M in WALK_RANDOM]


def vt_rows():
    return [("vt", "l320 qkv", family, (hw, pad), hw * nimg, limit) for hw, nimg in VT_SHAPES for pad in VT_PADS for limit in VT_LIMITS for family in FAMILIES]


def stats_rows():
    return [("stats", form, "random", layout, M, 0) for form in IDENT_FORMS for M in STATS_M for layout in LAYOUTS]


def poison_rows():
    return [("independence", form, "random", "slice", POISON_M, 0) for form in KERNEL_FORMS]


def all_rows():
    return sum((tail_rows(f) + walk_rows(f) for f in KERNEL_FORMS), []) + vt_rows() + stats_rows() + poison_rows()


# ------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------
def _fail(row, e):
    raise AssertionError(f"{row}: {e}") from None


@gpu
@pytest.mark.parametrize("form", KERNEL_FORMS)
def test_tails_and_store_layouts(hip, dev, form):
    """1. every M mod 128 edge (a wave with 1, 31, 32 live rows or none, one and two whole panels, a panel and a row), both families,
    both output layouts, the grid unlimited; two launches of a random case agree bit for bit"""
    worst, rows = 0.0, tail_rows(form)
    for row in rows:
        _, _, family, layout, M, _ = row
        case = make_case(form, M, family)
        try:
            win, stats, r = run_case(hip, dev, case, layout)
            if family == "random":
                again, stats2, _ = run_case(hip, dev, case, layout, check=False)
                assert torch.equal(win, again) and (stats is None or torch.equal(stats, stats2)), "a repeated launch changed bits"
        except AssertionError as e:
            _fail(row, e)
        worst = max(worst, r)
    report(f"panel-edges tails {form}: {len(rows)} cases, worst element at {worst:.3f} of the bound")


@gpu
@pytest.mark.parametrize("form", KERNEL_FORMS)
def test_panel_walk(hip, dev, form):
    """2. one, two and three workgroups walking two to six panels (ragged: workgroup 0 walks one more than workgroup 1): the float64
    gate, and the bits of the unlimited launch - the walk only changes who computes a panel"""
    worst, rows = 0.0, walk_rows(form)
    for row in rows:
        _, _, family, layout, M, limit = row
        case = make_case(form, M, family)
        try:
            with grid_limit(hip, 0):
                base, bstats, _ = run_case(hip, dev, case, layout)
            with grid_limit(hip, limit):
                win, stats, r = run_case(hip, dev, case, layout)
            assert torch.equal(win, base) and (stats is None or torch.equal(stats, bstats)), f"grid limit {limit} changed bits"
        except AssertionError as e:
            _fail(row, e)
        worst = max(worst, r)
    report(f"panel-edges walk {form}: {len(rows)} cases bit-identical to the unlimited launch, worst element at {worst:.3f} of the bound")


@gpu
@pytest.mark.parametrize("hw,nimg", VT_SHAPES)
def test_transposed_v(hip, dev, hw, nimg):
    """3. the fused Q K V projection with V^T: [Q | K] and V^T bit for bit the row-major N = 960 launch, unlimited and with one and
    two workgroups (a workgroup crosses sample boundaries); guard samples and pad columns untouched (run_case's `clean`)"""
    worst = 0.0
    for row in [r for r in vt_rows() if r[3][0] == hw and r[4] == hw * nimg]:
        _, form, family, (_, pad), M, limit = row
        case = make_case(form, M, family)
        try:
            with grid_limit(hip, 0):
                base, _, _ = run_case(hip, dev, case, "slice")
            with grid_limit(hip, limit):
                win, _, r = run_case(hip, dev, case, "slice", vt=(hw, pad))
            assert torch.equal(win, base), "[Q | K] / V^T differ from the row-major launch"
        except AssertionError as e:
            _fail(row, e)
        worst = max(worst, r)
    report(f"panel-edges V^T {nimg} samples of {hw} tokens: bit-identical to the row-major launch, worst element at {worst:.3f} of the bound")


@gpu
@pytest.mark.parametrize("form", IDENT_FORMS)
def test_emitted_statistics(hip, dev, form):
    """4. W = I, t = 0: the stored rows are the x rows bit for bit (the checker's exact branch; + r: the half-ulp bound), their emitted
    statistics within the one-pass entitlement; the relative rstd error per row class is reported"""
    classes, worst_mean = {}, 0.0
    for row in [r for r in stats_rows() if r[1] == form]:
        _, _, family, layout, M, _ = row
        case = make_case(form, M, family)
        try:
            win, stats, _ = run_case(hip, dev, case, layout)
            rm, per = check_stats(case, win, stats)
        except AssertionError as e:
            _fail(row, e)
        worst_mean = max(worst_mean, rm)
        for k, v in per.items():
            classes[k] = max(classes.get(k, 0.0), v)
    report(f"panel-edges statistics {form}: mean at {worst_mean:.3f} of its bound; worst relative rstd error " +
           ", ".join(f"{k}: {v:.1e}" for k, v in sorted(classes.items())))


@gpu
@pytest.mark.parametrize("form", KERNEL_FORMS)
def test_rows_are_independent(hip, dev, form):
    """5. a token is an MFMA column: one row of NaN (x, ln_stats, residual) leaves every other output row and statistic bit-identical"""
    case = make_case(form, POISON_M, "random")
    base, bstats, _ = run_case(hip, dev, case)
    for r in POISON_ROWS:
        win, stats, _ = run_case(hip, dev, case, poison=r, check=False)
        keep = torch.arange(case.M) != r
        assert torch.equal(win[keep], base[keep]), f"{form}: NaN in row {r} changed rows {sorted(set((win[keep] != base[keep]).nonzero()[:, 0].tolist()))[:8]}"
        assert stats is None or torch.equal(stats[keep], bstats[keep]), f"{form}: NaN in row {r} changed another row's statistics"


@gpu
def test_bindings_refuse_what_the_gate_relies_on(hip, dev):
    """6. a misaligned x window (ldx % 8 != 0; 4 columns in) and V^T with hw % 128 != 0 raise SdvHipError before any launch"""
    lin, ffn = make_case("l320 qkv", 128, "random"), make_case("ffn", 128, "random")
    dl, df = operands(lin, dev), operands(ffn, dev)
    out = torch.full((128, 2 * C), NAN, dtype=BF16, device=dev)
    for ld, c0 in ((C + 20, 8), (C + 24, 4)):
        bad = _window(lin.x, ld, c0, 4, 4, BF16, dev)
        with pytest.raises(hip.SdvHipError):
            hip.linear320(bad, dl["w"], dl["wx"], ln_stats=dl["st"], alpha=dl["alpha"], out=torch.full((128, 3 * C), NAN, dtype=BF16, device=dev))
        with pytest.raises(hip.SdvHipError):
            hip.ffn_geglu(bad, df["st"], df["w1p"], df["w1x"], df["w2p"], df["b2"], out=out[:, :C])
    store = torch.full((2, C, 64), NAN, dtype=BF16, device=dev)
    with pytest.raises(hip.SdvHipError):
        hip.linear320(dl["x"], dl["w"], dl["wx"], ln_stats=dl["st"], alpha=dl["alpha"], out=out, vt=store, hw=64)
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool(store.isnan().all())


# ------------------------------------------------------------------------------------------------
# the gate must bite, the tables must stay whole (CPU tier)
# ------------------------------------------------------------------------------------------------
def split3(v):
    """fp32 -> three bf16 pieces, as the kernel's split3 and weights.ffn_fold_columns: h + m + l = v to 24 bits"""
    h = bf16_round(v)
    m = bf16_round(v - h)
    return h, m, bf16_round(v - h - m)


def token_vector(mean, rstd):
    """the token side of the fold k-step (sdv_ffn.hip load_x): fp32 [M, 16] of bf16 values"""
    mh, mm, ml = split3(-mean.float())
    rh, rm, rl = split3(1.0 / rstd.float())
    z = torch.zeros_like(mh)
    return torch.stack([mh, mm, mh, ml, mh, mm, rh, rm, rh, rl, rh, rm, z, z, z, z], 1)


def fold_kstep(tok, wx):
    """the k-step's products summed in fp32, K position by K position: [M, N]"""
    acc = torch.zeros((tok.shape[0], wx.shape[0]))
    for k in range(16):
        acc = acc + tok[:, k:k + 1] * wx[:, k].float()[None]
    return acc


def emulate_stats(out_bf16_values):
    """the kernel's one-pass fp32 statistics of the stored rows"""
    y = out_bf16_values.float()
    n = y.shape[1]
    mean = y.sum(1) * (1.0 / n)
    var = ((y * y).sum(1) * (1.0 / n) - mean * mean).clamp_min(0.0)
    return torch.stack([mean, torch.rsqrt(var + EPS)], 1).double()


def emulate_kernel(case):
    """CPU stand-in for the kernel's OUTPUT (never a reference): the kernel's formula on the kernel's layouts - interleaved W1, the
    fold k-step against ffn_fold_columns, hidden activations rounded to bf16 and handed to ffn_w2_permute's K order - in fp32, ONE
    rounding at the end.  -> (out float64 [M, N], stats float64 or None)"""
    M = case.M
    mean = case.st[:, 0] if case.st is not None else torch.zeros(M)
    rstd = case.st[:, 1] if case.st is not None else torch.ones(M)
    tok = token_vector(mean, rstd)
    if case.kind == "ffn":
        P = case.P
        pre = (case.x @ P["w1p"].float().T + fold_kstep(tok, P["w1x"])) * rstd[:, None]
        tiles = pre.reshape(M, -1, 2, 16)                                       # 32-row tiles [16 value | 16 gate]
        hid = bf16_round(tiles[:, :, 0] * F.gelu(tiles[:, :, 1]))             # [M, 80, 16]: hidden channels 16 i + (8 b + 4 a + e)
        hid = hid.reshape(M, -1, 2, 2, 4).permute(0, 1, 3, 2, 4).reshape(M, -1)   # K position 8 a + 4 b + e: the accumulator hand-over
        out = bf16_round(case.x + P["b2"][None] + hid @ P["w2p"].float().T)
        return out.double(), None
    acc = case.x @ case.w.T + fold_kstep(tok, case.wx)
    if case.r is not None:
        out = bf16_round(case.r + acc)
    else:
        al = torch.ones(case.N) if case.alpha is None else case.alpha.repeat_interleave(C)
        out = bf16_round(acc * (rstd[:, None] * al[None]))
    return out.double(), emulate_stats(out) if case.stats else None


def _in_buffers(case, out64, stats64, poke=None, poke_stats=None):
    """out64 / stats64 as the windows of CPU OutBufs (the slice layout) -> what run_case hands the checker"""
    c0, ldo = layout_of("slice", case.N)
    ob = OutBuf(case.M, case.N, ldo, c0, BF16, "cpu")
    ob.flat[ob.idx] = out64.to(BF16)
    if poke is not None:
        ob.flat[poke(ob)] = 0.0
    win, clean = ob.take()
    stats = None
    if stats64 is not None:
        sb = OutBuf(case.M, 2, 2, 0, F32, "cpu")
        sb.flat[sb.idx] = stats64.float()
        if poke_stats is not None:
            sb.flat[poke_stats(sb)] = 0.0
        stats, sclean = sb.take()
        clean = clean and sclean
    return win, clean, stats


def test_reference_matches_the_definition():
    """float64, 1e-12 of the magnitudes; the bf16 rounding of W' is on both sides.  With TRUE statistics (and s the exact row sums)
    rstd (x W'^T - mean s) + t is F.layer_norm without affine followed by W' and t; the feed-forward reference (hidden rounding off)
    is x + F.linear(v gelu(g), W2, b2) with [v | g] from the UN-interleaved W1"""
    for K in (320, 640):
        x = random_rows(129, K, 5)[0].double()
        mean, var = x.mean(1), x.var(1, unbiased=False)
        rstd = torch.rsqrt(var + 1e-5)
        for src in ("q2", "qkv"):
            f = _lin_weights(K)[src]
            w, t, al = f["w"].double(), f["t"].double(), f["alpha"].double()
            ref, mag = linear_ref64(x, w, w.sum(1), t, mean, rstd, al)
            want = (F.layer_norm(x, (K,), eps=1e-5) @ w.T + t[None]) * al.repeat_interleave(C)[None]
            assert float(((ref - want).abs() / mag).max()) < 1e-12, (K, src)
        f = _lin_weights(K)["bias"]
        ref, mag = linear_ref64(x, f["w"].double(), f["s"].double(), f["t"].double())
        assert float(((ref - F.linear(x, f["w"].double(), f["t"].double())).abs() / mag).max()) < 1e-12
    x = random_rows(129, C, 6)[0].double()
    mean, rstd = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-5)
    g = torch.Generator().manual_seed(1)
    w1 = bf16_round(torch.randn(8 * C, C, generator=g) * C ** -0.5).double()           # un-interleaved [value | gate], already W'
    b1, w2, b2 = torch.randn(8 * C, generator=g).double() * 0.2, bf16_round(torch.randn(C, 4 * C, generator=g) / 36).double(), torch.randn(C, generator=g).double()
    w1i, b1i = weights.geglu_interleave(w1), weights.geglu_interleave(b1)
    ref, mag2, _ = ffn_ref64(x, mean, rstd, w1i, w1i.sum(1), b1i, w2, b2, round_hidden=False)
    pre = F.layer_norm(x, (C,), eps=1e-5) @ w1.T + b1[None]
    want = x + F.linear(pre[:, :4 * C] * F.gelu(pre[:, 4 * C:]), w2, b2)
    assert float(((ref - want).abs() / mag2).max()) < 1e-12
    r = bf16_round(torch.randn(129, C, generator=g)).double()
    f = _lin_weights(C)["bias"]
    ref, mag = linear_ref64(x, f["w"].double(), f["s"].double(), f["t"].double(), r=r)
    assert float(((ref - (F.linear(x, f["w"].double(), f["t"].double()) + r)).abs() / mag).max()) < 1e-12


def test_selector_construction_is_exact():
    """The operands the helpers build make the kernel's formula - evaluated by the CPU stand-in on the kernel's layouts - return the
    selected integers exactly, for every form; the reference agrees with the closed form of the module docstring."""
    for form in KERNEL_FORMS:
        for M in (33, 129):
            case = make_case(form, M, "selector")
            out, stats = emulate_kernel(case)
            if case.kind == "ffn":
                want = case.x + case.P["b2"][None] + sum(case.x[:, [sel_sigma(n + C * q) for n in range(C)]] for q in range(4))
            else:
                want = case.x[:, [sel_channel(n // C, n % C, case.K) for n in range(case.N)]]
                if case.alpha is not None:
                    want = want * case.alpha.repeat_interleave(C)[None]
                if case.r is not None:
                    want = want + case.r
            assert torch.equal(case.ref, want.double()), form
            assert float(want.abs().max()) < 256 and torch.equal(bf16_round(want), want)      # integers (times 2^k): exact in bf16
            assert torch.equal(out, case.ref), form
            assert check_against_float64(case, *_in_buffers(case, out, stats)) == 0.0


def test_fold_kstep_carries_24_bits():
    """The twelve products of the token vector and a ffn_fold_columns row, summed in fp32, are - mean s + t / rstd to 2^-22 of
    |mean s| + |t / rstd|.  Derivation: a value v = h + m + l in three bf16 pieces (round to nearest, 8 bits each) leaves
    |v - (h + m + l)| <= 2^-27 |v|; the k-step keeps the six leading cross terms of each product a b (a_h b_h, a_h b_m, a_m b_h,
    a_h b_l, a_l b_h, a_m b_m) and drops a_m b_l + a_l b_m + a_l b_l <= (2 * 2^-27 + 2^-36) |a b|: with the two residuals about
    2^-25 |a b| - "24-bit splits less the dropped cross terms".  1 / rstd is one fp32 division (2^-24 |t / rstd|).  Products of two
    bf16 are exact in fp32, so what is left is the rounding of the additions, which depends on their order (the matrix core's is
    its own).  Summed here per product, the five cross terms (<= 2^-8 of it) first and the leading term last, then the two products:
    each product's sum rounds once at its own scale (2^-24 |a b|; the cross terms' own additions round at 2^-32), the last addition
    at 2^-24 of the result: (1 + 1 + 1 + 1 / 2) 2^-24 = 0.875 * 2^-22 at the most.  (In plain K order - eleven roundings at the
    scale of the sum - the worst of these 4096 draws is 1.24 * 2^-22: not measured on the GPU, a property of this CPU sum.)"""
    g = torch.Generator().manual_seed(11)
    n = 4096
    mean = torch.randn(n, generator=g) * torch.exp(torch.empty(n).uniform_(-6, 6, generator=g))
    rstd = torch.exp(torch.empty(n).uniform_(-4, 6, generator=g))
    s = torch.randn(n, generator=g) * torch.exp(torch.empty(n).uniform_(-6, 3, generator=g))
    t = torch.randn(n, generator=g) * torch.exp(torch.empty(n).uniform_(-6, 3, generator=g))
    tok, wx = token_vector(mean, rstd), weights.ffn_fold_columns(s, t).float()
    assert bool((tok[:, 12:] == 0).all()) and bool((wx[:, 12:] == 0).all())
    part = []
    for order in ((3, 4, 5, 1, 2, 0), (9, 10, 11, 7, 8, 6)):          # K positions of (- mean) s and of t / rstd, the leading term last
        acc = torch.zeros(n)
        for k in order:
            acc = acc + tok[:, k] * wx[:, k]
        part.append(acc)
    got = part[0] + part[1]
    ms, tr = mean.double() * s.double(), t.double() / rstd.double()
    err = (got.double() - (tr - ms)).abs() / (ms.abs() + tr.abs())
    assert float(err.max()) <= 2.0 ** -22, float(err.max()) * 2.0 ** 22


def test_checker_rejects_planted_errors():
    """The checker accepts the stand-in's output and refuses it with each edge error planted."""
    def refused(case, out, stats, **poke):
        with pytest.raises(AssertionError):
            check_against_float64(case, *_in_buffers(case, out, stats, **poke))

    M = 129
    cases = [make_case(form, M, family) for form in KERNEL_FORMS for family in FAMILIES]
    for c in cases:
        out, stats = emulate_kernel(c)
        assert check_against_float64(c, *_in_buffers(c, out, stats)) <= 1.0, (c.form, c.family)
        o = out.clone()                                    # two rows of a panel swapped
        o[[9, 40]] = o[[40, 9]]
        refused(c, o, stats)
        o = out.clone()                                    # a 16-byte chunk taken from the neighbouring row
        o[33, 64:72] = out[34, 64:72]
        refused(c, o, stats)
        if c.N > C:                                        # a 320-column block shifted to the next block
            o = out.clone()
            o[:, C:2 * C] = out[:, :C]
            refused(c, o, stats)
        refused(c, out, stats, poke=lambda ob: int(ob.idx[-1, 0]) + ob.ld)          # a row past M written
        refused(c, out, stats, poke=lambda ob: ob.base - 1)                         # a guard column written
        refused(c, out, stats, poke=lambda ob: int(ob.idx[7, -1]) + 1)
        o = out.clone()                                    # a row left NaN
        o[M - 1] = NAN
        refused(c, o, stats)
        if c.form == "l320 qkv":                           # V^T tokens shifted by 8 (run_case moves V^T back behind [Q | K])
            o = out.clone()
            o[:, 2 * C:] = out[:, 2 * C:].roll(8, 0)
            refused(c, o, stats)
        if c.stats:
            st = stats.clone()                             # a stats_out row taken from the clamped row M - 1
            st[M - 2] = stats[M - 1]
            refused(c, out, st)
            refused(c, out, stats, poke_stats=lambda sb: int(sb.idx[-1, 0]) + 2)    # a stats_out row past M written
            st = stats.clone()
            st[40] = NAN
            refused(c, out, st)
        if c.exact:                                        # one bf16 ulp in a selector case
            o = out.clone()
            o[70, 11] = o[70, 11] + torch.exp2(torch.floor(torch.log2(o[70, 11].abs().clamp_min(1.0))) - 7)
            refused(c, o, stats)
    for form in IDENT_FORMS:                               # the statistics gate on the hard rows: an rstd taken from fp32 TWO-pass
        c = make_case(form, M, "random")                   # statistics of a neighbour row, a mean off by 1e-4 of the row scale
        out, stats = emulate_kernel(c)
        assert check_against_float64(c, *_in_buffers(c, out, stats)) <= 1.0, form
        st = stats.clone()
        st[50, 0] += 1e-4 * out[50].abs().mean()
        refused(c, out, st)
        st = stats.clone()
        st[50, 1] = stats[51, 1]
        refused(c, out, st)


def test_case_tables_cover_every_form():
    """Every kernel form runs in both families and both layouts at every tail, walks panels under every (limit, M) pair, is poisoned;
    the selector maps touch every 8-channel chunk; every window keeps the ABI's alignment - so that a later edit cannot thin the
    tables silently."""
    rows = all_rows()
    assert set(KERNEL_FORMS) == {"ffn", "l320 bias", "l320 bias+res", "l320 q2", "l320 qkv", "l640 bias", "l640 q2", "l640 qkv"}
    by = {}
    for group, form, family, layout, M, limit in rows:
        by.setdefault(group, set()).add((form, family, layout, M, limit))
    assert set(by) == {"tails", "walk", "vt", "stats", "independence"}
    assert by["tails"] == {(f, fam, lay, M, 0) for f in KERNEL_FORMS for fam in FAMILIES for lay in LAYOUTS for M in TAIL_M}
    assert {M % 128 for M in TAIL_M} >= {1, 31, 32, 33, 96, 97, 127, 0}
    for f in KERNEL_FORMS:
        assert {(M, lim) for ff, fam, _, M, lim in by["walk"] if ff == f and fam == "selector"} == {(M, lim) for lim, M in WALKS}
        assert {lim for ff, fam, _, M, lim in by["walk"] if ff == f and fam == "random"} == {1, 2, 3}
    for limit, M in WALKS:
        panels = -(-M // 128)
        assert panels > limit and M <= 700            # every workgroup walks; (2, .): 3 and 6 panels - one ragged, one even split
    assert {(-(-M // 128)) % 2 for lim, M in WALKS if lim == 2} == {0, 1}
    assert by["vt"] == {("l320 qkv", fam, (hw, pad), hw * n, lim) for hw, n in VT_SHAPES for pad in VT_PADS for lim in VT_LIMITS for fam in FAMILIES}
    assert by["stats"] == {(f, "random", lay, M, 0) for f in IDENT_FORMS for lay in LAYOUTS for M in STATS_M}
    assert by["independence"] == {(f, "random", "slice", POISON_M, 0) for f in KERNEL_FORMS} and max(POISON_ROWS) < POISON_M
    for K in (320, 640):
        for b in range(3 * K // C):
            cols = [sel_channel(b, j, K) for j in range(C)]
            assert len(set(cols[3:])) == C - 3 and {ch // 8 for ch in cols} == set(range(K // 8)), (K, b)
        assert len({tuple(sel_channel(b, j, K) for j in range(C)) for b in range(3 * K // C)}) == 3 * K // C
    assert {sel_sigma(j) // 8 for j in range(4 * C)} == set(range(C // 8))
    assert all(len({sel_sigma(n + C * q) for q in range(4)}) == 4 for n in range(C))
    for ncols in (320, 640, 960, 1920):
        for lay in LAYOUTS:
            c0, ldo = layout_of(lay, ncols)
            assert c0 % 8 == 0 and ldo % 8 == 0 and ldo >= ncols + c0 and ldo != LDR
    assert LDR % 8 == 0 and all(hw % 128 == 0 for hw, _ in VT_SHAPES) and all(p % 8 == 0 for p in VT_PADS)
    hard = make_case("l320 ident", 33, "random")
    assert hard.cls[:6] == ["constant"] * 5 + ["single element"] and int((hard.x[5] != 0).sum()) == 1
