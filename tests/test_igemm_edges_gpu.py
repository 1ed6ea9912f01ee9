"""Float64 edge-case gate of sdv_gemm_bf16 (csrc/sdv_gemm.hip): conv seams, M / N tails, the three store paths, the typed outputs,
the persistent tile walk, split-K at its smallest, the fp8 forms and the small-channel convs.

Every case compares EVERY output element with a float64 evaluation of the same (bf16 / e4m3) operands,

    |out - ref64| <= 0.5 ulp_bf16 (1 + 1e-3) + acc_eps * mag,     mag = sum |x||w| |alpha| + |bias| + |residual|

(helpers._half_ulp_ratio; acc_eps = 1e-5 for bf16 operands - test_kernels_gpu.py::test_gemm_is_correctly_rounded's bound - and 4e-5
for the fp8 forms - test_fp8_mx_form_matches_float64_on_exact_products').  Activation epilogues (epi 2 - 5): ref and mag go through
the activation in float64, the accumulation term is multiplied by 1.2 (the activations' largest slope) and 1e-6 (1 + |pre|) is added
for the fast transcendentals (sdv_common.h: absolute errors below 1.5e-7 / 0.8e-7).  GEGLU out = v gelu(g): the same reasoning per
factor - mag = mag_v |gelu(g)| + 1.2 |v| mag_g, + 1e-6 |v| (1 + |g|).  fp32 outputs drop the half-ulp term; the image forms are checked
against clamp(...) of the float64 value (out_mode 2 halves the accumulation term and adds the constant 0.5 to mag), their uint8 twin
against rint(255 f32) of the kernel's own fp32.

The reference is a gather written from the operation's definition (conv_geometry: for every output pixel and tap the input pixel
it reads, or none) - no im2col, F.conv2d or kernel code; the CPU tier checks it against F.conv2d.  Shapes are the smallest that
reach an edge: (3, 5, 7) - one tile spans three images plus a tail -, (9, 6, 6) - tile boundaries inside rows and across seams -,
(1, 24, 24) - one image larger than any tile -, (5, 1, 9) and (6, 2, 2) - a circular wrap lands on the pixel itself or its only
neighbour; Cout 328 leaves 8 valid columns in the second 320-wide tile.

Two input families per geometry case.  "random": bf16 randn, weights scaled by K^-0.5, the bound above.  "selector": small integers
that encode (image, y, x), one-hot weights - output channel 8 tap + j copies one input channel of tap `tap` - and no bias: the
output must EQUAL the shifted / wrapped / zero-padded input (torch.equal).

Memory discipline of every launch: the output is NaN before the launch and a window of a larger allocation with NaN guard rows in
front and behind and - when ldc > N - NaN columns beside it, bit-unchanged afterwards; X, X2, R and W are windows of NaN-padded
allocations too, so a halo read that should have been masked, or a row beyond M / column beyond N that is used, shows as NaN.  Every
launch stays inside the ABI's stated preconditions (sdv_hip.h, its "C / R" alignment contract included).

Worst element, as a fraction of the bound, measured on MI355X (one line per family in the parity report that conftest.report
appends to): conv geometry 0.981 - 0.992 (random; the selector family is exact), dense tails 0.993 without and 0.995 with a
residual on all six output variants, batched / typed outputs 0.988, epilogue operands 0.991 - 0.994, activations 0.987 - 0.990,
GEGLU 0.983, two sources 0.983 - 0.990, persistent walk 0.993 - 0.994, split-K 0.982, fp8 0.975 (both forms), small-channel convs
0.996.  These are the ONE rounding of the output - half a bf16 ulp is 1 / 1.001 of the bound; a CPU stand-in of the kernel's
arithmetic gives the same figures.  No case failed: the kernel honours its contract at every edge listed here.
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

gpu = pytest.mark.gpu          # (not a module-wide pytestmark: the checker's own tests below run in the CPU tier)

BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
NAN = float("nan")
GUARD = 8                      # NaN rows in front of and behind every output / residual window
U8_FILL = 171

# tile id -> (BM, BN, waves); 0 = the cost model picks
TILES = {1: (128, 128, 4), 2: (128, 64, 4), 3: (64, 64, 4), 4: (256, 128, 4), 6: (256, 320, 8), 7: (256, 256, 8), 8: (256, 128, 8),
         9: (128, 320, 8), 10: (256, 32, 4), 11: (256, 64, 4)}
ALL_TILES = (0,) + tuple(TILES)
FOUR_WAVE = tuple(t for t, (_, _, w) in TILES.items() if w == 4)
EIGHT_WAVE = tuple(t for t, (_, _, w) in TILES.items() if w == 8)
GEGLU_TILES = (0, 1, 2, 3, 4, 6, 7, 8, 9)
FP8_TILES = (0, 1, 6, 7, 9)
SPLIT_TILES = (0, 1, 2, 3)


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return bf16_round(torch.randn(shape, generator=g) * scale)


def _q8(t):
    """per-tensor e4m3 quantisation as the engine does it (test_kernels_gpu.py::_q8): the quantised VALUES (fp32) and the scale"""
    s = float(t.abs().max()) / 448.0
    return (t / s).to(FP8).float(), s


# ------------------------------------------------------------------------------------------------
# the operation, from its definition
# ------------------------------------------------------------------------------------------------
def out_hw(mode, H, W):
    return {1: (H, W), 2: ((H + 1) // 2, (W + 1) // 2), 3: (2 * H, 2 * W), 4: (2 * H, 2 * W)}[mode]


@functools.lru_cache(maxsize=64)
def conv_geometry(mode, n, H, W, circular):
    """For every OUTPUT pixel (image-major, raster order) and tap: the input pixel index it reads, -1 for a zero.  mode 4 (phase
    form): 2 x 2 taps on the low-resolution grid, plus the phase 2 py + px of every output pixel (its filter)."""
    Ho, Wo = out_hw(mode, H, W)
    img, oy, ox = [t.reshape(-1, 1) for t in torch.meshgrid(torch.arange(n), torch.arange(Ho), torch.arange(Wo), indexing="ij")]
    if mode == 4:
        ty, tx = [t.reshape(1, -1) for t in torch.meshgrid(torch.arange(2), torch.arange(2), indexing="ij")]
        vy, vx, ey, ex = oy // 2 - 1 + oy % 2 + ty, ox // 2 - 1 + ox % 2 + tx, H, W
        phase = (2 * (oy % 2) + ox % 2).reshape(-1)
    else:
        ky, kx = [t.reshape(1, -1) for t in torch.meshgrid(torch.arange(3), torch.arange(3), indexing="ij")]
        st = 2 if mode == 2 else 1
        vy, vx = oy * st + ky - 1, ox * st + kx - 1
        ey, ex = (2 * H, 2 * W) if mode == 3 else (H, W)          # mode 3: the taps move on the upsampled grid
        phase = None
    if circular:
        vy, vx = vy % ey, vx % ex
    ok = (vy >= 0) & (vy < ey) & (vx >= 0) & (vx < ex)
    if mode == 3:
        vy, vx = vy // 2, vx // 2
    src = torch.where(ok, (img * H + vy) * W + vx, torch.full_like(vy, -1))
    return src, phase


def accumulate(x, w, src, phase, N):
    """sum over taps and channels of x[src] * w in x's dtype: [rows, N].  w: [N, taps * K] (phase form: [4 N, 4 K])"""
    rows, taps = src.shape
    cols = (x[src.clamp_min(0)] * (src >= 0).unsqueeze(-1).to(x.dtype)).reshape(rows, taps * x.shape[1])
    if phase is None:
        return cols @ w.T
    out = torch.empty((rows, N), dtype=x.dtype)
    for p in range(4):
        out[phase == p] = cols[phase == p] @ w[p * N:(p + 1) * N].T
    return out


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.special.erf(t / math.sqrt(2.0)))


ACT64 = {2: lambda t: t * torch.sigmoid(t), 3: lambda t: torch.where(t > 0, t, 0.2 * t), 4: lambda t: t * torch.sigmoid(1.702 * t),
         5: _gelu64}


def selector_channel(o, K):
    """input channel that output channel o of the selector family copies: j = o % 8 < 3 -> the (image, y, x) code channels, the
    others walk every 8-channel chunk of [X | X2]"""
    return o % 8 if o % 8 < 3 else 8 * ((5 * o + o // 8) % (K // 8)) + o % 8


@functools.lru_cache(maxsize=512)
def make_case(mode, geom, C1, C2, N, circular=False, family="random", bias="col", res=False, epi=0, alpha=1.0, alpha_cols=0,
              out_mode=0, fp8=False, batch=1):
    """The operands (fp32 on the CPU, exactly representable in the kernel's operand type) and the float64 reference of one case.
    geom: (M,) dense, (n, H, W) conv.  bias: None, "col", "table0" / "tableL" (step-indexed table, first / last row), "row"
    (bias_mode 2).  batch > 1 (dense): `batch` row blocks of X against shared W and R."""
    K = C1 + C2
    taps = {0: 1, 4: 4}.get(mode, 9)
    seed = 1000 * mode + 97 * sum(geom) + 7 * len(geom) + K + 3 * N + (5 if circular else 0) + 11 * epi + batch
    if mode == 0:
        rows_in = rows_out = geom[0] * batch
        src, phase = torch.arange(rows_in).reshape(-1, 1), None
        code = torch.stack([torch.ones(rows_in), torch.arange(rows_in) // 16 + 1.0, torch.arange(rows_in) % 16 + 1.0], 1)
    else:
        n, H, W = geom
        assert batch == 1
        rows_in = n * H * W
        src, phase = conv_geometry(mode, n, H, W, circular)
        rows_out = src.shape[0]
        code = torch.stack([t.reshape(-1) + 1.0 for t in torch.meshgrid(torch.arange(n), torch.arange(H), torch.arange(W), indexing="ij")], 1)
    geglu = epi == 1
    if family == "selector":
        assert N == 72 and bias is None and not res and epi == 0 and not out_mode and not fp8
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.randint(-8, 9, (rows_in, K), generator=g).float()
        x[:, :3] = code                                                    # (image + 1, y + 1, x + 1): never 0 where a pixel is
        w3 = torch.zeros((N, K, 3, 3))
        for o in range(N):
            tap = (o // 8) % 9 if mode else 4
            w3[o, selector_channel(o, K), tap // 3, tap % 3] = 1.0
    else:
        x = _rnd((rows_in, K), seed)
        w3 = _rnd((N, K, 3, 3), seed + 1, (9 * K) ** -0.5 if mode else K ** -0.5)
    if mode == 0:
        w = w3[:, :, 1, 1].contiguous()
    elif mode == 4:
        w = weights.upconv_phase_w(w3, "cpu").float()                      # coincident taps summed in fp32, rounded once: the kernel's W
    else:
        w = w3.permute(0, 2, 3, 1).reshape(N, 9 * K).contiguous()          # OHWI
    if fp8:
        (x, sx), (w, sw) = _q8(x), _q8(w)
        alpha = alpha * sx * sw
    table, step, bvec = None, 0, None
    if bias in ("table0", "tableL"):
        table, step = _rnd((3, N), seed + 2), (0 if bias == "table0" else 2)
        bvec = table[step]
    elif bias == "col":
        bvec = _rnd((N,), seed + 2)
    elif bias == "row":
        assert mode == 0 and batch == 1
        bvec = _rnd((rows_out,), seed + 2)
    ncols = N // 2 if geglu else N
    r = _rnd((rows_out // batch, ncols), seed + 3) if res else None

    x64, w64 = x.double(), w.double()
    av = torch.full((N,), float(alpha), dtype=torch.float64)
    if alpha_cols:
        av[alpha_cols:] = 1.0
    acc, accmag = accumulate(x64, w64, src, phase, N), accumulate(x64.abs(), w64.abs(), src, phase, N)
    b64 = torch.zeros((1, N), dtype=torch.float64) if bvec is None else (bvec.double().reshape(-1, 1) if bias == "row" else bvec.double().reshape(1, -1))
    pre, premag = acc * av + b64, accmag * av.abs() + b64.abs()
    acc_eps = 4e-5 if fp8 else 1e-5
    half_ulp = out_mode == 0
    if geglu:
        half = N // 2
        v, gt, vm, gm = pre[:, :half], pre[:, half:], premag[:, :half], premag[:, half:]
        ref = v * _gelu64(gt)
        mag = vm * _gelu64(gt).abs() + 1.2 * v.abs() * gm + (1e-6 / acc_eps) * v.abs() * (1 + gt.abs())
    else:
        if r is not None:
            r64 = r.double().repeat(batch, 1)
            pre, premag = pre + r64, premag + r64.abs()
        if epi >= 2:
            ref = ACT64[epi](pre)
            mag = 1.2 * ACT64[epi](premag) + (1e-6 / acc_eps) * (1 + pre.abs())
        elif out_mode == 2:
            ref, mag = (pre / 2 + 0.5).clamp(0, 1), 0.5 * premag + 0.5
        elif out_mode == 3:
            ref, mag = pre.clamp(0, 1), premag
        else:
            ref, mag = pre, premag
    return SimpleNamespace(mode=mode, geom=geom, C1=C1, C2=C2, K=K, N=N, ncols=ncols, circular=circular, family=family, bias=bias,
                           bias_mode=2 if bias == "row" else 1, epi=epi, alpha=float(alpha), alpha_cols=alpha_cols, out_mode=out_mode,
                           fp8=fp8, batch=batch, x=x, w=w, bvec=bvec, table=table, step=step, r=r, src=src, phase=phase,
                           rows_in=rows_in, rows_out=rows_out, ref=ref, mag=mag, acc_eps=acc_eps, half_ulp=half_ulp,
                           exact=family == "selector")


# ------------------------------------------------------------------------------------------------
# the output window inside its guards, and THE checker
# ------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


class OutBuf:
    """`batch` windows of [rows, ncols] elements, leading dimension ld, `sC` elements apart, the first one c0 columns into row GUARD
    of one flat allocation that ends GUARD rows behind the last window; everything is NaN (uint8: 171) before the launch."""

    def __init__(self, rows, ncols, ld, c0, dtype, device, batch=1, sC=0):
        self.base, self.ld = GUARD * ld + c0, ld
        self.sC = sC if batch > 1 else 0
        size = self.base + (batch - 1) * self.sC + rows * ld + GUARD * ld
        self.flat = torch.full((size,), U8_FILL if dtype == torch.uint8 else NAN, dtype=dtype, device=device)
        self.fill_bits = _bits(torch.full((1,), U8_FILL if dtype == torch.uint8 else NAN, dtype=dtype))[0].item()
        b, m, c = torch.meshgrid(torch.arange(batch), torch.arange(rows), torch.arange(ncols), indexing="ij")
        self.idx = (self.base + b * self.sC + m * ld + c).reshape(batch * rows, ncols)
        self.arg = self.flat[self.base:]          # what the kernel gets as C / out_f32 / out_u8

    def take(self):
        """the windows as float64 [batch * rows, ncols] and whether every element outside them still holds the fill's bits"""
        flat = self.flat.cpu()
        win = flat[self.idx].double()
        bits = _bits(flat).clone()
        bits[self.idx] = self.fill_bits
        return win, bool((bits == self.fill_bits).all())


def check_against_float64(win, guards_clean, case, label=None):
    """THE check of this file: the guards bit-unchanged, every element finite and - selector family - equal to the float64 value,
    or within the bound of the module docstring.  Returns the worst ratio to that bound (and reports it first, when given a label)."""
    assert win.shape == case.ref.shape
    finite = bool(torch.isfinite(win).all())
    if case.exact:
        worst = 0.0 if torch.equal(win, case.ref) else float("inf")
    elif case.half_ulp:
        worst = float(_half_ulp_ratio(win, case.ref, case.mag, acc_eps=case.acc_eps).max())
    else:
        worst = float(((win - case.ref).abs() / (case.acc_eps * case.mag)).max())
    if not finite:
        worst = float("inf")
    if label is not None:
        report(f"igemm-edges {label}: worst element at {worst:.3f} of the bound")
    assert guards_clean, "the kernel wrote outside its output window (guard rows / columns beside the window)"
    assert finite, "non-finite output element: an element left unwritten, or NaN memory (a halo, a row beyond M, a column beyond N) was used"
    if case.exact:
        bad = (win != case.ref).nonzero()
        assert worst == 0.0, f"selector: {len(bad)} elements differ from the shifted input, first at {tuple(int(i) for i in bad[0])}"
    assert worst <= 1.0, f"worst element at {worst:.3f} of the bound"
    return worst


# ------------------------------------------------------------------------------------------------
# launching a case
# ------------------------------------------------------------------------------------------------
def _ru(v, m):
    return (v + m - 1) // m * m


def layout(variant, ncols):
    """(c0, ldc, r0, ldr) of the four output variants; ldr != ldc in all of them"""
    if variant == "contig":                    # no columns beside the window; staged where ncols % 8 == 0
        return 0, ncols, 0, _ru(ncols, 8) + 8
    if variant == "slice16":                   # a column slice 16 bytes into rows of ldc % 8 == 0: the staged path
        return 8, _ru(ncols, 8) + 16, 8, _ru(ncols, 8) + 24
    if variant == "slice8":                    # 8 bytes into rows of ldc % 4 == 0: the register-direct 8-byte path
        return 4, _ru(ncols, 8) + 12, 4, _ru(ncols, 8) + 20
    if variant == "slice8of8":                 # 8 (not 16) bytes into rows of ldc % 8 == 0: the kernel's POINTER test declines the
        return 4, _ru(ncols, 8) + 16, 4, _ru(ncols, 8) + 24          # staged path, the 8-byte path takes over
    if variant == "mixed":                     # ldc % 4 == 0, ldr % 4 != 0: a vector-capable C forced onto the scalar path by R
        return 8, _ru(ncols, 8) + 16, 4, _ru(ncols, 4) + 6
    assert variant == "scalar"                 # ldc % 4 != 0
    return 4, _ru(ncols, 4) + 9, 4, _ru(ncols, 4) + 6


def _window(t2d, ld, c0, front, back, dtype, dev):
    """t2d as a window of a NaN allocation [front + rows + back, ld], c0 columns in"""
    rows, cols = t2d.shape
    buf = torch.full((front + rows + back, ld), NAN)
    buf[front:front + rows, c0:c0 + cols] = t2d
    return buf.to(dtype).to(dev)[front:front + rows, c0:c0 + cols]


_DEVICE_OPERANDS = {}          # id(case) -> its device tensors: apart from make_case's cache of CPU cases, which holds no GPU memory


def operands(case, dev):
    """X (X2), W, bias on the device, made once per case: column prefixes of wider NaN-padded buffers with NaN rows around them"""
    d = _DEVICE_OPERANDS.setdefault(id(case), {})
    if not d:
        d["case"] = case                       # (keeps id(case) unique for as long as the entry lives)
        dt, c0 = (FP8, 16) if case.fp8 else (BF16, 8)
        d["x"] = _window(case.x[:, :case.C1], case.C1 + 2 * c0, c0, 4, 4, dt, dev)
        d["x2"] = _window(case.x[:, case.C1:], case.C2 + 3 * c0, c0, 4, 4, dt, dev) if case.C2 else None
        w = weights.geglu_interleave(case.w) if case.epi == 1 else case.w
        d["w"] = _window(w, w.shape[1], 0, 0, 4, dt, dev)
        b = case.table if case.table is not None else case.bvec
        if b is not None and case.epi == 1:
            b = weights.geglu_interleave(b)
        d["bias"] = b.to(dev) if b is not None else None
        d["step"] = torch.tensor([case.step], dtype=torch.int32, device=dev) if case.table is not None else None
    return d


def run_case(hip, dev, case, tile, variant="slice16", sC=0, gn=False, label=None, check=True):
    """One launch of `case` on `tile` into a fresh NaN output; returns (window float64, worst ratio, OutBuf(s))."""
    d = operands(case, dev)
    c0, ldc, r0, ldr = layout(variant, case.ncols)
    rows = case.rows_out // case.batch
    if case.out_mode:
        c0, ldc = (0, case.ncols) if variant == "contig" else (4, case.ncols + 8)
    ob = OutBuf(rows, case.ncols, ldc, c0, F32 if case.out_mode else BF16, dev, case.batch, sC or rows * ldc)
    u8 = OutBuf(rows, case.ncols, ldc, c0, torch.uint8, dev) if case.out_mode >= 2 else None
    res = _window(case.r, ldr, r0, GUARD, GUARD, BF16, dev) if case.r is not None else None
    kw = dict(M=rows, Hin=0, Win=0, Hout=0, Wout=0)
    if case.mode:
        n, H, W = case.geom
        Ho, Wo = (H, W) if case.mode == 4 else out_hw(case.mode, H, W)
        kw = dict(M=n * Ho * Wo, Hin=H, Win=W, Hout=Ho, Wout=Wo)
    hip.gemm(d["x"], d["w"], None if case.out_mode else ob.arg, N=case.N, K=case.K, ldx=d["x"].stride(0), ldw=d["w"].stride(0), ldc=ldc,
             bias=d["bias"], bias_mode=case.bias_mode, residual=res, ldr=ldr if res is not None else 0, x2=d["x2"],
             C1=case.C1 if case.C2 else 0, ldx2=d["x2"].stride(0) if case.C2 else 0, alpha=case.alpha, epi=case.epi, mode=case.mode,
             circular=case.circular, batch=case.batch, sX=rows * d["x"].stride(0) if case.batch > 1 else 0, sW=0,
             sC=ob.sC, sR=0, step_ptr=d["step"], bias_step_stride=case.N if d["step"] is not None else 0, tile=tile,
             alpha_cols=case.alpha_cols, out_mode=case.out_mode, out_f32=ob.arg if case.out_mode else None,
             out_u8=u8.arg if u8 is not None else None, gn_hw=rows if gn else 0, **kw)
    torch.cuda.synchronize()
    win, clean = ob.take()
    worst = check_against_float64(win, clean, case, label) if check else None
    if u8 is not None:                        # round-half-even of 255 x the kernel's own fp32, in fp32 as the kernel computes it
        w8, clean8 = u8.take()
        assert clean8 and torch.equal(w8, (win.float() * 255.0).round().double()), "uint8 image output != rint(255 f32)"
    return win, worst, ob


def _sweep(hip, dev, name, rows):
    """run every (case, tile, keywords) row, report the family's worst ratio in ONE line"""
    worst, where = 0.0, None
    for case, tile, kw in rows:
        try:
            _, r, _ = run_case(hip, dev, case, tile, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: mode {case.mode} geom {case.geom} C1 {case.C1} C2 {case.C2} N {case.N} circular {case.circular} "
                                 f"{case.family} bias {case.bias} epi {case.epi} tile {tile} {kw}: {e}") from None
        if r >= worst:
            worst, where = r, (case.geom, case.K, case.N, tile)
    report(f"igemm-edges {name}: {len(rows)} launches, worst element at {worst:.3f} of the bound {where}")


# ------------------------------------------------------------------------------------------------
# the case tables (walked by test_case_tables_cover_every_tile on the CPU tier)
# ------------------------------------------------------------------------------------------------
SHAPES = [((3, 5, 7), 64, 72), ((3, 5, 7), 128, 328), ((9, 6, 6), 128, 40), ((1, 24, 24), 64, 328), ((5, 1, 9), 64, 40), ((6, 2, 2), 64, 72)]
SHAPES_S2 = SHAPES + [((1, 9, 9), 64, 40), ((2, 6, 6), 128, 72)]
SHAPES_UP = [((3, 3, 5), 64, 72), ((3, 3, 5), 128, 328), ((2, 4, 4), 128, 40), ((5, 1, 9), 64, 40), ((6, 2, 2), 64, 72)]
GEOMETRY_SHAPES = {1: SHAPES, 2: SHAPES_S2, 3: SHAPES_UP, 4: SHAPES_UP}
GEOMETRY_PARAMS = [(mode, circular, family) for mode in (1, 2, 3, 4) for circular in (False, True) for family in ("random", "selector")]


def geometry_rows(mode, circular, family):
    sel = family == "selector"
    return [(("geometry", mode, circular, family), tile, dict(mode=mode, geom=g, C1=cin, C2=0, N=72 if sel else cout, circular=circular,
                                                               family=family, bias=None if sel else "col"), {})
            for g, cin, cout in GEOMETRY_SHAPES[mode] for tile in ALL_TILES]


VARIANTS = ("contig", "slice16", "slice8", "slice8of8", "mixed", "scalar")
DENSE_PARAMS = [(variant, res) for variant in VARIANTS for res in (False, True) if res or variant != "mixed"]


def dense_rows(variant, res):
    return [(("dense", variant, res), tile, dict(mode=0, geom=(M,), C1=K, C2=0, N=N, res=res), dict(variant=variant))
            for M in (1, 33, 129, 257) for N in (8, 40, 77, 130, 328) for K in (64, 192) for tile in ALL_TILES]


def typed_rows():
    rows = [(("typed", "batch2 sR=0"), tile, dict(mode=0, geom=(33,), C1=64, C2=0, N=40, res=True, batch=2), dict(variant=v))
            for tile in ALL_TILES for v in ("slice16", "slice8", "scalar")]
    for tile in (0,) + FOUR_WAVE:
        rows += [(("typed", "f32"), tile, dict(mode=0, geom=(33,), C1=64, C2=0, N=4, out_mode=1), dict(variant="slice16")),
                 (("typed", "f32"), tile, dict(mode=0, geom=(129,), C1=64, C2=0, N=77, out_mode=1), dict(variant="contig")),
                 (("typed", "f32"), tile, dict(mode=0, geom=(33,), C1=64, C2=0, N=40, out_mode=1, batch=3), dict(variant="slice16", sC=33 * 48 + 6)),
                 (("typed", "f32"), tile, dict(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=4, out_mode=1), dict(variant="contig"))]
    for tile in FOUR_WAVE:
        rows += [(("typed", f"image {om}"), tile, dict(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=3, out_mode=om, alpha=a), dict(variant=v))
                 for om, a in ((2, 3.0), (3, 2.0)) for v in ("contig", "slice16")]
    return rows


def epilogue_rows():
    rows = []
    for tile in ALL_TILES:
        for b in ("table0", "tableL"):
            rows.append((("epilogue", "bias table"), tile, dict(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=72, bias=b, res=True), {}))
            rows.append((("epilogue", "bias table"), tile, dict(mode=0, geom=(129,), C1=64, C2=0, N=130, bias=b), dict(variant="slice8")))
        for M in (33, 257):
            rows.append((("epilogue", "bias_mode 2"), tile, dict(mode=0, geom=(M,), C1=64, C2=0, N=72, bias="row", alpha=0.25), {}))
            rows.append((("epilogue", "bias_mode 2"), tile, dict(mode=0, geom=(M,), C1=64, C2=0, N=77, bias="row", alpha=0.25), dict(variant="scalar")))
        for ac in (8, 136, 320):
            rows.append((("epilogue", "alpha_cols"), tile, dict(mode=0, geom=(129,), C1=64, C2=0, N=328, alpha=0.37, alpha_cols=ac), {}))
            rows.append((("epilogue", "alpha_cols"), tile, dict(mode=0, geom=(129,), C1=64, C2=0, N=328, alpha=0.37, alpha_cols=ac, res=True),
                         dict(variant="slice8")))
        for v in ("slice16", "slice8", "scalar"):
            rows.append((("epilogue", "epi 2"), tile, dict(mode=0, geom=(129,), C1=64, C2=0, N=72 if v != "scalar" else 77, epi=2, res=v == "slice16"),
                         dict(variant=v)))
        rows.append((("epilogue", "epi 2"), tile, dict(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=328, epi=2), {}))
    for tile in (0,) + FOUR_WAVE:
        for epi in (3, 4, 5):
            for v in ("slice16", "slice8", "scalar"):
                rows.append((("epilogue", f"epi {epi}"), tile, dict(mode=0, geom=(129,), C1=64, C2=0, N=40 if v != "scalar" else 77, epi=epi), dict(variant=v)))
            rows.append((("epilogue", f"epi {epi}"), tile, dict(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=72, epi=epi, res=True), {}))
    for tile in GEGLU_TILES:
        for N in (96, 672):
            for v in ("slice16", "slice8"):
                rows.append((("epilogue", "geglu"), tile, dict(mode=0, geom=(129,), C1=64, C2=0, N=N, epi=1), dict(variant=v)))
    return rows


TWO_SOURCE_PARAMS = [(mode, family) for mode in (0, 1, 2) for family in ("random", "selector")]


def two_source_rows(mode, family):
    sel = family == "selector"
    return [(("two sources", mode, family), tile, dict(mode=mode, geom=(129,) if mode == 0 else (3, 5, 7), C1=c1, C2=c2, N=72, circular=circ,
                                                       family=family, bias=None if sel else "col", res=not sel), {})
            for c1, c2 in ((64, 128), (128, 64), (64, 64)) for circ in ((False,) if mode == 0 else (False, True)) for tile in ALL_TILES]


def walk_rows():
    """(group, tile, case keywords, number of output tiles) - 5 and 7 tiles of each 8-wave tile, with 9 (odd), 1 (odd) and 2 (even)
    K slabs per tile: the LDS slot of a tile's first slab alternates from tile to tile in the odd runs and stays put in the even one"""
    rows = []
    for tile in EIGHT_WAVE:
        BM = TILES[tile][0]
        for ntiles in (5, 7):
            nimg = ((ntiles - 1) * BM) // 121 + 1          # 11 x 11 pixels per image: the last tile is partly filled
            assert (ntiles - 1) * BM < nimg * 121 <= ntiles * BM
            rows.append((("walk", "conv 9 slabs"), tile, dict(mode=1, geom=(nimg, 11, 11), C1=64, C2=0, N=40), ntiles))
            for K in (64, 128):
                rows.append((("walk", f"dense {K // 64} slabs"), tile, dict(mode=0, geom=((ntiles - 1) * BM + 33,), C1=K, C2=0, N=72, res=True), ntiles))
    return rows


def split_rows():
    rows = []
    for tile in SPLIT_TILES:
        for g in ((1, 4, 4), (3, 5, 7)):
            rows.append((("split-K", "conv 2 splits"), tile, dict(mode=1, geom=g, C1=256, C2=0, N=72, res=True), {}))
            for c1, c2 in ((64, 192), (192, 64)):
                rows.append((("split-K", "two sources"), tile, dict(mode=1, geom=g, C1=c1, C2=c2, N=72, bias="tableL", res=True), {}))
            rows.append((("split-K", "conv 4 splits"), tile, dict(mode=1, geom=g, C1=512, C2=0, N=72, circular=True, bias="table0"), {}))
            for mode in (2, 3):
                rows.append((("split-K", f"mode {mode}"), tile, dict(mode=mode, geom=g, C1=256, C2=0, N=72, circular=True, bias="tableL", res=True), {}))
        for K in (2048, 2112):
            rows.append((("split-K", "dense"), tile, dict(mode=0, geom=(33,), C1=K, C2=0, N=72, res=True), {}))
    return rows


FP8_PARAMS = [1, 2]


def fp8_rows(form):
    rows = []
    for tile in FP8_TILES:
        for cin in (64, 128):
            for circ in (False, True):
                rows.append((("fp8", form), tile, dict(mode=1, geom=(3, 5, 7), C1=cin, C2=0, N=72, circular=circ, fp8=True, res=True), {}))
        for K in (64, 192):
            rows.append((("fp8", form), tile, dict(mode=0, geom=(33,), C1=K, C2=0, N=72, fp8=True), {}))
    return rows


def all_tables():
    """family -> (rows, the tiles every group of that family has to run on)"""
    t = {"geometry": (sum((geometry_rows(*p) for p in GEOMETRY_PARAMS), []), ALL_TILES),
         "dense": (sum((dense_rows(*p) for p in DENSE_PARAMS), []), ALL_TILES),
         "two sources": (sum((two_source_rows(*p) for p in TWO_SOURCE_PARAMS), []), ALL_TILES),
         "walk": (walk_rows(), EIGHT_WAVE),
         "split-K": (split_rows(), SPLIT_TILES),
         "fp8": (sum((fp8_rows(f) for f in FP8_PARAMS), []), FP8_TILES)}
    typed, epi = typed_rows(), epilogue_rows()
    t["typed: bf16 batch"] = ([r for r in typed if r[0][1].startswith("batch")], ALL_TILES)
    t["typed: f32"] = ([r for r in typed if r[0][1] == "f32"], (0,) + FOUR_WAVE)
    t["typed: image"] = ([r for r in typed if r[0][1].startswith("image")], FOUR_WAVE)
    t["epilogue operands"] = ([r for r in epi if r[0][1] in ("bias table", "bias_mode 2", "alpha_cols", "epi 2")], ALL_TILES)
    t["epilogue activations"] = ([r for r in epi if r[0][1] in ("epi 3", "epi 4", "epi 5")], (0,) + FOUR_WAVE)
    t["epilogue geglu"] = ([r for r in epi if r[0][1] == "geglu"], GEGLU_TILES)
    return t


def _cases(rows):
    return [(make_case(**kw), tile, extra) for _, tile, kw, extra in rows]


# ------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,circular,family", GEOMETRY_PARAMS)
def test_conv_geometry(hip, dev, mode, circular, family):
    """1. seams, tails and wraps of every conv form on every tile"""
    _sweep(hip, dev, f"conv geometry mode {mode} {'circular' if circular else 'zero'} {family}", _cases(geometry_rows(mode, circular, family)))


@gpu
@pytest.mark.parametrize("variant,res", DENSE_PARAMS)
def test_dense_tails_and_store_paths(hip, dev, variant, res):
    """2. M and N tails through the staged, the 8-byte and the scalar store path, with and without a residual of another ld"""
    _sweep(hip, dev, f"dense tails {variant}{' +residual' if res else ''}", _cases(dense_rows(variant, res)))


@gpu
def test_batched_and_typed_outputs(hip, dev):
    """2. batch 2 against a shared residual; fp32 outputs (N = 4, ldc = 77, a batch stride that is no multiple of 4); image outputs"""
    _sweep(hip, dev, "batched / typed outputs", _cases(typed_rows()))


@gpu
def test_epilogue_operands_at_the_tails(hip, dev):
    """3. bias table rows, per-row bias, alpha_cols across a tile edge, every activation, GEGLU with one output group in the last tile"""
    rows = epilogue_rows()
    for group in sorted({r[0][1] for r in rows}):
        _sweep(hip, dev, f"epilogue {group}", _cases([r for r in rows if r[0][1] == group]))


@gpu
@pytest.mark.parametrize("mode,family", TWO_SOURCE_PARAMS)
def test_two_sources(hip, dev, mode, family):
    """4. [X | X2] as column prefixes of two wider NaN-padded buffers"""
    _sweep(hip, dev, f"two sources mode {mode} {family}", _cases(two_source_rows(mode, family)))


@gpu
@pytest.mark.parametrize("tile", EIGHT_WAVE)
def test_persistent_tile_walk(hip, dev, tile):
    """5. the 8-wave tiles walking 5 and 7 output tiles with 1, 2 and 3 workgroups: the float64 gate, and the bits of the same
    launch with the limit off and with one workgroup per tile (sdv_hip.h: "bit-identical results")"""
    lib = hip.load()
    prev_limit, prev_persist = lib.sdv_gemm_set_grid_limit(0), lib.sdv_gemm_set_persistent(1)
    worst = 0.0
    try:
        for _, t, kw, ntiles in [r for r in walk_rows() if r[1] == tile]:
            case = make_case(**kw)
            BM, BN, _ = TILES[t]
            assert -(-case.rows_out // BM) * -(-case.N // BN) == ntiles
            base, r, _ = run_case(hip, dev, case, t)
            worst = max(worst, r)
            for limit, persist in ((1, 1), (2, 1), (3, 1), (0, 0)):
                lib.sdv_gemm_set_grid_limit(limit)
                lib.sdv_gemm_set_persistent(persist)
                win, r, _ = run_case(hip, dev, case, t)
                worst = max(worst, r)
                assert torch.equal(win, base), f"{kw} tile {t}: grid limit {limit} persistent {persist} changed bits"
            lib.sdv_gemm_set_grid_limit(0)
            lib.sdv_gemm_set_persistent(1)
    finally:
        lib.sdv_gemm_set_grid_limit(prev_limit)
        lib.sdv_gemm_set_persistent(prev_persist)
    report(f"igemm-edges persistent walk tile {tile}: worst element at {worst:.3f} of the bound")


@gpu
def test_split_k_at_its_smallest(hip, dev):
    """6. two and four splits, a split that starts inside a (tap, source) segment, an uneven share; the reduce kernel's statistics"""
    worst = 0.0
    for group, tile, kw, _ in split_rows():
        case = make_case(**kw)
        win, r, _ = run_case(hip, dev, case, tile)
        assert hip.LAST_SPLIT_K >= (4 if group[1] == "conv 4 splits" and tile else 2), f"{kw} tile {tile}: meant to take the split-K path ({hip.LAST_SPLIT_K})"
        again, _, _ = run_case(hip, dev, case, tile)
        assert torch.equal(win, again), f"{kw} tile {tile}: a repeated split launch changed bits"
        worst = max(worst, r)
    report(f"igemm-edges split-K: worst element at {worst:.3f} of the bound")
    for tile in SPLIT_TILES:          # N = 72: the second 64-column block of the reduce kernel holds 8 columns
        case = make_case(mode=1, geom=(2, 4, 4), C1=256, C2=0, N=72, res=True)
        win, _, ob = run_case(hip, dev, case, tile, gn=True)
        assert hip.LAST_SPLIT_K >= 2
        g = ob.arg._sdv_gn.p.cpu().double()                   # [blocks of 32 rows, (sum, sumsq), N]
        of = win.view(-1, 32, case.N)
        assert torch.allclose(g[:, 0], of.sum(1), rtol=1e-5, atol=1e-4) and torch.allclose(g[:, 1], (of * of).sum(1), rtol=1e-5, atol=1e-4), tile


@gpu
@pytest.mark.parametrize("form", FP8_PARAMS)
def test_fp8_forms(hip, dev, form, monkeypatch):
    """7. e4m3 operands: nine K images (the MX form's last slab is half dead), eighteen, one and three"""
    monkeypatch.setattr(hip, "FP8_MX", form - 1)
    _sweep(hip, dev, f"fp8 form {form}", _cases(fp8_rows(form)))


@gpu
def test_small_channel_convs(hip, dev):
    """8. conv3x3_cin_small (Cin 4 and 8) and conv3x3_c4 (im2col + GEMM): the same checker; the im2col rows against a CPU gather"""
    worst = 0.0
    for geom in ((3, 5, 7), (5, 1, 9)):
        n, H, W = geom
        for circular in (False, True):
            for cin, cout in ((4, 72), (8, 40)):
                case = make_case(mode=1, geom=geom, C1=64, C2=0, N=cout, circular=circular)
                # the SAME case with all but the first `cin` channels zero: x and w of the small kernels are its leading channels
                x = case.x[:, :cin]
                w = case.w.view(cout, 9, 64)[:, :, :cin]
                small = SimpleNamespace(**{**vars(case), "ref": None})
                acc = accumulate(x.double(), w.reshape(cout, -1).double(), case.src, None, cout)
                small.ref = acc + case.bvec.double()
                small.mag = accumulate(x.double().abs(), w.reshape(cout, -1).double().abs(), case.src, None, cout) + case.bvec.double().abs()
                xb = _window(x, cin, 0, 16, 16, BF16, dev)
                wb = _window(w.reshape(cout, -1), 9 * cin, 0, 0, 4, BF16, dev)
                ob = OutBuf(case.rows_out, cout, cout, 0, BF16, dev)
                hip.conv3x3_cin_small(xb, wb, case.bvec.to(dev), nimg=n, H=H, W=W, circular=circular, out=ob.arg)
                torch.cuda.synchronize()
                worst = max(worst, check_against_float64(*ob.take(), small))
                if cin == 4:
                    cols = OutBuf(case.rows_out, 64, 64, 0, BF16, dev)
                    torch.ops.sdv.k_im2col3x3_c4(xb, cols.arg, n, H, W, circular)
                    torch.cuda.synchronize()
                    got, clean = cols.take()
                    want = torch.zeros((case.rows_out, 64), dtype=torch.float64)
                    want[:, :36] = (x.double()[case.src.clamp_min(0)] * (case.src >= 0).unsqueeze(-1)).reshape(-1, 36)
                    assert clean and torch.equal(got, want), f"im2col rows {geom} circular {circular}"
                    ob = OutBuf(case.rows_out, cout, cout, 0, BF16, dev)
                    hip.conv3x3_c4(xb, weights.conv_w_c4(w.permute(0, 2, 1).reshape(cout, 4, 3, 3), dev), case.bvec.to(dev), nimg=n, H=H, W=W,
                                   circular=circular, out=ob.arg.view(-1)[:case.rows_out * cout].view(case.rows_out, cout))
                    torch.cuda.synchronize()
                    worst = max(worst, check_against_float64(*ob.take(), small))
    report(f"igemm-edges small-channel convs: worst element at {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------------
# the gate must bite, the tables must stay whole (CPU tier)
# ------------------------------------------------------------------------------------------------
def emulate_kernel(case, src=None, bias_row=None):
    """CPU stand-in for the kernel's OUTPUT (never a reference): fp32 products and sums of the bf16 operands, alpha / bias /
    residual in fp32, ONE rounding.  `src`: the gather table to use (the planted errors change it)."""
    acc = accumulate(case.x, case.w, case.src if src is None else src, case.phase, case.N) * case.alpha
    if case.bvec is not None:
        acc = acc + (case.table[bias_row] if bias_row is not None else case.bvec)
    if case.r is not None:
        acc = acc + case.r
    return bf16_round(acc).double()


def _in_buffer(case, out64, poke=None):
    """out64 as the window of a CPU OutBuf (the slice16 layout) -> what OutBuf.take() hands the checker"""
    c0, ldc, _, _ = layout("slice16", case.ncols)
    ob = OutBuf(case.rows_out, case.ncols, ldc, c0, BF16, "cpu")
    ob.flat[ob.idx] = out64.to(BF16)
    if poke is not None:
        ob.flat[poke(ob)] = 0.0
    return ob.take()


def test_reference_gather_matches_conv2d():
    """conv_geometry + accumulate - the reference of this file - against F.conv2d on F.pad / F.interpolate in float64"""
    for mode in (1, 2, 3, 4):
        for circular in (False, True):
            for n, H, W in ((3, 5, 7), (5, 1, 9), (6, 2, 2), (1, 9, 9), (2, 6, 6)):
                case = make_case(mode=mode if mode != 4 else 3, geom=(n, H, W), C1=64, C2=0, N=40, circular=circular)
                x = case.x.double().view(n, H, W, 64).permute(0, 3, 1, 2)
                w = case.w.double().view(40, 3, 3, 64).permute(0, 3, 1, 2)
                if mode >= 3:
                    x = F.interpolate(x, scale_factor=2.0, mode="nearest")
                x = F.pad(x, (1, 1, 1, 1), mode="circular" if circular else "constant")
                want = F.conv2d(x, w, case.bvec.double(), stride=2 if mode == 2 else 1).permute(0, 2, 3, 1).reshape(-1, 40)
                if mode != 4:
                    assert torch.allclose(case.ref, want, rtol=1e-12, atol=1e-12), (mode, circular, n, H, W)
                else:       # the phase form with UNROUNDED phase filters is the same function
                    src, phase = conv_geometry(4, n, H, W, circular)
                    w3 = case.w.double().view(40, 3, 3, 64).permute(0, 3, 1, 2)
                    groups = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
                    w4 = torch.stack([torch.stack([w3[:, :, groups[py][ty]][:, :, :, groups[px][tx]].sum((2, 3)) for ty in (0, 1) for tx in (0, 1)], 1)
                                      for py in (0, 1) for px in (0, 1)]).reshape(4 * 40, 4 * 64)
                    got = accumulate(case.x.double(), w4, src, phase, 40) + case.bvec.double()
                    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), (mode, circular, n, H, W)


def test_checker_rejects_planted_edge_errors():
    """The checker accepts the stand-in and refuses it with each edge error planted."""
    def refused(case, out64, poke=None):
        with pytest.raises(AssertionError):
            check_against_float64(*_in_buffer(case, out64, poke), case)

    def row(case, img, y, x):
        n, H, W = case.geom
        return (img * H + y) * W + x

    zero = [make_case(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=72), make_case(mode=1, geom=(9, 6, 6), C1=128, C2=0, N=40),
            make_case(mode=1, geom=(1, 24, 24), C1=64, C2=0, N=328)]
    circ = [make_case(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=72, circular=True), make_case(mode=1, geom=(9, 6, 6), C1=128, C2=0, N=40, circular=True)]
    table = make_case(mode=1, geom=(3, 5, 7), C1=64, C2=0, N=72, bias="tableL", res=True)
    others = [table, make_case(mode=2, geom=(1, 9, 9), C1=64, C2=0, N=40, circular=True), make_case(mode=3, geom=(3, 3, 5), C1=64, C2=0, N=72),
              make_case(mode=4, geom=(2, 4, 4), C1=128, C2=0, N=40, circular=True), make_case(mode=0, geom=(129,), C1=64, C2=128, N=72, res=True)]
    sel = [make_case(mode=m, geom=(3, 5, 7), C1=64, C2=c2, N=72, circular=c, family="selector", bias=None)
           for m, c2, c in ((1, 0, False), (1, 64, True), (2, 0, False), (3, 0, True), (4, 0, False))]
    worst = max(check_against_float64(*_in_buffer(c, emulate_kernel(c)), c) for c in zero + circ + others + sel)
    assert worst <= 1.0

    for c in zero:
        n, H, W = c.geom
        src = c.src.clone()                                   # one tap dropped at one corner pixel
        src[row(c, 0, 0, W - 1), 4] = -1
        refused(c, emulate_kernel(c, src))
        if n > 1:
            src = c.src.clone()                               # one seam pixel sees the neighbouring image: (0, H-1, 2)'s lower tap reads (1, 0, 2)
            assert src[row(c, 0, H - 1, 2), 7] == -1
            src[row(c, 0, H - 1, 2), 7] = row(c, 1, 0, 2)
            refused(c, emulate_kernel(c, src))
        out = emulate_kernel(c)                               # the last valid row left unwritten
        out[-1] = NAN
        refused(c, out)
        out = emulate_kernel(c)                               # two 8-column groups swapped beside a tile edge (column 64, 32 for N = 40)
        e = 64 if c.N >= 72 else 32
        out[:, e - 8:e], out[:, e:e + 8] = out[:, e:e + 8].clone(), out[:, e - 8:e].clone()
        refused(c, out)
        refused(c, emulate_kernel(c), poke=lambda ob: ob.base - 1)                         # one guard element changed: beside the first row,
        refused(c, emulate_kernel(c), poke=lambda ob: int(ob.idx[-1, -1]) + ob.ld)         # below the last one,
        refused(c, emulate_kernel(c), poke=lambda ob: 0)                                   # the first guard row
    for c in circ:                                            # a circular wrap answered with zeros on one edge pixel
        n, H, W = c.geom
        src = c.src.clone()
        src[row(c, n - 1, 2, 0), 3] = -1
        refused(c, emulate_kernel(c, src))
    refused(table, emulate_kernel(table, bias_row=1))         # the bias row of the wrong step
    for c in sel:                                             # selector: one output pixel taken from (y, x + 1)
        out = emulate_kernel(c)
        Wo = out_hw(c.mode, *c.geom[1:])[1]
        out[Wo + 1] = out[Wo + 2]
        refused(c, out)


def test_misaligned_c_and_r_are_refused_on_the_host(hip):
    """sdv_hip.h "C / R": where ldc (and ldr) promise the 8-byte epilogue - and in every GEGLU launch - C and R off an 8-byte
    address, or batch strides that move them off it, are an argument error of sdv_gemm_bf16, found before anything is launched
    (so this runs without a GPU; launches that honour the contract cannot be tried here - the GPU tier makes thousands)."""
    import ctypes
    lib = hip.load()

    def refused(word, **kw):
        a = hip.GemmArgs()
        a.X, a.W, a.C = 4096, 8192, 16384
        a.M, a.N, a.K, a.ldx, a.ldw, a.ldc, a.tile = 64, 64, 64, 64, 64, 64, 1
        for k, v in kw.items():
            setattr(a, k, v)
        assert lib.sdv_gemm_bf16(ctypes.byref(a), None) == -1 and word in lib.sdv_last_error(), (kw, lib.sdv_last_error())

    refused(b"8-byte aligned", C=16384 + 2)
    refused(b"8-byte aligned", C=16384 + 4, ldc=68)
    refused(b"8-byte aligned", C=16384 + 6, ldc=72, tile=6)
    refused(b"8-byte aligned", R=32768 + 4, ldr=72)
    refused(b"8-byte aligned", C=16384 + 4, epi=1, ldc=32)
    refused(b"batch strides", batch=2, sC=64 * 64 + 2)
    refused(b"batch strides", batch=2, sC=64 * 64, R=32768, ldr=64, sR=64 * 64 + 6)


@gpu
def test_misaligned_c_is_refused_through_the_binding(hip, dev):
    """the same refusal as SdvHipError, with nothing launched: the output keeps its NaN"""
    x, w = torch.zeros((64, 64), dtype=BF16, device=dev), torch.zeros((64, 64), dtype=BF16, device=dev)
    out = torch.full((64 * 64 + 8,), NAN, dtype=BF16, device=dev)
    with pytest.raises(hip.SdvHipError, match="8-byte aligned"):
        hip.gemm(x, w, out[2:], M=64, N=64, K=64, ldx=64, ldw=64, ldc=64, tile=1)
    torch.cuda.synchronize()
    assert bool(out.isnan().all())


def test_case_tables_cover_every_tile():
    """Every group of every family runs on every tile the family allows, every case can be built, and the selector's channel map
    touches every 8-channel chunk of both sources - so that a later edit cannot thin the tables silently."""
    tables = all_tables()
    assert set(tables) == {"geometry", "dense", "two sources", "walk", "split-K", "fp8", "typed: bf16 batch", "typed: f32", "typed: image",
                           "epilogue operands", "epilogue activations", "epilogue geglu"}
    for name, (rows, allowed) in tables.items():
        groups = {}
        for r in rows:
            groups.setdefault(r[0], set()).add(r[1])
        assert groups, name
        for g, tiles in groups.items():
            assert tiles == set(allowed), f"{name} {g}: tiles {sorted(tiles)} != {sorted(allowed)}"
    assert {r[0][1:] for r in tables["geometry"][0]} == set(GEOMETRY_PARAMS)
    assert {r[2]["geom"] for r in tables["geometry"][0] if r[2]["mode"] == 1} >= {(3, 5, 7), (9, 6, 6), (1, 24, 24), (5, 1, 9), (6, 2, 2)}
    assert {r[2]["geom"] for r in tables["geometry"][0] if r[2]["mode"] == 2} >= {(1, 9, 9), (2, 6, 6)}
    assert {r[2]["geom"] for r in tables["geometry"][0] if r[2]["mode"] in (3, 4)} >= {(3, 3, 5), (2, 4, 4)}
    assert {(r[2]["geom"][0], r[2]["N"], r[2]["C1"]) for r in tables["dense"][0]} == {(M, N, K) for M in (1, 33, 129, 257)
                                                                                     for N in (8, 40, 77, 130, 328) for K in (64, 192)}
    for K in (64, 128, 192):
        assert {selector_channel(o, K) // 8 for o in range(72)} == set(range(K // 8)), K
        assert len({((o // 8) % 9, selector_channel(o, K)) for o in range(72)}) == 72
    for c0, ldc, r0, ldr in [layout(v, n) for v in VARIANTS for n in (8, 40, 77, 130, 328, 48, 336)]:
        assert c0 % 4 == 0 and r0 % 4 == 0 and ldc != ldr            # (every pointer offset is a multiple of 4 elements)
    assert all(layout("slice16", n)[1] % 8 == 0 and layout("slice8", n)[1] % 4 == 0 and layout("slice8", n)[3] % 4 == 0 and
               layout("scalar", n)[1] % 4 and layout("scalar", n)[3] % 4 and layout("slice8of8", n)[1] % 8 == 0 and
               layout("slice8of8", n)[0] % 8 == 4 and layout("mixed", n)[1] % 4 == 0 and layout("mixed", n)[3] % 4 for n in (8, 40, 77, 130, 328))
    make_case(**tables["split-K"][0][0][2])          # (the cases themselves are built - and cached - by the GPU tier)
