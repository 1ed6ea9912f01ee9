"""Per-kernel parity of libsdv_hip.so (through the C ABI) against plain PyTorch fp32 references of the
same op, on bf16-representable inputs.  Tolerances: elementwise kernels ~fp32 roundoff / 1 bf16 ulp;
MFMA kernels (bf16 in, fp32 accumulate, bf16 out) rel-L2 <= 4e-3 against fp32 (SURVEY.md 8c ladder).
A rel-L2 gate does not see a single wrong pixel: the ragged ends of sdv_gemm_bf16 - conv seams and wraps, M / N tails, the staged /
8-byte / scalar store paths, typed outputs, the persistent tile walk, split-K, fp8, the small-channel convs, on every tile - are
gated element by element against float64, inside NaN guards, by test_igemm_edges_gpu.py (the attention kernels' by
test_attention_edges_gpu.py)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, bf16_round, rel_l2
from helpers import _attn_ref64, _half_ulp_ratio

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
MFMA_TOL = 4e-3


def rnd(shape, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return bf16_round(torch.randn(shape, generator=g) * scale).to(dev)


# ------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------
ALL_TILES = [1, 2, 3, 4, 6, 7, 8, 9, 10, 11]      # (12 - 14 of ABI <= 9 - ring tiles, transposed tile - are gone)


@pytest.mark.parametrize("tile", ALL_TILES)
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (200, 320, 320), (64, 77, 64), (1024, 640, 1280), (33, 130, 64),
                                   (1000, 960, 192)])
def test_gemm_dense(hip, dev, tile, M, N, K):
    x, w = rnd((M, K), dev, 1), rnd((N, K), dev, 2, K ** -0.5)
    bias = rnd((N,), dev, 3)
    res = rnd((M, N), dev, 4)
    ref = x @ w.T + bias + res
    out = hip.linear(x.to(BF16), w.to(BF16), bias, residual=res.to(BF16), tile=tile)
    torch.cuda.synchronize()
    assert out.shape == (M, N)
    assert rel_l2(out.float(), ref) < MFMA_TOL


@pytest.mark.parametrize("tile", [0, 1, 3, 6, 7, 9])
def test_gemm_is_correctly_rounded(hip, dev, tile):
    """Parity ladder step 2, element by element: against a float64 evaluation of the SAME bf16 inputs every
    output must lie within half a bf16 ulp (the one rounding the kernel performs) plus fp32 accumulation noise
    (1e-5 * sum |x_k w_k|; a CPU emulation of the kernel's arithmetic stays below 1e-6 of that sum).  This is ~100x tighter
    than the rel-L2 bound of the other tests and catches any dropped / doubled K slice or misplaced fragment."""
    M, N, K = 384, 640, 1280
    x, w = rnd((M, K), dev, 11), rnd((N, K), dev, 12, K ** -0.5)
    bias, res = rnd((N,), dev, 13), rnd((M, N), dev, 14)
    xd, wd, bd, rd = x.double().cpu(), w.double().cpu(), bias.double().cpu(), res.double().cpu()
    ref = xd @ wd.T + bd + rd
    mag = xd.abs() @ wd.abs().T + bd.abs() + rd.abs()
    out = hip.linear(x.to(BF16), w.to(BF16), bias, residual=res.to(BF16), tile=tile).float().cpu().double()
    ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(ref.abs(), out.abs()).clamp_min(1e-30))) - 7)
    ratio = (out - ref).abs() / (0.5 * ulp * (1 + 1e-3) + 1e-5 * mag)
    assert float(ratio.max()) <= 1.0, f"tile {tile}: error {float(ratio.max()):.3f} x the rounding + accumulation bound"


def test_gemm_asymmetric_identity(hip, dev):
    """A = I against an asymmetric B catches transposed / permuted fragment layouts exactly."""
    n = 256
    x = torch.eye(n, device=dev)
    w = bf16_round(torch.arange(n * n, dtype=F32).reshape(n, n) % 251 - 125.0).to(dev)
    for tile in ALL_TILES:
        out = hip.linear(x.to(BF16), w.to(BF16), tile=tile)
        torch.cuda.synchronize()
        assert torch.equal(out.float(), w.T.contiguous()), f"tile {tile}"


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 6, 7, 8, 9])
def test_gemm_epilogues(hip, dev, tile):
    M, N, K = 384, 256, 192
    x, w = rnd((M, K), dev, 5), rnd((N, K), dev, 6, K ** -0.5)
    bias_n, bias_m = rnd((N,), dev, 7), rnd((M,), dev, 8)
    # alpha + per-m bias
    out = torch.empty((M, N), dtype=BF16, device=dev)
    hip.gemm(x.to(BF16), w.to(BF16), out, M=M, N=N, K=K, ldx=K, ldw=K, ldc=N, bias=bias_m, bias_mode=2, alpha=0.25,
             tile=tile)
    assert rel_l2(out.float(), 0.25 * (x @ w.T) + bias_m[:, None]) < MFMA_TOL
    # alpha on the leading columns only (fused [Q | K] projection: Q pre-scaled for the attention kernel)
    out = hip.linear(x.to(BF16), w.to(BF16), bias_n, alpha=0.37, alpha_cols=96, tile=tile)
    ref = x @ w.T
    ref[:, :96] *= 0.37
    assert rel_l2(out.float(), ref + bias_n) < MFMA_TOL
    # SiLU epilogue
    out = hip.linear(x.to(BF16), w.to(BF16), bias_n, epi=2, tile=tile)
    assert rel_l2(out.float(), F.silu(x @ w.T + bias_n)) < MFMA_TOL
    # two K sources (skip-connection concat)
    K1 = 128
    out = hip.linear(x[:, :K1].contiguous().to(BF16), w.to(BF16), bias_n, x2=x[:, K1:].contiguous().to(BF16), tile=tile)
    assert rel_l2(out.float(), x @ w.T + bias_n) < MFMA_TOL


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 6, 7, 8, 9])
def test_gemm_geglu(hip, dev, tile):
    from stable_diffusion_videos_amd.weights import geglu_interleave
    M, Cc, K = 320, 128, 64          # proj: K -> 8*Cc... here value/gate halves of size 4*Cc = 512
    half = 4 * Cc
    x, w = rnd((M, K), dev, 9), rnd((2 * half, K), dev, 10, K ** -0.5)
    b = rnd((2 * half,), dev, 11)
    y = x @ w.T + b
    ref = y[:, :half] * F.gelu(y[:, half:])
    out = hip.linear(x.to(BF16), geglu_interleave(w).to(BF16), geglu_interleave(b), epi=1, tile=tile)
    torch.cuda.synchronize()
    assert out.shape == (M, half)
    assert rel_l2(out.float(), ref) < MFMA_TOL


def test_geglu_gate_saturates_at_infinity(hip, dev):
    """the rearranged exact-erf GELU of the GEGLU epilogue (sdv_common.h gelu_erf_fast_f) ended in fma(-|x|, h, max(x, 0)) -
    at a gate of +inf that is fma(-inf, 0, inf) = NaN where gelu(+inf) = +inf, so an overflowed gate poisoned the residual stream instead of
    saturating.  |x| is capped now: gate +inf -> value * inf = +-inf (no NaN), gate -inf -> value * (-0) = 0, NaN stays NaN."""
    from stable_diffusion_videos_amd.weights import geglu_interleave
    M, K, N = 64, 64, 64                                   # N = [32 value | 32 gate] columns
    x = torch.ones((M, K), device=dev)
    w = torch.zeros((N, K), device=dev)
    w[:32] = 1.0 / K                                       # value = 1 + bias_value
    b = torch.zeros(N, device=dev)
    b[:32] = 1.0                                           # value = 2
    b[32:40] = 3.0e38                                      # gate pre-activation finite but huge: gelu = itself
    b[40:48] = float("inf")                                # gate +inf
    b[48:56] = float("-inf")                               # gate -inf
    b[56:64] = 2.0                                         # an ordinary gate
    for tile in (0, 1, 6):
        out = hip.linear(x.to(BF16), geglu_interleave(w).to(BF16), geglu_interleave(b), epi=1, tile=tile).float()
        assert not torch.isnan(out).any(), tile
        assert torch.isinf(out[:, 0:16]).all() and (out[:, 0:16] > 0).all(), tile       # 2 * 3e38 and 2 * inf
        assert (out[:, 16:24] == 0).all(), tile
        assert torch.allclose(out[:, 24:32], torch.full((M, 8), 2.0 * float(F.gelu(torch.tensor(2.0))), device=dev), rtol=1e-2), tile


def test_gemm_refuses_the_launch_forms_removed_in_abi_10(hip, dev):
    """ABI 10 dropped the experiments of rounds 2-4 from the product library: the LDS-ring tiles 12 / 13, the transposed 320 x 256
    tile 14 and the column-side LayerNorm fold it carried (the V^T projections - replaced by the fused QKV projection + row-major V
    in the attention kernel).  A caller that still asks for them gets an argument error, not another tile."""
    x, w = rnd((256, 128), dev, 301).to(BF16), rnd((64, 128), dev, 302).to(BF16)
    for tile in (5, 12, 13, 14):
        with pytest.raises(hip.SdvHipError):
            hip.linear(x, w, tile=tile)


@pytest.mark.parametrize("tile", [0, 1, 6, 7, 9])
@pytest.mark.parametrize("M,C,N2", [(512, 320, 640), (300, 640, 1280), (4096, 320, 2560), (100096, 320, 640)])
def test_gemm_layernorm_fold(hip, dev, tile, M, C, N2):
    """LayerNorm folded into the GEMMs around it (BasicTransformerBlock.norm1/2/3, reached from unet(...) at
    stable_diffusion_pipeline.py:418): the producer GEMM emits (mean, rstd) of the rows it stores, the consumers multiply the
    UN-normalised rows with gamma-scaled weights - against F.layer_norm + F.linear in fp32.  The fused projection with an alpha
    on its leading columns (to_q / to_k / to_v), GEGLU, and a large row mean (|mean| = 8 sigma)."""
    from stable_diffusion_videos_amd.weights import geglu_interleave, ln_fold
    x, w0 = rnd((M, C), dev, 110), rnd((C, C), dev, 111, C ** -0.5)
    b0, res = rnd((C,), dev, 112), rnd((M, C), dev, 113)
    res[:, :] += 8.0                                              # a residual stream with a large common mode
    res = bf16_round(res)
    gamma, beta = 1.0 + 0.3 * rnd((C,), dev, 114), 0.2 * rnd((C,), dev, 115)
    # producer: y = x W0^T + b0 + res, plus the statistics of the bf16 rows it wrote
    y, st = hip.linear(x.to(BF16), w0.to(BF16), b0, residual=res.to(BF16), want_stats=True, tile=tile)
    yf = y.float()
    mean, var = yf.mean(1), yf.var(1, unbiased=False)
    assert torch.allclose(st[:, 0], mean, rtol=1e-5, atol=1e-4)
    assert torch.allclose(st[:, 1], torch.rsqrt(var + 1e-5), rtol=2e-3)
    ln = F.layer_norm(yf, (C,), gamma, beta, 1e-5)
    # consumer, row-side, with an alpha on the leading columns (pre-scaled Q)
    w1, b1 = rnd((N2, C), dev, 116, C ** -0.5), rnd((N2,), dev, 117)
    qs = 0.23
    wq, sq, tq = ln_fold(w1[: N2 // 2], gamma, beta, b1[: N2 // 2], dev, scale=qs)
    wk, sk, tk = ln_fold(w1[N2 // 2:], gamma, beta, b1[N2 // 2:], dev)
    out = hip.linear(y, torch.cat([wq, wk]), torch.cat([tq, tk]), alpha=qs, alpha_cols=N2 // 2, ln=(st, torch.cat([sq, sk])),
                     tile=tile)
    ref = ln @ w1.T + b1
    ref[:, : N2 // 2] *= qs
    assert rel_l2(out.float(), ref) < MFMA_TOL
    # GEGLU consumer
    wg, sg, tg = ln_fold(geglu_interleave(w1), gamma, beta, geglu_interleave(b1), dev)
    out = hip.linear(y, wg, tg, epi=1, ln=(st, sg), tile=tile)
    full = ln @ w1.T + b1
    assert rel_l2(out.float(), full[:, : N2 // 2] * F.gelu(full[:, N2 // 2:])) < MFMA_TOL


@pytest.mark.parametrize("tile", [1, 6, 7, 9])
@pytest.mark.parametrize("M,C", [(131072, 320), (32768, 640), (8192, 1280), (4100, 320)])
def test_layernorm_fold_on_pipeline_like_rows_is_deterministic_and_elementwise_bounded(hip, dev, tile, M, C):
    """The regression test of round 4's open item.  What broke there: the column-side LayerNorm fold of the transposed
    V^T projection, with its per-row operands staged through LDS, raced on the 4-wave 128 x 128 tile - 11 of 11 repeated launches
    differed, a dozen lanes of one wave got a wrong value for one column (profiles/round5_vt_fold_diag_*.txt) - and no kernel test
    saw it, because (a) they compared ONE launch per tile, (b) by rel-L2, and (c) on zero-mean rows, where a fold operand that is
    off hides behind the bf16 rounding.  That launch form is gone (fused QKV projection + row-major V); this test holds the fold
    that remains - row-side, the fused [Q * qs | K | V] projection exactly as UNetEngine launches it - to the standard that would
    have caught it: rows like the UNet's residual stream (|mean| up to ~10 sigma, rstd 0.5 .. 30, so that acc - mean * s cancels
    most of acc), chip-filling M, SIX launches per tile that must agree bit for bit, and every element against a float64
    evaluation of the same fold within half a bf16 ulp + 2e-5 of the magnitudes that went into it."""
    from stable_diffusion_videos_amd.weights import ln_fold
    g = torch.Generator(device=dev).manual_seed(11 + C)
    mu = torch.randn(M, 1, device=dev, generator=g) * 3.0
    sd = torch.exp(torch.empty(M, 1, device=dev).uniform_(-3.4, 0.7, generator=g))
    x = (mu + sd * torch.randn((M, C), device=dev, generator=g)).to(BF16)
    xf = x.float()
    st = torch.stack([xf.mean(1), torch.rsqrt(xf.var(1, unbiased=False) + 1e-5)], 1).contiguous()      # what the producer's epilogue emits
    gamma, beta = 1.0 + 0.3 * rnd((C,), dev, 114), 0.2 * rnd((C,), dev, 115)
    qs = hip.q_prescale(40)
    parts = [ln_fold(rnd((C, C), dev, 120 + i, C ** -0.5), gamma, beta, None, dev, scale=qs if i == 0 else 1.0) for i in range(3)]
    w, s_, t_ = (torch.cat([p_[j] for p_ in parts]).contiguous() for j in range(3))
    outs = [hip.linear(x, w, t_, alpha=qs, alpha_cols=C, ln=(st, s_), tile=tile) for _ in range(6)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"tile {tile}: repeated launches differ"
    al = torch.ones(3 * C, dtype=torch.float64, device=dev)
    al[:C] = qs
    x64, w64 = x.double(), w.double()
    m64, r64 = st[:, :1].double(), st[:, 1:].double()
    ref = (x64 @ w64.T - m64 * s_.double()[None, :]) * (r64 * al[None, :]) + t_.double()[None, :]
    mag = (x64.abs() @ w64.abs().T + m64.abs() * s_.double().abs()[None, :]) * (r64 * al[None, :]) + t_.double().abs()[None, :]
    d = (outs[0].double() - ref).abs()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
    ratio = d / (0.5 * ulp + 2e-5 * mag)
    from conftest import report
    report(f"LayerNorm fold (fused QKV, tile {tile}, M={M}, C={C}): 6 launches bit-identical, worst element at {float(ratio.max()):.3f} of "
           f"(half ulp + 2e-5 magnitudes)")
    assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize("tile", [6])
@pytest.mark.parametrize("M,N,K,use_res,geglu", [(8192, 1280, 1280, False, False), (8192, 1280, 1280, True, False),
                                                   (32768, 640, 640, False, False), (16384, 2560, 320, False, True),
                                                   (131072, 320, 320, True, False), (100000, 320, 320, False, False),
                                                   (70000, 640, 640, True, False), (40000, 2560, 320, False, True)])
def test_gemm_store_sequence_is_deterministic_under_load(hip, dev, tile, M, N, K, use_res, geglu):
    """Chip-filling launches of the 256 x 320 tile (more tiles than CUs, so every workgroup WALKS tiles with the next tile's first K
    slab in flight across the epilogue; ragged M), repeated: every repeat is bit-identical and no element is off.  (The
    row-major store sequence once overwrote the first data register of a buffer_store_dwordx4 in the next instruction slot:
    lanes 12..15 of every 16 then stored the NEXT item's column index - a few thousand elements per launch, different ones
    each time, invisible to a rel-L2 gate on a small matrix.  tools/epi_race_diag.py is the locator.)"""
    from stable_diffusion_videos_amd.weights import geglu_interleave
    x, w = rnd((M, K), dev, 301).to(BF16), rnd((N, K), dev, 302, K ** -0.5).to(BF16)
    bias = rnd((N,), dev, 303)
    res = rnd((M, N), dev, 304).to(BF16) if use_res else None
    y = x.float() @ w.float().T + bias
    if geglu:
        ref = y[:, : N // 2] * F.gelu(y[:, N // 2:])
        wk, bk = geglu_interleave(w.float()).to(BF16), geglu_interleave(bias)
    else:
        ref, wk, bk = y + (res.float() if use_res else 0.0), w, bias
    tol = 0.02 * float(ref.abs().max())
    outs = []
    for _ in range(4):
        outs.append(hip.linear(x, wk, bk, residual=res, epi=1 if geglu else 0, tile=tile))
    torch.cuda.synchronize()
    assert int(((outs[0].float() - ref).abs() > tol).sum()) == 0
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_gemm_batched_transposed_output(hip, dev):
    """The V^T projection: per-sample [C, L] = Wv [C, K] . X[b] [L, K]^T with a padded leading dim."""
    B, L, Cc, K, ld = 3, 77, 128, 64, 128
    wv, x = rnd((Cc, K), dev, 12, K ** -0.5), rnd((B, L, K), dev, 13)
    out = torch.zeros((B, Cc, ld), dtype=BF16, device=dev)
    hip.gemm(wv.to(BF16), x.to(BF16), out, M=Cc, N=L, K=K, ldx=K, ldw=K, ldc=ld, batch=B, sX=0, sW=L * K, sC=Cc * ld)
    ref = torch.einsum("ck,blk->bcl", wv, x)
    assert rel_l2(out[:, :, :L].float(), ref) < MFMA_TOL
    assert float(out[:, :, L:].float().abs().max()) == 0.0     # padding untouched


def test_gemm_argument_errors(hip, dev):
    x = torch.zeros((64, 96), dtype=BF16, device=dev)
    w = torch.zeros((64, 96), dtype=BF16, device=dev)
    with pytest.raises(hip.SdvHipError):
        hip.linear(x, w)                       # K = 96 is not a multiple of 64
    with pytest.raises(hip.SdvHipError):
        hip.linear(x.cpu(), w)                 # no CPU fallback


# ------------------------------------------------------------------------------------------------
# conv3x3 (implicit GEMM)
# ------------------------------------------------------------------------------------------------
def conv_ref(x_nhwc, w, bias, mode, circular):
    x = x_nhwc.permute(0, 3, 1, 2)
    if mode == 3:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    stride = 2 if mode == 2 else 1
    if circular:
        x = F.pad(x, (1, 1, 1, 1), mode="circular")
        y = F.conv2d(x, w, bias, stride=stride, padding=0)
    else:
        y = F.conv2d(x, w, bias, stride=stride, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("tile", [0, 1, 6, 9, 10, 11])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("n,H,W,Cin,Cout", [(2, 16, 16, 64, 128), (1, 12, 20, 128, 64), (3, 8, 8, 320, 320),
                                            (2, 24, 24, 64, 640)])
def test_conv3x3(hip, dev, tile, mode, circular, n, H, W, Cin, Cout):
    from stable_diffusion_videos_amd.weights import conv_w
    x = rnd((n, H, W, Cin), dev, 20)
    w = rnd((Cout, Cin, 3, 3), dev, 21, (9 * Cin) ** -0.5)
    bias = rnd((Cout,), dev, 22)
    ref = conv_ref(x, w, bias, mode, circular)
    out = hip.conv3x3(x.reshape(-1, Cin).to(BF16), conv_w(w, dev), bias, nimg=n, H=H, W=W, mode=mode, circular=circular,
                      tile=tile)
    torch.cuda.synchronize()
    assert out.shape[0] == ref.shape[0] * ref.shape[1] * ref.shape[2]
    assert rel_l2(out.float().reshape(ref.shape), ref) < MFMA_TOL


@pytest.mark.parametrize("tile,mode", [(0, 1), (6, 1), (1, 1), (0, 2), (0, 3)])
def test_conv3x3_is_correctly_rounded(hip, dev, tile, mode):
    """Parity ladder step 2 for the implicit-GEMM conv on the UNet's real 64x64-level shape (320 -> 320 channels, 64 x 64
    pixels, 2 images): EVERY output pixel within half a bf16 ulp + fp32 accumulation noise of a float64 convolution of the
    same bf16 inputs - a wrong halo pixel, a dropped tap or a swapped K tile in one corner of one tile fails it (a rel-L2
    gate does not see a single bad pixel among 2.6 M outputs)."""
    from stable_diffusion_videos_amd.weights import conv_w
    n, H, W, Cin, Cout = 2, 64, 64, 320, 320
    x = rnd((n, H, W, Cin), dev, 60)
    w = rnd((Cout, Cin, 3, 3), dev, 61, (9 * Cin) ** -0.5)
    bias = rnd((Cout,), dev, 62)
    xd, wd, bd = x.double().cpu(), w.double().cpu(), bias.double().cpu()
    ref = conv_ref(xd, wd, bd, mode, False)
    mag = conv_ref(xd.abs(), wd.abs(), bd.abs(), mode, False)
    out = hip.conv3x3(x.reshape(-1, Cin).to(BF16), conv_w(w, dev), bias, nimg=n, H=H, W=W, mode=mode, tile=tile)
    torch.cuda.synchronize()
    ratio = _half_ulp_ratio(out.double().cpu().reshape(ref.shape), ref, mag)
    assert float(ratio.max()) <= 1.0, f"tile {tile} mode {mode}: {float(ratio.max()):.3f} x the rounding + accumulation bound"


@pytest.mark.parametrize("tile", [0, 1, 6, 9])
@pytest.mark.parametrize("circular", [False, True])
@pytest.mark.parametrize("n,H,W,Cin,Cout", [(2, 16, 16, 64, 128), (1, 12, 20, 128, 64), (3, 8, 8, 320, 320), (1, 6, 10, 64, 40)])
def test_upconv_phase_form(hip, dev, tile, circular, n, H, W, Cin, Cout):
    """Upsample2D (nearest 2x + conv3x3) as four 2x2 phase filters (sdv_gemm_bf16 mode 4, 4/9 of the multiplies) against the
    fp32 F.interpolate + F.conv2d reference and against the gather-on-the-fly 9-tap kernel (mode 3).  The phase filters sum
    coincident taps in fp32 and round ONCE to bf16: a few e-4 of extra relative error, inside the MFMA tolerance."""
    from stable_diffusion_videos_amd.weights import conv_w, upconv_phase_w
    x = rnd((n, H, W, Cin), dev, 30)
    w = rnd((Cout, Cin, 3, 3), dev, 31, (9 * Cin) ** -0.5)
    bias = rnd((Cout,), dev, 32)
    ref = conv_ref(x, w, bias, 3, circular)
    out = hip.upconv3x3_phase(x.reshape(-1, Cin).to(BF16), upconv_phase_w(w.cpu(), dev), bias, nimg=n, H=H, W=W,
                              circular=circular, tile=tile)
    torch.cuda.synchronize()
    assert out.shape == (n * 4 * H * W, Cout)
    assert rel_l2(out.float().reshape(ref.shape), ref) < MFMA_TOL
    nine = hip.conv3x3(x.reshape(-1, Cin).to(BF16), conv_w(w, dev), bias, nimg=n, H=H, W=W, mode=3, circular=circular)
    assert rel_l2(out.float(), nine.float()) < MFMA_TOL


def test_conv3x3_concat_residual_steptable(hip, dev):
    """ResBlock conv forms: two-source channel concat, residual add, per-step bias table."""
    from stable_diffusion_videos_amd.weights import conv_w
    n, H, W, C1, C2, Cout = 2, 16, 16, 128, 64, 128
    x1, x2 = rnd((n, H, W, C1), dev, 23), rnd((n, H, W, C2), dev, 24)
    w = rnd((Cout, C1 + C2, 3, 3), dev, 25, (9 * (C1 + C2)) ** -0.5)
    table = rnd((5, Cout), dev, 26)
    res = rnd((n, H, W, Cout), dev, 27)
    step = torch.tensor([3], dtype=torch.int32, device=dev)
    ref = conv_ref(torch.cat([x1, x2], -1), w, table[3], 1, False) + res
    for tile in (0, 1, 2, 3, 6, 7, 8, 9):
        out = hip.conv3x3(x1.reshape(-1, C1).to(BF16), conv_w(w, dev), table, nimg=n, H=H, W=W,
                          x2=x2.reshape(-1, C2).to(BF16), residual=res.reshape(-1, Cout).to(BF16), step_ptr=step,
                          bias_step_stride=Cout, tile=tile)
        assert rel_l2(out.float().reshape(ref.shape), ref) < MFMA_TOL, tile


def test_conv_small_channel_kernels(hip, dev):
    from stable_diffusion_videos_amd.weights import conv_w
    n, H, W = 2, 16, 16
    for circular in (False, True):
        # Cin = 4 -> 320 (UNet conv_in)
        x, w, b = rnd((n, H, W, 4), dev, 30), rnd((320, 4, 3, 3), dev, 31, 1 / 6), rnd((320,), dev, 32)
        out = hip.conv3x3_cin_small(x.reshape(-1, 4).to(BF16), conv_w(w, dev), b, nimg=n, H=H, W=W, circular=circular)
        ref = conv_ref(x, w, b, 1, circular)
        assert rel_l2(out.float().reshape(ref.shape), ref) < 3e-3
        # the same conv on the matrix cores: im2col (4 ch -> one 64-wide K tile) + dense GEMM
        from stable_diffusion_videos_amd.weights import conv_w_c4
        out2 = hip.conv3x3_c4(x.reshape(-1, 4).to(BF16), conv_w_c4(w.cpu(), dev), b, nimg=n, H=H, W=W, circular=circular)
        assert rel_l2(out2.float().reshape(ref.shape), ref) < 3e-3
        # 320 -> 4, fp32 out (UNet conv_out)
        x, w, b = rnd((n, H, W, 320), dev, 33), rnd((4, 320, 3, 3), dev, 34, (9 * 320) ** -0.5), rnd((4,), dev, 35)
        # on the matrix cores (what UNetEngine runs): N = 4 in one 32-column MFMA tile, fp32 from the accumulators
        o2 = torch.empty((n * H * W, 4), dtype=F32, device=dev)
        hip.conv3x3(x.reshape(-1, 320).to(BF16), conv_w(w, dev), b, nimg=n, H=H, W=W, circular=circular, out_mode=1, out_f32=o2)
        assert rel_l2(o2.view(n, H, W, 4), conv_ref(x, w, b, 1, circular)) < 1e-5
    # 128 -> 3 with the image epilogue (VAE conv_out): clamp(v/2+0.5) and round-half-even uint8
    x, w, b = rnd((n, H, W, 128), dev, 36), rnd((3, 128, 3, 3), dev, 37, 2 * (9 * 128) ** -0.5), rnd((3,), dev, 38)
    ref = (conv_ref(x, w, b, 1, False) / 2 + 0.5).clamp(0, 1)
    u = None
    # through the igemm's image epilogue (what VAEDecoderEngine runs), every 4-wave tile
    for tile in (0, 1, 2, 3, 10, 11):
        f2 = torch.empty((n * H * W, 3), dtype=F32, device=dev)
        u2 = torch.zeros((n * H * W, 3), dtype=torch.uint8, device=dev)
        hip.conv3x3(x.reshape(-1, 128).to(BF16), conv_w(w, dev), b, nimg=n, H=H, W=W, out_mode=2, out_f32=f2, out_u8=u2, tile=tile)
        assert float((f2.view_as(ref) - ref).abs().max()) < 1e-5, tile
        assert torch.equal(u2.cpu(), torch.from_numpy((f2.cpu().numpy() * 255).round().astype("uint8")))
        if u is not None:
            assert int((u2.int() - u.int()).abs().max()) <= 1                    # (two fp32 summation orders: ties may flip)
        u = u2
    with pytest.raises(hip.SdvHipError):      # the 8-wave tiles do not carry the typed outputs
        hip.conv3x3(x.reshape(-1, 128).to(BF16), conv_w(w, dev), b, nimg=n, H=H, W=W, out_mode=2, out_u8=u2, tile=6)


@pytest.mark.parametrize("tile", [0, 2, 3, 10, 11])
def test_conv3x3_dense_block_forms(hip, dev, tile):
    """The RRDBNet conv forms: input = a column prefix of a wider row-major buffer, output written into a column slice
    of the SAME buffer (dense concat through ldx / ldc), LeakyReLU(0.2) epilogue, zero-padded K for Cin = 96, and
    the scaled residual of conv5 (0.2 * (conv + b) + x)."""
    from stable_diffusion_videos_amd.weights import conv_w_kpad
    n, H, W, nf, g, ld = 2, 20, 12, 64, 32, 192
    M = n * H * W
    buf = rnd((M, ld), dev, 60)                                   # [x | x1 | junk ...] - junk must not leak into results
    ref_in = buf[:, :nf + g].reshape(n, H, W, nf + g).clone()
    w = rnd((g, nf + g, 3, 3), dev, 61, (9 * (nf + g)) ** -0.5)
    b = rnd((g,), dev, 62)
    ref = F.leaky_relu(conv_ref(ref_in, w, b, 1, False), 0.2).reshape(M, g)
    wk = conv_w_kpad(w.cpu(), dev)
    assert wk.shape == (g, 9 * 128)
    bb = buf.to(BF16)
    keep = bb.clone()
    hip.conv3x3(bb[:, :128], wk, b, nimg=n, H=H, W=W, out=bb[:, nf + g:nf + 2 * g], epi=3, tile=tile)
    torch.cuda.synchronize()
    assert rel_l2(bb[:, nf + g:nf + 2 * g].float(), ref) < MFMA_TOL
    assert torch.equal(bb[:, :nf + g], keep[:, :nf + g]) and torch.equal(bb[:, nf + 2 * g:], keep[:, nf + 2 * g:])
    # conv5 form: all 192 columns in, 64 out into another buffer, residual = x, alpha = 0.2 with pre-scaled bias
    w5 = rnd((nf, ld, 3, 3), dev, 63, (9 * ld) ** -0.5)
    b5 = rnd((nf,), dev, 64)
    src = rnd((M, ld), dev, 65)
    ref5 = 0.2 * conv_ref(src.reshape(n, H, W, ld), w5, b5, 1, False).reshape(M, nf) + src[:, :nf]
    dst = torch.zeros((M, ld), dtype=BF16, device=dev)
    sb = src.to(BF16)
    hip.conv3x3(sb, conv_w_kpad(w5.cpu(), dev), b5 * 0.2, nimg=n, H=H, W=W, out=dst[:, :nf], residual=sb[:, :nf], alpha=0.2,
                tile=tile)
    torch.cuda.synchronize()
    assert rel_l2(dst[:, :nf].float(), ref5) < MFMA_TOL
    assert float(dst[:, nf:].float().abs().max()) == 0.0


def test_esrgan_glue_kernels(hip, dev):
    g = torch.Generator().manual_seed(70)
    img = torch.randint(0, 256, (2, 9, 7, 3), generator=g, dtype=torch.uint8).to(dev)
    x4 = hip.rgb_u8_to_bf16_c4(img)
    ref = torch.zeros((2 * 9 * 7, 4))
    ref[:, :3] = img.cpu().reshape(-1, 3).float() / 255.0
    assert torch.equal(x4.cpu().float(), bf16_round(ref))
    a, b = rnd((50, 192), dev, 71).to(BF16), rnd((50, 64), dev, 72).to(BF16)
    out = torch.zeros((50, 128), dtype=BF16, device=dev)
    hip.axpby(a[:, 64:128], b, out[:, 32:96], 0.2, 1.0)
    torch.cuda.synchronize()
    exp = bf16_round(0.2 * a[:, 64:128].float() + b.float())
    assert float((out[:, 32:96].float() - exp).abs().max()) <= 1e-6 + float(exp.abs().max()) * 2 ** -8
    assert float(out[:, :32].float().abs().max()) == 0.0 and float(out[:, 96:].float().abs().max()) == 0.0
    hip.axpby(out[:, 32:96], b, b, 0.0, 1.0)                       # in place, identity
    # conv_last form: 64 -> 3 with clamp(v, 0, 1) -> uint8 (RealESRGANer post-processing)
    from stable_diffusion_videos_amd.weights import conv_w
    n, H, W = 2, 10, 12
    x, w, bias = rnd((n, H, W, 64), dev, 73), rnd((3, 64, 3, 3), dev, 74, 2 * (9 * 64) ** -0.5), rnd((3,), dev, 75) + 0.5
    f = torch.empty((n * H * W, 3), dtype=F32, device=dev)
    u = torch.empty((n * H * W, 3), dtype=torch.uint8, device=dev)
    hip.conv3x3(x.reshape(-1, 64).to(BF16), conv_w(w, dev), bias, nimg=n, H=H, W=W, out_mode=3, out_f32=f, out_u8=u)
    ref = conv_ref(x, w, bias, 1, False).clamp(0, 1)
    assert float((f.view_as(ref) - ref).abs().max()) < 1e-5
    assert torch.equal(u.cpu(), torch.from_numpy((f.cpu().numpy() * 255).round().astype("uint8")))


def test_latent_affine(hip, dev):
    x = torch.randn((2 * 8 * 8, 4), device=dev)
    wpq, b = torch.randn((4, 4), device=dev), torch.randn(4, device=dev)
    out = torch.empty((2 * 8 * 8, 4), dtype=BF16, device=dev)
    hip.latent_affine(x, wpq, b, 1 / 0.18215, out, x.shape[0], 4)
    ref = (x / 0.18215) @ wpq.T + b
    assert rel_l2(out.float(), ref) < 3e-3


@pytest.mark.parametrize("n,H,C1,C2,Cout,mode,circular", [(2, 8, 1280, 0, 1280, 1, False), (2, 8, 1280, 1280, 1280, 1, False), (8, 8, 1280, 0, 1280, 1, True),
                                                         (2, 16, 640, 640, 1280, 2, False), (1, 8, 320, 0, 640, 3, False)])
def test_conv3x3_split_k_small_batches(hip, dev, n, H, C1, C2, Cout, mode, circular):
    """Split-K (sdv_hip.h split_k) on the low-resolution convs of a 1 - 4-frame call (ResnetBlock2D / downsampler convs of
    unet(...), stable_diffusion_pipeline.py:418, at walk()'s default batch_size = 1, :571): a handful of output tiles against K up to
    23 040.  The split launch - partial sums in fp32, second pass adds them in split order, then alpha / step-indexed bias / residual and
    ONE rounding - against float64 per element (half a bf16 ulp + 1e-5 sum |x w|), bit-identical across repeats, and within an fp32
    summation-order distance of the unsplit launch; two-source concat, stride 2, nearest-2x, circular padding, bias table."""
    from stable_diffusion_videos_amd.weights import conv_w
    x, x2 = rnd((n, H, H, C1), dev, 70), (rnd((n, H, H, C2), dev, 71) if C2 else None)
    w = rnd((Cout, C1 + C2, 3, 3), dev, 72, (9 * (C1 + C2)) ** -0.5)
    table = rnd((3, Cout), dev, 73)
    step = torch.tensor([2], dtype=torch.int32, device=dev)
    xin = torch.cat([x, x2], -1) if C2 else x
    ref = conv_ref(xin.double(), w.double(), table[2].double(), mode, circular)
    mag = conv_ref(xin.double().abs(), w.double().abs(), table[2].double().abs(), mode, circular)
    Ho = ref.shape[1]
    res = rnd((n * Ho * Ho, Cout), dev, 74).to(BF16)
    ref = ref + res.double().view_as(ref)
    mag = mag + res.double().abs().view_as(ref)
    kw = dict(nimg=n, H=H, W=H, mode=mode, circular=circular, x2=x2.reshape(-1, C2).to(BF16) if C2 else None, residual=res, step_ptr=step,
              bias_step_stride=Cout)
    outs = []
    for _ in range(3):
        outs.append(hip.conv3x3(x.reshape(-1, C1).to(BF16), conv_w(w, dev), table, **kw))
        assert hip.LAST_SPLIT_K >= 2, "this shape is meant to take the split-K path"
    torch.cuda.synchronize()
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    d = (outs[0].double().view_as(ref) - ref).abs()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
    assert float((d / (0.5 * ulp + 1e-5 * mag)).max()) <= 1.0
    prev, hip.SPLIT_K = hip.SPLIT_K, False
    try:
        plain = hip.conv3x3(x.reshape(-1, C1).to(BF16), conv_w(w, dev), table, **kw)
        assert hip.LAST_SPLIT_K == 1
    finally:
        hip.SPLIT_K = prev
    assert rel_l2(outs[0].float(), plain.float()) < 5e-4          # two fp32 summation orders, one bf16 rounding each
    # the GroupNorm statistics of a split launch leave its second pass: (sum, sumsq) per 32-row block and channel of the STORED values
    o = hip.conv3x3(x.reshape(-1, C1).to(BF16), conv_w(w, dev), table, gn=True, **kw)
    assert hip.LAST_SPLIT_K >= 2 and torch.equal(o, outs[0])
    g = o._sdv_gn
    of = o.float().view(-1, 32, Cout)
    assert torch.allclose(g.p[:, 0], of.sum(1), rtol=1e-5, atol=1e-4) and torch.allclose(g.p[:, 1], (of * of).sum(1), rtol=1e-5, atol=1e-4)


def test_gemm_split_k_dense_and_its_limits(hip, dev):
    """Dense GEMMs with few rows and a long K split as well (ff.net.2 of the 8 x 8 block at 1 frame per call: M = 128, K = 5120); launches
    that carry an activation, a LayerNorm fold or statistics, large M, or a short K do not."""
    x, w, b = rnd((128, 5120), dev, 80).to(BF16), rnd((1280, 5120), dev, 81, 5120 ** -0.5).to(BF16), rnd((1280,), dev, 82)
    res = rnd((128, 1280), dev, 83).to(BF16)
    out = hip.linear(x, w, b, residual=res)
    assert hip.LAST_SPLIT_K >= 2
    ref = x.double() @ w.double().T + b.double() + res.double()
    mag = x.double().abs() @ w.double().abs().T + b.double().abs() + res.double().abs()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)
    assert float(((out.double() - ref).abs() / (0.5 * ulp + 1e-5 * mag)).max()) <= 1.0
    hip.linear(x, w, b, epi=2)
    assert hip.LAST_SPLIT_K == 1                                  # SiLU epilogue: not a plain launch
    hip.linear(rnd((8192, 5120), dev, 84).to(BF16), w, b)
    assert hip.LAST_SPLIT_K == 1                                  # enough tiles without it
    hip.linear(x[:, :320].contiguous(), w[:, :320].contiguous(), b)
    assert hip.LAST_SPLIT_K == 1                                  # K too short to share out


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def attn_ref(q, k, v, heads, scale):
    B, Lq, Cc = q.shape
    dh = Cc // heads
    qh = q.view(B, Lq, heads, dh).transpose(1, 2)
    kh = k.view(B, -1, heads, dh).transpose(1, 2)
    vh = v.view(B, -1, heads, dh).transpose(1, 2)
    a = torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1)
    return (a @ vh).transpose(1, 2).reshape(B, Lq, Cc)


@pytest.mark.parametrize("dh", [40, 64, 80, 160])
@pytest.mark.parametrize("Lq,Lk", [(256, 256), (200, 77), (4096, 4096), (64, 100), (4, 4), (1200, 77), (1024, 128)])
def test_attention(hip, dev, dh, Lq, Lk):
    if Lq == 4096 and dh not in (40, 64):
        pytest.skip("4096-token self-attention only exists at the 40/64-wide heads")
    B, heads = 2, 2
    Cc = heads * dh
    q, k, v = rnd((B, Lq, Cc), dev, 40), rnd((B, Lk, Cc), dev, 41), rnd((B, Lk, Cc), dev, 42)
    scale = dh ** -0.5
    ref = attn_ref(q, k, v, heads, scale)
    ldv = (Lk + 63) // 64 * 64
    vt = torch.zeros((B, Cc, ldv), dtype=BF16, device=dev)
    vt[:, :, :Lk] = v.transpose(1, 2).to(BF16)
    out = torch.empty((B * Lq, Cc), dtype=BF16, device=dev)
    hip.attention(q.reshape(-1, Cc).to(BF16), k.reshape(-1, Cc).to(BF16), vt, out, B=B, H=heads, Lq=Lq, Lk=Lk, dh=dh, ldq=Cc,
                  ldk=Cc, ldv=ldv, ldo=Cc, scale=scale)
    torch.cuda.synchronize()
    assert rel_l2(out.float().view(B, Lq, Cc), ref) < 6e-3
    # the same attention with V ROW-MAJOR (sdv_hip.h v_rowmajor: the V columns of a fused [K | V] / [Q | K | V] projection, transposed
    # by the kernel's LDS read): the PV MFMAs see the same operands in the same order, so the result is the same BITS - except
    # where the transposed form runs its own kernel (the resident text cross-attention form, Lk <= 128: other tile walk, same math)
    kv = torch.cat([k, v], -1).reshape(-1, 2 * Cc).to(BF16).contiguous()
    out_r = torch.full((B * Lq, Cc), float("nan"), dtype=BF16, device=dev)
    hip.attention(q.reshape(-1, Cc).to(BF16), kv, kv, out_r, B=B, H=heads, Lq=Lq, Lk=Lk, dh=dh, ldq=Cc, ldk=2 * Cc, ldv=2 * Cc,
                  ldo=Cc, scale=scale, v_off=Cc, v_rowmajor=True)
    torch.cuda.synchronize()
    assert rel_l2(out_r.float().view(B, Lq, Cc), ref) < 6e-3
    if Lk > 128 or dh == 160:
        assert torch.equal(out_r, out), "row-major V and transposed V must give the same bits"


@pytest.mark.parametrize("vrm", [False, True])
@pytest.mark.parametrize("dh,Lq,Lk,qscale,prescaled", [(40, 4096, 4096, 1.0, True), (40, 4096, 4096, 5.0, True), (40, 4096, 77, 1.0, True),
                                                       (80, 1024, 1024, 1.0, True), (80, 1024, 1024, 5.0, True), (160, 256, 256, 1.0, True),
                                                       (64, 1024, 1024, 5.0, True), (40, 4096, 4096, 1.0, False), (64, 1024, 1024, 5.0, False),
                                                       (64, 2304, 2304, 5.0, True)])
def test_attention_elementwise_bound(hip, dev, dh, Lq, Lk, qscale, prescaled, vrm):
    """Element-by-element bound against a float64 softmax(QK^T)V of the same bf16 inputs, on the UNet's real attention
    shapes (64 x 64 level: dh 40, 4096 tokens; cross-attention: 77 keys).  The kernel rounds P to bf16 before the PV MFMA,
    so the bound is half a bf16 ulp of the output plus 2^-6 * sum_k p_k |v_k| (measured worst case 0.1 - 0.4 of that on
    MI355X) - a dropped or doubled key tile moves an output by ~1/64 of sum p |v| per tile at these sizes and fails it,
    which the 6e-3 rel-L2 gate cannot see.  The channel pattern of V makes every key tile visible: channel d of V is 1 on the
    keys of tile d (mod dh) and random noise elsewhere.  qscale = 5 multiplies Q so that the logits have the spread of a
    TRAINED model's self-attention (std ~5 instead of ~1): the running max then jumps by more than the deferral threshold
    in most tiles and the O-rescale branch runs all the time instead of never.
    ``vrm``: V row-major inside a fused [Q | K | V] buffer (how UNetEngine's self-attention calls the kernel since round 5)
    instead of a transposed V^T tensor (the text cross-attention).
    ``prescaled`` is how the engines call the kernel: Q arrives as q * scale * log2(e), rounded to bf16 once by its
    projection GEMM.  (With raw Q the 40 / 80-wide-head kernels pre-multiply and round a second time: at qscale 5 that
    measured 1.9 x this bound / 4.6e-3 rel-L2 instead of 0.34 x / 1.9e-3 - why the product path pre-scales in the GEMM.)"""
    B, heads = 1, 8
    Cc = heads * dh
    scale = dh ** -0.5
    if prescaled:
        q = rnd((B, Lq, Cc), dev, 70, qscale * hip.q_prescale(dh))       # what the projection GEMM hands over
        q_true = q.double().cpu() / hip.q_prescale(dh)                   # the q this bf16 value stands for
    else:
        q = rnd((B, Lq, Cc), dev, 70, qscale)
        q_true = q.double().cpu()
    k = rnd((B, Lk, Cc), dev, 71)
    v = rnd((B, Lk, Cc), dev, 72, 0.25)
    tile_of_key = (torch.arange(Lk, device=dev) // 64) % dh
    for h in range(heads):
        v[0, torch.arange(Lk, device=dev), h * dh + tile_of_key] = 1.0
    ref, mag = _attn_ref64(q_true, k.double().cpu(), v.double().cpu(), heads, scale)
    ldv = (Lk + 63) // 64 * 64
    vt = torch.zeros((B, Cc, ldv), dtype=BF16, device=dev)
    vt[:, :, :Lk] = v.transpose(1, 2).to(BF16)
    out = torch.empty((B * Lq, Cc), dtype=BF16, device=dev)
    if vrm:
        kv = torch.cat([k, v], -1).reshape(-1, 2 * Cc).to(BF16).contiguous()
        hip.attention(q.reshape(-1, Cc).to(BF16), kv, kv, out, B=B, H=heads, Lq=Lq, Lk=Lk, dh=dh, ldq=Cc, ldk=2 * Cc, ldv=2 * Cc,
                      ldo=Cc, scale=scale, v_off=Cc, q_prescaled=prescaled, v_rowmajor=True)
    else:
        hip.attention(q.reshape(-1, Cc).to(BF16), k.reshape(-1, Cc).to(BF16), vt, out, B=B, H=heads, Lq=Lq, Lk=Lk, dh=dh, ldq=Cc,
                      ldk=Cc, ldv=ldv, ldo=Cc, scale=scale, q_prescaled=prescaled)
    torch.cuda.synchronize()
    o64 = out.double().cpu().view(B, Lq, Cc)
    ratio = _half_ulp_ratio(o64, ref, mag, acc_eps=2.0 ** -6)
    from conftest import report
    report(f"attention dh={dh} Lq={Lq} Lk={Lk} qscale={qscale} prescaled={prescaled} v_rowmajor={vrm}: worst element at {float(ratio.max()):.3f} of "
           f"(half ulp + 2^-6 sum p|v|), rel-L2 {rel_l2(o64, ref):.2e}")
    assert float(ratio.max()) <= 1.0


def test_attention_fused_qk_buffer_and_online_rescale(hip, dev):
    """Q and K interleaved in one [M, 2C] buffer (as the UNet produces them), and a spiked key late in
    the sequence so the running-max rescale branch really fires."""
    B, heads, dh, L = 1, 8, 40, 512
    Cc = heads * dh
    q, k, v = rnd((B, L, Cc), dev, 43), rnd((B, L, Cc), dev, 44), rnd((B, L, Cc), dev, 45)
    k[:, 400] = bf16_round(8.0 * q[:, 17])          # query 17 gets a huge score at key 400 (7th KV tile)
    scale = dh ** -0.5
    ref = attn_ref(q, k, v, heads, scale)
    qk = torch.cat([q, k], -1).reshape(-1, 2 * Cc).to(BF16).contiguous()
    vt = v.transpose(1, 2).to(BF16).contiguous()
    out = torch.empty((B * L, Cc), dtype=BF16, device=dev)
    hip.attention(qk, qk, vt, out, B=B, H=heads, Lq=L, Lk=L, dh=dh, ldq=2 * Cc, ldk=2 * Cc, ldv=L, ldo=Cc, scale=scale,
                  k_off=Cc)
    assert rel_l2(out.float().view(B, L, Cc), ref) < 6e-3
    assert float((out.float().view(B, L, Cc)[0, 17] - ref[0, 17]).abs().max()) < 0.05
    # ... and Q, K, V in one [M, 3C] buffer, V read row-major (UNetEngine's self-attention): the same bits
    qkv = torch.cat([q, k, v], -1).reshape(-1, 3 * Cc).to(BF16).contiguous()
    out3 = torch.empty((B * L, Cc), dtype=BF16, device=dev)
    hip.attention(qkv, qkv, qkv, out3, B=B, H=heads, Lq=L, Lk=L, dh=dh, ldq=3 * Cc, ldk=3 * Cc, ldv=3 * Cc, ldo=Cc, scale=scale,
                  k_off=Cc, v_off=2 * Cc, v_rowmajor=True)
    assert torch.equal(out3, out)


@pytest.mark.parametrize("dh,L", [(64, 77), (64, 200), (40, 130), (80, 77), (160, 64)])
def test_attention_causal(hip, dev, dh, L):
    """CLIP text encoder form: causal mask, Lq = Lk = 77 (ragged last KV tile), fused [Q | K] buffer."""
    B, heads = 3, 2
    Cc = heads * dh
    q, k, v = rnd((B, L, Cc), dev, 47), rnd((B, L, Cc), dev, 48), rnd((B, L, Cc), dev, 49)
    scale = dh ** -0.5
    qh, kh, vh = (t.view(B, L, heads, dh).transpose(1, 2) for t in (q, k, v))
    mask = torch.full((L, L), float("-inf"), device=dev).triu(1)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2) * scale + mask, -1) @ vh).transpose(1, 2).reshape(B, L, Cc)
    ldv = (L + 63) // 64 * 64
    vt = torch.zeros((B, Cc, ldv), dtype=BF16, device=dev)
    vt[:, :, :L] = v.transpose(1, 2).to(BF16)
    qk = torch.cat([q, k], -1).reshape(-1, 2 * Cc).to(BF16).contiguous()
    out = torch.empty((B * L, Cc), dtype=BF16, device=dev)
    hip.attention(qk, qk, vt, out, B=B, H=heads, Lq=L, Lk=L, dh=dh, ldq=2 * Cc, ldk=2 * Cc, ldv=ldv, ldo=Cc, scale=scale,
                  k_off=Cc, causal=True)
    torch.cuda.synchronize()
    assert rel_l2(out.float().view(B, L, Cc), ref) < 6e-3
    # token 0 sees only itself: its output is exactly (bf16 of) v[0]
    assert float((out.float().view(B, L, Cc)[:, 0] - v[:, 0]).abs().max()) < 2e-2
    # what CLIPTextEngine runs since round 5: [Q | K | V] in one buffer, V row-major (rows of the NEXT sample follow a sample's
    # last key: the ragged last key tile must read them as zeros - the buffer descriptor's range ends at this sample's last row)
    qkv = torch.cat([q, k, v], -1).reshape(-1, 3 * Cc).to(BF16).contiguous()
    out3 = torch.full((B * L, Cc), float("nan"), dtype=BF16, device=dev)
    hip.attention(qkv, qkv, qkv, out3, B=B, H=heads, Lq=L, Lk=L, dh=dh, ldq=3 * Cc, ldk=3 * Cc, ldv=3 * Cc, ldo=Cc, scale=scale,
                  k_off=Cc, v_off=2 * Cc, causal=True, v_rowmajor=True)
    torch.cuda.synchronize()
    assert torch.equal(out3, out)


def test_clip_glue_kernels(hip, dev):
    """embed_tokens and the quick_gelu / exact-GELU GEMM epilogues (CLIP text MLP)."""
    g = torch.Generator().manual_seed(80)
    V, L, D = 50, 77, 64
    tok, pos = torch.randn((V, D), generator=g).to(dev), torch.randn((L, D), generator=g).to(dev)
    ids = torch.randint(0, V, (3, L), generator=g).to(dev)
    out = hip.embed_tokens(ids, tok, pos)
    assert torch.equal(out.float().cpu(), bf16_round((tok[ids] + pos[None]).reshape(-1, D).cpu()))
    M, N, K = 231, 192, 128
    x, w, b = rnd((M, K), dev, 81), rnd((N, K), dev, 82, K ** -0.5), rnd((N,), dev, 83)
    y = x @ w.T + b
    for tile in (0, 1, 3):
        q = hip.linear(x.to(BF16), w.to(BF16), b, epi=4, tile=tile)
        assert rel_l2(q.float(), y * torch.sigmoid(1.702 * y)) < MFMA_TOL
        e = hip.linear(x.to(BF16), w.to(BF16), b, epi=5, tile=tile)
        assert rel_l2(e.float(), F.gelu(y)) < MFMA_TOL


def test_softmax_rows(hip, dev):
    s = rnd((64, 512), dev, 46, 3.0)
    sb = s.to(BF16).contiguous()
    hip.softmax_rows_(sb, 64, 512, 512)
    assert rel_l2(sb.float(), torch.softmax(s, -1)) < 4e-3


def test_softmax_rows_f32_and_fp32_scores(hip, dev):
    """The VAE mid-block attention's score path: Q K^T leaves the igemm as fp32 (out_mode 1, any N, batched) - within fp32
    summation error of a float64 product, i.e. NOT rounded to bf16 - and sdv_softmax_rows_f32 turns the fp32 rows into bf16
    probabilities rounded once (half a bf16 ulp of the float64 softmax of the same fp32 scores, + the fast exponential)."""
    nb, HW, C = 3, 256, 128
    qk = rnd((nb * HW, 2 * C), dev, 47).to(BF16)
    s = torch.full((nb, HW, HW), float("nan"), dtype=torch.float32, device=dev)
    hip.gemm(qk, qk, None, M=HW, N=HW, K=C, ldx=2 * C, ldw=2 * C, ldc=HW, alpha=C ** -0.5, batch=nb, sX=HW * 2 * C, sW=HW * 2 * C,
             sC=HW * HW, w_off=C, out_mode=1, out_f32=s)
    q, k = qk.view(nb, HW, 2 * C)[..., :C].double(), qk.view(nb, HW, 2 * C)[..., C:].double()
    ref = torch.einsum("bqc,bkc->bqk", q, k) * C ** -0.5
    mag = torch.einsum("bqc,bkc->bqk", q.abs(), k.abs()) * C ** -0.5
    assert float(((s.double() - ref).abs() / mag).max()) < 1e-5                      # bf16 storage would show 2e-3 here
    p = torch.empty((nb * HW, HW), dtype=BF16, device=dev)
    hip.softmax_rows_f32(s, p, nb * HW, HW, HW, HW)
    pref = torch.softmax(s.double().view(nb * HW, HW) , -1)
    ulp = torch.exp2(torch.floor(torch.log2(pref.clamp_min(1e-30))) - 7)
    assert float(((p.double() - pref).abs() / (0.5 * ulp + 1e-6 * pref)).max()) <= 1.05
    with pytest.raises(hip.SdvHipError, match="image output forms"):
        hip.gemm(qk, qk, None, M=HW, N=HW, K=C, ldx=2 * C, ldw=2 * C, ldc=HW, out_mode=2, out_f32=s)


# ------------------------------------------------------------------------------------------------
# norms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,HW,C1,C2,groups,silu", [(2, 256, 320, 0, 32, True), (3, 64, 640, 320, 32, True),
                                                     (1, 4096, 128, 0, 32, False), (2, 16, 1280, 1280, 32, True),
                                                     (2, 100, 64, 0, 32, False)])
def test_groupnorm(hip, dev, n, HW, C1, C2, groups, silu):
    C = C1 + C2
    x1 = rnd((n, HW, C1), dev, 50) * 2 + 0.5
    x1 = bf16_round(x1)
    x2 = bf16_round(rnd((n, HW, C2), dev, 51) - 0.3) if C2 else None
    gamma, beta = rnd((C,), dev, 52) * 0.1 + 1, rnd((C,), dev, 53) * 0.1
    xc = torch.cat([x1, x2], -1) if C2 else x1
    ref = F.group_norm(xc.permute(0, 2, 1), groups, gamma, beta, 1e-5).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    out = hip.groupnorm(x1.reshape(-1, C1).to(BF16), gamma, beta, nimg=n, HW=HW, groups=groups, eps=1e-5, silu=silu,
                        x2=x2.reshape(-1, C2).to(BF16) if C2 else None)
    torch.cuda.synchronize()
    err = (out.float().view(n, HW, C) - ref).abs()
    assert float(err.max()) < 0.03 and rel_l2(out.float().view(n, HW, C), ref) < 4e-3


@pytest.mark.parametrize("C", [64, 320, 640, 1280])
def test_layernorm(hip, dev, C):
    x = bf16_round(rnd((300, C), dev, 54) * 1.5 + 0.2)
    gamma, beta = rnd((C,), dev, 55) * 0.1 + 1, rnd((C,), dev, 56) * 0.1
    out = hip.layernorm(x.to(BF16), gamma, beta, 1e-5)
    assert rel_l2(out.float(), F.layer_norm(x, (C,), gamma, beta, 1e-5)) < 4e-3


# ------------------------------------------------------------------------------------------------
# interpolation, CFG + DDIM, embeddings
# ------------------------------------------------------------------------------------------------
def test_slerp_matches_reference_golden(hip, dev):
    """HIP slerp vs the vectors produced by the reference's own slerp (tests/golden/make_golden.py).

    Not bit-exact by construction, and the bound says by how much: the reference reduces ``dot`` and evaluates arccos / sin in
    float32 numpy scalars (utils.py:51-59; pairwise fp32 sums over 16384 elements move ``dot`` by ~1e-7), the kernel reduces and
    evaluates the two coefficients in fp64 and rounds them to fp32 ONCE, then forms ``s0 * v0 + s1 * v1`` with one fused
    multiply-add where numpy rounds both products.  Emulating exactly that arithmetic on the CPU against the golden vectors gives
    max |d| = 4.8e-7 = 1 ulp of the largest element (4.22) on the seeded pair, 2.4e-7 / 1.2e-7 on the (anti)parallel pairs; the
    gate is 2 ulp of the largest element of each golden frame (~9.5e-7; it was a flat 2e-5 = 40 ulp in round 2)."""
    for name in ("slerp_seed42_1337_fp32", "slerp_parallel_fp32", "slerp_antiparallel_fp32"):
        d = np.load(GOLDEN / f"{name}.npz")
        v0, v1 = torch.from_numpy(d["v0"]).to(dev), torch.from_numpy(d["v1"]).to(dev)
        ts = d["ts"]
        stats = hip.slerp_stats(v0.contiguous(), v1.contiguous())
        T = torch.tensor(ts, dtype=F32, device=dev)
        out = hip.slerp_batch(v0, v1, stats, T, C_=1, HW=v0.numel(), to_hwc=False)
        for i, t in enumerate(ts):
            gold = torch.from_numpy(d[f"t{int(t * 100):03d}"]).to(dev).flatten()
            tol = 2.0 * float(np.spacing(np.float32(gold.abs().max().item())))
            err = float((out[i] - gold).abs().max())
            assert err <= tol, (name, t, err, tol)
    # fp16 in -> fp16 out, the reference's own fp16 behaviour (its numpy round trip reduces dot and the norms in float16,
    # utils.py:45-61): the HIP path takes the SAME fp16 endpoints (exact in fp32), interpolates in fp32 and is compared with the
    # reference's fp16 frames.  Tolerance, stated: one float16 ulp of the frame's largest element (1.95e-3 at |x| < 4) - half an
    # ulp is the reference's own output rounding, the rest its float16 products and float16 dot (an fp32 / fp64 evaluation of
    # the same formula sits 1.5e-3 ... 1.8e-3 from the golden frames, measured on the CPU); the endpoints t = 0 / 1 are exact.
    d = np.load(GOLDEN / "slerp_seed7_8_fp16.npz")
    v0, v1 = torch.from_numpy(d["v0"].astype(np.float32)).to(dev), torch.from_numpy(d["v1"].astype(np.float32)).to(dev)
    stats = hip.slerp_stats(v0.contiguous(), v1.contiguous())
    out = hip.slerp_batch(v0, v1, stats, torch.tensor(d["ts"], dtype=F32, device=dev), C_=1, HW=v0.numel(), to_hwc=False)
    for i, t in enumerate(d["ts"]):
        gold = torch.from_numpy(d[f"t{int(t * 100):03d}"].astype(np.float32)).to(dev).flatten()
        err = float((out[i] - gold).abs().max())
        tol = 0.0 if t in (0.0, 1.0) else float(np.spacing(np.float16(gold.abs().max().item())))
        assert err <= tol, ("slerp_seed7_8_fp16", t, err, tol)
    # NHWC output layout + public slerp() helper
    from stable_diffusion_videos_amd.utils import slerp
    d = np.load(GOLDEN / "slerp_seed42_1337_fp32.npz")
    v0, v1 = torch.from_numpy(d["v0"]).to(dev), torch.from_numpy(d["v1"]).to(dev)
    got = slerp(0.5, v0, v1)
    assert got.shape == v0.shape and float((got.cpu() - torch.from_numpy(d["t050"])).abs().max()) <= 2.0 * float(np.spacing(np.float32(np.abs(d["t050"]).max())))
    stats = hip.slerp_stats(v0, v1)
    hwc = hip.slerp_batch(v0, v1, stats, torch.tensor([0.5], device=dev), C_=4, HW=64 * 64, to_hwc=True)
    assert torch.allclose(hwc.view(64, 64, 4).permute(2, 0, 1), got[0], atol=1e-6)
    # bf16 endpoints: the reference raises (numpy has no bf16); the HIP path interpolates in fp32
    assert slerp(0.25, v0.to(BF16), v1.to(BF16)).dtype == BF16


def test_lerp(hip, dev):
    a, b = torch.randn(77 * 768, device=dev), torch.randn(77 * 768, device=dev)
    T = torch.tensor([0.0, 0.3, 0.5, 0.9, 1.0], device=dev)
    o32 = torch.empty((5, a.numel()), device=dev)
    o16 = torch.empty((5, a.numel()), dtype=BF16, device=dev)
    hip.lerp_batch(a, b, T, out_f32=o32, out_bf16=o16)
    for i, t in enumerate(T.tolist()):
        ref = torch.lerp(a, b, t)
        assert float((o32[i] - ref).abs().max()) < 1e-6
        assert torch.equal(o16[i], ref.to(BF16)) or float((o16[i].float() - ref).abs().max()) < 0.02
    assert torch.equal(o32[0], a) and torch.equal(o32[-1], b)


def test_cfg_ddim_step_matches_oracle(hip, dev):
    from oracle.scheduler import DDIMScheduler as OracleDDIM
    from stable_diffusion_videos_amd.scheduler import DDIMScheduler
    for ptype in ("epsilon", "v_prediction"):
        osch, sch = OracleDDIM(prediction_type=ptype), DDIMScheduler(prediction_type=ptype)
        osch.set_timesteps(50)
        sch.set_timesteps(50)
        assert sch.timesteps.tolist() == osch.timesteps.tolist() == list(range(981, 0, -20))
        coefs = sch.coefficient_table(0.0).to(dev)
        B, n = 2, 2 * 8 * 8 * 4
        x = torch.randn(n)
        eps2 = torch.randn(2 * n)
        g = 7.5
        step = torch.zeros(1, dtype=torch.int32, device=dev)
        lat = x.clone().to(dev)
        x2 = torch.empty(2 * n, dtype=BF16, device=dev)
        ref = x.clone()
        for i, t in enumerate(osch.timesteps[:4]):
            e = eps2[:n] + g * (eps2[n:] - eps2[:n])
            ref = osch.step(e, t, ref)
            hip.cfg_ddim_step(eps2.to(dev), lat, x2, coefs, step, None, g, True, n)
            hip.step_counter_add(step, 1)
            assert float((lat.cpu() - ref).abs().max()) < 5e-5 * max(1.0, float(ref.abs().max())), (ptype, i)
            assert torch.equal(x2[:n], lat.to(BF16)) and torch.equal(x2[n:], lat.to(BF16))
        assert int(step.item()) == 4


@pytest.mark.parametrize("name", ["PNDMScheduler", "LMSDiscreteScheduler", "EulerDiscreteScheduler", "EulerAncestralDiscreteScheduler",
                                  "DPMSolverMultistepScheduler"])
@pytest.mark.parametrize("ptype", ["epsilon", "v_prediction"])
def test_cfg_multistep_step_matches_oracle(hip, dev, name, ptype):
    """``sdv_cfg_multistep_step`` (guidance + scheduler.step + the next scale_model_input, one launch) driven by the product's
    coefficient table, against the oracle's CLASSIC stateful scheduler (stable_diffusion_pipeline.py:415, :422-426 with the
    schedulers of :71-78) on the same sequence of model outputs - all evaluations of a 12-step schedule, incl. PLMS's repeated
    second timestep and the history ring wrapping around."""
    from oracle import scheduler as O
    from stable_diffusion_videos_amd import scheduler as P
    o, p = getattr(O, name)(prediction_type=ptype), getattr(P, name)(prediction_type=ptype)
    o.set_timesteps(12)
    p.set_timesteps(12)
    table = p.fused_table().to(dev)
    n, g = 2 * 8 * 8 * 4, 7.5
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(n, generator=gen) * float(o.init_noise_sigma)
    lat, ref = x.clone().to(dev), x.clone().double()
    x2 = torch.empty(2 * n, dtype=BF16, device=dev)
    hist, xsave = torch.zeros((4, n), device=dev), torch.zeros(n, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    noise = torch.randn((len(o.timesteps), n), generator=gen)
    for i, t in enumerate(o.timesteps):
        eps2 = torch.randn(2 * n, generator=gen)
        e = (eps2[:n] + g * (eps2[n:] - eps2[:n])).double()
        ref = o.step(e, t, ref, variance_noise=noise[i].double())
        hip.cfg_multistep_step(eps2.to(dev), lat, x2, hist, xsave, table, step, noise.to(dev) if p.stochastic else None, g, True, n)
        hip.step_counter_add(step, 1)
        assert float((lat.cpu().double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())), (name, ptype, i)
        if i + 1 < len(o.timesteps):      # the next evaluation's scaled model input, both CFG halves
            want = o.scale_model_input(lat.cpu(), o.timesteps[i + 1]).to(BF16)
            assert float((x2[:n].cpu().float() - want.float()).abs().max()) <= 2 ** -7 * float(want.float().abs().max())
            assert torch.equal(x2[:n], x2[n:])
    assert int(step.item()) == len(o.timesteps) == (13 if name == "PNDMScheduler" else 12)


def test_timestep_embedding_and_linear_small(hip, dev):
    from oracle.models import timestep_embedding
    ts = torch.tensor([981.0, 501.0, 1.0], device=dev)
    got = hip.timestep_embedding(ts, 320, True, 0.0)
    ref = timestep_embedding(ts.cpu(), 320, True, 0)
    assert float((got.cpu() - ref).abs().max()) < 2e-4     # fp32 sin/cos of arguments up to ~1e3
    x, w, b, add = torch.randn(7, 320, device=dev), rnd((1280, 320), dev, 60, 320 ** -0.5), torch.randn(1280, device=dev), \
        torch.randn(1280, device=dev)
    out = hip.linear_small(x, w.to(BF16), b, add, silu_in=True)
    assert rel_l2(out, F.silu(x) @ w.T + b + add) < 1e-5


def test_layout_helpers(hip, dev):
    x = torch.randn(3, 4, 5, 7, device=dev)
    assert torch.equal(hip.nchw_to_nhwc(x), x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(hip.nhwc_to_nchw(hip.nchw_to_nhwc(x)), x)
    assert torch.equal(hip.f32_to_bf16(x), x.to(BF16))


def test_torch_custom_ops_run_the_same_kernels(hip, dev):
    """torch.ops.sdv.* (stable_diffusion_videos_amd/ops.py) forward to the same C-ABI launches as the ctypes wrappers."""
    import stable_diffusion_videos_amd  # noqa: F401  (registers the ops)
    from stable_diffusion_videos_amd.weights import conv_w, upconv_phase_w
    x, w, b = rnd((256, 128), dev, 90).to(BF16), rnd((192, 128), dev, 91, 128 ** -0.5).to(BF16), rnd((192,), dev, 92)
    assert torch.equal(torch.ops.sdv.linear(x, w, b), hip.linear(x, w, b))
    xc = rnd((2 * 8 * 8, 64), dev, 93).to(BF16)
    wc = rnd((64, 64, 3, 3), dev, 94, 576 ** -0.5)
    assert torch.equal(torch.ops.sdv.conv3x3(xc, conv_w(wc, dev), None, 2, 8, 8), hip.conv3x3(xc, conv_w(wc, dev), None, nimg=2, H=8, W=8))
    up = torch.ops.sdv.upsample_conv3x3(xc, upconv_phase_w(wc.cpu(), dev), None, 2, 8, 8)
    assert up.shape == (2 * 16 * 16, 64) and torch.equal(up, hip.upconv3x3_phase(xc, upconv_phase_w(wc.cpu(), dev), None, nimg=2, H=8, W=8))
    q, k, v = rnd((2, 100, 80), dev, 95), rnd((2, 77, 80), dev, 96), rnd((2, 77, 80), dev, 97)
    vt = torch.zeros((2, 80, 128), dtype=BF16, device=dev)
    vt[:, :, :77] = v.transpose(1, 2).to(BF16)
    o = torch.ops.sdv.attention(q.to(BF16), k.to(BF16), vt, 2, 40 ** -0.5)
    assert rel_l2(o.float(), attn_ref(q, k, v, 2, 40 ** -0.5)) < 6e-3
    g, be = rnd((128,), dev, 98), rnd((128,), dev, 99)
    assert torch.equal(torch.ops.sdv.layer_norm(x, g, be), hip.layernorm(x, g, be))
    assert torch.equal(torch.ops.sdv.group_norm(x, g, be, 2, 32, 1e-5, True), hip.groupnorm(x, g, be, nimg=2, HW=128, groups=32, eps=1e-5, silu=True))
    a, bb = rnd((1, 77, 64), dev, 100), rnd((1, 77, 64), dev, 101)
    T = torch.tensor([0.0, 0.25, 1.0], device=dev)
    assert torch.allclose(torch.ops.sdv.lerp_batch(a, bb, T), torch.stack([torch.lerp(a[0], bb[0], float(t)) for t in T]), atol=1e-6)
    s3 = torch.ops.sdv.slerp_batch(a, bb, T)
    assert s3.shape == (3, 77, 64) and torch.equal(s3[0], a[0]) and torch.equal(s3[2], bb[0])


# ------------------------------------------------------------------------------------------------
# fp8 (OCP e4m3) operands - BASELINE config 5
# ------------------------------------------------------------------------------------------------
def _q8(t, amax=None):
    """per-tensor e4m3 quantisation as the engine does it: scale = amax / 448, q = fp8(t / scale)."""
    s = float(t.abs().max() if amax is None else amax) / 448.0
    return (t / s).to(torch.float8_e4m3fn), s


@pytest.mark.parametrize("mx", [0, 1])
@pytest.mark.parametrize("tile", [0, 1, 6, 7, 9])
def test_gemm_and_conv_fp8_operands(hip, dev, tile, mx, monkeypatch):
    """sdv_gemm_bf16 with fp8 = 1 (v_mfma_f32_32x32x16_fp8_fp8) and fp8 = 2 (the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4
    with unit scales, twice the rate): against fp32 arithmetic on the SAME quantised values - what remains is fp32
    accumulation order and the bf16 output rounding, i.e. the bf16 kernels' own tolerance."""
    monkeypatch.setattr(hip, "FP8_MX", mx)
    M, N, K = 777, 640, 1280
    x, w = rnd((M, K), dev, 120), rnd((N, K), dev, 121, K ** -0.5)
    bias, res = rnd((N,), dev, 122), rnd((M, N), dev, 123)
    x8, sx = _q8(x)
    w8, sw = _q8(w)
    out = hip.linear(x8, w8, bias, residual=res.to(BF16), alpha=sx * sw, tile=tile)
    ref = (x8.float() * sx) @ (w8.float() * sw).T + bias + res
    assert rel_l2(out.float(), ref) < MFMA_TOL
    # how far fp8 is from the bf16 arithmetic on this data (reported, not gated: ~2^-4 relative per element / sqrt(K))
    full = x @ w.T + bias + res
    from conftest import report
    if tile == 0:
        report(f"fp8 GEMM (form {1 + mx}) vs unquantised fp32: rel-L2 {rel_l2(out.float(), full):.2e}")
    # conv3x3 (two-source concat, residual), NHWC
    n, H, W, C1, C2, Cout = 2, 16, 16, 128, 64, 320
    xa, xb = rnd((n, H, W, C1), dev, 124), rnd((n, H, W, C2), dev, 125)
    wc = rnd((Cout, C1 + C2, 3, 3), dev, 126, (9 * (C1 + C2)) ** -0.5)
    bc, rc = rnd((Cout,), dev, 127), rnd((n, H, W, Cout), dev, 128)
    amax = max(float(xa.abs().max()), float(xb.abs().max()))
    xa8, sa = _q8(xa, amax)
    xb8, _ = _q8(xb, amax)
    wc8, swc = _q8(wc)
    w_ohwi = wc8.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
    out = hip.conv3x3(xa8.reshape(-1, C1), w_ohwi, bc, nimg=n, H=H, W=W, x2=xb8.reshape(-1, C2), residual=rc.reshape(-1, Cout).to(BF16),
                      alpha=sa * swc, tile=tile)
    ref = conv_ref(torch.cat([xa8.float(), xb8.float()], -1) * sa, wc8.float() * swc, bc, 1, False) + rc
    assert rel_l2(out.float().reshape(ref.shape), ref) < MFMA_TOL


@pytest.mark.parametrize("tile", [0, 1, 6, 7, 9])
def test_fp8_mx_form_matches_float64_on_exact_products(hip, dev, tile, monkeypatch):
    """fp8 = 2 on shapes whose number of 64-wide K images is ODD (the K loop's last slab carries a dead image: K = 320 dense, 5
    images; 9 x 320 / 64 = 45 for the ResBlock conv of the 64^2 level; K = 64: one live image in all) and EVEN (K = 640), with
    enough tiles that the 8-wave tiles walk persistently.  e4m3 x e4m3 products are exact in fp32, so against float64 on the
    same bytes only the accumulation (and the bf16 output rounding) remains.  Bound: half a bf16 ulp + 4e-5 sum|x w| - the fp8
    MFMAs do not accumulate like an fp32 FMA chain (measured on MI355X: worst element 1.3e-5 sum|x w| at K = 320 for BOTH
    forms, to the digit - the two instructions sum the same products the same way; the bf16 MFMA stays below 1e-5; both forms
    are reported side by side).  An operand in the wrong K position, a K image counted twice or dropped, or a dead image that
    is not zero all show up at 1e-1."""
    from conftest import report

    def worst_dense(form, M, N, K):
        monkeypatch.setattr(hip, "FP8_MX", form - 1)
        x8, sx = _q8(rnd((M, K), dev, 140 + K))
        w8, sw = _q8(rnd((N, K), dev, 141 + K, K ** -0.5))
        out = hip.linear(x8, w8, None, alpha=sx * sw, tile=tile).double()
        assert torch.equal(out, hip.linear(x8, w8, None, alpha=sx * sw, tile=tile).double())       # (deterministic across launches)
        xd, wd = x8.double() * sx, w8.double() * sw
        ref = xd @ wd.T
        err = ((out - ref).abs() - ref.abs() * 2.0 ** -8).clamp_min(0.0)            # what half a bf16 ulp does not explain ...
        return float((err / (xd.abs() @ wd.abs().T + 1e-30)).max())                # ... in units of sum|x w|

    def worst_conv(form, n, H, W, Cin, Cout):
        monkeypatch.setattr(hip, "FP8_MX", form - 1)
        x8, sx = _q8(rnd((n, H, W, Cin), dev, 150 + Cin))
        wc8, sw = _q8(rnd((Cout, Cin, 3, 3), dev, 151 + Cin, (9 * Cin) ** -0.5))
        w_ohwi = wc8.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous()
        out = hip.conv3x3(x8.reshape(-1, Cin), w_ohwi, None, nimg=n, H=H, W=W, alpha=sx * sw, tile=tile).double().reshape(n, H, W, Cout)
        xd, wd = x8.double() * sx, wc8.double() * sw
        ref = F.conv2d(xd.permute(0, 3, 1, 2), wd, None, 1, 1).permute(0, 2, 3, 1)
        mag = F.conv2d(xd.abs().permute(0, 3, 1, 2), wd.abs(), None, 1, 1).permute(0, 2, 3, 1)
        err = ((out - ref).abs() - ref.abs() * 2.0 ** -8).clamp_min(0.0)
        return float((err / (mag + 1e-30)).max())

    for shape in [(70000, 320, 320), (4099, 960, 640), (333, 64, 64)]:
        e1, e2 = worst_dense(1, *shape), worst_dense(2, *shape)
        if tile == 0:
            report(f"fp8 dense {shape}: accumulation error beyond the output rounding, worst element: plain fp8 {e1:.1e}, MX form {e2:.1e} (x sum|xw|)")
        assert e1 <= 4e-5 and e2 <= 4e-5, f"dense {shape} tile {tile}: {e1:.2e} / {e2:.2e} sum|xw|"
    # the SD-1.4 64^2-level ResBlock conv shape (Cin = 320: 45 K images, 96 tiles of 256 rows), and a 960-channel one
    for shape in [(6, 64, 64, 320, 320), (2, 32, 32, 960, 640)]:
        e1, e2 = worst_conv(1, *shape), worst_conv(2, *shape)
        if tile == 0:
            report(f"fp8 conv {shape}: worst element: plain fp8 {e1:.1e}, MX form {e2:.1e} (x sum|xw|)")
        assert e1 <= 4e-5 and e2 <= 4e-5, f"conv {shape} tile {tile}: {e1:.2e} / {e2:.2e} sum|xw|"


def test_groupnorm_fp8_output(hip, dev):
    """sdv_groupnorm_apply_fp8: the e4m3 bytes are the round-to-nearest quantisation of the bf16 kernel's fp32 result."""
    n, HW, C = 2, 256, 320
    x = rnd((n * HW, C), dev, 130)
    g, b = 1.0 + 0.2 * rnd((C,), dev, 131), 0.1 * rnd((C,), dev, 132)
    y = F.silu(F.group_norm(x.view(n, HW, C).transpose(1, 2), 32, g, b, 1e-5)).transpose(1, 2).reshape(n * HW, C)
    s = float(y.abs().max()) / 448.0
    q = hip.groupnorm(x.to(BF16), g, b, nimg=n, HW=HW, groups=32, eps=1e-5, silu=True, fp8_scale=s)
    assert q.dtype == torch.float8_e4m3fn and q.shape == (n * HW, C)
    d = (q.float() * s - y).abs()
    ulp = torch.exp2(torch.floor(torch.log2((y.abs() / s).clamp_min(2.0 ** -6))) - 3) * s      # e4m3: 3 mantissa bits
    assert float((d / ulp).max()) <= 0.75      # half an ulp + the fp32 differences of the two evaluations of y


# ------------------------------------------------------------------------------------------------
# GroupNorm statistics out of the producing igemm's epilogue (sdv_gemm_args.gn_out + sdv_groupnorm_finalize)
# ------------------------------------------------------------------------------------------------
def _gn_ref_blocks(out, nblocks):
    o = out.float().view(nblocks, 32, -1)
    return o.sum(1), (o * o).sum(1)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 6, 7, 8, 9])
@pytest.mark.parametrize("kind", ["dense", "dense_res", "conv", "conv_res", "conv_s2", "dense_batch2"])
def test_igemm_epilogue_emits_groupnorm_statistics(hip, dev, tile, kind):
    """Every (32-row block, channel) entry of gn_out is the (sum, sumsq) of the bf16 values the launch STORED - compared with a
    float64 reduction of the output tensor itself (so the check is independent of the GEMM's own accuracy): the fp32 in-kernel
    sums of 32 values differ by <= 32 * 2^-24 relative of sum|x| / sum x^2.  Ragged N (320 on 256-column tiles), several tiles
    per launch, all tiles that carry the row-major store sequence."""
    nimg, H, W, Cin, Cout = 3, 16, 16, 128, 320
    x = rnd((nimg * H * W, Cin), dev, 201).to(BF16)
    bias = rnd((Cout,), dev, 203)
    if kind.startswith("dense"):
        w = rnd((Cout, Cin), dev, 202, Cin ** -0.5).to(BF16)
        if kind == "dense_batch2":          # the CFG-shared proj_out: two batches read one residual (batch stride 0)
            M = nimg * H * W
            x2b = torch.cat([x, rnd((M, Cin), dev, 205).to(BF16)])
            res = rnd((M, Cout), dev, 204).to(BF16)
            out = torch.empty((2 * M, Cout), dtype=BF16, device=dev)
            hip.gemm(x2b, w, out, M=M, N=Cout, K=Cin, ldx=Cin, ldw=Cin, ldc=Cout, bias=bias, residual=res, ldr=Cout, batch=2,
                     sX=M * Cin, sW=0, sC=M * Cout, sR=0, gn_hw=H * W, tile=tile)
            nb_img = 2 * nimg
        else:
            res = rnd((nimg * H * W, Cout), dev, 204).to(BF16) if kind == "dense_res" else None
            out = hip.linear(x, w, bias, residual=res, gn_hw=H * W, tile=tile)
            nb_img = nimg
        Ho = H
    else:
        w = rnd((Cout, 9 * Cin), dev, 202, (9 * Cin) ** -0.5).to(BF16)
        mode = 2 if kind == "conv_s2" else 1
        Ho = H // 2 if mode == 2 else H
        res = rnd((nimg * Ho * Ho, Cout), dev, 204).to(BF16) if kind == "conv_res" else None
        out = hip.conv3x3(x, w, bias, nimg=nimg, H=H, W=W, mode=mode, residual=res, gn=True, tile=tile)
        nb_img = nimg
    torch.cuda.synchronize()
    g = getattr(out, "_sdv_gn", None)
    assert g is not None and (g.nimg, g.HW, g.C, g.nrep) == (nb_img, Ho * Ho, Cout, 1)
    nblocks = out.shape[0] // 32
    assert tuple(g.p.shape) == (nblocks, 2, Cout) and g.bpi == Ho * Ho // 32
    s_ref, q_ref = _gn_ref_blocks(out.double(), nblocks)
    a_ref, _ = _gn_ref_blocks(out.double().abs(), nblocks)
    assert float(((g.p[:, 0].double() - s_ref).abs() / (a_ref + 1e-30)).max()) < 4e-6
    assert float(((g.p[:, 1].double() - q_ref).abs() / (q_ref + 1e-30)).max()) < 4e-6


def test_upconv_phase_form_emits_groupnorm_statistics(hip, dev):
    from stable_diffusion_videos_amd.weights import upconv_phase_w
    nimg, H, W, C = 2, 16, 16, 320
    x = rnd((nimg * H * W, C), dev, 211).to(BF16)
    w = rnd((C, C, 3, 3), dev, 212, (9 * C) ** -0.5)
    out = hip.upconv3x3_phase(x, upconv_phase_w(w.cpu(), dev), rnd((C,), dev, 213), nimg=nimg, H=H, W=W, gn=True)
    torch.cuda.synchronize()
    g = out._sdv_gn
    assert (g.nimg, g.HW, g.C, g.nrep, g.bpi, g.rep_stride) == (nimg, 4 * H * W, C, 4, H * W // 32, nimg * H * W // 32)
    # per image and channel: the four phases' blocks of the image add up to the image's sums
    p = g.p.double().view(4, nimg, H * W // 32, 2, C).sum((0, 2))
    o = out.double().view(nimg, 4 * H * W, C)
    assert float(((p[:, 0] - o.sum(1)).abs() / o.abs().sum(1)).max()) < 4e-6
    assert float(((p[:, 1] - (o * o).sum(1)).abs() / (o * o).sum(1)).max()) < 4e-6


@pytest.mark.parametrize("concat", [False, True])
def test_groupnorm_on_epilogue_statistics_matches_the_statistics_pass(hip, dev, concat):
    """GroupNorm fed by the producers' statistics (finalize + apply) against the same GroupNorm with its own statistics pass over
    the same tensors.  960 channels / 32 groups = 30 per group: with a 640 + 320 concat the group [630, 660) straddles the seam,
    which is why the producers emit per-channel sums.  The two agree to fp32 summation order: <= 1 bf16 ulp on a few elements
    (or 1e-4 absolute where the normalised value cancels to ~0 and an ulp of the result means nothing)."""
    nimg, H, C1, C2 = 4, 32, 640, 320
    HW = H * H
    xa = rnd((nimg * HW, 128), dev, 221).to(BF16)
    a = hip.linear(xa, rnd((C1, 128), dev, 222, 128 ** -0.5).to(BF16), rnd((C1,), dev, 223), gn_hw=HW)
    b = hip.upconv3x3_phase(rnd((nimg * HW // 4, 128), dev, 224).to(BF16), __import__("stable_diffusion_videos_amd.weights", fromlist=["x"]).upconv_phase_w(
        rnd((C2, 128, 3, 3), dev, 225, (9 * 128) ** -0.5).cpu(), dev), rnd((C2,), dev, 226), nimg=nimg, H=H // 2, W=H // 2, gn=True) if concat else None
    C = C1 + (C2 if concat else 0)
    gamma, beta = 1.0 + 0.1 * rnd((C,), dev, 227), 0.1 * rnd((C,), dev, 228)
    seen = []
    hip.LAUNCH_HOOK = lambda kind, info, fn: (seen.append(kind), fn())
    try:
        fast = hip.groupnorm(a, gamma, beta, nimg=nimg, HW=HW, groups=32, eps=1e-5, silu=True, x2=b)
    finally:
        hip.LAUNCH_HOOK = None
    assert seen == ["gn_finalize", "gn_apply"]
    a2, b2 = a.clone(), (b.clone() if concat else None)          # clones carry no statistics -> the statistics pass runs
    seen.clear()
    hip.LAUNCH_HOOK = lambda kind, info, fn: (seen.append(kind), fn())
    try:
        slow = hip.groupnorm(a2, gamma, beta, nimg=nimg, HW=HW, groups=32, eps=1e-5, silu=True, x2=b2)
    finally:
        hip.LAUNCH_HOOK = None
    assert seen == ["gn_stats", "gn_apply"]
    torch.cuda.synchronize()
    d = (fast.float() - slow.float()).abs()
    ulp = torch.exp2(torch.floor(torch.log2(slow.float().abs().clamp_min(1e-30))) - 7)
    assert bool(((d <= ulp) | (d <= 1e-4)).all()) and float((d > 0).float().mean()) < 0.02
    ref_in = torch.cat([a.float(), b.float()], 1) if concat else a.float()
    ref = F.silu(F.group_norm(ref_in.view(nimg, HW, C).transpose(1, 2), 32, gamma, beta, 1e-5)).transpose(1, 2).reshape(nimg * HW, C)
    assert rel_l2(fast.float(), ref) < 4e-3
    # a tensor whose statistics describe another shape is not trusted: half the images -> the statistics pass
    seen.clear()
    hip.LAUNCH_HOOK = lambda kind, info, fn: (seen.append(kind), fn())
    try:
        if not concat:
            hip.groupnorm(a, gamma, beta, nimg=nimg // 2, HW=2 * HW, groups=32, eps=1e-5, silu=True)
    finally:
        hip.LAUNCH_HOOK = None
    assert concat or seen == ["gn_stats", "gn_apply"]
    # ... and neither is a tensor that an in-place writer touched after the producer attached its statistics: the
    # version counter moved, so the statistics pass runs and the result is the GroupNorm of what the tensor holds NOW
    if not concat:
        a.mul_(0.5).add_(0.25)
        seen.clear()
        hip.LAUNCH_HOOK = lambda kind, info, fn: (seen.append(kind), fn())
        try:
            moved = hip.groupnorm(a, gamma, beta, nimg=nimg, HW=HW, groups=32, eps=1e-5, silu=True)
        finally:
            hip.LAUNCH_HOOK = None
        assert seen == ["gn_stats", "gn_apply"]
        ref = F.silu(F.group_norm(a.float().view(nimg, HW, C).transpose(1, 2), 32, gamma, beta, 1e-5)).transpose(1, 2).reshape(nimg * HW, C)
        assert rel_l2(moved.float(), ref) < 4e-3
