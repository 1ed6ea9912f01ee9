"""The 8-wave 256 x 320 igemm tile on v_mfma_f32_16x16x32_bf16 (csrc/sdv_gemm.hip "M16"): what a wrong accumulator layout would break.

With the 16 x 16 MFMA a lane owns row 16 hm + (lane & 15) and channels 16 hn + 4 (lane >> 4) .. + 3 of every 32 x 32 block, where it
owned row lane & 31 and channels 8 q + 4 (lane >> 5) before, and a K slab is two 32-deep k-steps instead of four 16-deep ones.  Every
test forces tile 6 and uses the case builders and THE checker of test_igemm_edges_gpu.py (its float64 element bound; its docstring
derives it).

* exact layout probe: integer operands whose products, sums, bias and residual stay below 256 in magnitude - exact in fp32 AND in the
  bf16 output - so every element must EQUAL the float64 value: a lane / row / channel mix-up, a k-step read from the wrong 16-byte
  chunk or a slab buffer used twice changes integers.  One, two and three K slabs: both k-steps of both slab buffers.
* the LayerNorm-fold + GEGLU epilogue (value / gate pairs now sit in neighbouring 16-row accumulators), the row statistics and the
  GroupNorm statistics epilogues, the conv forms, the two-source K walk, the persistent walk, and bit-identity across repeats and M.

Statistics tolerances are those the suite already holds the same epilogues to (test_kernels_gpu.py::test_gemm_layernorm_fold,
test_igemm_edges_gpu.py::test_split_k_at_its_smallest): fp32 sums of <= 320 bf16 values against float64 sums of the SAME stored values,
rtol 1e-5 + atol 1e-4 (320 x 2^-24 = 1.9e-5 of the mean magnitude at worst), rstd rtol 2e-3 (the finalize kernel's fast rsqrt).
"""
import functools
from types import SimpleNamespace

import pytest
import torch

from conftest import report
from test_igemm_edges_gpu import BF16, TILES, check_against_float64, make_case, run_case, walk_rows, _gelu64

pytestmark = pytest.mark.gpu
TILE = 6


@functools.lru_cache(maxsize=64)
def integer_case(M, N, K, variant):
    """make_case's dense case with integer operands: x in [-3, 3], 40 weights of +-1 per output channel (|sum| <= 120), bias in
    [-8, 8], residual in [-16, 16]: |result| <= 144, every intermediate an integer below 2^8."""
    base = make_case(mode=0, geom=(M,), C1=K, C2=0, N=N, bias="col" if variant == "bias" else None, res=variant == "residual")
    g = torch.Generator(device="cpu").manual_seed(7 * M + 3 * N + K)
    x = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.zeros((N, K))
    for n in range(N):
        idx = torch.randperm(K, generator=g)[:40]
        w[n, idx] = torch.randint(0, 2, (40,), generator=g).float() * 2 - 1
    bvec = torch.randint(-8, 9, (N,), generator=g).float() if variant == "bias" else None
    r = torch.randint(-16, 17, (M, N), generator=g).float() if variant == "residual" else None
    ref = x.double() @ w.double().T
    if bvec is not None:
        ref = ref + bvec.double()
    if r is not None:
        ref = ref + r.double()
    assert float(ref.abs().max()) <= 256
    c = SimpleNamespace(**vars(base))
    c.x, c.w, c.bvec, c.r, c.ref, c.exact = x, w, bvec, r, ref, True
    return c


@pytest.mark.parametrize("variant", ["plain", "residual", "bias"])
def test_exact_layout_probe(hip, dev, variant):
    for M in (33, 257):
        for N in (40, 328):
            for K in (64, 128, 192):
                try:
                    run_case(hip, dev, integer_case(M, N, K, variant), TILE)
                except AssertionError as e:
                    raise AssertionError(f"M {M} N {N} K {K} {variant}: {e}") from None


def test_geglu_with_layernorm_fold(hip, dev):
    """M 257, N 64 (32 outputs), K 128: out = v gelu(g), (v | g) = rstd (x (gamma o W)^T - mean s) + t.  Bound: the edges gate's GEGLU
    bound with the fold's magnitudes - (|x||W| + |mean||s|) rstd + |t| - in the place of |x||w| + |bias|."""
    from stable_diffusion_videos_amd.weights import geglu_interleave, ln_fold
    M, N, K = 257, 64, 128
    base = make_case(mode=0, geom=(M,), C1=K, C2=0, N=N, epi=1)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (base.x + 1.5).to(BF16)                                          # rows with a common mode: acc - mean s cancels
    xf = x.float()
    st = torch.stack([xf.mean(1), torch.rsqrt(xf.var(1, unbiased=False) + 1e-5)], 1).contiguous()
    gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    wg, sg, tg = ln_fold(geglu_interleave(base.w).to(dev), gamma.to(dev), beta.to(dev), geglu_interleave(base.bvec).to(dev), dev)
    out = hip.linear(x.to(dev), wg, tg, epi=1, ln=(st.to(dev), sg), tile=TILE)
    again = hip.linear(x.to(dev), wg, tg, epi=1, ln=(st.to(dev), sg), tile=TILE)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))
    # float64 of the same folded operands, de-interleaved: rows [16 value | 16 gate] per 32 -> (value half, gate half)
    w64, s64, t64 = wg.cpu().double(), sg.cpu().double(), tg.cpu().double()
    m64, r64 = st[:, :1].double(), st[:, 1:].double()
    pre = (xf.double() @ w64.T - m64 * s64[None]) * r64 + t64[None]
    mag = (xf.double().abs() @ w64.abs().T + m64.abs() * s64.abs()[None]) * r64 + t64.abs()[None]
    blk = lambda t: t.view(M, N // 32, 2, 16)
    v, gt, vm, gm = (blk(pre)[:, :, 0].reshape(M, -1), blk(pre)[:, :, 1].reshape(M, -1), blk(mag)[:, :, 0].reshape(M, -1),
                     blk(mag)[:, :, 1].reshape(M, -1))
    case = SimpleNamespace(ref=v * _gelu64(gt), mag=vm * _gelu64(gt).abs() + 1.2 * v.abs() * gm + (1e-6 / 1e-5) * v.abs() * (1 + gt.abs()),
                           exact=False, half_ulp=True, acc_eps=1e-5)
    worst = check_against_float64(out.cpu().double(), True, case)
    report(f"igemm 16x16 MFMA: GEGLU + LayerNorm fold on tile 6: worst element at {worst:.3f} of the bound")


def test_row_statistics(hip, dev):
    """FEAT 3 at M 257, N 320, K 64: the output against float64, (mean, rstd) against float64 of the rows as stored"""
    case = make_case(mode=0, geom=(257,), C1=64, C2=0, N=320, res=True)
    x, w, b, r = (t.to(dev) for t in (case.x.to(BF16), case.w.to(BF16), case.bvec, case.r.to(BF16)))
    y, st = hip.linear(x, w, b, residual=r, want_stats=True, tile=TILE)
    y2, st2 = hip.linear(x, w, b, residual=r, want_stats=True, tile=TILE)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16)) and torch.equal(st, st2)
    check_against_float64(y.cpu().double(), True, case)
    y64 = y.cpu().double()
    assert torch.allclose(st[:, 0].cpu().double(), y64.mean(1), rtol=1e-5, atol=1e-4)
    assert torch.allclose(st[:, 1].cpu().double(), torch.rsqrt(y64.var(1, unbiased=False) + 1e-5), rtol=2e-3)


def _gn_matches(p, win, N):
    g, of = p.cpu().double(), win.view(-1, 32, N)
    return torch.allclose(g[:, 0], of.sum(1), rtol=1e-5, atol=1e-4) and torch.allclose(g[:, 1], (of * of).sum(1), rtol=1e-5, atol=1e-4)


def test_groupnorm_statistics(hip, dev):
    """FEAT 4: conv 2 x 8 x 8, C 64 -> 320 and 64 -> 64 (with a residual: the fp32 slab) emit (sum, sumsq) per 32-row block and
    channel of the values as stored; 3 images of 5 x 7 (35 pixels: no whole 32-row blocks, the launch emits none) still has to be
    right; the dense form with 64 rows per image at M 192."""
    for geom, N, res in (((2, 8, 8), 320, False), ((2, 8, 8), 64, True), ((3, 5, 7), 64, False)):
        case = make_case(mode=1, geom=geom, C1=64, C2=0, N=N, res=res)
        win, _, ob = run_case(hip, dev, case, TILE, gn=True)
        if case.rows_out % 32 == 0:
            assert _gn_matches(ob.arg._sdv_gn.p, win, N), (geom, N)
        else:
            assert not hasattr(ob.arg, "_sdv_gn")
    case = make_case(mode=0, geom=(192,), C1=64, C2=0, N=320)
    out = hip.linear(case.x.to(BF16).to(dev), case.w.to(BF16).to(dev), case.bvec.to(dev), tile=TILE, gn_hw=64)
    torch.cuda.synchronize()
    win = out.cpu().double()
    check_against_float64(win, True, case)
    assert out._sdv_gn.p.shape == (6, 2, 320) and _gn_matches(out._sdv_gn.p, win, 320)


GEOMS = ((3, 5, 7), (9, 6, 6), (1, 9, 9), (3, 3, 5), (2, 4, 4))


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("circular", [False, True])
def test_conv_forms(hip, dev, mode, circular):
    worst = 0.0
    for geom in GEOMS:
        _, r, _ = run_case(hip, dev, make_case(mode=mode, geom=geom, C1=64, C2=0, N=72, circular=circular), TILE)
        worst = max(worst, r)
    report(f"igemm 16x16 MFMA: conv mode {mode} {'circular' if circular else 'zero'} on tile 6: worst element at {worst:.3f} of the bound")


def test_two_sources_and_the_persistent_walk(hip, dev):
    for mode in (0, 1):
        run_case(hip, dev, make_case(mode=mode, geom=(129,) if mode == 0 else (3, 5, 7), C1=64, C2=64, N=72, res=True), TILE)
    lib = hip.load()
    prev = lib.sdv_gemm_set_grid_limit(0)
    try:
        for _, t, kw, ntiles in [r for r in walk_rows() if r[1] == TILE and r[3] == 5]:
            case = make_case(**kw)
            assert -(-case.rows_out // TILES[t][0]) * -(-case.N // TILES[t][1]) == 5
            lib.sdv_gemm_set_grid_limit(0)
            base, _, _ = run_case(hip, dev, case, TILE)
            lib.sdv_gemm_set_grid_limit(2)                      # two workgroups walk the five tiles
            win, _, _ = run_case(hip, dev, case, TILE)
            assert torch.equal(win, base), kw
    finally:
        lib.sdv_gemm_set_grid_limit(prev)


def test_bits_do_not_depend_on_repeats_or_on_m(hip, dev):
    """the same launch twice, and rows 0 .. 32 of an M = 33 call against the same rows of an M = 545 call (three M tiles): the
    benchmark's forced-tile parity check compares batch sizes bit for bit"""
    case = make_case(mode=0, geom=(545,), C1=192, C2=0, N=320, res=True)
    x, w, b, r = (t.to(dev) for t in (case.x.to(BF16), case.w.to(BF16), case.bvec, case.r.to(BF16)))
    big = hip.linear(x, w, b, residual=r, tile=TILE)
    big2 = hip.linear(x, w, b, residual=r, tile=TILE)
    small = hip.linear(x[:33], w, b, residual=r[:33], tile=TILE)
    torch.cuda.synchronize()
    check_against_float64(big.cpu().double(), True, case)
    assert torch.equal(big.view(torch.int16), big2.view(torch.int16))
    assert torch.equal(small.view(torch.int16), big[:33].view(torch.int16))
