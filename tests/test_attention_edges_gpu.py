"""Float64 edge-case gate of every sdv_attention_bf16 kernel variant, and of the two row-softmax kernels.

The launcher picks a code path from (dh, Lq, Lk, causal, V form) alone: the software-pipelined two-query-tile kernel (PP), the
resident K / V^T form of the text cross-attention (RES), the generic one-query-tile kernel with its two softmax bodies, each with
V transposed or row-major, in head-major or query-major grid order.  Every case here compares EVERY output element with a float64
softmax(QK^T scale)V of the same bf16 inputs under the bound test_kernels_gpu.py::test_attention_elementwise_bound uses -
|out - ref| <= 0.5 ulp_bf16 (1 + 1e-3) + 2^-6 sum_k p_k |v_k| - at the smallest shapes that reach the ragged ends of each path:
query counts that leave a partly filled last query block (and whole waves past Lq), one key in the last key tile, B * H = 9 (a
second group of 8 grid slots with 7 of them empty), a resident workgroup that walks fewer than 8 query blocks.

The inputs make an error at an edge LARGE: sentinel keys (key j = 8 x query i, so that j owns row i's softmax if - and only if -
it is seen), a V whose channel t is 1.0 on the keys of tile t, peaked logits (the rescale branch runs in most tiles) and a
common-mode shift of every logit of a row by ~ +-100 log2 units.  Memory the kernels may read but must not use (the rows behind a
sample's last key) is NaN, the output is NaN before the launch and has NaN guard rows behind it.

test_checker_rejects_planted_edge_errors runs without a GPU: it feeds the checker a CPU stand-in of the kernels' arithmetic and
then the same with an edge error planted, and wants the first accepted and each of the others refused."""
import functools
from types import SimpleNamespace

import pytest
import torch

from conftest import bf16_round, report
from helpers import _attn_ref64, _half_ulp_ratio
from stable_diffusion_videos_amd import hip as sdv_hip

gpu = pytest.mark.gpu          # (not a module-wide pytestmark: the checker's own test below runs in the CPU tier)

BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
PAD = 8        # unused leading columns of every row-major buffer: head h starts 16 + 2 h dh bytes into a row, never on a 128-byte line
GUARD = 64     # NaN rows behind the last sample: what a ragged last key tile reaches behind the last sample's last key


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return bf16_round(torch.randn(shape, generator=g) * scale)


def _bits(t):
    return t.view(torch.int16)


# ------------------------------------------------------------------------------------------------
# inputs, the float64 reference (made once per case) and the checker
# ------------------------------------------------------------------------------------------------
KINDS = ("plain", "peaked", "tilev", "sentinel")                 # every non-causal family
CAUSAL_KINDS = ("plain", "peaked", "tilev", "diag", "next")      # "diag": key i owns row i; "next": key i + 1 would, if row i saw it
CAUSAL_ROWS = (0, 31, 32, 63, 64, -2)


def sentinel_pairs(Lq, Lk):
    """(query, key) pairs of the non-causal sentinel inputs: the last valid key and the first key of the last (ragged) key tile,
    for the first, a middle and the last valid query row.  (sample, head) number n takes pair n of the cycle."""
    rows = sorted({0, Lq // 2, Lq - 1})
    keys = sorted({Lk - 1, 64 * ((Lk - 1) // 64)}, reverse=True)
    return [(rows[n % len(rows)], keys[n % len(keys)]) for n in range(len(rows) * len(keys))]


@functools.lru_cache(maxsize=4)
def make_case(dh, B, H, Lq, Lk, kind, causal=False):
    """bf16-exact q (PRE-SCALED by scale * log2(e), as the projection GEMMs hand it over), k, v as fp32 [B, L, H * dh] on the CPU, and
    the float64 reference of the q these values stand for."""
    assert kind in KINDS + CAUSAL_KINDS + ("common",) and (not causal or Lq == Lk)
    Cc = H * dh
    pre = sdv_hip.q_prescale(dh)
    seed = 7919 * dh + 31 * Lq + 17 * Lk + 5 * B + len(kind) + (3 if causal else 0)
    q = _rnd((B, Lq, Cc), seed, (5.0 if kind == "peaked" else 1.0) * pre)      # peaked: logits with the spread of a trained model
    k = _rnd((B, Lk, Cc), seed + 1)
    v = _rnd((B, Lk, Cc), seed + 2, 0.25 if kind == "tilev" else 1.0)
    heads = [slice(h * dh, (h + 1) * dh) for h in range(H)]
    if kind == "tilev":            # channel t (mod dh) of V is 1.0 on the keys of tile t: a dropped or doubled key tile moves that channel
        keys = torch.arange(Lk)
        for sl in heads:
            v[:, keys, sl.start + (keys // 64) % dh] = 1.0
    if kind == "common":           # channel 0: q' = +-1, k + 100 -> every logit of a row moves by ~ +-100 log2 units; softmax must not care
        sign = (1 - 2 * (torch.arange(Lq) % 2)).float()
        for sl in heads:
            q[:, :, sl.start] = sign
            k[:, :, sl.start] = bf16_round(k[:, :, sl.start] + 100.0)
    q_true = q.double() / pre
    if kind == "sentinel":
        pairs = sentinel_pairs(Lq, Lk)
        for b in range(B):
            for h, sl in enumerate(heads):
                i, j = pairs[(b * H + h) % len(pairs)]
                k[b, j, sl] = bf16_round((8.0 * q_true[b, i, sl]).float())
    if kind in ("diag", "next"):
        step = 1 if kind == "next" else 0
        for i in sorted({r % Lq for r in CAUSAL_ROWS if -Lq <= r < Lq}):
            if i + step < Lk:
                k[:, i + step] = bf16_round((8.0 * q_true[:, i]).float())
    ref, mag = _attn_ref64(q_true, k.double(), v.double(), H, dh ** -0.5, causal)
    return SimpleNamespace(dh=dh, B=B, H=H, Lq=Lq, Lk=Lk, Cc=Cc, kind=kind, causal=causal, q=q, k=k, v=v, ref=ref, mag=mag)


def check_against_float64(out64, case, label=None):
    """THE check of this file: every element finite and within half a bf16 ulp + 2^-6 sum_k p_k |v_k| of the float64 reference.
    Returns the worst ratio to that bound (and reports it first, when given a label)."""
    assert out64.shape == case.ref.shape
    finite = bool(torch.isfinite(out64).all())
    ratio = _half_ulp_ratio(out64, case.ref, case.mag, acc_eps=2.0 ** -6)
    worst = float(ratio.max()) if finite else float("inf")
    if label is not None:
        report(f"{label}: worst element at {worst:.3f} of (half ulp + 2^-6 sum p|v|)")
    assert finite, "non-finite output element"
    assert worst <= 1.0, f"element {tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])} at {worst:.3f} of the bound"
    if case.causal:                # token 0 sees only itself; one key in all: P = 1, l = 1 - the output is v[0] to the bit
        assert torch.equal(out64[:, 0], case.v[:, 0].double()), "causal row 0 must be exactly v[0]"
    if case.Lk == 1:
        assert torch.equal(out64, case.v[:, :1].double().expand_as(out64)), "one key: the output is exactly v[0]"
    return worst


class Buffers:
    """The device tensors of one (case, V form) as the engines lay them out.  form "vt": V transposed [B][H dh][ldv] (the text
    cross-attention), "rm": V row-major beside K.  Non-causal: Q alone, [K] or [K | V]; causal (Lq = Lk): fused [Q | K] or [Q | K | V].
    Row-major buffers have PAD unused leading columns and GUARD rows behind the last sample, all NaN; V^T has zeros in its padding
    columns up to roundup(Lk, 64) (the documented contract) and 8 NaN columns behind them that no key tile reaches."""

    def __init__(self, case, form, dev):
        c = self.case = case
        self.rm = form == "rm"

        def rows(parts, L):
            t = torch.full((c.B * L + GUARD, PAD + sum(p.shape[-1] for p in parts)), NAN)
            t[:c.B * L, PAD:] = torch.cat(parts, -1).reshape(c.B * L, -1)
            return t.to(BF16).to(dev)
        kparts = [c.k, c.v] if self.rm else [c.k]
        if c.causal:
            self.qbuf = self.kbuf = rows([c.q] + kparts, c.Lq)
            self.q_off, self.k_off = PAD, PAD + c.Cc
        else:
            self.qbuf, self.kbuf = rows([c.q], c.Lq), rows(kparts, c.Lk)
            self.q_off = self.k_off = PAD
        self.ldq, self.ldk = self.qbuf.shape[1], self.kbuf.shape[1]
        if self.rm:
            self.vbuf, self.v_off, self.ldv = self.kbuf, self.k_off + c.Cc, self.ldk
        else:
            lk64 = (c.Lk + 63) // 64 * 64
            vt = torch.zeros((c.B, c.Cc, lk64 + 8))
            vt[:, :, lk64:] = NAN
            vt[:, :, :c.Lk] = c.v.transpose(1, 2)
            self.vbuf, self.v_off, self.ldv = vt.to(BF16).to(dev), 0, lk64 + 8
        self.inputs = [(t, _bits(t).clone()) for t in {id(t): t for t in (self.qbuf, self.kbuf, self.vbuf)}.values()]

    def run(self, hip, b0=0, nB=None, h0=0, nH=None):
        """Launch on samples [b0, b0 + nB) and heads [h0, h0 + nH) of the case (default: all) with the same buffers and leading
        dimensions; returns the written window as bf16 [nB * Lq, nH * dh] on the CPU after checking that nothing else was written."""
        c = self.case
        nB, nH = c.B if nB is None else nB, c.H if nH is None else nH
        q_off = self.q_off + b0 * c.Lq * self.ldq + h0 * c.dh
        k_off = self.k_off + b0 * c.Lk * self.ldk + h0 * c.dh
        if self.rm:
            v_off = self.v_off + b0 * c.Lk * self.ldv + h0 * c.dh
        else:
            assert nH == c.H or nB == 1          # (V^T: a sample's heads follow each other, the samples H * dh rows apart)
            v_off = (b0 * c.H + h0) * c.dh * self.ldv
        obuf = torch.full((nB * c.Lq + GUARD, PAD + c.Cc), NAN, dtype=BF16, device=self.qbuf.device)
        c0 = PAD + h0 * c.dh
        hip.attention(self.qbuf, self.kbuf, self.vbuf, obuf[:, c0:], B=nB, H=nH, Lq=c.Lq, Lk=c.Lk, dh=c.dh, ldq=self.ldq, ldk=self.ldk,
                      ldv=self.ldv, ldo=PAD + c.Cc, scale=c.dh ** -0.5, q_off=q_off, k_off=k_off, v_off=v_off, causal=c.causal,
                      q_prescaled=True, v_rowmajor=self.rm)
        torch.cuda.synchronize()
        o = obuf.cpu()
        win = o[:nB * c.Lq, c0:c0 + nH * c.dh].clone()
        o[:nB * c.Lq, c0:c0 + nH * c.dh] = NAN
        assert bool(o.isnan().all()), "the kernel wrote outside its output window (guard rows / other columns)"
        return win

    def assert_inputs_unchanged(self):
        for t, before in self.inputs:
            assert torch.equal(_bits(t), before), "an input buffer (V^T padding, NaN guard rows included) changed"


def same_kernel_for_both_v_forms(c):
    """Where the row-major and the transposed V run the same kernel - and so give the same bits (test_kernels_gpu.py::test_attention)"""
    return c.Lk > 128 or c.dh == 160 or c.causal


def run_case(hip, dev, family, forms, dh, B, H, Lq, Lk, kind, causal=False):
    case = make_case(dh, B, H, Lq, Lk, kind, causal)
    outs = {}
    for form in forms:
        buf = Buffers(case, form, dev)
        outs[form] = buf.run(hip)
        buf.assert_inputs_unchanged()
        check_against_float64(outs[form].double().view(B, Lq, case.Cc), case,
                              label=f"attention-edges {family} dh={dh} B={B} H={H} Lq={Lq} Lk={Lk} causal={causal} {kind} V={form}")
    if len(outs) == 2 and same_kernel_for_both_v_forms(case):
        assert torch.equal(_bits(outs["rm"]), _bits(outs["vt"])), "row-major V and transposed V must give the same bits"


BOTH = ("vt", "rm")

# 1. PP: dh 40, not causal, Lk % 64 == 0, Lq >= 1024 - two query tiles per wave, 256 queries per workgroup
PP_CASES = [(B, H, Lq, Lk, kind) for B, H, Lq, Lk in [(3, 3, 1100, 192),     # last 256-query block: 76 rows - whole second tiles and waves past Lq
                                                       (3, 3, 1024, 64),      # one key tile: prologue and epilogue of the pipeline only
                                                       (3, 3, 1100, 640),
                                                       (3, 3, 1300, 128),     # V^T form: query-major grid order
                                                       (1, 8, 1100, 192)] for kind in KINDS] + [(3, 3, 1100, 192, "common")]


@gpu
@pytest.mark.parametrize("B,H,Lq,Lk,kind", PP_CASES)
def test_pipelined_two_tile_kernel(hip, dev, B, H, Lq, Lk, kind):
    run_case(hip, dev, "PP", BOTH, 40, B, H, Lq, Lk, kind)


# 2. RES: V^T form, not causal, Lk <= 128, dh <= 80 - eight query blocks walked per workgroup over resident key tiles
RES_SHAPES = [(1157, 77),      # 10 query blocks: two workgroups, the second walks 2 blocks, the last block has 5 rows
              (1157, 65),      # one key in the second tile
              (900, 64), (900, 128),          # (Lq 900: dh 40 stays off PP)
              (130, 127), (1, 1)]
RES_CASES = [(dh, Lq, Lk, kind) for dh in (40, 64, 80) for Lq, Lk in RES_SHAPES for kind in KINDS] + [(dh, 1157, 77, "common") for dh in (40, 64, 80)]


@gpu
@pytest.mark.parametrize("dh,Lq,Lk,kind", RES_CASES)
def test_resident_cross_attention_kernel(hip, dev, dh, Lq, Lk, kind):
    run_case(hip, dev, "RES", ("vt",), dh, 3, 3, Lq, Lk, kind)


# 3. generic, not causal: one query tile per wave; PADM / ONES softmax at dh 40 / 80, the plain one at dh 64 / 160
GEN_CASES = [(dh, BOTH, Lq, Lk, kind) for dh in (40, 64, 80, 160) for Lq, Lk in [(200, 200), (130, 129), (70, 320), (1, 192), (144, 144)] for kind in KINDS]
GEN_CASES += [(dh, BOTH if dh == 160 else ("rm",), 200, 77, kind) for dh in (40, 64, 80, 160) for kind in KINDS]   # rm: zeros past num_records
GEN_CASES += [(160, ("vt",), 200, 64, kind) for kind in KINDS]       # dh 160, V^T, Lk <= 128: query-major order WITHOUT the resident form
GEN_CASES += [(dh, BOTH, 200, 200, "common") for dh in (40, 64, 80, 160)]


@gpu
@pytest.mark.parametrize("dh,forms,Lq,Lk,kind", GEN_CASES)
def test_generic_kernel(hip, dev, dh, forms, Lq, Lk, kind):
    run_case(hip, dev, "generic", forms, dh, 3, 3, Lq, Lk, kind)


# 4. causal: V^T with a fused [Q | K] buffer, row-major V in a fused [Q | K | V] buffer
CAUSAL_CASES = [(dh, L, kind) for dh in (40, 64, 80, 160) for L in (65, 77, 130, 257) for kind in CAUSAL_KINDS]
CAUSAL_CASES += [(40, 1040, kind) for kind in CAUSAL_KINDS]          # Lq >= 1024 and Lk % 64 == 0 need not causal to reach PP
CAUSAL_CASES += [(dh, 130, "common") for dh in (40, 64, 80, 160)]


@gpu
@pytest.mark.parametrize("dh,L,kind", CAUSAL_CASES)
def test_causal_kernel(hip, dev, dh, L, kind):
    run_case(hip, dev, "causal", BOTH, dh, 3, 3, L, L, kind, causal=True)


# ------------------------------------------------------------------------------------------------
# bit-level contracts: the dispatch depends on (dh, Lq, Lk, causal, V form) only
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("family,forms,dh,Lq,Lk,causal", [("PP", BOTH, 40, 1100, 192, False), ("RES", ("vt",), 80, 1157, 77, False),
                                                          ("generic", BOTH, 64, 130, 129, False), ("generic", BOTH, 160, 200, 77, False),
                                                          ("causal", BOTH, 40, 77, 77, True)])
def test_batch_head_invariance_and_determinism(hip, dev, family, forms, dh, Lq, Lk, causal):
    """A sample's rows do not depend on the samples beside it, a head's columns not on the heads beside it (one call on the middle
    head alone: H = 1, pointers moved to its columns, the same leading dimensions), and a repeated launch gives the same bits."""
    B, H = 3, 3
    case = make_case(dh, B, H, Lq, Lk, "peaked", causal)
    for form in forms:
        buf = Buffers(case, form, dev)
        full = buf.run(hip)
        check_against_float64(full.double().view(B, Lq, case.Cc), case)
        assert torch.equal(_bits(buf.run(hip)), _bits(full)), f"{family} V={form}: a repeated launch changed bits"
        for b in range(B):
            assert torch.equal(_bits(buf.run(hip, b0=b, nB=1)), _bits(full[b * Lq:(b + 1) * Lq])), f"{family} V={form}: sample {b} alone differs"
        alone = buf.run(hip, b0=1, nB=1, h0=1, nH=1)
        assert torch.equal(_bits(alone), _bits(full[Lq:2 * Lq, dh:2 * dh])), f"{family} V={form}: the middle head alone differs"
        buf.assert_inputs_unchanged()


# ------------------------------------------------------------------------------------------------
# the gate must bite (CPU tier)
# ------------------------------------------------------------------------------------------------
def emulate_kernel(case, weight):
    """CPU stand-in for a kernel's OUTPUT (never a reference): P = exp2(s - row max) rounded to bf16, the row sum taken over the
    rounded P, one rounding of the output.  ``weight`` [Lq, Lk]: how often query i's sums take key j - 1 where the mask lets it see
    the key, 0 where not; the planted errors below change it."""
    out = torch.empty((case.B, case.Lq, case.Cc), dtype=torch.float64)
    for b in range(case.B):
        for h in range(case.H):
            sl = slice(h * case.dh, (h + 1) * case.dh)
            s = case.q[b, :, sl].double() @ case.k[b, :, sl].double().T            # log2 units: Q is pre-scaled
            s = s.masked_fill(weight == 0, float("-inf"))
            p = bf16_round(torch.exp2(s - s.max(-1, keepdim=True).values).float()).double() * weight
            out[b, :, sl] = bf16_round(((p @ case.v[b, :, sl].double()) / p.sum(-1, keepdim=True)).float()).double()
    return out


def test_checker_rejects_planted_edge_errors():
    """The checker accepts the stand-in on every input kind and refuses it with each edge error planted, on the input kind that
    was made to show that error."""
    def weight(c, shift=0):
        w = torch.ones((c.Lq, c.Lk), dtype=torch.float64)
        return w.tril(shift) if c.causal else w

    ragged = [make_case(40, 1, 2, 130, 77, kind) for kind in KINDS + ("common",)]        # last query block: 2 rows; last key tile: 13 keys
    tiles = [make_case(64, 1, 2, 70, 200, kind) for kind in KINDS]                       # four key tiles, the last with 8 keys
    causal = [make_case(dh, 1, 2, 77, 77, kind, True) for dh in (40, 64) for kind in CAUSAL_KINDS + ("common",)]
    worst = max(check_against_float64(emulate_kernel(c, weight(c)), c) for c in ragged + tiles + causal)
    assert worst <= 0.5               # (the stand-in sits well inside the bound: 0.26 of it here, 0.33 at most on the GPU cases' inputs)
    by_kind = lambda cases, kind: [c for c in cases if c.kind == kind]

    def refused(c, out):
        with pytest.raises(AssertionError):
            check_against_float64(out, c)

    for c in by_kind(ragged, "sentinel") + by_kind(tiles, "sentinel"):       # the last valid key dropped
        w = weight(c)
        w[:, c.Lk - 1] = 0
        refused(c, emulate_kernel(c, w))
    for c in by_kind(causal, "next"):                                        # the causal mask shifted by +1: row i sees key i + 1
        refused(c, emulate_kernel(c, weight(c, +1)))
    for c in by_kind(causal, "diag"):                                        # ... by -1: row i does not see key i
        w = weight(c, -1)
        w[0, 0] = 1                                                          # (row 0 keeps its key: the error left is the mask's alone)
        refused(c, emulate_kernel(c, w))
    for c in by_kind(ragged, "tilev") + by_kind(tiles, "tilev") + by_kind(causal, "tilev"):
        for factor in (0, 2):                                                # one whole key tile dropped / doubled
            tile = 1 if c.Lk > 128 else 0
            w = weight(c)
            w[:, 64 * tile:64 * (tile + 1)] *= factor
            if c.causal:
                w[:64] = weight(c)[:64]                                      # (the rows whose every key is in that tile keep it)
            refused(c, emulate_kernel(c, w))
    for c in ragged:                                                         # the last, partly filled query block computed with the
        out = emulate_kernel(c, weight(c))                                   # previous block's rows
        n = c.Lq % 128
        out[:, c.Lq - n:] = out[:, c.Lq - n - 128:c.Lq - 128]
        refused(c, out)


# ------------------------------------------------------------------------------------------------
# row softmax kernels: 256 threads x 8 columns per pass - 2048 columns is one pass, 2056 a second one with a single active thread
# ------------------------------------------------------------------------------------------------
SOFTMAX_COLS = [8, 2048, 2056, 4096]
ROWS = 5


def _scores(cols, seed):
    """fp32 scores with the spread of the VAE mid-block's, row 3 with a single value ~80 above the rest (the others' probabilities
    underflow towards 0, nothing may become NaN)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    s = torch.randn((ROWS, cols), generator=g) * 3.0
    s[3, (cols * 5) // 7] += 80.0
    return s


def _softmax_ratio(p64, ref):
    """|p - ref| relative to half a bf16 ulp of ref + 1e-6 ref (the fast exponential): test_softmax_rows_f32_and_fp32_scores' bound"""
    ulp = torch.exp2(torch.floor(torch.log2(ref.clamp_min(1e-30))) - 7)
    return float(((p64 - ref).abs() / (0.5 * ulp + 1e-6 * ref)).max())


@gpu
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows_f32_every_element(hip, dev, cols):
    lds, ldp = cols + 4, cols + 8
    s = torch.full((ROWS, lds), NAN)
    s[:, :cols] = _scores(cols, 90 + cols)
    p = torch.full((ROWS, ldp), 7.0, dtype=BF16, device=dev)
    hip.softmax_rows_f32(s.to(dev), p, ROWS, cols, lds, ldp)
    torch.cuda.synchronize()
    p = p.cpu()
    assert bool((p[:, cols:] == 7.0).all()), "the padding columns of P lost their prefill"
    assert bool(torch.isfinite(p).all())
    ratio = _softmax_ratio(p[:, :cols].double(), torch.softmax(s[:, :cols].double(), -1))
    report(f"softmax_rows_f32 cols={cols}: worst element at {ratio:.3f} of (half ulp + 1e-6 p)")
    assert ratio <= 1.05


@gpu
@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_rows_bf16_every_element(hip, dev, cols):
    """In place over bf16 scores: the float64 softmax of the bf16 inputs, rounded once - the same bound as the fp32 form (the
    arithmetic between load and store is the same: fp32 fast exponential, fp32 sums, one rounding)."""
    ld = cols + 8
    s = torch.full((ROWS, ld), 7.0)
    s[:, :cols] = bf16_round(_scores(cols, 190 + cols))
    sb = s.to(BF16).to(dev)
    hip.softmax_rows_(sb, ROWS, cols, ld)
    torch.cuda.synchronize()
    sb = sb.cpu()
    assert bool((sb[:, cols:] == 7.0).all()), "the padding columns were written"
    assert bool(torch.isfinite(sb).all())
    ratio = _softmax_ratio(sb[:, :cols].double(), torch.softmax(s[:, :cols].double(), -1))
    report(f"softmax_rows_bf16 cols={cols}: worst element at {ratio:.3f} of (half ulp + 1e-6 p)")
    assert ratio <= 1.05
