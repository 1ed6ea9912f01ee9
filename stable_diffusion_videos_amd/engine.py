"""MI355X-native executors for the two networks on the walk hot path.

``UNetEngine.forward``      replaces ``self.unet(x, t, encoder_hidden_states=ctx).sample``
                            (/root/reference/stable_diffusion_videos/stable_diffusion_pipeline.py:418)
``VAEDecoderEngine.decode`` replaces ``self.vae.decode(latents).sample`` + the image epilogue
                            (stable_diffusion_pipeline.py:432-438, numpy_to_pil :450)

Both are built from the same few objects: ``_Res`` (one body for the bf16 and the fp8 ResBlock), ``_Transformer``, ``_ConvIn``,
``_Down`` / ``_Up``, grouped per resolution into ``_Level``; tests/launch_trace.py pins what each of them launches.

Everything is NHWC / token-major bf16 in HBM ([N*H*W, C] row-major), so the UNet's conv <-> transformer
boundaries need no permutes.  Each method only enqueues HIP kernels - through the wrappers of ``hip``, each of which
dispatches one ``torch.ops.sdv.k_*`` custom op onto the C ABI of libsdv_hip.so - on the current stream: a whole denoise
step is therefore capturable in one hipGraph.

What is hoisted out of the 50-step loop (the reference recomputes all of it every step):
  * the timestep-embedding MLP and the 22 ``time_emb_proj`` projections: the walk uses the same timestep
    for every sample, so they collapse to a [steps, Cout] bias table per ResBlock, folded into conv1's bias
    and indexed on-device by a step counter (graph replay needs no new arguments);
  * the cross-attention K / V projections of the text context (constant over all steps).
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import hip
from .config import UNetConfig, VAEConfig
from .weights import StateDict, conv_w, conv_w_c4, ffn_fold_columns, ffn_w2_permute, geglu_interleave, lin_w, ln_fold, upconv_phase_w, vec

BF16 = torch.bfloat16
F32 = torch.float32

# Optional block observer used by the block-wise parity tests (tests/test_blockwise_gpu.py): called as
# TAP(diffusers_module_name, dict(kind=..., x=..., [x2=...], out=..., nimg=, H=, W=)) after every block of a forward /
# decode with the block's actual HBM inputs and output, so that the oracle's module of the same name can be run on exactly
# what the engine's block saw ("teacher forcing").  None = no overhead; never set inside a graph capture.
TAP = None


def _tap(name: str, kind: str, **kw):
    if TAP is not None:
        TAP(name, dict(kind=kind, **kw))


# tools/contention_probe.py: tensors BETWEEN the kernels of a block (LayerNorm row statistics, the GEGLU hidden rows) that no block
# boundary shows - callback (name, tensor), None = no overhead
TAP_AUX = None


def _aux(name: str, what: str, t):
    if TAP_AUX is not None and t is not None:
        TAP_AUX(f"{name}:{what}", t)


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _quant_w(w_bf16: torch.Tensor):
    """bf16 weight matrix -> (e4m3 bytes, per-tensor scale): w ~ q * scale, scale = amax / 448."""
    wf = w_bf16.float()
    scale = max(float(wf.abs().max()), 1e-12) / hip.FP8_MAX       # (an all-zero matrix must not give scale 0 -> NaN weights)
    assert scale > 0 and scale < float("inf"), "fp8 weight scale must be finite"
    return (wf / scale).to(hip.FP8).contiguous(), scale


def _act_scale(y_bf16: torch.Tensor, prev) -> float:
    """Per-tensor e4m3 scale of an activation from one calibration sample: 2 x amax / 448 (e4m3 is floating point, the factor
    2 of head-room costs no precision), running maximum over the calibration forwards, floored so that an all-zero sample
    (a zero-filled warm-up buffer) cannot produce scale 0 (division by zero in the GroupNorm apply)."""
    s = 2.0 * max(float(y_bf16.float().abs().max()), 1e-6) / hip.FP8_MAX
    return s if prev is None else max(s, prev)


# ------------------------------------------------------------------------------------------------
# shared blocks
# ------------------------------------------------------------------------------------------------
class _Res:
    """ResnetBlock2D: GN+SiLU -> conv3x3 (+temb bias) -> GN+SiLU -> conv3x3 (+ shortcut/residual)."""

    def __init__(self, sd: StateDict, p: str, device, groups: int, eps: float, has_temb: bool, fp8: bool = False):
        self.name = p
        self.g1, self.b1 = vec(sd[p + ".norm1.weight"], device), vec(sd[p + ".norm1.bias"], device)
        self.w1 = conv_w(sd[p + ".conv1.weight"], device)
        self.c1_bias = vec(sd[p + ".conv1.bias"], device)
        self.g2, self.b2 = vec(sd[p + ".norm2.weight"], device), vec(sd[p + ".norm2.bias"], device)
        self.w2 = conv_w(sd[p + ".conv2.weight"], device)
        self.c2_bias = vec(sd[p + ".conv2.bias"], device)
        self.cout = self.w1.shape[0]
        self.groups, self.eps = groups, eps
        if has_temb:
            self.wt = lin_w(sd[p + ".time_emb_proj.weight"], device)
            self.bt = vec(sd[p + ".time_emb_proj.bias"], device)
        else:
            self.wt = None
        if p + ".conv_shortcut.weight" in sd:
            self.ws = lin_w(sd[p + ".conv_shortcut.weight"], device)
            self.bs = vec(sd[p + ".conv_shortcut.bias"], device)
        else:
            self.ws = None
        self.bias_table: Optional[torch.Tensor] = None  # [steps, Cout] = conv1.bias + time_emb_proj(silu(emb_t))
        # fp8 mode (BASELINE config 5): both 3x3 convs take OCP e4m3 activations (written by the GroupNorm+SiLU apply pass,
        # half the bytes) and e4m3 weights; per-tensor scales, fp32 accumulation, bf16 out.  Weight scale = amax / 448; the
        # activation scales are calibrated on the first forward (2 x amax / 448: e4m3 is floating point, head-room is free).
        self.fp8 = fp8
        if fp8:
            (w1_8, sw1), (w2_8, sw2) = _quant_w(self.w1), _quant_w(self.w2)
            self.w8, self.sw = (w1_8, w2_8), (sw1, sw2)
            self.sx: List[Optional[float]] = [None, None]     # e4m3 scales of the activations conv1 / conv2 read
            self.calibrating = False           # UNetEngine.fp8_calibration(): widen the scales on every forward (eager only)

    def prepare_timesteps(self, emb: torch.Tensor):
        self.bias_table = hip.linear_small(emb, self.wt, self.bt, add=self.c1_bias, silu_in=True)

    def _gn_silu(self, i: int, x, x2, gamma, beta, gn):
        """GroupNorm + SiLU of x (++ x2) in the operand format of the conv behind it, conv1 (i = 0) or conv2 (1) -> (the
        activation, that conv's alpha)."""
        if not self.fp8:
            return hip.groupnorm(x, gamma, beta, x2=x2, **gn), 1.0
        # Activation scales: set by an explicit calibration run (UNetEngine.fp8_calibration - the pipeline runs a fixed pilot
        # denoise BEFORE the graph warm-up, so the scales never come from a zero-filled capture buffer and are the same on every
        # rank / resume); a bare engine (tests, tools) calibrates lazily on its first eager forward.
        if self.sx[i] is None or self.calibrating:
            self.sx[i] = _act_scale(hip.groupnorm(x, gamma, beta, x2=x2, **gn), self.sx[i])
        return hip.groupnorm(x, gamma, beta, x2=x2, fp8_scale=self.sx[i], **gn), self.sx[i] * self.sw[i]

    def __call__(self, x, x2, nimg, H, W, step_ptr, circular, out=None):
        """``out``: where the block's result goes (a row range of a larger tensor when the caller walks the batch in
        cache-sized chunks of images, UNetEngine._segment)."""
        gn = dict(nimg=nimg, HW=H * W, groups=self.groups, eps=self.eps, silu=True)
        # (gn=True: the conv's epilogue also emits the per-channel statistics of what it stores, so norm2 - and, for conv2 below, the
        #  next block's GroupNorm - runs no statistics pass of its own; hip.groupnorm picks them up from the tensor.  An fp8 conv has
        #  no such epilogue: hip.gn_epilogue_ok refuses it)
        conv = dict(nimg=nimg, H=H, W=W, circular=circular, gn=True)
        w1, w2 = self.w8 if self.fp8 else (self.w1, self.w2)
        h, alpha = self._gn_silu(0, x, x2, self.g1, self.b1, gn)
        if self.wt is not None:
            h = hip.conv3x3(h, w1, self.bias_table, step_ptr=step_ptr, bias_step_stride=self.cout, alpha=alpha, **conv)
        else:
            h = hip.conv3x3(h, w1, self.c1_bias, alpha=alpha, **conv)
        h, alpha = self._gn_silu(1, h, None, self.g2, self.b2, gn)
        assert self.ws is not None or x2 is None
        sc = hip.linear(x, self.ws, self.bs, x2=x2) if self.ws is not None else x
        out = hip.conv3x3(h, w2, self.c2_bias, residual=sc, alpha=alpha, out=out, **conv)
        _tap(self.name, "resnet", x=x, x2=x2, out=out, nimg=nimg, H=H, W=W)
        return out


class _ConvIn:
    """conv_in of the UNet / the VAE decoder: from 4 channels on the matrix cores (im2col to one 64-wide K tile, whose epilogue emits
    the GroupNorm statistics), from any other small count on the direct kernel."""

    def __init__(self, sd: StateDict, p: str, device):
        self.name = p
        w = sd[p + ".weight"]
        self.c4 = w.shape[1] == 4
        self.w = conv_w_c4(w.cpu(), device) if self.c4 else conv_w(w, device)
        self.b = vec(sd[p + ".bias"], device)

    def __call__(self, x, nimg, H, W, circular):
        if self.c4:
            out = hip.conv3x3_c4(x, self.w, self.b, nimg=nimg, H=H, W=W, circular=circular, gn=True)
        else:
            out = hip.conv3x3_cin_small(x, self.w, self.b, nimg=nimg, H=H, W=W, circular=circular)
        _tap(self.name, "conv", x=x, out=out, nimg=nimg, H=H, W=W)
        return out


class _Down:
    """Downsample2D: conv3x3 stride 2.  Returns the rows and their new height and width."""

    def __init__(self, sd: StateDict, p: str, device):
        self.name = p
        self.w, self.b = conv_w(sd[p + ".conv.weight"], device), vec(sd[p + ".conv.bias"], device)

    def __call__(self, x, nimg, H, W, circular):
        out = hip.conv3x3(x, self.w, self.b, nimg=nimg, H=H, W=W, mode=2, circular=circular, gn=True)
        _tap(self.name, "down", x=x, out=out, nimg=nimg, H=H, W=W)
        return out, (H + 1) // 2, (W + 1) // 2


class _Up:
    """Upsample2D (nearest 2x + conv3x3) in phase form (weights.upconv_phase_w).  Returns the rows and their new height and width."""

    def __init__(self, sd: StateDict, p: str, device):
        self.name = p
        self.w, self.b = upconv_phase_w(sd[p + ".conv.weight"], device), vec(sd[p + ".conv.bias"], device)

    def __call__(self, x, nimg, H, W, circular):
        out = hip.upconv3x3_phase(x, self.w, self.b, nimg=nimg, H=H, W=W, circular=circular, gn=True)
        _tap(self.name, "up", x=x, out=out, nimg=nimg, H=H, W=W)
        return out, 2 * H, 2 * W


class _Level(NamedTuple):
    """One resolution level of a down or an up path."""
    res: List[_Res]
    attn: list                  # the _Transformer behind each ResBlock, or empty
    resample: Optional[object]  # the _Down / _Up that leaves the level; None at the last one

    def pairs(self):
        return zip(self.res, self.attn or [None] * len(self.res))


class _Proj:
    """One token projection of the transformer block,  y = alpha (LN?(x) W^T) + b (+ residual) (+ the row statistics of y),  with its
    weights in the operand format of each kernel that can run it: the igemm tiles (hip.linear) and, where the panel kernel has a form
    for its width (hip.linear320: C = 320, and C = 640 without a residual), that one.  Which of the two runs is decided here and
    nowhere else, so a caller cannot pair one kernel's weights with the other's fold terms."""

    def __init__(self, parts, bias, device, ln=None, panel_widths=()):
        """``parts``: [(weight [N_i, C], alpha_i)], stacked along N; alpha_i multiplies those output columns (the pre-scale of a Q
        projection; only the first may differ from 1).  ``ln``: (gamma, beta) of the LayerNorm that feeds the projection, folded into
        it (weights.ln_fold / sdv_hip.h ln_side): the GEMM that PRODUCES x also emits its row statistics, this one reads the
        un-normalised x.  ``panel_widths``: the C for which the panel kernel has a form of this projection."""
        assert ln is None or bias is None
        if ln is None:
            (w, self.alpha), = parts
            assert self.alpha == 1.0
            self.w, self.b, self.s = lin_w(w, device), vec(bias, device), None
            self.alpha_cols = 0
        else:
            folded = [ln_fold(w, *ln, None, device, scale=a) for w, a in parts]
            self.w = torch.cat([f[0] for f in folded], 0).contiguous()
            self.s = torch.cat([f[1] for f in folded]).contiguous()
            self.b = torch.cat([f[2] for f in folded]).contiguous()          # t of ln_fold, alpha_i already in it
            self.alpha = parts[0][1]
            self.alpha_cols = folded[0][0].shape[0] if len(parts) > 1 else 0      # (alpha on the leading columns only)
        self.N, C = self.w.shape
        # rows of the WHOLE call from which the panel form runs (None: igemm only).  Small calls: a persistent panel kernel with fewer
        # panels than CUs loses to the igemm's small tiles; C = 320 takes the panel at every size
        self.panel_from = None
        if C in panel_widths and hip.LINEAR320 and (C == 320 or hip.LINEAR640):
            self.panel_from = 0 if C == 320 else (hip.PANEL_MIN_ROWS_QKV640 if len(parts) == 3 else hip.PANEL_MIN_ROWS_LIN640)
            # panel operands: bias / LayerNorm fold in the fold k-step (wx), one alpha per block of 320 output columns.  The kernel
            # multiplies the whole bracket by alpha * rstd, so the fold columns carry t / alpha
            if ln is None:
                self.wx, self.al = ffn_fold_columns(torch.zeros(self.N, dtype=torch.float32, device=device), self.b), None
            else:
                self.wx = ffn_fold_columns(self.s, torch.cat([f[2] / a for f, (_, a) in zip(folded, parts)]))
                self.al = torch.tensor([a for w, a in parts for _ in range(w.shape[0] // 320)], dtype=torch.float32, device=device)
        # C = 320 fused Q / K / V: the panel kernel can store the V third TRANSPOSED per sample (``vt`` / ``hw`` of the call)
        self.vt_form = C == 320 and len(parts) == 3 and self.panel_from is not None and hip.QKV_VT

    def _panel(self, rows: int) -> bool:
        # (hip.FORCE_TILE - "run what the big batch runs" - takes the panel kernels at any size)
        return self.panel_from is not None and (rows >= self.panel_from or bool(hip.FORCE_TILE))

    def __call__(self, x, rows, ln_stats=None, residual=None, want_stats=False, out=None, stats_out=None, vt=None, hw=0, gn_hw=0):
        """``rows``: the rows of the whole call, which choose the kernel - so that the CFG-shared prefix (x holds half of them) takes
        the kernels the unshared forward takes.  ``ln_stats``: the producer's row statistics (a projection built with ``ln``)."""
        if self._panel(rows):
            return hip.linear320(x, self.w, self.wx, ln_stats=ln_stats, alpha=self.al, residual=residual, out=out,
                                 want_stats=want_stats, stats_out=stats_out, vt=vt, hw=hw)
        assert vt is None and stats_out is None
        return hip.linear(x, self.w, self.b, residual=residual, out=out, alpha=self.alpha, alpha_cols=self.alpha_cols,
                          ln=(ln_stats, self.s) if self.s is not None else None, want_stats=want_stats, gn_hw=gn_hw)

    def shared(self, x, rows, residual, want_stats=False, out=None, gn_hw=0):
        """The two CFG halves of x [rows, C] against ONE residual [rows / 2, N] - the stream they still share - read with batch
        stride 0; writes both halves."""
        assert self.s is None
        Mb, (N, K) = rows // 2, self.w.shape
        if out is None:
            out = torch.empty((rows, N), dtype=BF16, device=x.device)
        if self._panel(rows):       # (the same kernel, row for row, as the unshared forward runs: the shared prefix stays EXACT)
            st = torch.empty((rows, 2), dtype=torch.float32, device=x.device) if want_stats else None
            for half in (slice(0, Mb), slice(Mb, 2 * Mb)):
                self(x[half], rows, residual=residual, out=out[half], want_stats=want_stats, stats_out=st[half] if want_stats else None)
        else:
            st = hip.gemm(x, self.w, out, M=Mb, N=N, K=K, ldx=K, ldw=K, ldc=N, bias=self.b, residual=residual, ldr=N, batch=2,
                          sX=Mb * K, sW=0, sC=Mb * N, sR=0, want_stats=want_stats, gn_hw=gn_hw)
        return (out, st) if want_stats else out


class _FeedForward:
    """x + ff.net.2(GEGLU(ff.net.0(norm3(x)))), norm3 folded into ff.net.0: two igemm launches, or - C = 320 - ONE launch
    (sdv_ffn_geglu_bf16) in which the hidden activations never leave the registers and the LayerNorm fold's per-column terms ride in
    the matrix product (w1x)."""

    def __init__(self, sd: StateDict, p: str, name: str, ln, device):
        self.name = name
        self.w1, self.s1, self.b1 = ln_fold(geglu_interleave(sd[p + ".net.0.proj.weight"]), *ln,
                                            geglu_interleave(sd[p + ".net.0.proj.bias"]), device)
        self.w2, self.b2 = lin_w(sd[p + ".net.2.weight"], device), vec(sd[p + ".net.2.bias"], device)
        self.fused = hip.FFN_FUSED and self.w2.shape[0] == 320
        if self.fused:
            self.w1x = ffn_fold_columns(self.s1, self.b1)
            self.w2p = ffn_w2_permute(self.w2)

    def __call__(self, h, rows, ln_stats):
        """``rows``: the rows of the whole call (below hip.PANEL_MIN_ROWS_FFN the persistent fused kernel leaves most CUs idle)."""
        if self.fused and (rows >= hip.PANEL_MIN_ROWS_FFN or bool(hip.FORCE_TILE)):
            return hip.ffn_geglu(h, ln_stats, self.w1, self.w1x, self.w2p, self.b2)
        g = hip.linear(h, self.w1, self.b1, epi=1, ln=(ln_stats, self.s1))   # [M, 4C]
        _aux(self.name, "ff_hidden", g)
        return hip.linear(g, self.w2, self.b2, residual=h)


class _Transformer:
    """Transformer2DModel with one BasicTransformerBlock (self-attn, text cross-attn, GEGLU FF)."""

    def __init__(self, sd: StateDict, p: str, device, heads: int, groups: int):
        self.name = p
        self.gn_g, self.gn_b = vec(sd[p + ".norm.weight"], device), vec(sd[p + ".norm.bias"], device)
        b = p + ".transformer_blocks.0"
        self.C = sd[p + ".proj_in.weight"].shape[0]
        self.heads = heads
        self.dh = self.C // heads
        self.groups = groups
        qs = hip.q_prescale(self.dh)       # softmax scale * log2(e): the alpha of every Q projection (hip.attention, q_prescaled)
        ln1, ln2, ln3 = ((sd[f"{b}.norm{i}.weight"], sd[f"{b}.norm{i}.bias"]) for i in (1, 2, 3))
        free = (320, 640)                  # panel forms: every projection at C = 320, the residual-free ones at C = 640 too
        self.proj_in = _Proj([(sd[p + ".proj_in.weight"], 1.0)], sd[p + ".proj_in.bias"], device, panel_widths=free)
        # attn1.to_q / to_k / to_v as ONE projection [3C, C] = [Wq' ; Wk' ; Wv'] (norm1 folded into all three): the attention
        # kernel reads Q, K and V straight out of its [tokens, 3C] output - V row-major, transposed in the kernel's LDS read
        # (sdv_attention_bf16 v_rowmajor) - so the self-attention is 2 launches.  Rounds 2-4 ran a separate TRANSPOSED V^T
        # projection (column-side LayerNorm fold) per block; DESIGN.md tells what went wrong with it.
        self.qkv1 = _Proj([(sd[f"{b}.attn1.to_q.weight"], qs), (sd[f"{b}.attn1.to_k.weight"], 1.0), (sd[f"{b}.attn1.to_v.weight"], 1.0)],
                          None, device, ln=ln1, panel_widths=free)
        self.to_out1 = _Proj([(sd[f"{b}.attn1.to_out.0.weight"], 1.0)], sd[f"{b}.attn1.to_out.0.bias"], device, panel_widths=(320,))
        self.q2 = _Proj([(sd[f"{b}.attn2.to_q.weight"], qs)], None, device, ln=ln2, panel_widths=free)
        self.wk2 = lin_w(sd[f"{b}.attn2.to_k.weight"], device)
        self.wv2 = lin_w(sd[f"{b}.attn2.to_v.weight"], device)
        self.to_out2 = _Proj([(sd[f"{b}.attn2.to_out.0.weight"], 1.0)], sd[f"{b}.attn2.to_out.0.bias"], device, panel_widths=(320,))
        self.ff = _FeedForward(sd, b + ".ff", p, ln3, device)
        # (always the igemm: its epilogue emits the GroupNorm statistics of the block's output)
        self.proj_out = _Proj([(sd[p + ".proj_out.weight"], 1.0)], sd[p + ".proj_out.bias"], device)
        # per batch size: (K [N*Lc, C], V^T [N, C, ldv] zero padded, Lc) - persistent so captured graphs stay valid
        self.ctx: Dict[int, tuple] = {}            # the (K, V^T, Lc) the next forward of a given batch size uses
        self.ctx_by_len: Dict[tuple, tuple] = {}

    def prepare_context(self, ctx: torch.Tensor, nimg: int, Lc: int):
        """ctx: bf16 [nimg*Lc, D].  K = ctx Wk^T ; V^T[n] = Wv ctx[n]^T  (constant across denoise steps)."""
        C, D = self.C, ctx.shape[1]
        ldv = _round_up(Lc, 64)
        ent = self.ctx_by_len.get((nimg, Lc))
        if ent is None:
            # keyed by (nimg, Lc) and never freed: captured graphs hold raw pointers into these buffers, so a call with a
            # different context length must not reallocate the ones an older graph still reads
            ent = (torch.empty((nimg * Lc, C), dtype=BF16, device=ctx.device),
                   torch.zeros((nimg, C, ldv), dtype=BF16, device=ctx.device), Lc)
            self.ctx_by_len[(nimg, Lc)] = ent
        self.ctx[nimg] = ent
        hip.linear(ctx, self.wk2, out=ent[0])
        hip.gemm(self.wv2, ctx, ent[1], M=C, N=Lc, K=D, ldx=D, ldw=D, ldc=ldv, batch=nimg, sX=0, sW=Lc * D,
                 sC=C * ldv)

    def __call__(self, x, nimg, H, W, shared_prefix: bool = False, out=None, ctx_of=None):
        """``out`` / ``ctx_of=(batch size the context was prepared for, first image)``: this call handles images
        [first, first + nimg) of a larger batch and writes their rows of a larger tensor (UNetEngine._segment)."""
        out = self._forward(x, nimg, H, W, shared_prefix, out, ctx_of)
        _tap(self.name, "transformer", x=x, out=out, nimg=nimg // 2 if shared_prefix else nimg, H=H, W=W, shared_prefix=shared_prefix)
        return out

    def _context(self, nimg, ctx_of):
        if ctx_of is None:
            return self.ctx[nimg]
        total, first = ctx_of
        ctx_k, ctx_vt, Lc = self.ctx[total]
        return ctx_k[first * Lc:(first + nimg) * Lc], ctx_vt[first:first + nimg], Lc

    def _forward(self, x, nimg, H, W, shared_prefix: bool = False, out=None, ctx_of=None):
        """x: [nimg*HW, C] tokens.  With ``shared_prefix`` x holds only nimg/2 samples whose two CFG copies
        (unconditional / conditional) are still identical: everything up to the cross-attention - GroupNorm, proj_in,
        the whole self-attention, the cross-attention query - is computed ONCE, and the batch doubles where the
        text context first enters (returns nimg samples).

        The three LayerNorms live inside the projections they feed: each producer emits the (mean, rstd) of its rows (st1 .. st3)."""
        C, HW, heads, dh = self.C, H * W, self.heads, self.dh
        nb = nimg // 2 if shared_prefix else nimg          # samples in the context-free prefix
        Mb, M = nb * HW, nimg * HW                         # (every projection chooses its kernel by M, the rows of the WHOLE call)
        scale = dh ** -0.5
        h = hip.groupnorm(x, self.gn_g, self.gn_b, nimg=nb, HW=HW, groups=self.groups, eps=1e-6, silu=False)
        h, st1 = self.proj_in(h, M, want_stats=True)
        _tap(self.name, "tf_in", x=x, out=h, nimg=nb, H=H, W=W)
        h_in = h
        # --- self attention ---
        o = torch.empty((Mb, C), dtype=BF16, device=x.device)
        if self.qkv1.vt_form and HW % 128 == 0:
            # [Q * qs | K] row-major + V TRANSPOSED per sample, straight out of the projection's epilogue: the attention kernel's
            # one-read-per-fragment form (4 % faster than the transposing LDS reads of the row-major V at dh 40)
            vt = torch.empty((nb, C, HW), dtype=BF16, device=x.device)
            qk = self.qkv1(h, M, ln_stats=st1, vt=vt, hw=HW)
            hip.attention(qk, qk, vt, o, B=nb, H=heads, Lq=HW, Lk=HW, dh=dh, ldq=2 * C, ldk=2 * C, ldv=HW, ldo=C, scale=scale, k_off=C,
                          q_prescaled=True)
        else:
            qkv = self.qkv1(h, M, ln_stats=st1)              # [Mb, 3C] = [Q * qs | K | V]
            hip.attention(qkv, qkv, qkv, o, B=nb, H=heads, Lq=HW, Lk=HW, dh=dh, ldq=3 * C, ldk=3 * C, ldv=3 * C, ldo=C,
                          scale=scale, k_off=C, v_off=2 * C, q_prescaled=True, v_rowmajor=True)
        h, st2 = self.to_out1(o, M, residual=h, want_stats=True)
        _tap(self.name, "tf_attn1", x=h_in, out=h, nimg=nb, H=H, W=W)
        h_in = h
        # --- cross attention on the text context ---
        q = self.q2(h, M, ln_stats=st2)
        o2 = torch.empty((M, C), dtype=BF16, device=x.device)
        ctx_k, ctx_vt, Lc = self._context(nimg, ctx_of)
        if not shared_prefix:
            hip.attention(q, ctx_k, ctx_vt, o2, B=nimg, H=heads, Lq=HW, Lk=Lc, dh=dh, ldq=C, ldk=C, ldv=ctx_vt.shape[2],
                          ldo=C, scale=scale, q_prescaled=True)
            h, st3 = self.to_out2(o2, M, residual=h, want_stats=True)
        else:
            # same queries against the unconditional and the conditional context; the residual stream h is still
            # shared, so the output projection reads it with batch stride 0 and writes both halves
            for half in range(2):
                hip.attention(q, ctx_k[half * nb * Lc:], ctx_vt[half * nb:], o2[half * Mb:], B=nb, H=heads, Lq=HW, Lk=Lc,
                              dh=dh, ldq=C, ldk=C, ldv=ctx_vt.shape[2], ldo=C, scale=scale, q_prescaled=True)
            h, st3 = self.to_out2.shared(o2, M, residual=h, want_stats=True)
        _tap(self.name, "tf_attn2", x=h_in, out=h, nimg=nb, H=H, W=W, shared_prefix=shared_prefix)
        _aux(self.name, "st3", st3)
        h_in = h
        # --- GEGLU feed-forward ---
        h = self.ff(h, M, st3)
        _tap(self.name, "tf_ff", x=h_in, out=h, nimg=nimg, H=H, W=W)
        if not shared_prefix:
            out = self.proj_out(h, M, residual=x, out=out, gn_hw=HW)
        else:
            out = self.proj_out.shared(h, M, residual=x, out=out, gn_hw=HW)       # residual x is the shared (nb-sample) input
        _tap(self.name, "tf_out", x=h, x2=x, out=out, nimg=nimg, H=H, W=W, shared_prefix=shared_prefix)
        return out


# ------------------------------------------------------------------------------------------------
# UNet
# ------------------------------------------------------------------------------------------------
class UNetEngine:
    def __init__(self, cfg: UNetConfig, sd: StateDict, device, tiled: bool = False, fp8: bool = False):
        hip.load()
        self.cfg, self.device, self.tiled = cfg, torch.device(device), tiled
        self.fp8 = fp8                         # e4m3 operands in the ResBlock 3x3 convs (40 % of the UNet's FLOPs)
        self.config = cfg                      # ``pipe.unet.config.sample_size`` (reference :268)
        self.in_channels = cfg.in_channels     # ``pipe.unet.in_channels`` (reference :367)
        ch = cfg.block_out_channels
        g, eps = cfg.norm_num_groups, cfg.norm_eps
        dev = self.device
        self.conv_in = _ConvIn(sd, "conv_in", dev)
        self.t_w1, self.t_b1 = lin_w(sd["time_embedding.linear_1.weight"], dev), vec(sd["time_embedding.linear_1.bias"], dev)
        self.t_w2, self.t_b2 = lin_w(sd["time_embedding.linear_2.weight"], dev), vec(sd["time_embedding.linear_2.bias"], dev)
        self.res: List[_Res] = []
        self.tfm: List[_Transformer] = []

        def res(p):
            r = _Res(sd, p, dev, g, eps, True, fp8=fp8)
            self.res.append(r)
            return r

        def tfm(p, level):
            t = _Transformer(sd, p, dev, cfg.heads(level), g)
            self.tfm.append(t)
            return t

        last = len(ch) - 1
        self.down: List[_Level] = []
        for i, typ in enumerate(cfg.down_block_types):
            blk = _Level([], [], _Down(sd, f"down_blocks.{i}.downsamplers.0", dev) if i != last else None)
            for j in range(cfg.layers_per_block):
                blk.res.append(res(f"down_blocks.{i}.resnets.{j}"))
                if typ.startswith("CrossAttn"):
                    blk.attn.append(tfm(f"down_blocks.{i}.attentions.{j}", i))
            self.down.append(blk)
        self.mid = (res("mid_block.resnets.0"), tfm("mid_block.attentions.0", last), res("mid_block.resnets.1"))
        self.up: List[_Level] = []
        for i, typ in enumerate(cfg.up_block_types):
            blk = _Level([], [], _Up(sd, f"up_blocks.{i}.upsamplers.0", dev) if i != last else None)
            for j in range(cfg.layers_per_block + 1):
                blk.res.append(res(f"up_blocks.{i}.resnets.{j}"))
                if typ.startswith("CrossAttn"):
                    blk.attn.append(tfm(f"up_blocks.{i}.attentions.{j}", last - i))
            self.up.append(blk)
        self.out_g, self.out_b = vec(sd["conv_norm_out.weight"], dev), vec(sd["conv_norm_out.bias"], dev)
        self.conv_out_w = conv_w(sd["conv_out.weight"], dev)
        self.conv_out_b = vec(sd["conv_out.bias"], dev)
        self.groups, self.eps = g, eps
        self.num_steps = 0
        self.fp8_calibrated = False

    def fp8_calibration(self, on: bool, ok: bool = True, restore=None):
        """While on, every (eager) forward WIDENS the e4m3 activation scales of the ResBlock convs to cover what it sees
        (running maximum); turning it off freezes them and - when the run succeeded (``ok``) - marks the engine calibrated.
        ``ok=False`` (the calibration run raised): the scales go back to ``restore`` (``fp8_scales()`` taken before the run)
        and the engine stays uncalibrated.  Host synchronising - never inside a graph capture."""
        for r in self.res:
            if r.fp8:
                r.calibrating = bool(on)
        if not on:
            if ok:
                self.fp8_calibrated = True
            elif restore is not None:
                for r, scales in zip([r for r in self.res if r.fp8], restore):
                    r.sx = list(scales)

    def fp8_scales(self):
        return [tuple(r.sx) for r in self.res if r.fp8]

    def set_fp8_scales(self, scales):
        for r, (a, b) in zip([r for r in self.res if r.fp8], scales):
            r.sx = [float(a), float(b)]
        self.fp8_calibrated = True

    # -- per-walk preparation ----------------------------------------------------------------
    def prepare_timesteps(self, timesteps: Sequence[int]):
        """Build the per-ResBlock [steps, Cout] bias tables for this timestep schedule."""
        cfg = self.cfg
        ts = torch.tensor([float(t) for t in timesteps], dtype=F32, device=self.device)
        t_emb = hip.timestep_embedding(ts, cfg.block_out_channels[0], cfg.flip_sin_to_cos, float(cfg.freq_shift))
        e = hip.linear_small(t_emb, self.t_w1, self.t_b1)
        emb = hip.linear_small(e, self.t_w2, self.t_b2, silu_in=True)     # [steps, temb]
        for r in self.res:
            r.prepare_timesteps(emb)
        self.num_steps = len(timesteps)

    def prepare_context(self, ctx: torch.Tensor):
        """ctx: [nimg, Lc, D] (any float dtype) -> cache cross-attention K / V^T in every transformer block."""
        nimg, Lc, D = ctx.shape
        c = ctx.reshape(nimg * Lc, D)
        c = hip.f32_to_bf16(c.float()) if c.dtype != BF16 else c.contiguous()
        for t in self.tfm:
            t.prepare_context(c, nimg, Lc)

    def release(self, nimg: int):
        """Free the per-batch-size buffers (the cross-attention K / V^T of the text context) of ``nimg`` samples.  Only when no
        captured graph of that batch size is alive - they hold raw pointers into these buffers."""
        for t in self.tfm:
            for key in [k for k in t.ctx_by_len if k[0] == nimg]:
                del t.ctx_by_len[key]
            t.ctx.pop(nimg, None)

    def reserve(self, nimg: int, H: int, W: int):
        """(Rounds 1-4 allocated the self-attention's V^T workspaces here, outside of graph capture.  Since the fused QKV projection
        a forward has no persistent workspace of its own; kept as a no-op for callers that still announce their batch size.)"""

    # -- cache blocking ----------------------------------------------------------------------
    # At 128 frames (256 samples) every activation of the 64 x 64 level is 671 MB: each kernel of a ResBlock / transformer
    # block streams its input from HBM and its output back, ~37 passes per transformer block, and the K <= 640 GEMMs, the
    # GroupNorm passes and the residual adds are bound by exactly those bytes (DESIGN (d)).  Every op of a block is local to
    # one image, so the block can just as well run image chunk by image chunk: with a chunk's activation well under the
    # 256 MiB Infinity Cache the producer's output is still on chip when its consumer reads it, and the chunk loop re-uses the
    # same intermediate buffers.  Same kernels, same per-row arithmetic - only the launch order changes
    # (tests/test_model_gpu.py::test_cache_blocked_forward).  The chunk is given in ROWS (tokens) so that every launch of a
    # chunk covers a whole number of 256-workgroup rounds of the persistent 256-row tiles (65536 rows = one round).
    chunk_rows = int(os.environ.get("SDV_CHUNK_ROWS", "0"))

    def _chunk_images(self, HW: int, nimg: int) -> int:
        """Images per chunk for a [nimg*HW, C] activation (0 = run the whole batch at once)."""
        env = os.environ.get("SDV_CHUNK_ROWS")              # (read per call: tools/chunk_ab.py flips it between forwards)
        rows = int(env) if env is not None else self.chunk_rows
        levels = os.environ.get("SDV_CHUNK_LEVELS")         # optional: comma list of HW values the blocking applies to
        if rows <= 0 or TAP is not None or (levels and str(HW) not in levels.split(",")):
            return 0
        n = max(1, rows // HW)
        return n if nimg >= 2 * n else 0

    def _segment(self, r: "_Res", t: Optional["_Transformer"], h, skip, nimg: int, nb: int, hh: int, ww: int, step_ptr, circ,
                 first: bool = False):
        """One ResBlock and the transformer block behind it (if any), cache-blocked over images when that pays."""
        HW = hh * ww
        n = 0 if first else self._chunk_images(HW, nimg)
        if n == 0:
            h = r(h, skip, nb if first else nimg, hh, ww, step_ptr, circ)
            if t is not None:
                h = t(h, nimg, hh, ww, shared_prefix=first)
            return h
        out = torch.empty((nimg * HW, r.cout), dtype=BF16, device=self.device)
        parts = []
        for lo in range(0, nimg, n):
            m = min(n, nimg - lo)
            # (the chunks carry their slice of the producers' GroupNorm statistics, and the chunks' own statistics are joined
            #  again below: the chunked forward normalises with exactly the numbers of the whole-batch forward)
            hs = hip.gn_slice(h, lo, m, HW)
            sk = hip.gn_slice(skip, lo, m, HW) if skip is not None else None
            o = out[lo * HW:(lo + m) * HW]
            if t is None:
                r(hs, sk, m, hh, ww, step_ptr, circ, out=o)
            else:
                y = r(hs, sk, m, hh, ww, step_ptr, circ)
                t(y, m, hh, ww, out=o, ctx_of=(nimg, lo))
            parts.append(o)
        hip.gn_join(parts, out)
        return out

    # -- one denoise forward -----------------------------------------------------------------
    def forward(self, x: torch.Tensor, nimg: int, H: int, W: int, step_ptr: torch.Tensor,
                cfg_shared: bool = False) -> torch.Tensor:
        """x: bf16 NHWC [nimg*H*W, Cin]; returns eps fp32 NHWC [nimg, H, W, Cout].  The timestep is
        the ``*step_ptr``-th entry of the schedule given to ``prepare_timesteps``.

        ``cfg_shared``: the two halves of x are the same latents (classifier-free guidance,
        ``torch.cat([latents] * 2)`` at stable_diffusion_pipeline.py:414).  Until the text context enters at the first
        cross-attention the two copies compute identical values, so conv_in, the first ResBlock and the first
        transformer's self-attention run on nimg/2 samples only."""
        circ = self.tiled
        shared = bool(cfg_shared) and nimg % 2 == 0 and bool(self.down[0].attn)
        nb = nimg // 2 if shared else nimg
        h = self.conv_in(x[: nb * H * W], nb, H, W, circ)
        if shared:
            h0 = torch.empty((nimg * H * W, h.shape[1]), dtype=BF16, device=self.device)   # skip tensor for the up path
            h0[: nb * H * W].copy_(h)
            h0[nb * H * W:].copy_(h)
            hip.gn_repeat(h, h0, 2)         # (its GroupNorm statistics are conv_in's, twice)
            skips = [h0]
        else:
            skips = [h]
        hh, ww = H, W
        for bi, blk in enumerate(self.down):
            for j, (r, t) in enumerate(blk.pairs()):
                first = shared and bi == 0 and j == 0
                h = self._segment(r, t, h, None, nimg, nb, hh, ww, step_ptr, circ, first)
                skips.append(h)
            if blk.resample is not None:
                h, hh, ww = blk.resample(h, nimg, hh, ww, circ)
                skips.append(h)
        r0, t0, r1 = self.mid
        h = r0(h, None, nimg, hh, ww, step_ptr, circ)
        h = t0(h, nimg, hh, ww)
        h = r1(h, None, nimg, hh, ww, step_ptr, circ)
        for blk in self.up:
            for r, t in blk.pairs():
                h = self._segment(r, t, h, skips.pop(), nimg, nb, hh, ww, step_ptr, circ)
            if blk.resample is not None:
                h, hh, ww = blk.resample(h, nimg, hh, ww, circ)
        h_in = h
        h = hip.groupnorm(h, self.out_g, self.out_b, nimg=nimg, HW=hh * ww, groups=self.groups, eps=self.eps, silu=True)
        eps = torch.empty((nimg, hh, ww, self.cfg.out_channels), dtype=F32, device=self.device)
        # conv_out 320 -> 4 on the matrix cores (one 32-column MFMA tile, fp32 straight from the accumulators)
        hip.conv3x3(h, self.conv_out_w, self.conv_out_b, nimg=nimg, H=hh, W=ww, circular=circ, out_mode=1,
                    out_f32=eps.view(-1, self.cfg.out_channels))
        _tap("conv_out", "out", x=h_in, out=eps.view(-1, self.cfg.out_channels), nimg=nimg, H=hh, W=ww)
        return eps


# ------------------------------------------------------------------------------------------------
# VAE decoder
# ------------------------------------------------------------------------------------------------
class VAEDecoderEngine:
    def __init__(self, cfg: VAEConfig, sd: StateDict, device, tiled: bool = False):
        hip.load()
        self.cfg, self.device, self.tiled = cfg, torch.device(device), tiled
        self.config = cfg
        dev = self.device
        g = cfg.norm_num_groups
        ch = list(reversed(cfg.block_out_channels))
        lc = cfg.latent_channels
        self.pq_w = sd["post_quant_conv.weight"].reshape(lc, lc).contiguous().to(dev, F32)
        self.pq_b = vec(sd["post_quant_conv.bias"], dev)
        self.conv_in = _ConvIn(sd, "decoder.conv_in", dev)
        self.mid_res = [_Res(sd, f"decoder.mid_block.resnets.{i}", dev, g, 1e-6, False) for i in range(2)]
        a = "decoder.mid_block.attentions.0"
        self.a_g, self.a_b = vec(sd[a + ".group_norm.weight"], dev), vec(sd[a + ".group_norm.bias"], dev)
        self.a_wqk = lin_w(torch.cat([sd[a + ".to_q.weight"], sd[a + ".to_k.weight"]], 0), dev)
        self.a_bqk = vec(torch.cat([sd[a + ".to_q.bias"], sd[a + ".to_k.bias"]], 0), dev)
        self.a_wv, self.a_bv = lin_w(sd[a + ".to_v.weight"], dev), vec(sd[a + ".to_v.bias"], dev)
        self.a_wo, self.a_bo = lin_w(sd[a + ".to_out.0.weight"], dev), vec(sd[a + ".to_out.0.bias"], dev)
        self.up = [_Level([_Res(sd, f"decoder.up_blocks.{i}.resnets.{j}", dev, g, 1e-6, False) for j in range(cfg.layers_per_block + 1)],
                          [], _Up(sd, f"decoder.up_blocks.{i}.upsamplers.0", dev) if i != len(ch) - 1 else None)
                   for i in range(len(ch))]
        self.out_g, self.out_b = vec(sd["decoder.conv_norm_out.weight"], dev), vec(sd["decoder.conv_norm_out.bias"], dev)
        self.conv_out_w, self.conv_out_b = conv_w(sd["decoder.conv_out.weight"], dev), vec(sd["decoder.conv_out.bias"], dev)
        self.groups = g
        self.scale_factor = 2 ** (len(cfg.block_out_channels) - 1)
        self.score_chunk_bytes = 512 << 20      # mid-block attention: bytes of [HW, HW] bf16 scores materialised at a time

    def _attention(self, x, nimg, H, W):
        C, HW = x.shape[1], H * W
        n = hip.groupnorm(x, self.a_g, self.a_b, nimg=nimg, HW=HW, groups=self.groups, eps=1e-6, silu=False)
        qk = hip.linear(n, self.a_wqk, self.a_bqk)                                   # [M, 2C]
        vt = torch.empty((nimg, C, HW), dtype=BF16, device=x.device)
        hip.gemm(self.a_wv, n, vt, M=C, N=HW, K=C, ldx=C, ldw=C, ldc=HW, bias=self.a_bv, bias_mode=2, batch=nimg,
                 sX=0, sW=HW * C, sC=C * HW)                                         # V^T (+ bias per channel)
        o = torch.empty((nimg * HW, C), dtype=BF16, device=x.device)
        # The one place a score matrix is materialised (1 head x 512 channels: the flash kernel has no dh = 512 instance - 128 Q
        # registers + 256 accumulators per 32 queries).  The scores leave the Q K^T GEMM as fp32 (out_mode 1) and are rounded ONCE,
        # as probabilities, by the softmax - what the flash kernels do in registers; rounds 1-3 stored them as bf16 first and this
        # was the weakest block of the decoder.  Chunks of images whose fp32 scores + bf16 probabilities stay under 512 MiB.
        per = max(1, self.score_chunk_bytes // (6 * HW * HW))
        s = torch.empty((min(per, nimg), HW, HW), dtype=F32, device=x.device)
        pr = torch.empty((min(per, nimg), HW, HW), dtype=BF16, device=x.device)
        for i0 in range(0, nimg, per):
            nb = min(per, nimg - i0)
            hip.gemm(qk, qk, None, M=HW, N=HW, K=C, ldx=2 * C, ldw=2 * C, ldc=HW, alpha=C ** -0.5, batch=nb,
                     sX=HW * 2 * C, sW=HW * 2 * C, sC=HW * HW, x_off=i0 * HW * 2 * C, w_off=i0 * HW * 2 * C + C,
                     out_mode=1, out_f32=s)                                          # S = Q K^T / sqrt(C), fp32
            hip.softmax_rows_f32(s, pr, nb * HW, HW, HW, HW)
            hip.gemm(pr, vt, o, M=HW, N=C, K=HW, ldx=HW, ldw=HW, ldc=C, batch=nb, sX=HW * HW, sW=C * HW, sC=HW * C,
                     w_off=i0 * C * HW, out_off=i0 * HW * C)
        out = hip.linear(o, self.a_wo, self.a_bo, residual=x, gn_hw=HW)
        _tap("decoder.mid_block.attentions.0", "vae_attention", x=x, out=out, nimg=nimg, H=H, W=W)
        return out

    def decode(self, latents: torch.Tensor, want_float: bool = False):
        """latents: fp32 NHWC [B, h, w, 4] (UNSCALED, as they leave the denoise loop).  Returns
        (uint8 NHWC images [B, 8h, 8w, 3], optional fp32 NHWC images in [0,1])."""
        B, h, w, lc = latents.shape
        circ = self.tiled
        z = torch.empty((B * h * w, lc), dtype=BF16, device=self.device)
        hip.latent_affine(latents.contiguous(), self.pq_w, self.pq_b, 1.0 / self.cfg.scaling_factor, z, B * h * w, lc)
        _tap("post_quant_conv", "post_quant", x=latents.reshape(B * h * w, lc), out=z, nimg=B, H=h, W=w)
        x = self.conv_in(z, B, h, w, circ)
        x = self.mid_res[0](x, None, B, h, w, None, circ)
        x = self._attention(x, B, h, w)
        x = self.mid_res[1](x, None, B, h, w, None, circ)
        for blk in self.up:
            for r in blk.res:
                x = r(x, None, B, h, w, None, circ)
            if blk.resample is not None:
                x, h, w = blk.resample(x, B, h, w, circ)
        x_in = x
        x = hip.groupnorm(x, self.out_g, self.out_b, nimg=B, HW=h * w, groups=self.groups, eps=1e-6, silu=True)
        oc = self.cfg.out_channels
        u8 = torch.empty((B, h, w, oc), dtype=torch.uint8, device=self.device)
        f32 = torch.empty((B, h, w, oc), dtype=F32, device=self.device) if want_float else None
        # conv_out 128 -> 3 on the matrix cores with the image epilogue (clamp(v / 2 + 0.5) -> round-half-even uint8)
        hip.conv3x3(x, self.conv_out_w, self.conv_out_b, nimg=B, H=h, W=w, circular=circ, out_mode=2,
                    out_f32=f32.view(-1, oc) if f32 is not None else None, out_u8=u8.view(-1, oc))
        _tap("decoder.conv_out", "vae_out", x=x_in, out=f32.view(-1, oc) if f32 is not None else u8.view(-1, oc), nimg=B, H=h, W=w)
        return u8, f32
