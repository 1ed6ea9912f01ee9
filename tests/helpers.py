"""Shared builders for the parity tests: an oracle module (CPU fp32) and the matching HIP engine from ONE
seeded, bf16-exact synthetic state dict - so any difference is activation arithmetic, not weights."""
from __future__ import annotations

import torch

from oracle import models as om
from stable_diffusion_videos_amd import config as cfgs
from stable_diffusion_videos_amd import weights


def oracle_unet_cfg(c: cfgs.UNetConfig) -> om.UNetConfig:
    return om.UNetConfig(sample_size=c.sample_size, in_channels=c.in_channels, out_channels=c.out_channels,
                         block_out_channels=tuple(c.block_out_channels), down_block_types=tuple(c.down_block_types),
                         up_block_types=tuple(c.up_block_types), layers_per_block=c.layers_per_block,
                         cross_attention_dim=c.cross_attention_dim, attention_head_dim=c.attention_head_dim,
                         norm_num_groups=c.norm_num_groups, norm_eps=c.norm_eps,
                         use_linear_projection=c.use_linear_projection, flip_sin_to_cos=c.flip_sin_to_cos,
                         freq_shift=c.freq_shift)


def oracle_vae_cfg(c: cfgs.VAEConfig) -> om.VAEConfig:
    return om.VAEConfig(latent_channels=c.latent_channels, out_channels=c.out_channels,
                        block_out_channels=tuple(c.block_out_channels), layers_per_block=c.layers_per_block,
                        norm_num_groups=c.norm_num_groups, scaling_factor=c.scaling_factor)


def _materialise(module_cls, cfg, sd):
    with torch.device("meta"):
        m = module_cls(cfg)
    # proj_in/proj_out are stored as [C, C, 1, 1] convs or [C, C] linears depending on the config
    fixed = {k: v.reshape(m.state_dict()[k].shape) for k, v in sd.items()}
    m.load_state_dict(fixed, assign=True, strict=True)
    return m.eval()


def make_oracle_unet(c: cfgs.UNetConfig, sd):
    return _materialise(om.UNet2DConditionModel, oracle_unet_cfg(c), sd)


def make_oracle_vae(c: cfgs.VAEConfig, sd):
    return _materialise(om.AutoencoderKLDecoder, oracle_vae_cfg(c), sd)


def unet_pair(c: cfgs.UNetConfig, device, seed=0, tiled=False, fp8=False):
    from stable_diffusion_videos_amd.engine import UNetEngine
    sd = weights.synthetic_state_dict(weights.unet_shapes(c), seed=seed)
    return make_oracle_unet(c, sd), UNetEngine(c, sd, device, tiled=tiled, fp8=fp8)


def vae_pair(c: cfgs.VAEConfig, device, seed=1, tiled=False):
    from stable_diffusion_videos_amd.engine import VAEDecoderEngine
    sd = weights.synthetic_state_dict(weights.vae_decoder_shapes(c), seed=seed)
    return make_oracle_vae(c, sd), VAEDecoderEngine(c, sd, device, tiled=tiled)


def _half_ulp_ratio(out64, ref64, mag64, acc_eps=1e-5):
    """|out - ref| relative to (half a bf16 ulp of the result + fp32 accumulation noise acc_eps * sum |terms|)."""
    ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(ref64.abs(), out64.abs()).clamp_min(1e-30))) - 7)
    return (out64 - ref64).abs() / (0.5 * ulp * (1 + 1e-3) + acc_eps * mag64)


def _attn_ref64(q, k, v, heads, scale, causal=False):
    """float64 softmax(QK^T scale) V per head, plus sum_k p_k |v_k| (the scale of the P-rounding error).
    ``causal``: query i sees the keys j <= i."""
    B, Lq, Cc = q.shape
    dh = Cc // heads
    out = torch.empty((B, Lq, Cc), dtype=torch.float64)
    mag = torch.empty_like(out)
    hidden = torch.ones((Lq, k.shape[1]), dtype=torch.bool).triu(1) if causal else None
    for b in range(B):
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            s = q[b, :, sl] @ k[b, :, sl].T * scale
            if causal:
                s = s.masked_fill(hidden, float("-inf"))
            p = torch.softmax(s, -1)
            out[b, :, sl] = p @ v[b, :, sl]
            mag[b, :, sl] = p @ v[b, :, sl].abs()
    return out, mag
