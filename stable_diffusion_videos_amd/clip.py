"""What ``text.CLIPTextEngine`` and ``vision.CLIPVisionEngine`` share: the config check, the residency rule, and the CLIP pre-LN
encoder layer - LayerNorm, the fused [Wq; Wk; Wv] projection with the softmax scale on Q, the attention the engine brings, out-proj +
residual, LayerNorm, fc1 with quick_gelu / gelu in its epilogue, fc2 + residual: 6 launches and the engine's attention."""
from __future__ import annotations

import torch

from . import hip
from .weights import lin_w, vec


class Engine:
    """A CLIP tower on the HIP kernels: its weights are re-laid out (``_prepare(device)`` of the subclass: any device, "meta"
    included) when it is moved to a GPU; there is no CPU path."""

    def __init__(self, cfg, state_dict):
        who = type(self).__name__
        if cfg.hidden_size % cfg.num_attention_heads or cfg.hidden_size // cfg.num_attention_heads not in (40, 64, 80, 160):
            raise ValueError(f"{who}: head dim must be one of 40 / 64 / 80 / 160 (the SD text encoders and ViT-L/14 use 64)")
        if cfg.hidden_act not in ("quick_gelu", "gelu"):
            raise ValueError(f"{who}: unsupported hidden_act {cfg.hidden_act}")
        self.config = cfg
        self.state_dict_ = state_dict
        self.device = torch.device("cpu")
        self._w = None

    def state_dict(self):
        return self.state_dict_

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and (self._w is None or device != self.device):
            hip.load()
            self._w = self._prepare(device)
        self.device = device
        return self


class EncoderLayer:
    """One layer's weights in the kernels' layout, from the state dict ``sd`` (keys ``<p>layer_norm1.weight`` ...) on ``device``."""

    def __init__(self, sd, p: str, device, cfg, eps: float):
        a = p + "self_attn."
        self.D = cfg.hidden_size
        self.dh = self.D // cfg.num_attention_heads
        self.epi = 4 if cfg.hidden_act == "quick_gelu" else 5
        self.eps = eps
        qs = hip.q_prescale(self.dh)
        self.ln1 = (vec(sd[p + "layer_norm1.weight"], device), vec(sd[p + "layer_norm1.bias"], device))
        self.ln2 = (vec(sd[p + "layer_norm2.weight"], device), vec(sd[p + "layer_norm2.bias"], device))
        # q / k / v as one projection [3D, D]; the attention kernel reads V row-major out of its output
        self.wqkv = lin_w(torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]], 0), device)
        # the Q third of the bias carries the softmax scale * log2(e) that the projection's alpha puts on Q
        self.bqkv = vec(torch.cat([sd[a + "q_proj.bias"].float() * qs, sd[a + "k_proj.bias"].float(), sd[a + "v_proj.bias"].float()], 0),
                        device)
        self.wo, self.bo = lin_w(sd[a + "out_proj.weight"], device), vec(sd[a + "out_proj.bias"], device)
        self.w1, self.b1 = lin_w(sd[p + "mlp.fc1.weight"], device), vec(sd[p + "mlp.fc1.bias"], device)
        self.w2, self.b2 = lin_w(sd[p + "mlp.fc2.weight"], device), vec(sd[p + "mlp.fc2.bias"], device)

    def __call__(self, x, o, attend, stage=None):
        """x: bf16 [M, D] hidden rows -> the rows after the MLP.  ``attend(qkv, o)`` launches the attention over
        qkv [M, 3D] = [Q * qs | K | V] into ``o`` [M, D]; ``stage(name, x, out)`` is told the input and output of "attn" and "mlp"."""
        h = hip.layernorm(x, *self.ln1, eps=self.eps)
        attend(hip.linear(h, self.wqkv, self.bqkv, alpha=hip.q_prescale(self.dh), alpha_cols=self.D), o)
        y = hip.linear(o, self.wo, self.bo, residual=x)
        if stage is not None:
            stage("attn", x, y)
        h = hip.layernorm(y, *self.ln2, eps=self.eps)
        f = hip.linear(h, self.w1, self.b1, epi=self.epi)
        out = hip.linear(f, self.w2, self.b2, residual=y)
        if stage is not None:
            stage("mlp", y, out)
        return out
