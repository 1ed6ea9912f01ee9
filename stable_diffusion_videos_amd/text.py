"""Text side of the walk path: ``tokenizer(...)`` and ``text_encoder(ids)[0]`` as the reference calls them
(stable_diffusion_pipeline.py:291-306, :340-348, :811-819).

``CLIPTextEngine`` is the CLIP text transformer (``transformers.CLIPTextModel`` in the reference) on the HIP kernels:
token + position embedding gather, the pre-LN encoder layers of ``clip.EncoderLayer`` (shared with the vision tower of the
safety checker) around ONE launch of the flash attention kernel with its causal mask over the whole batch, final LayerNorm.
It is on the path but not hot (2 forwards per clip + 1 per walk, ~13 GFLOP each).  Same call shape as the reference's module:
``text_encoder(ids)[0]`` is ``last_hidden_state``.

Offline there are neither CLIP weights nor ``vocab.json`` / ``merges.txt``.  When a model directory with
``text_encoder/`` / ``tokenizer/`` sub-directories is given the real weights / ``CLIPTokenizer`` are used; otherwise
seeded synthetic weights and ``HashTokenizer`` (deterministic, clearly synthetic ids: BOS + one id per whitespace
word + EOS padding), which is all the throughput and parity harness needs.
"""
from __future__ import annotations

import hashlib
from pathlib import Path
from types import SimpleNamespace
from typing import List, Optional, Union

import torch

from . import hip
from .clip import EncoderLayer, Engine
from .config import TextConfig
from .weights import clip_text_shapes, load_clip_text, synthetic_state_dict, vec


class HashTokenizer:
    """Stand-in for CLIPTokenizer with the same call shape (``padding="max_length"``, ``truncation=True``,
    ``return_tensors="pt"`` -> object with ``.input_ids``) and ``model_max_length``."""

    def __init__(self, cfg: TextConfig):
        self.model_max_length = cfg.max_position_embeddings
        self.bos, self.eos = cfg.bos_token_id, cfg.eos_token_id
        self.n_words = min(cfg.bos_token_id, cfg.eos_token_id)  # ids below the special tokens
        self.is_synthetic = True

    def _ids(self, text: str, max_length: int, truncation: bool) -> List[int]:
        words = text.lower().split()
        ids = [int.from_bytes(hashlib.sha256(w.encode()).digest()[:4], "little") % (self.n_words - 1) + 1 for w in words]
        ids = [self.bos] + ids + [self.eos]
        if truncation and len(ids) > max_length:
            ids = ids[: max_length - 1] + [self.eos]
        return ids + [self.eos] * (max_length - len(ids))

    def __call__(self, text: Union[str, List[str]], padding="max_length", max_length: Optional[int] = None,
                 truncation: bool = False, return_tensors="pt"):
        texts = [text] if isinstance(text, str) else list(text)
        max_length = max_length or self.model_max_length
        rows = [self._ids(t, max_length, truncation) for t in texts]
        width = max(len(r) for r in rows)
        rows = [r + [self.eos] * (width - len(r)) for r in rows]
        return SimpleNamespace(input_ids=torch.tensor(rows, dtype=torch.long))

    def batch_decode(self, ids):
        return ["<synthetic ids>" for _ in ids]


def load_tokenizer(model_dir: Optional[Path], cfg: TextConfig):
    if model_dir is not None and (Path(model_dir) / "tokenizer" / "vocab.json").exists():
        from transformers import CLIPTokenizer
        return CLIPTokenizer.from_pretrained(str(Path(model_dir) / "tokenizer"))
    return HashTokenizer(cfg)


class CLIPTextEngine(Engine):
    """``text_encoder(ids)[0]`` of the reference on the HIP kernels.  Weights are re-laid out at ``.to(device)``."""

    def _prepare(self, device):
        sd, c = self.state_dict_, self.config
        return {"tok": sd["embeddings.token_embedding.weight"].to(device, torch.float32).contiguous(),
                "pos": sd["embeddings.position_embedding.weight"].to(device, torch.float32).contiguous(),
                "fin": (vec(sd["final_layer_norm.weight"], device), vec(sd["final_layer_norm.bias"], device)),
                "layers": [EncoderLayer(sd, f"encoder.layers.{i}.", device, c, 1e-5) for i in range(c.num_hidden_layers)]}

    @torch.no_grad()
    def __call__(self, input_ids: torch.Tensor, *args, **kwargs):
        """input_ids int64 [B, L] -> (last_hidden_state fp32 [B, L, D],) - index 0 as the reference takes it (:819)."""
        if self._w is None or not input_ids.is_cuda:
            raise hip.SdvHipError("CLIPTextEngine runs on the MI355X HIP path only (no CPU fallback): call .to('cuda') and "
                                  "pass GPU-resident ids")
        c = self.config
        ids = input_ids.to(torch.int64)
        if ids.shape[1] > c.max_position_embeddings:
            raise ValueError(f"sequence length {ids.shape[1]} exceeds max_position_embeddings {c.max_position_embeddings}")
        if int(ids.min()) < 0 or int(ids.max()) >= c.vocab_size:
            raise IndexError(f"token id outside [0, {c.vocab_size})")
        return (self._forward(ids),)

    def _forward(self, ids: torch.Tensor) -> torch.Tensor:
        """Checked ids int64 [B, L] -> last_hidden_state: only launches from here on."""
        c, w = self.config, self._w
        B, L = ids.shape
        D, H = c.hidden_size, c.num_attention_heads
        dh = D // H

        def attend(qkv, o):           # one causal launch over the batch
            hip.attention(qkv, qkv, qkv, o, B=B, H=H, Lq=L, Lk=L, dh=dh, ldq=3 * D, ldk=3 * D, ldv=3 * D, ldo=D,
                          scale=dh ** -0.5, k_off=D, v_off=2 * D, causal=True, q_prescaled=True, v_rowmajor=True)

        x = hip.embed_tokens(ids, w["tok"], w["pos"])                                          # [B*L, D]
        o = torch.empty_like(x)
        for layer in w["layers"]:
            x = layer(x, o, attend)
        out = hip.layernorm(x, *w["fin"], eps=1e-5)
        return out.float().view(B, L, D)


def build_text_encoder(cfg: TextConfig, model_dir: Optional[Path] = None, seed: int = 0) -> CLIPTextEngine:
    """Real weights from ``<model_dir>/text_encoder`` when present (its ``config.json`` overrides ``cfg``), otherwise
    the same architecture with seeded synthetic weights."""
    if model_dir is not None and (Path(model_dir) / "text_encoder" / "config.json").exists():
        import json
        data = json.loads((Path(model_dir) / "text_encoder" / "config.json").read_text())
        data = data.get("text_config", data)
        cfg = TextConfig(**{k: data[k] for k in TextConfig.__dataclass_fields__ if k in data})
        return CLIPTextEngine(cfg, load_clip_text(model_dir, clip_text_shapes(cfg)))
    return CLIPTextEngine(cfg, synthetic_state_dict(clip_text_shapes(cfg), seed=seed))
