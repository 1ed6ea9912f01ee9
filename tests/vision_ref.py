"""float64 restatements the safety-checker tests share (test infrastructure, no product code): the CLIP vision tower
(``transformers.CLIPVisionModelWithProjection``), the checker head (diffusers ``StableDiffusionSafetyChecker.forward``) and PIL's
bicubic resize + ``CLIPImageProcessor`` crop.  tests/test_vision_cpu.py pins them to the real libraries through
tests/golden/clip_vision_tiny.npz; the GPU tests then use them as the oracle at shapes too large for a fixture."""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden"
F64 = torch.float64


def load_fixture():
    z = np.load(GOLDEN / "clip_vision_tiny.npz")
    sd = {}
    for k in z.files:
        if k.startswith("sd::"):
            name = k[4:]
            while name.startswith("vision_model."):
                name = name[len("vision_model."):]
            sd[name] = (torch.from_numpy(z[k].astype(np.int32)) << 16).view(torch.float32)
    return z, sd


def bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def patch_rows(pixel_values: torch.Tensor, P: int, Kpad: int) -> torch.Tensor:
    """NCHW pixel values -> rows [n * G * G, Kpad] in (c, py, px) column order, zero-padded: what the stride-P patch
    convolution multiplies with its flattened weight [hidden, 3 * P * P]."""
    n, C, S, _ = pixel_values.shape
    G = S // P
    r = pixel_values.reshape(n, C, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(n * G * G, C * P * P)
    out = torch.zeros((n * G * G, Kpad), dtype=pixel_values.dtype)
    out[:, :C * P * P] = r
    return out


def unpatch_rows(rows: torch.Tensor, n: int, S: int, P: int) -> torch.Tensor:
    """inverse of ``patch_rows`` (pad columns dropped) -> [n, 3, S, S]"""
    G = S // P
    r = rows[:, :3 * P * P].reshape(n, G, G, 3, P, P).permute(0, 3, 1, 4, 2, 5)
    return r.reshape(n, 3, S, S)


# bf16 storage roundings on the path through each stage of the vision engine (vision.py), counted as oracle/blockwise.py counts a
# block's: the stage's output rounding included, its input (the engine's own tensor under teacher forcing) exact
STAGE_ROUNDINGS = {
    "embed": 1,      # patch GEMM + position / class row
    "pre_ln": 1,     # pre_layrnorm out
    "attn": 5,       # LN1 out, [Q | K | V] (one buffer), P (in registers), attention out, out-proj + residual
    "mlp": 3,        # LN2 out, fc1 + activation out, fc2 + residual
    "head": 1,       # post_layernorm out (the projection leaves in fp32)
}


def stage_kind(name: str) -> str:
    return name.rsplit(".", 1)[-1]


def tower_stages(layers: int):
    return ["embed", "pre_ln"] + [f"layers.{i}.{k}" for i in range(layers) for k in ("attn", "mlp")] + ["head"]


def tower_roundings(layers: int) -> int:
    """roundings on the whole path: 3 + 8 per layer"""
    return sum(STAGE_ROUNDINGS[stage_kind(s)] for s in tower_stages(layers))


def stage64(sd, name: str, x, heads: int, patch: int, act: str = "quick_gelu", eps: float = 1e-5, store=None):
    """One stage of the tower in float64 on the input ``x`` (pixel values [n, 3, S, S] for "embed", tokens [n, T, D] otherwise;
    "head" returns image_embeds [n, projection_dim]).  ``store(t)`` is applied wherever the HIP engine keeps a tensor in bf16
    (identity by default); passing ``bf16`` gives the IDEAL bf16-storage engine: exact arithmetic, only the storage roundings."""
    store = store or (lambda t: t)
    w = {k: v.to(F64) for k, v in sd.items() if k.startswith(("embeddings.", "pre_layrnorm.", "post_layernorm.", "visual_projection."))
         or (name.startswith("layers.") and k.startswith("encoder." + name.rsplit(".", 1)[0] + "."))}
    x = x.to(F64)
    n, D = x.shape[0], w["embeddings.class_embedding"].numel()
    dh = D // heads

    def ln(t, key):
        return store(torch.nn.functional.layer_norm(t, (D,), w[key + ".weight"], w[key + ".bias"], eps))

    def lin(t, key):
        return t @ w[key + ".weight"].T + w[key + ".bias"]

    kind = stage_kind(name)
    if kind == "embed":
        pe = torch.nn.functional.conv2d(x, w["embeddings.patch_embedding.weight"], stride=patch).flatten(2).transpose(1, 2)    # [n, NP, D]
        pos = w["embeddings.position_embedding.weight"]
        return store(torch.cat([(w["embeddings.class_embedding"] + pos[0]).expand(n, 1, D), pe + pos[1:]], dim=1))
    if kind == "pre_ln":
        return ln(x, "pre_layrnorm")
    if kind == "head":
        return ln(x[:, 0], "post_layernorm") @ w["visual_projection.weight"].T
    p = "encoder." + name.rsplit(".", 1)[0] + "."
    if kind == "attn":
        y = ln(x, p + "layer_norm1")
        # the engine stores [Q * scale * log2(e) | K | V] once; the factor on Q is exact in neither, the rounding is one
        qs = dh ** -0.5 * math.log2(math.e)
        q = store(lin(y, p + "self_attn.q_proj") * qs) / qs
        k = store(lin(y, p + "self_attn.k_proj"))
        v = store(lin(y, p + "self_attn.v_proj"))
        T = q.shape[1]
        q, k, v = (t.reshape(n, T, heads, dh).transpose(1, 2) for t in (q, k, v))
        s = q @ k.transpose(-1, -2) * dh ** -0.5
        pr = torch.exp(s - s.amax(-1, keepdim=True))
        o = (store(pr) @ v) / pr.sum(-1, keepdim=True)
        o = store(o.transpose(1, 2).reshape(n, T, D))
        return store(lin(o, p + "self_attn.out_proj") + x)
    if kind == "mlp":
        f = lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")
        f = f * torch.sigmoid(1.702 * f) if act == "quick_gelu" else torch.nn.functional.gelu(f)
        return store(lin(store(f), p + "mlp.fc2") + x)
    raise ValueError(name)


def num_layers(sd) -> int:
    return 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))


def vision_forward64(sd, pixel_values, heads: int, patch: int, act: str = "quick_gelu", eps: float = 1e-5, store=None):
    """image_embeds [n, projection_dim] float64: the stages of ``stage64`` in order."""
    x = pixel_values
    for name in tower_stages(num_layers(sd)):
        x = stage64(sd, name, x, heads, patch, act, eps, store)
    return x


def safety_head64(embeds, concept, special, thr_c, thr_s):
    """diffusers StableDiffusionSafetyChecker.forward in float64 -> (flags bool [n], scores [n, special | concept])"""
    e, c, s = (t.to(F64) for t in (embeds, concept, special))

    def cos(a, b):
        return (a / a.norm(dim=-1, keepdim=True)) @ (b / b.norm(dim=-1, keepdim=True)).T

    sp = cos(e, s) - thr_s.to(F64)
    adj = torch.where((sp > 0).any(dim=1, keepdim=True), 0.01, 0.0).to(F64)
    co = cos(e, c) - thr_c.to(F64) + adj
    return (co > 0).any(dim=1), torch.cat([sp, co], dim=1)


# ------------------------------------------------------------------------------------------------
# PIL bicubic (Resample.c) + CLIPImageProcessor geometry, float64, no uint8 rounding anywhere
# ------------------------------------------------------------------------------------------------
def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def pil_taps64(in_size: int, out_size: int):
    """list of (first source index, normalised weights) per output sample"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    taps = []
    for i in range(out_size):
        centre = (i + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), in_size)
        ww = np.array([_cubic((x - centre + 0.5) / fs) for x in range(lo, hi)], dtype=np.float64)
        taps.append((lo, ww / ww.sum()))
    return taps


def resize_geometry64(H: int, W: int, S: int):
    Hr, Wr = (S, int(S * W / H)) if H <= W else (int(S * H / W), S)
    return Hr, Wr, (Hr - S) // 2, (Wr - S) // 2


def pil_resize_crop64(img_u8: np.ndarray, S: int) -> np.ndarray:
    """uint8 [H, W, 3] -> float64 grey levels [S, S, 3]: horizontal pass, vertical pass, centre crop"""
    H, W, _ = img_u8.shape
    Hr, Wr, top, left = resize_geometry64(H, W, S)
    src = img_u8.astype(np.float64)
    tx, ty = pil_taps64(W, Wr), pil_taps64(H, Hr)
    hor = np.stack([np.tensordot(w, src[:, lo:lo + len(w)], axes=(0, 1)) for lo, w in tx[left:left + S]], axis=1)      # [H, S, 3]
    return np.stack([np.tensordot(w, hor[lo:lo + len(w)], axes=(0, 0)) for lo, w in ty[top:top + S]], axis=0)          # [S, S, 3]


def preprocess64(frames_u8: np.ndarray, S: int, mean, std) -> torch.Tensor:
    """uint8 [n, H, W, 3] -> normalised pixel values float64 [n, 3, S, S] (CLIPImageProcessor without any rounding)"""
    out = np.stack([pil_resize_crop64(f, S) for f in frames_u8])
    out = (out / 255.0 - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    return torch.from_numpy(out).permute(0, 3, 1, 2).contiguous()
