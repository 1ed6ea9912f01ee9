"""Safety checker of the reference's ``__call__`` (stable_diffusion_pipeline.py:440-447) on the HIP path:

    safety_checker_input = self.feature_extractor(self.numpy_to_pil(image), return_tensors="pt")     :441
    image, has_nsfw_concept = self.safety_checker(images=image, clip_input=...pixel_values)          :442-447

``CLIPVisionEngine`` is ``transformers.CLIPVisionModelWithProjection`` on the encoder layer ``text.CLIPTextEngine`` runs too
(``clip.EncoderLayer``), with one non-causal attention launch per image; ``SafetyCheckerEngine`` puts the two kernels of
csrc/sdv_vision.hip around it:
``hip.clip_preprocess_patches`` (CLIPImageProcessor + the patch convolution's im2col, uint8 frames in HBM -> GEMM operand) and
``hip.safety_screen`` (cosine head + black-out).  No CPU fallback: off the GPU the engines raise ``SdvHipError``.

Token layout.  An image has T = (S/P)^2 + 1 tokens (257 for ViT-L/14 at 224), not a multiple of 32.  Activations are
[n * Tpad, D] with Tpad = roundup(T, 32): every image's rows start at a multiple of 32.  LayerNorms and GEMMs run over all rows
(rows are independent; what the pad rows hold never matters); the attention runs per image with Lq = Lk = T on that image's
row block, so a pad row is never a key, a value or a written query row.

The checker head (diffusers ``StableDiffusionSafetyChecker.forward``, third-party arithmetic restated): with cos(a, b) the cosine
similarity of the L2-normalised vectors,

    special[i, j] = cos(image_embeds[i], special_care_embeds[j]) - special_care_embeds_weights[j] + 0
    adj[i]        = 0.01 if any_j special[i, j] > 0 else 0
    concept[i, j] = cos(image_embeds[i], concept_embeds[j]) - concept_embeds_weights[j] + adj[i]
    has_nsfw[i]   = any_j concept[i, j] > 0

and every flagged image is replaced by zeros (``images[idx] = np.zeros(images[idx].shape)``).
"""
from __future__ import annotations

import logging
import math
from pathlib import Path
from typing import Optional, Tuple

import numpy as np
import torch

from . import hip
from .clip import EncoderLayer, Engine
from .config import VisionConfig, vision_from_json
from .weights import SAFETY_HEAD_KEYS, lin_w, load_safety_checker, synthetic_safety_checker, vec, vision_shapes

logger = logging.getLogger("stable_diffusion_videos_amd")

CLIP_IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)

# Test hook, as ``engine.TAP``: called as TAP(stage, {"x": the stage's input in HBM (None for "embed"), "out": its output}) after
# every stage of ``CLIPVisionEngine`` - "embed", "pre_ln", "layers.<i>.attn", "layers.<i>.mlp", "head" - so that each can be checked
# on its own against a float64 restatement fed the engine's own input (tests/test_vision_gpu.py).  None = no overhead.
TAP = None


# ------------------------------------------------------------------------------------------------
# PIL's bicubic resize as tap tables (host, float64)
# ------------------------------------------------------------------------------------------------
def _bicubic(x: np.ndarray, a: float = -0.5) -> np.ndarray:
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    far = (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resample_taps(in_size: int, out_size: int, first: int = 0, count: Optional[int] = None):
    """The 1-D taps of ``PIL.Image.resize(..., BICUBIC)`` from ``in_size`` to ``out_size`` samples, for the output samples
    [first, first + count): (off int32 [count], cnt int32 [count], w float64 [count, taps]).  Output sample i reads the source
    samples off[i] ... off[i] + cnt[i] - 1 with the weights w[i, :cnt[i]] (zero beyond).  PIL (Resample.c, precompute_coeffs):
    scale = in / out, filter scale fs = max(scale, 1) (the kernel is stretched - antialiased - when shrinking), support 2 fs,
    centre (i + 0.5) scale, window [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the image, weight
    bicubic((x + 0.5 - centre) / fs) with a = -0.5, normalised to sum 1."""
    count = out_size - first if count is None else count
    if in_size < 1 or out_size < 1 or first < 0 or count < 1 or first + count > out_size:
        raise ValueError(f"resample_taps: bad geometry in={in_size} out={out_size} window=[{first}, {first + count})")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    taps = int(math.ceil(support)) * 2 + 1
    off = np.zeros(count, dtype=np.int32)
    cnt = np.zeros(count, dtype=np.int32)
    w = np.zeros((count, taps), dtype=np.float64)
    for k in range(count):
        centre = (first + k + 0.5) * scale
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), in_size)
        xs = np.arange(lo, hi, dtype=np.float64)
        ww = _bicubic((xs - centre + 0.5) / fs)
        s = ww.sum()
        if s != 0.0:
            ww = ww / s
        off[k], cnt[k] = lo, hi - lo
        w[k, :hi - lo] = ww
    return off, cnt, w


def resize_geometry(H: int, W: int, S: int) -> Tuple[int, int, int, int]:
    """``CLIPImageProcessor``: shortest edge -> S keeping the aspect ratio (the long edge is int(S * long / short)), then a centre
    crop of S x S.  Returns (resized H, resized W, crop top, crop left)."""
    if H <= W:
        Hr, Wr = S, int(S * W / H)
    else:
        Hr, Wr = int(S * H / W), S
    return Hr, Wr, (Hr - S) // 2, (Wr - S) // 2


def preprocess_taps(H: int, W: int, S: int):
    """The two tap tables of the crop window for frames of H x W: ((x_off, x_cnt, x_w), (y_off, y_cnt, y_w)), weights fp32, as CPU
    tensors (``SafetyCheckerEngine`` keeps the device copies, one set per frame size)."""
    Hr, Wr, top, left = resize_geometry(H, W, S)
    out = []
    for size, resized, first in ((W, Wr, left), (H, Hr, top)):
        off, cnt, w = resample_taps(size, resized, first, S)
        out.append((torch.from_numpy(off), torch.from_numpy(cnt), torch.from_numpy(w.astype(np.float32)).contiguous()))
    return tuple(out)


class FeatureExtractor:
    """What the pipeline's constructor asks for next to a safety checker (reference :101-104): the ``CLIPImageProcessor``
    settings the preprocess kernel applies.  Not callable - the frames never leave the GPU for it."""

    def __init__(self, size: int = 224, image_mean=CLIP_IMAGE_MEAN, image_std=CLIP_IMAGE_STD):
        self.size = {"shortest_edge": int(size)}
        self.crop_size = {"height": int(size), "width": int(size)}
        self.image_mean = [float(v) for v in image_mean]
        self.image_std = [float(v) for v in image_std]
        self.resample = "bicubic"


def _tower_key(sd, key):
    for p in ("", "vision_model.", "vision_model.vision_model."):
        if p + key in sd:
            return sd[p + key]
    raise KeyError(key)


class CLIPVisionEngine(Engine):
    """``CLIPVisionModelWithProjection(pixel_values).image_embeds`` on the HIP kernels, from the patch-embedding GEMM operand
    (``hip.clip_preprocess_patches``; column order (c, py, px), K padded to a multiple of 64)."""

    def __init__(self, cfg: VisionConfig, state_dict):
        super().__init__(cfg, state_dict)
        if cfg.image_size % cfg.patch_size or cfg.hidden_size % 8:
            raise ValueError("CLIPVisionEngine: image_size must be a multiple of patch_size and hidden_size of 8")
        self.T = cfg.num_tokens
        self.Tpad = (self.T + 31) // 32 * 32

    def _prepare(self, device):        # (the patch embedding is padded on the host)
        c = self.config
        sd = {k: _tower_key(self.state_dict_, k) for k in self._keys()}
        D, K = c.hidden_size, 3 * c.patch_size ** 2
        wp = torch.zeros((D, hip.patch_kpad(c.patch_size)), dtype=torch.float32)
        wp[:, :K] = sd["embeddings.patch_embedding.weight"].float().reshape(D, K)
        pos = sd["embeddings.position_embedding.weight"].float()
        return {"patch": lin_w(wp, device),
                # position embeddings of the patch tokens: the residual of the patch GEMM; class token row = class + position 0
                "pos": pos[1:].contiguous().to(device, torch.bfloat16),
                "cls": (sd["embeddings.class_embedding"].float() + pos[0]).to(device, torch.bfloat16),
                "pre": (vec(sd["pre_layrnorm.weight"], device), vec(sd["pre_layrnorm.bias"], device)),
                "post": (vec(sd["post_layernorm.weight"], device), vec(sd["post_layernorm.bias"], device)),
                "proj": lin_w(sd["visual_projection.weight"], device),
                "layers": [EncoderLayer(sd, f"encoder.layers.{i}.", device, c, c.layer_norm_eps) for i in range(c.num_hidden_layers)]}

    def _keys(self):
        return [k for k in vision_shapes(self.config) if k not in SAFETY_HEAD_KEYS]

    def _need_gpu(self, t: torch.Tensor):
        if self._w is None or not t.is_cuda:
            raise hip.SdvHipError("CLIPVisionEngine runs on the MI355X HIP path only (no CPU fallback): call .to('cuda') and "
                                  "pass GPU-resident tensors")

    @torch.no_grad()
    def embed(self, patches: torch.Tensor, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Patch rows bf16 [n * (S/P)^2, Kpad] -> embeddings bf16 [n * Tpad, D] BEFORE pre_layrnorm: row 0 of every image's block
        is class_embedding + position 0, rows 1 ... T - 1 are patch GEMM (no bias) + position, rows T ... Tpad - 1 are left as
        ``out`` holds them (zeros when the buffer is allocated here)."""
        self._need_gpu(patches)
        c, w = self.config, self._w
        D, T, Tpad, NP = c.hidden_size, self.T, self.Tpad, self.T - 1
        if tuple(patches.shape) != (n * NP, w["patch"].shape[1]):
            raise hip.SdvHipError(f"CLIPVisionEngine: expected patch rows {(n * NP, w['patch'].shape[1])}, got {tuple(patches.shape)}")
        x = torch.zeros((n * Tpad, D), dtype=torch.bfloat16, device=patches.device) if out is None else out
        xv = x.view(n, Tpad, D)
        for b in range(n):
            hip.linear(patches[b * NP:(b + 1) * NP], w["patch"], None, residual=w["pos"], out=xv[b, 1:T])
        xv[:, 0] = w["cls"]
        if TAP is not None:
            TAP("embed", {"x": None, "out": x})
        return x

    @torch.no_grad()
    def encode(self, x: torch.Tensor, n: int) -> torch.Tensor:
        """Embeddings bf16 [n * Tpad, D] (``embed``) -> image_embeds fp32 [n, projection_dim]."""
        self._need_gpu(x)
        c, w = self.config, self._w
        D, H, T, Tpad = c.hidden_size, c.num_attention_heads, self.T, self.Tpad
        dh = D // H
        if tuple(x.shape) != (n * Tpad, D) or not x.is_contiguous():
            raise hip.SdvHipError(f"CLIPVisionEngine: expected contiguous embeddings {(n * Tpad, D)}, got {tuple(x.shape)}")
        eps = c.layer_norm_eps

        def attend(qkv, o):              # per image: Lq = Lk = T inside its Tpad-row block - pad rows never reach the softmax
            for b in range(n):
                blk = qkv[b * Tpad:(b + 1) * Tpad]
                hip.attention(blk, blk, blk, o[b * Tpad:(b + 1) * Tpad], B=1, H=H, Lq=T, Lk=T, dh=dh, ldq=3 * D, ldk=3 * D,
                              ldv=3 * D, ldo=D, scale=dh ** -0.5, k_off=D, v_off=2 * D, causal=False, q_prescaled=True,
                              v_rowmajor=True)

        x0, x = x, hip.layernorm(x, *w["pre"], eps=eps)
        if TAP is not None:
            TAP("pre_ln", {"x": x0, "out": x})
        o = torch.zeros_like(x)          # (the attention writes the T real rows of every image; the pad rows stay zero)
        for i, layer in enumerate(w["layers"]):
            x = layer(x, o, attend, TAP and (lambda name, xin, out: TAP(f"layers.{i}.{name}", {"x": xin, "out": out})))
        pooled = hip.layernorm(x.view(n, Tpad, D)[:, 0].contiguous(), *w["post"], eps=eps)        # class token only
        embeds = hip.linear_small(pooled.float(), w["proj"])                                      # fp32 [n, projection_dim]
        if TAP is not None:
            TAP("head", {"x": x, "out": embeds})
        return embeds

    def __call__(self, patches: torch.Tensor, n: int) -> torch.Tensor:
        return self.encode(self.embed(patches, n), n)


class SafetyCheckerEngine:
    """``StableDiffusionSafetyChecker`` on GPU-resident uint8 frames: preprocess -> vision tower -> head + black-out.

    ``engine(frames_u8)`` -> (flags torch.bool [n] on the host, scores fp32 [n, 3 + 17] = [special | concept] on the device);
    flagged frames are zeroed IN PLACE.  ``engine(images=, clip_input=)`` is the reference's call shape (:442-447): numpy NHWC
    float images in [0, 1] -> (images with the flagged ones zeroed, list of bool); ``clip_input`` is ignored - the pixel values are
    recomputed on the GPU from the images' uint8 form (numpy_to_pil's rounding), which is what the reference's feature extractor
    is fed."""

    def __init__(self, cfg: VisionConfig, state_dict, image_mean=CLIP_IMAGE_MEAN, image_std=CLIP_IMAGE_STD):
        self.config = cfg
        self.state_dict_ = state_dict
        self.vision = CLIPVisionEngine(cfg, state_dict)
        self.feature_extractor = FeatureExtractor(cfg.image_size, image_mean, image_std)
        self.device = torch.device("cpu")
        self.is_synthetic = False
        self._head = None
        self._taps = {}

    def state_dict(self):
        return self.state_dict_

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            if self._head is not None:
                raise hip.SdvHipError("SafetyCheckerEngine cannot be moved off the GPU (no CPU fallback)")
            return self
        if self._head is None or device != self.device:
            self.vision.to(device)
            sd = self.state_dict_
            self._head = {"concept": vec(sd["concept_embeds"], device), "special": vec(sd["special_care_embeds"], device)}
            self.concept_thresholds = vec(sd["concept_embeds_weights"], device)
            self.special_care_thresholds = vec(sd["special_care_embeds_weights"], device)
            self._taps = {}
        self.device = device
        return self

    def _need_gpu(self, t):
        if self._head is None or not torch.is_tensor(t) or not t.is_cuda:
            raise hip.SdvHipError("SafetyCheckerEngine runs on the MI355X HIP path only (no CPU fallback): call .to('cuda') and "
                                  "pass GPU-resident uint8 frames")

    def preprocess(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """uint8 NHWC frames in HBM -> patch rows (``hip.clip_preprocess_patches``); the tap tables are built on the host once per
        frame size and kept on the device."""
        self._need_gpu(frames_u8)
        c, fe = self.config, self.feature_extractor
        H, W = int(frames_u8.shape[1]), int(frames_u8.shape[2])
        if (H, W) not in self._taps:
            tx, ty = preprocess_taps(H, W, c.image_size)
            self._taps[(H, W)] = (tuple(t.to(self.device) for t in tx), tuple(t.to(self.device) for t in ty))
        tx, ty = self._taps[(H, W)]
        return hip.clip_preprocess_patches(frames_u8, tx, ty, S=c.image_size, P=c.patch_size, mean=fe.image_mean, std=fe.image_std)

    @torch.no_grad()
    def screen(self, frames_u8: torch.Tensor):
        """-> (flags int32 [n], scores fp32 [n, 20]), both left on the device (nothing here synchronises with the host)."""
        self._need_gpu(frames_u8)
        n = frames_u8.shape[0]
        embeds = self.vision(self.preprocess(frames_u8), n)
        return hip.safety_screen(embeds, self._head["concept"], self._head["special"], self.concept_thresholds,
                                 self.special_care_thresholds, frames_u8)

    @torch.no_grad()
    def __call__(self, frames_u8: Optional[torch.Tensor] = None, *, images=None, clip_input=None):
        if images is not None:
            if self._head is None:
                raise hip.SdvHipError("SafetyCheckerEngine runs on the MI355X HIP path only (no CPU fallback): call .to('cuda')")
            arr = np.asarray(images)
            u8 = (torch.from_numpy(np.ascontiguousarray(arr)).to(self.device, torch.float32) * 255).round().clamp(0, 255).to(torch.uint8)
            flags, _ = self.screen(u8.contiguous())
            has = [bool(v) for v in flags.cpu().tolist()]
            out = np.array(arr, copy=True)
            for i, bad in enumerate(has):
                if bad:
                    out[i] = np.zeros(out[i].shape)
            return out, has
        flags, scores = self.screen(frames_u8)
        return flags.cpu().bool(), scores


def build_safety_checker(model_dir: Optional[Path] = None, seed: int = 0, cfg: Optional[VisionConfig] = None) -> SafetyCheckerEngine:
    """Real weights from ``<model_dir>/safety_checker`` when present (its ``config.json`` decides the architecture), otherwise the
    same architecture (``cfg``, default ViT-L/14) with seeded synthetic weights - flagged and logged, as the text encoder's are."""
    if model_dir is not None and (Path(model_dir) / "safety_checker" / "config.json").exists():
        cfg = vision_from_json(Path(model_dir) / "safety_checker" / "config.json")
        mean, std = CLIP_IMAGE_MEAN, CLIP_IMAGE_STD
        pre = Path(model_dir) / "feature_extractor" / "preprocessor_config.json"
        if pre.exists():
            import json
            data = json.loads(pre.read_text())
            mean, std = data.get("image_mean", mean), data.get("image_std", std)
        return SafetyCheckerEngine(cfg, load_safety_checker(model_dir, vision_shapes(cfg)), mean, std)
    cfg = cfg or VisionConfig()
    logger.warning("safety checker: no safety_checker/ directory on disk - building the CLIP vision tower (%d layers x %d) and the "
                   "checker head with seeded SYNTHETIC weights; its flags mean nothing", cfg.num_hidden_layers, cfg.hidden_size)
    eng = SafetyCheckerEngine(cfg, synthetic_safety_checker(cfg, seed=seed))
    eng.is_synthetic = True
    return eng
