#!/usr/bin/env python
"""Golden vectors for the safety checker's vision side (stable_diffusion_pipeline.py:441-447): the REAL
``transformers.CLIPVisionModelWithProjection`` run in this container on seeded weights and pixel values, and PIL's own bicubic
resize + centre crop (what ``CLIPImageProcessor`` calls) on three smooth images.  Writes tests/golden/clip_vision_tiny.npz.

    python tests/golden/make_golden_clip_vision.py

Size: ~0.7 MB, more than the text fixtures' 0.33 / 0.49 MB.  It is what the model the tests need costs: hidden 128, 2 layers,
intermediate 256, a 14 x 14 x 3 patch embedding and a 64-wide projection are ~350 k parameters, stored as 2 bytes each (the
high half of a bf16-exact fp32) - random bits that do not compress; pixel values and the PIL cases add ~0.15 MB.
"""
import os
from pathlib import Path

import numpy as np
import PIL
import torch
import transformers
from PIL import Image
from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection

OUT = Path(__file__).resolve().parent

# (H, W, S): frame size and crop size of the preprocessing cases
PRE_CASES = ((96, 64, 56), (40, 72, 56), (128, 128, 28))


def smooth_image(H, W, seed):
    """Two low-frequency sinusoids and a ramp per channel, inside [32, 223]: far enough from 0 / 255 that the clamp PIL applies
    when it rounds to uint8 between and after its two passes never engages (bicubic overshoot of a smooth image is tiny)."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.empty((H, W, 3))
    for c in range(3):
        fy, fx, gy, gx = rng.uniform(0.5, 2.0, 4)
        p1, p2 = rng.uniform(0, 2 * np.pi, 2)
        s = np.sin(2 * np.pi * (fy * y / H + fx * x / W) + p1) + np.sin(2 * np.pi * (gy * y / H - gx * x / W) + p2)     # [-2, 2]
        ramp = (x / max(W - 1, 1) + y / max(H - 1, 1)) - 1.0                                                          # [-1, 1]
        img[..., c] = 127.5 + 95.5 * (s + ramp) / 3.0                                                                  # [32, 223]
    out = np.round(img).astype(np.uint8)
    assert out.min() >= 32 and out.max() <= 223
    return out


def pil_resize_crop(img, S):
    H, W = img.shape[:2]
    if H <= W:
        Hr, Wr = S, int(S * W / H)
    else:
        Hr, Wr = int(S * H / W), S
    r = np.asarray(Image.fromarray(img).resize((Wr, Hr), Image.BICUBIC))
    top, left = (Hr - S) // 2, (Wr - S) // 2
    return r[top:top + S, left:left + S]


def main():
    torch.manual_seed(11)
    # head dim 64 = the head dim of the checker's ViT-L/14 (1024 / 16); 56 / 14 = 4 -> 16 patches + class token = 17 tokens
    cfg = CLIPVisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=56,
                           patch_size=14, projection_dim=64, hidden_act="quick_gelu")
    model = CLIPVisionModelWithProjection(cfg).float().eval()
    with torch.no_grad():
        for p in model.parameters():                # default init is tiny (std 0.02): widen it so that the
            p.mul_(2.0)                             # non-linearities are exercised (as the text fixture does)
            p.copy_(p.to(torch.bfloat16).float())   # bf16-representable: the bf16 HIP path shares them exactly
    pixel_values = torch.randn(3, 3, 56, 56).to(torch.bfloat16).float()
    with torch.no_grad():
        embeds = model(pixel_values=pixel_values).image_embeds
    arrays = {"sd::" + k: (v.contiguous().view(torch.int32) >> 16).to(torch.int16).numpy()
              for k, v in model.state_dict().items() if v.is_floating_point()}
    pre = {}
    for i, (H, W, S) in enumerate(PRE_CASES):
        img = smooth_image(H, W, seed=100 + i)
        pre[f"pre{i}_in"] = img
        pre[f"pre{i}_out"] = pil_resize_crop(img, S)
    path = OUT / "clip_vision_tiny.npz"
    np.savez_compressed(path, pixel_values=pixel_values.numpy(), image_embeds=embeds.numpy(), num_heads=np.int64(2),
                        patch_size=np.int64(14), image_size=np.int64(56), hidden_act=np.array("quick_gelu"),
                        pre_cases=np.array(PRE_CASES, dtype=np.int64), transformers_version=np.array(transformers.__version__),
                        pil_version=np.array(PIL.__version__), **arrays, **pre)
    print(embeds.shape, float(embeds.abs().mean()), sorted(k for k in arrays)[:3], os.path.getsize(path))


if __name__ == "__main__":
    main()
