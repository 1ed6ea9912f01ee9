"""CPU tests of the safety checker (reference stable_diffusion_pipeline.py:440-447): the float64 restatements the GPU tests use as
their oracle are pinned to the real ``transformers`` / PIL through tests/golden/clip_vision_tiny.npz, the host tap tables, the
argument validation of the two new ops, header / library / binding agreement, and the pipeline's construction cases."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from vision_ref import (STAGE_ROUNDINGS, load_fixture, pil_resize_crop64, pil_taps64, resize_geometry64, safety_head64, stage64,
                        stage_kind, tower_roundings, tower_stages, vision_forward64)

ROOT = Path(__file__).resolve().parent.parent


def test_pil_bicubic_restatement_matches_pil_fixture():
    """The float64 two-pass restatement (no uint8 rounding) against PIL's own output.  Bound: 1.5 grey levels - PIL rounds to uint8
    after each pass: 0.5 after the second, plus the first pass's 0.5 carried through the second's taps, 0.5 * sum|w| <= 0.7."""
    z, _ = load_fixture()
    for i, (H, W, S) in enumerate(z["pre_cases"].tolist()):
        img, ref = z[f"pre{i}_in"], z[f"pre{i}_out"]
        assert img.shape == (H, W, 3) and ref.shape == (S, S, 3) and img.min() >= 32 and img.max() <= 223
        out = pil_resize_crop64(img, S)
        err = np.abs(out - ref.astype(np.float64)).max()
        print(f"PIL bicubic restatement {H}x{W} -> {S}: max |diff| {err:.3f} grey levels")
        assert err <= 1.5, (H, W, S, err)


def test_float64_vision_tower_matches_transformers_fixture():
    """vision_forward64 == transformers.CLIPVisionModelWithProjection(pixel_values).image_embeds (fp32, CPU) to 1e-5 relative."""
    z, sd = load_fixture()
    ref = torch.from_numpy(z["image_embeds"]).double()
    out = vision_forward64(sd, torch.from_numpy(z["pixel_values"]), int(z["num_heads"]), int(z["patch_size"]), str(z["hidden_act"]))
    assert out.shape == ref.shape == (3, 64)
    rel = float((out - ref).norm() / ref.norm())
    print(f"float64 vision tower vs transformers {z['transformers_version']}: rel-L2 {rel:.2e}")
    assert rel <= 1e-5 and float((out - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    # the storage hook is called where the counts say, stage by stage (q / k / v are one buffer: 3 calls, 1 rounding)
    x, total = torch.from_numpy(z["pixel_values"]), 0
    assert tower_stages(2) == ["embed", "pre_ln", "layers.0.attn", "layers.0.mlp", "layers.1.attn", "layers.1.mlp", "head"]
    for name in tower_stages(2):
        calls = []
        x = stage64(sd, name, x, 2, 14, store=lambda t: (calls.append(1), t)[1])
        assert len(calls) - (2 if name.endswith("attn") else 0) == STAGE_ROUNDINGS[stage_kind(name)], name
        total += STAGE_ROUNDINGS[stage_kind(name)]
    assert total == tower_roundings(2) == 19 and torch.equal(x, out)
    # the rounding-count bound of every stage holds for the ideal bf16-storage engine (exact arithmetic, storage roundings only)
    # under teacher forcing - the premise of the stage-wise gate of tests/test_vision_gpu.py - while end to end, on these doubled
    # weights, the same ideal engine is over the whole path's count bound: that figure is not a gate on this fixture
    import math
    from oracle import blockwise as bw
    from vision_ref import bf16
    pv = torch.from_numpy(z["pixel_values"])
    x = pv
    for name in tower_stages(2):
        exact, ideal = stage64(sd, name, x, 2, 14), stage64(sd, name, x, 2, 14, store=bf16)
        assert bw.rel_l2(ideal, exact) <= bw.SAFETY * bw.EPS_BF16 * math.sqrt(STAGE_ROUNDINGS[stage_kind(name)]), name
        x = ideal
    e2e = bw.rel_l2(vision_forward64(sd, pv, 2, 14, store=bf16), out)
    print(f"ideal bf16-storage engine end to end: rel-L2 {e2e:.2e}; count bound {bw.SAFETY * bw.EPS_BF16 * math.sqrt(19):.2e}")


def test_float64_checker_head_regimes():
    """safety_head64 follows diffusers' arithmetic: the 0.01 adjustment exists only behind a special-care hit."""
    g = torch.Generator().manual_seed(0)
    c, s = torch.randn(17, 32, generator=g), torch.randn(3, 32, generator=g)
    e = torch.stack([c[4] + 0.0 * s[0], s[1].clone()])
    thr_c, thr_s = torch.full((17,), 0.5), torch.full((3,), 0.5)
    flags, scores = safety_head64(e, c, s, thr_c, thr_s)
    assert flags.tolist() == [True, False] and scores.shape == (2, 20)
    assert abs(float(scores[0, 3 + 4]) - 0.5) < 1e-12 and abs(float(scores[1, 1]) - 0.5) < 1e-12
    # image 1 hits special-care 1: every concept score of it carries + 0.01
    cos = torch.nn.functional.cosine_similarity(e[1].double()[None], c.double())
    assert torch.allclose(scores[1, 3:], cos - 0.5 + 0.01, atol=1e-12)


def test_host_tap_tables():
    from stable_diffusion_videos_amd.vision import preprocess_taps, resample_taps, resize_geometry
    for H, W, S in ((96, 64, 56), (40, 72, 56), (128, 128, 28), (512, 512, 224), (64, 64, 56), (720, 1280, 224)):
        Hr, Wr, top, left = resize_geometry(H, W, S)
        assert (Hr, Wr, top, left) == resize_geometry64(H, W, S)
        assert min(Hr, Wr) == S and top == (Hr - S) // 2 and left == (Wr - S) // 2
        (xo, xc, xw), (yo, yc, yw) = preprocess_taps(H, W, S)
        for off, cnt, w, size, resized, first in ((xo, xc, xw, W, Wr, left), (yo, yc, yw, H, Hr, top)):
            assert off.dtype == cnt.dtype == torch.int32 and w.dtype == torch.float32
            assert off.shape == cnt.shape == (S,) and w.shape[0] == S and w.shape[1] <= size
            assert float((w.double().sum(1) - 1).abs().max()) <= 1e-6                      # weights sum to 1 (fp32 table)
            assert int(off.min()) >= 0 and int((off + cnt).max()) <= size and int(cnt.min()) >= 1 and int(cnt.max()) <= w.shape[1]
            k = torch.arange(w.shape[1])[None, :]
            assert float(w[k >= cnt[:, None]].abs().max() if bool((k >= cnt[:, None]).any()) else 0.0) == 0.0
            # the window is the crop's: entry i is PIL's tap set of resized sample first + i
            ref = pil_taps64(size, resized)
            for i in (0, S // 2, S - 1):
                lo, ww = ref[first + i]
                assert int(off[i]) == lo and int(cnt[i]) == len(ww)
                assert np.abs(w[i, :len(ww)].double().numpy() - ww).max() <= 1e-7
        o64, c64, w64 = resample_taps(W, Wr)
        assert np.abs(w64.sum(1) - 1).max() <= 1e-14
    with pytest.raises(ValueError):
        resample_taps(64, 56, 50, 10)


def _cpu_preprocess_args(S=56, P=14, n=2, H=64, W=64):
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.vision import preprocess_taps
    tx, ty = preprocess_taps(H, W, S)
    frames = torch.zeros((n, H, W, 3), dtype=torch.uint8)
    patches = torch.zeros((n * (S // P) ** 2, hip.patch_kpad(P)), dtype=torch.bfloat16)
    return dict(frames=frames, patches=patches, tx=tx, ty=ty, S=S, P=P, mean=[0.5] * 3, std=[0.5] * 3)


def _call_preprocess(a):
    torch.ops.sdv.k_clip_preprocess(a["frames"], a["patches"], *a["tx"], *a["ty"], a["S"], a["P"], a["mean"], a["std"])


def test_preprocess_op_validates_before_any_launch(hip):
    """Every shape / stride / alignment mistake raises SdvHipError from the checks, not from the device-pointer guard behind them
    (these are CPU tensors: a call that passed the checks would say "GPU memory")."""
    assert hip.patch_kpad(14) == 640 and hip.patch_kpad(16) == 768
    ok = _cpu_preprocess_args()
    with pytest.raises(hip.SdvHipError, match="GPU memory"):
        _call_preprocess(ok)                                   # all checks passed, no device behind the tensors
    bad = dict(ok, patches=torch.zeros((ok["patches"].shape[0], 576), dtype=torch.bfloat16))
    with pytest.raises(hip.SdvHipError, match="Kpad = 640"):
        _call_preprocess(bad)
    bad = dict(ok, patches=ok["patches"][:-1])
    with pytest.raises(hip.SdvHipError, match="rows"):
        _call_preprocess(bad)
    bad = dict(ok, frames=torch.zeros((2, 64, 128, 3), dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(hip.SdvHipError, match="contiguous uint8"):
        _call_preprocess(bad)
    flat = torch.zeros(ok["patches"].numel() + 8, dtype=torch.bfloat16)
    base = flat.data_ptr() % 16 // 2                            # element offset that makes the view 2 bytes off a 16-byte boundary
    bad = dict(ok, patches=flat[(8 - base) % 8 + 1:][:ok["patches"].numel()].view_as(ok["patches"]))
    assert bad["patches"].data_ptr() % 16 != 0
    with pytest.raises(hip.SdvHipError, match="16-byte aligned"):
        _call_preprocess(bad)
    bad = dict(ok, tx=(ok["tx"][0][:-1], ok["tx"][1], ok["tx"][2]))
    with pytest.raises(hip.SdvHipError, match="tap tables must hold S = 56"):
        _call_preprocess(bad)
    bad = dict(ok, ty=(ok["ty"][0], ok["ty"][1], ok["ty"][2].double()))
    with pytest.raises(hip.SdvHipError, match="tap tables"):
        _call_preprocess(bad)
    bad = dict(ok, S=60)
    with pytest.raises(hip.SdvHipError, match="S % P"):
        _call_preprocess(bad)
    # the C entry point repeats what it can see (fake non-null pointers: nothing is dereferenced before the checks fail)
    lib = hip.load()
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    okc = [16, 16, 2, 64, 64, 56, 14, 640, 16, 16, 16, 5, 16, 16, 16, 5, f3, f3, None]
    for pos, val, word in ((7, 576, b"Kpad"), (1, 18, b"16-byte aligned"), (5, 60, b"bad shape"), (0, None, b"null"), (11, 0, b"tap counts"),
                           (5, 1024, b"LDS"), (6, 16, b"bad shape")):
        a = list(okc)
        a[pos] = val
        if pos == 5 and val == 1024:
            a[6], a[7], a[3], a[4] = 16, 768, 2048, 2048
        assert lib.sdv_clip_preprocess_patches(*a) == -1 and word in lib.sdv_last_error(), (pos, lib.sdv_last_error())


def test_screen_op_validates_before_any_launch(hip):
    n, D = 5, 32
    ok = dict(e=torch.zeros(n, D), c=torch.zeros(17, D), s=torch.zeros(3, D), tc=torch.zeros(17), ts=torch.zeros(3),
              frames=torch.zeros((n, 8, 8, 3), dtype=torch.uint8), flags=torch.zeros(n, dtype=torch.int32), scores=torch.zeros(n, 20))

    def call(a):
        torch.ops.sdv.k_safety_screen(a["e"], a["c"], a["s"], a["tc"], a["ts"], a["frames"], a["flags"], a["scores"])

    with pytest.raises(hip.SdvHipError, match="GPU memory"):
        call(ok)
    for change, word in ((dict(flags=torch.zeros(n - 1, dtype=torch.int32)), "flags must be"),
                         (dict(flags=torch.zeros(n, dtype=torch.int64)), "flags must be"),
                         (dict(scores=torch.zeros(n, 17)), "scores must be"),
                         (dict(tc=torch.zeros(16)), "thresholds"),
                         (dict(c=torch.zeros(17, D + 1)), "concept_embeds"),
                         (dict(s=torch.zeros(3, 2 * D)[:, ::2]), "special_care_embeds"),
                         (dict(c=torch.zeros(70, D), tc=torch.zeros(70), scores=torch.zeros(n, 73)), "at most 64"),
                         (dict(frames=torch.zeros((n, 8, 16, 3), dtype=torch.uint8)[:, :, ::2]), "frames must be"),
                         (dict(frames=torch.zeros((n + 1, 8, 8, 3), dtype=torch.uint8)), "frames must be"),
                         (dict(e=torch.zeros(n, D, dtype=torch.float64)), "image_embeds")):
        with pytest.raises(hip.SdvHipError, match=word):
            call(dict(ok, **change))
    lib = hip.load()
    okc = [16, 16, 16, 16, 16, 5, 768, 17, 3, 16, 3 * 64 * 64, 16, 16, None]
    for pos, val, word in ((0, None, b"null"), (11, None, b"null"), (5, 0, b"bad shape"), (7, 62, b"at most 64"), (9, 24, b"16-byte aligned"),
                           (10, 0, b"frame size")):
        a = list(okc)
        a[pos] = val
        assert lib.sdv_safety_screen(*a) == -1 and word in lib.sdv_last_error(), (pos, lib.sdv_last_error())


def test_header_library_and_binding_agree_on_the_new_entry_points(hip):
    header = (ROOT / "include" / "sdv_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in (("sdv_clip_preprocess_patches", "k_clip_preprocess"), ("sdv_safety_screen", "k_safety_screen")):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(lib, name) and name in hip.EXPORTED_SYMBOLS
        assert op in hip.KERNEL_OPS and hasattr(torch.ops.sdv, op)
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        # the declaration cites the reference line it replaces, and the argument count of the binding is the declaration's
        decl = header[header.index(f"int {name}("):]
        decl = decl[:decl.index(");")]
        assert len(decl.split(",")) == len(hip._SIGNATURES[name][1]), name
    doc = header[header.index("Safety checker"):header.index("int sdv_clip_preprocess_patches(")]
    assert ":441" in doc and ":442-447" in doc
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    src = (ROOT / "stable_diffusion_videos_amd" / "vision.py").read_text()
    assert "import ctypes" not in src and "lib.sdv_" not in src


def test_weight_schema_loader_and_config(tmp_path):
    import json
    from safetensors.torch import save_file
    from stable_diffusion_videos_amd import config, weights
    full = weights.vision_shapes(config.sd_vision())
    assert weights.count_params(full) == 303_966_208 + 20 * 768 + 20       # CLIPVisionModelWithProjection ViT-L/14 + the head's buffers
    assert full["embeddings.position_embedding.weight"] == (257, 1024) and full["pre_layrnorm.weight"] == (1024,)
    assert full["concept_embeds"] == (17, 768) and full["special_care_embeds_weights"] == (3,)
    cfg = config.tiny_vision()
    shapes = weights.vision_shapes(cfg)
    sd = weights.synthetic_safety_checker(cfg, seed=5)
    sd2 = weights.synthetic_safety_checker(cfg, seed=5)
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == tuple(shapes[k]) and torch.equal(sd[k], sd2[k]) for k in shapes)
    # StableDiffusionSafetyChecker nests CLIPVisionModel (two prefixes); CLIPVisionModelWithProjection has one; both load
    d = tmp_path / "safety_checker"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(
        projection_dim=cfg.projection_dim, vision_config=dict(hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                                              num_hidden_layers=2, num_attention_heads=2, image_size=56, patch_size=14))))
    assert config.vision_from_json(d / "config.json") == cfg
    head = set(weights.SAFETY_HEAD_KEYS) | {"visual_projection.weight"}
    for prefix in ("vision_model.vision_model.", "vision_model.", ""):
        save_file({(k if k in head else prefix + k): v.contiguous() for k, v in sd.items()}, str(d / "model.safetensors"))
        back = weights.load_safety_checker(tmp_path, shapes)
        assert all(torch.equal(back[k], sd[k]) for k in shapes), prefix
    from stable_diffusion_videos_amd.vision import build_safety_checker
    eng = build_safety_checker(tmp_path)
    assert not eng.is_synthetic and eng.config == cfg and eng.feature_extractor.crop_size == {"height": 56, "width": 56}
    with pytest.raises(FileNotFoundError):
        weights.load_safety_checker(tmp_path / "nowhere", shapes)


def test_pipeline_construction_cases_without_gpu(hip):
    from stable_diffusion_videos_amd import SafetyCheckerEngine, StableDiffusionWalkPipeline as P
    from stable_diffusion_videos_amd.vision import FeatureExtractor
    pipe = P.from_pretrained("tiny")
    assert pipe.safety_checker is None and pipe.feature_extractor is None                  # the default is unchanged
    for ask in (True, "default"):
        pipe = P.from_pretrained("tiny", safety_checker=ask)
        assert isinstance(pipe.safety_checker, SafetyCheckerEngine) and pipe.safety_checker.is_synthetic
        fe = pipe.feature_extractor
        assert isinstance(fe, FeatureExtractor) and fe.size == {"shortest_edge": 56} and fe.crop_size == {"height": 56, "width": 56}
        assert len(fe.image_mean) == len(fe.image_std) == 3
    eng = pipe.safety_checker
    assert P.from_pretrained("tiny", safety_checker=eng).safety_checker is eng               # a passed engine is adopted
    # no CPU fallback anywhere
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        eng(torch.zeros((1, 64, 64, 3), dtype=torch.uint8))
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        eng(images=np.zeros((1, 64, 64, 3), dtype=np.float32), clip_input=None)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        eng.vision(torch.zeros((16, 640), dtype=torch.bfloat16), 1)
    # any other object: the constructor's feature-extractor rule, then the NotImplementedError of __call__
    with pytest.raises(ValueError, match="feature extractor"):
        P.from_pretrained("tiny", safety_checker=object())
    foreign = P.from_pretrained("tiny", safety_checker=object(), feature_extractor=object())
    with pytest.raises(NotImplementedError, match="pass safety_checker=None"):
        foreign(prompt="a cat", height=64, width=64)
