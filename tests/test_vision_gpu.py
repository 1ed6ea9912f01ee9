"""GPU tests of the safety checker (reference stable_diffusion_pipeline.py:440-447): the preprocess kernel against the float64
restatement of PIL + CLIPImageProcessor and against PIL's own output, the vision tower against transformers' vectors and the
float64 restatement (tests/vision_ref.py, pinned in tests/test_vision_cpu.py), the screen kernel against the float64 head, and the
pipeline wiring end to end."""
import math

import numpy as np
import pytest
import torch

from conftest import report
from oracle import blockwise as bw
from vision_ref import (STAGE_ROUNDINGS, bf16, load_fixture, patch_rows, preprocess64, safety_head64, stage64, stage_kind,
                        tower_roundings, tower_stages, unpatch_rows, vision_forward64)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENTINEL = -12352.0       # (exact in bf16) fills the guard band behind the preprocess output


# ------------------------------------------------------------------------------------------------
# 1. preprocess kernel
# ------------------------------------------------------------------------------------------------
def _preprocess_cases():
    z, _ = load_fixture()
    cases = []
    for i, (H, W, S) in enumerate(z["pre_cases"].tolist()):
        cases.append((f"fixture {H}x{W}->{S}", z[f"pre{i}_in"][None], S, z[f"pre{i}_out"][None]))
    rng = np.random.RandomState(3)
    cases.append(("512x512->224", rng.randint(0, 256, (1, 512, 512, 3)).astype(np.uint8), 224, None))
    cases.append(("64x64->28 n=3", rng.randint(0, 256, (3, 64, 64, 3)).astype(np.uint8), 28, None))
    return cases


@pytest.mark.parametrize("case", _preprocess_cases(), ids=lambda c: c[0])
def test_preprocess_kernel(hip, dev, case):
    """Per element: |out - float64 restatement| <= 2^-8 |ref| (the bf16 rounding of the normalised value, half an ulp) + 1e-3 grey
    levels (two fp32 passes of <= 12 taps on values <= 255: ~24 roundings of 2^-24 * 255 each, two orders below) expressed in
    normalised units, 1e-3 / (255 std).  Against PIL's uint8 output the grey-level term is 1.5 (test_vision_cpu.py).  Pad columns
    are exactly zero; a sentinel band behind the output is untouched."""
    from stable_diffusion_videos_amd.vision import CLIP_IMAGE_MEAN as MEAN, CLIP_IMAGE_STD as STD, preprocess_taps
    name, frames, S, pil_out = case
    P = 14
    n, H, W, _ = frames.shape
    G, Kpad = S // P, hip.patch_kpad(P)
    rows, guard = n * G * G, 4096
    flat = torch.full((rows * Kpad + guard,), SENTINEL, dtype=BF16, device=dev)
    out = flat[:rows * Kpad].view(rows, Kpad)
    tx, ty = preprocess_taps(H, W, S)
    res = hip.clip_preprocess_patches(torch.from_numpy(frames).to(dev), tuple(t.to(dev) for t in tx), tuple(t.to(dev) for t in ty),
                                      S=S, P=P, mean=MEAN, std=STD, out=out)
    torch.cuda.synchronize()
    assert res is out
    got = flat.cpu().double()
    assert bool((got[rows * Kpad:] == SENTINEL).all()), "the kernel wrote behind its output"
    got = got[:rows * Kpad].view(rows, Kpad)
    assert float(got[:, 3 * P * P:].abs().max()) == 0.0, "pad columns must be exactly zero"
    img = unpatch_rows(got, n, S, P)
    ref = preprocess64(frames, S, MEAN, STD)
    std = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    mean = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    bound = ref.abs() * 2.0 ** -8 + 1e-3 / (255.0 * std)
    ratio = float(((img - ref).abs() / bound).max())
    grey = float(((img - ref).abs() * 255.0 * std).max())
    report(f"clip preprocess {name}: max |err| / bound {ratio:.3f} (max {grey:.4f} grey levels incl. the bf16 rounding)")
    assert ratio <= 1.0
    if pil_out is not None:
        pil = (torch.from_numpy(pil_out.astype(np.float64)).permute(0, 3, 1, 2) / 255.0 - mean) / std
        bound = pil.abs() * 2.0 ** -8 + 1.5 / (255.0 * std)
        ratio = float(((img - pil).abs() / bound).max())
        report(f"clip preprocess {name} vs PIL's uint8 output: max |err| / bound {ratio:.3f}")
        assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------
# 2 / 3. vision tower
# ------------------------------------------------------------------------------------------------
def count_bound(roundings: int) -> float:
    """oracle/blockwise.py's tolerance for a path of ``roundings`` bf16 storage roundings (``blockwise.bound`` for a count that is
    not in its table): rel-L2 <= SAFETY * EPS_BF16 * sqrt(n).  Nothing here is measured on the GPU."""
    return bw.SAFETY * bw.EPS_BF16 * math.sqrt(roundings)


def _engine(cfg, sd, dev):
    from stable_diffusion_videos_amd.vision import CLIPVisionEngine
    return CLIPVisionEngine(cfg, sd).to(dev)


def _run_tapped(eng, call):
    """``call()`` with ``vision.TAP`` recording every stage's input and output (fp32 CPU copies, pad rows dropped)"""
    from stable_diffusion_videos_amd import vision
    recs = []

    def strip(t):
        if t is None or t.dim() != 2 or t.shape[0] % eng.Tpad or t.shape[1] != eng.config.hidden_size:
            return None if t is None else t.detach().float().cpu()
        return t.detach().float().cpu().view(-1, eng.Tpad, t.shape[1])[:, :eng.T].clone()

    vision.TAP = lambda name, rec: recs.append((name, strip(rec["x"]), strip(rec["out"])))
    try:
        out = call()
        torch.cuda.synchronize()
    finally:
        vision.TAP = None
    return out, recs


def _stage_gate(label, eng, recs, sd, pixel_values):
    """The gate, as oracle/blockwise.py gates the UNet: every stage of the engine against the float64 restatement of that stage
    run on the input the ENGINE's stage saw (teacher forcing), so that what is left between them is only the bf16 roundings inside
    the stage - whose count gives the tolerance (vision_ref.STAGE_ROUNDINGS).  Returns the worst ratio rel-L2 / bound."""
    c = eng.config
    assert [r[0] for r in recs] == tower_stages(c.num_hidden_layers)
    rows = []
    for name, x, out in recs:
        ref = stage64(sd, name, pixel_values if name == "embed" else x, c.num_attention_heads, c.patch_size, c.hidden_act, c.layer_norm_eps)
        rows.append((name, bw.rel_l2(out, ref), count_bound(STAGE_ROUNDINGS[stage_kind(name)])))
    report(f"clip vision engine {label}, stage by stage (rel-L2 / count bound): " +
           ", ".join(f"{n} {r:.2e} / {b:.2e}" for n, r, b in rows))
    bad = [(n, r, b) for n, r, b in rows if not r <= b]
    assert not bad, f"stages over their rounding-count bound: {bad}"
    return max(r / b for _, r, b in rows)


def test_vision_tower_tiny_matches_transformers_fixture(hip, dev):
    """Fixture weights and pixel values (real transformers.CLIPVisionModelWithProjection), n = 1 and n = 3.

    Gate: every stage against its rounding-count bound, teacher-forced (``_stage_gate``) - where the count bound's premise (gains
    ~ 1 between the roundings, oracle/blockwise.py) holds.  The float64 stages are pinned to transformers end to end by
    tests/test_vision_cpu.py (1.5e-6).

    End to end against transformers' image_embeds the count bound SAFETY * EPS_BF16 * sqrt(19) = 1.06e-2 is NOT valid on this
    fixture: its weights are doubled (as the text fixture's), the 19 roundings are amplified on their way to the output, and
    even the ideal bf16-storage engine - the float64 restatement with exact arithmetic and one rounding at each counted place -
    sits at 1.29e-2 (n = 1) / 1.08e-2 (n = 3).  Measured engine: 1.29e-2 / 1.08e-2.  The end-to-end figure is therefore reported,
    and asserted separately against SAFETY x the ideal engine's own error (``blockwise.end_to_end_bound``'s reasoning: an engine
    whose every rounding is a correct bf16 rounding is one more draw of that error)."""
    from stable_diffusion_videos_amd import config
    z, sd = load_fixture()
    cfg = config.tiny_vision()
    eng = _engine(cfg, sd, dev)
    pv = torch.from_numpy(z["pixel_values"])
    ref = torch.from_numpy(z["image_embeds"]).double()
    outs = {}
    for n in (1, 3):
        patches = patch_rows(pv[:n], cfg.patch_size, hip.patch_kpad(cfg.patch_size)).to(BF16).to(dev)     # (bf16-exact values)
        out, recs = _run_tapped(eng, lambda: eng(patches, n))
        assert out.shape == (n, 64) and out.dtype == torch.float32
        outs[n] = out.cpu()
        _stage_gate(f"tiny fixture n={n}", eng, recs, sd, pv[:n])
        ideal = bw.rel_l2(vision_forward64(sd, pv[:n], 2, 14, store=bf16), vision_forward64(sd, pv[:n], 2, 14))
        rel = bw.rel_l2(outs[n], ref[:n])
        report(f"clip vision engine tiny n={n} vs transformers {z['transformers_version']}, end to end: rel-L2 {rel:.2e} (ideal bf16-storage "
               f"engine {ideal:.2e}; count bound {count_bound(tower_roundings(2)):.2e} - not valid end to end on doubled weights)")
        assert rel <= bw.SAFETY * ideal, "end to end: more than SAFETY x the ideal bf16-storage engine's error"
    assert torch.equal(outs[3][:1], outs[1]), "the first image of a batch of 3 must be bit-identical to the batch of 1"
    assert torch.equal(eng(patches, 3).cpu(), outs[3]), "the tap must not change the result"


@pytest.mark.parametrize("shape", ["tiny-width 26 tokens", "ViT-L width 257 tokens"])
def test_vision_tower_ragged_and_production_width(hip, dev, shape):
    """Seeded (variance-preserving) weights against the float64 restatement at token counts that are no multiple of 32 (26) / of
    the production model (257): every stage against its rounding-count bound, teacher-forced, AND the whole tower against the
    count bound of the whole path, SAFETY * EPS_BF16 * sqrt(3 + 8 layers) - with gains ~ 1 the premise holds end to end here.  The
    pad rows T ... Tpad of the embeddings poisoned with 1e4 change nothing, bit for bit."""
    from stable_diffusion_videos_amd import config, weights
    if shape.startswith("tiny"):
        cfg = config.VisionConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, image_size=70,
                                  projection_dim=64)
    else:
        cfg = config.VisionConfig(num_hidden_layers=1)
    sd = weights.synthetic_safety_checker(cfg, seed=21)
    eng = _engine(cfg, sd, dev)
    n, S, P = 2, cfg.image_size, cfg.patch_size
    assert eng.T == cfg.num_tokens == (26 if S == 70 else 257) and eng.Tpad == (32 if S == 70 else 288)
    g = torch.Generator().manual_seed(4)
    pv = torch.randn((n, 3, S, S), generator=g).to(BF16).float()
    patches = patch_rows(pv, P, hip.patch_kpad(P)).to(BF16).to(dev)
    x = None

    def call():
        nonlocal x
        x = eng.embed(patches, n)
        return eng.encode(x.clone(), n)

    out, recs = _run_tapped(eng, call)
    tower = {k: v for k, v in sd.items() if k not in weights.SAFETY_HEAD_KEYS}
    _stage_gate(shape, eng, recs, tower, pv)
    exact = vision_forward64(tower, pv, cfg.num_attention_heads, P)
    rel, tol = bw.rel_l2(out.cpu(), exact), count_bound(tower_roundings(cfg.num_hidden_layers))
    report(f"clip vision engine {shape}, end to end: rel-L2 {rel:.2e} vs float64 (count bound {tol:.2e})")
    assert rel <= tol
    xv = x.view(n, eng.Tpad, cfg.hidden_size)
    assert float(xv[:, eng.T:].abs().max()) == 0.0
    xv[:, eng.T:] = 1e4
    again = eng.encode(x, n)
    torch.cuda.synchronize()
    assert torch.equal(again, out), "pad rows reached the result"


# ------------------------------------------------------------------------------------------------
# 4. screen kernel
# ------------------------------------------------------------------------------------------------
def test_safety_screen_kernel(hip, dev):
    D, n = 768, 5
    g = torch.Generator().manual_seed(12)
    c, s = torch.randn((17, D), generator=g), torch.randn((3, D), generator=g)
    e = torch.stack([torch.randn(D, generator=g), torch.randn(D, generator=g),     # 0, 1: nothing near a threshold
                     s[1] + c[5],                                                   # 2: special-care hit; concept 5 tipped by the 0.01 only
                     c[9].clone(),                                                  # 3: a plain concept hit
                     s[0].clone()])                                                 # 4: special-care hit that tips nothing
    thr_c, thr_s = torch.full((17,), 0.5), torch.full((3,), 0.5)
    cos25 = float(torch.nn.functional.cosine_similarity(e[2].double(), c[5].double(), dim=0))
    thr_c[5] = cos25 + 0.005                                                        # concept[2, 5] = -0.005 + 0.01 = +0.005
    ref_flags, ref_scores = safety_head64(e, c, s, thr_c, thr_s)
    assert ref_flags.tolist() == [False, False, True, True, False]
    assert float(ref_scores[2, 3:].max()) == float(ref_scores[2, 3 + 5]) and 0.004 < float(ref_scores[2, 8]) < 0.006
    rng = np.random.RandomState(5)
    frames = torch.from_numpy(rng.randint(1, 256, (n, 10, 7, 3)).astype(np.uint8))      # 210 bytes a frame: 16-byte pieces straddle frames
    dv = [t.to(dev) for t in (e, c, s, thr_c, thr_s)]
    fr = frames.to(dev)
    flags, scores = hip.safety_screen(*dv, fr)
    torch.cuda.synchronize()
    err = float((scores.cpu().double() - ref_scores).abs().max())
    margin = float(ref_scores.abs().min())
    report(f"safety screen: max score error {err:.2e} (fp32 cosine), smallest |score| {margin:.2e}")
    assert margin >= 100.0 * err, "a constructed score sits too close to 0 for the flags to be decided by fp32"
    assert err <= 1e-5
    assert flags.dtype == torch.int32 and flags.cpu().bool().tolist() == ref_flags.tolist()
    out = fr.cpu()
    for i in range(n):
        if ref_flags[i]:
            assert int(out[i].max()) == 0, i
        else:
            assert torch.equal(out[i], frames[i]), i
    # n = 1, flagged and not; without frames only the head runs
    for i in (3, 0):
        f1 = frames[i:i + 1].to(dev)
        fl, sc = hip.safety_screen(dv[0][i:i + 1].contiguous(), *dv[1:], f1)
        assert bool(fl.cpu()[0]) == bool(ref_flags[i]) and float((sc.cpu().double() - ref_scores[i:i + 1]).abs().max()) <= 1e-5
        assert int(f1.max()) == 0 if ref_flags[i] else torch.equal(f1.cpu(), frames[i:i + 1])
    fl, _ = hip.safety_screen(*dv, None)
    assert fl.cpu().bool().tolist() == ref_flags.tolist()


# ------------------------------------------------------------------------------------------------
# 5. pipeline
# ------------------------------------------------------------------------------------------------
def test_pipeline_with_safety_checker(hip, dev, tmp_path):
    from PIL import Image
    from stable_diffusion_videos_amd import SafetyCheckerEngine, StableDiffusionWalkPipeline as P
    plain = P.from_pretrained("tiny").to(dev)
    pipe = P.from_pretrained("tiny", safety_checker=True).to(dev)
    eng = pipe.safety_checker
    assert isinstance(eng, SafetyCheckerEngine) and pipe.feature_extractor is eng.feature_extractor
    B = 2

    def run(p, output_type):
        emb = torch.cat([p.embed_text("a cat"), p.embed_text("a dog")])
        lat = torch.cat([p.init_noise(5, (1, 4, 8, 8)), p.init_noise(6, (1, 4, 8, 8))])
        return p(text_embeddings=emb, latents=lat, height=64, width=64, num_inference_steps=2, output_type=output_type)

    ref_u8 = run(plain, "numpy_u8")
    ref_np = run(plain, "np")
    assert ref_u8.nsfw_content_detected is None and int(ref_u8.images.max()) > 0
    # flag all
    eng.concept_thresholds.fill_(-1.0)
    out = run(pipe, "pil")
    assert out.nsfw_content_detected == [True] * B and len(out.images) == B
    assert all(isinstance(im, Image.Image) and np.asarray(im).shape == (64, 64, 3) and int(np.asarray(im).max()) == 0 for im in out.images)
    out = run(pipe, "np")
    assert out.nsfw_content_detected == [True] * B and out.images.shape == (B, 64, 64, 3) and float(np.abs(out.images).max()) == 0.0
    image, has = pipe(text_embeddings=pipe.embed_text("a cat"), latents=pipe.init_noise(5, (1, 4, 8, 8)), height=64, width=64,
                      num_inference_steps=2, output_type="numpy_u8", return_dict=False)
    assert has == [True] and int(image.max()) == 0
    pipe.make_clip_frames("a cat", "a dog", 1, 2, num_interpolation_steps=2, save_path=tmp_path / "clip", num_inference_steps=2,
                          height=64, width=64, batch_size=2)
    files = sorted((tmp_path / "clip").glob("frame*.png"))
    assert len(files) == 2 and all(int(np.asarray(Image.open(f)).max()) == 0 for f in files)
    # flag none: the frames are the checker-less pipeline's, byte for byte
    eng.concept_thresholds.fill_(1.0)
    eng.special_care_thresholds.fill_(1.0)
    out = run(pipe, "numpy_u8")
    assert out.nsfw_content_detected == [False] * B and np.array_equal(out.images, ref_u8.images)
    out = run(pipe, "np")
    assert out.nsfw_content_detected == [False] * B and np.array_equal(out.images, ref_np.images)
    # the reference's call shape of the checker itself (:442-447)
    imgs, has = eng(images=ref_np.images, clip_input=None)
    assert has == [False] * B and np.array_equal(imgs, ref_np.images)
    eng.concept_thresholds.fill_(-1.0)
    imgs, has = eng(images=ref_np.images, clip_input=None)
    assert has == [True] * B and float(np.abs(imgs).max()) == 0.0
    flags, scores = eng(torch.from_numpy(ref_u8.images).to(dev))
    assert flags.dtype == torch.bool and flags.tolist() == [True] * B and tuple(scores.shape) == (B, 20)
