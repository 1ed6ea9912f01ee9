"""Network- and pipeline-level parity of the HIP path against the CPU oracle (same bf16-exact synthetic
weights, same seeded inputs), plus the API-shape tests that mirror the reference's own three tests
(/root/reference/tests/test_pipeline.py:41-81: they assert only that the output exists).

Stated tolerances (bf16 HIP path vs fp32 oracle; SURVEY.md 8c ladder - "parity unpinned" for these
networks because diffusers cannot be run to pin the oracle).  Every gate sits 3 dB under the value measured on
MI355X (profiles/round2_parity_report.txt), so a regression that doubles the error fails:
  * one UNet forward            PSNR >= 46 dB on eps (peak = max |eps_oracle|; measured 48.5 - 49.7)
  * VAE decode                  PSNR >= 45.5 dB on the [0,1] image (measured 48.6 / 49.8), uint8 max-abs reported
  * full frame, 2 - 10 steps    PSNR >= 39 dB on the image (measured 42.0 - 43.4)
  * BASELINE config 1, 50 steps see test_baseline_config1_50_steps_vs_golden
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import bf16_round, psnr, rel_l2, report
from helpers import unet_pair, vae_pair

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def _unet_io(c, nimg, h, w, Lc, seed):
    g = torch.Generator().manual_seed(seed)
    x = bf16_round(torch.randn((nimg, c.in_channels, h, w), generator=g))
    ctx = bf16_round(torch.randn((nimg, Lc, c.cross_attention_dim), generator=g))
    return x, ctx


def _run_unet(engine, x, ctx, timesteps, step_index, dev):
    nimg, _, h, w = x.shape
    engine.prepare_timesteps(timesteps)
    engine.prepare_context(ctx.to(dev))
    step = torch.tensor([step_index], dtype=torch.int32, device=dev)
    x2 = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).to(dev, BF16).contiguous()
    eps = engine.forward(x2, nimg, h, w, step)
    torch.cuda.synchronize()
    return eps.permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("tiled", [False, True])
def test_tiny_unet_forward(hip, dev, tiled):
    from stable_diffusion_videos_amd import config as cfgs
    c = cfgs.tiny_unet()
    oracle, engine = unet_pair(c, dev, tiled=tiled)
    if tiled:
        for m in oracle.modules():
            if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3):
                m.padding_mode = "circular"
                m._reversed_padding_repeated_twice = (1, 1, 1, 1)
    x, ctx = _unet_io(c, 2, 16, 16, 77, 0)
    ts = [981, 501, 21]
    got = _run_unet(engine, x, ctx, ts, 1, dev)
    with torch.no_grad():
        ref = oracle(x, torch.tensor(501), ctx)
    p = psnr(got, ref)
    report(f"tiny unet (tiled={tiled}) eps PSNR {p:.1f} dB, rel-L2 {rel_l2(got, ref):.2e}")
    assert p >= (45.5 if tiled else 46.5)


def test_sd14_unet_forward_small_latent(hip, dev):
    """The real SD-v1-4 UNet architecture (859.52 M parameters, all channel widths / head sizes) on a
    16x16 latent so the CPU oracle finishes in seconds."""
    from stable_diffusion_videos_amd import config as cfgs
    c = cfgs.sd14_unet()
    oracle, engine = unet_pair(c, dev)
    x, ctx = _unet_io(c, 2, 16, 16, 77, 1)
    got = _run_unet(engine, x, ctx, [981, 961], 0, dev)
    with torch.no_grad():
        ref = oracle(x, torch.tensor(981), ctx)
    p = psnr(got, ref)
    report(f"SD-1.4 unet eps PSNR {p:.1f} dB, rel-L2 {rel_l2(got, ref):.2e}, |eps|max {float(ref.abs().max()):.3f}")
    assert p >= 46.5


def test_sd21_unet_forward_small_latent(hip, dev):
    """SD-2.1 variant: 64-wide heads, linear projections, 1024-d text context."""
    from stable_diffusion_videos_amd import config as cfgs
    c = cfgs.sd21_unet()
    oracle, engine = unet_pair(c, dev)
    x, ctx = _unet_io(c, 1, 16, 16, 77, 2)
    got = _run_unet(engine, x, ctx, [981], 0, dev)
    with torch.no_grad():
        ref = oracle(x, torch.tensor(981), ctx)
    p = psnr(got, ref)
    report(f"SD-2.1 unet eps PSNR {p:.1f} dB")
    assert p >= 46.5


def test_sd14_unet_forward_fp8_convs(hip, dev):
    """BASELINE config 5 ("SD-v1-4 fp8 (CDNA4 fp8 MFMA)"): the SD-v1-4 UNet with e4m3 operands in its 44 ResBlock convolutions
    (per-tensor scales, calibrated on the first forward) against the fp32 oracle AND against the bf16 HIP path on the same
    inputs - the parity ladder of the fp8 mode, stated in dB."""
    from stable_diffusion_videos_amd import config as cfgs
    c = cfgs.sd14_unet()
    oracle, eng8 = unet_pair(c, dev, fp8=True)
    _, eng16 = unet_pair(c, dev)
    x, ctx = _unet_io(c, 2, 16, 16, 77, 1)
    got8 = _run_unet(eng8, x, ctx, [981, 961], 0, dev)       # first call calibrates the activation scales
    got8b = _run_unet(eng8, x, ctx, [981, 961], 0, dev)
    got16 = _run_unet(eng16, x, ctx, [981, 961], 0, dev)
    with torch.no_grad():
        ref = oracle(x, torch.tensor(981), ctx)
    assert torch.equal(got8, got8b)
    p8, p16, p816 = psnr(got8, ref), psnr(got16, ref), psnr(got8, got16, peak=float(ref.abs().max()))
    report(f"SD-1.4 unet, fp8 ResBlock convs: eps PSNR {p8:.1f} dB vs oracle (bf16 path {p16:.1f} dB), {p816:.1f} dB vs the bf16 path")
    assert p8 >= 33.5          # measured 36.7 dB (the bf16 path: 49.6 dB)


@pytest.mark.parametrize("arch", ["tiny", "sd"])
def test_vae_decode(hip, dev, arch):
    from oracle.pipeline import decode_latents, numpy_to_uint8
    from stable_diffusion_videos_amd import config as cfgs
    c = cfgs.tiny_vae() if arch == "tiny" else cfgs.sd_vae()
    oracle, engine = vae_pair(c, dev)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn((2, 4, 8, 8), generator=g) * 0.18215 * 0.6
    ref = decode_latents(oracle, lat)                                   # fp32 NHWC [0,1]
    u8, f32 = engine.decode(lat.permute(0, 2, 3, 1).contiguous().to(dev), want_float=True)
    torch.cuda.synchronize()
    got = f32.cpu().numpy()
    p = psnr(torch.from_numpy(got), torch.from_numpy(ref), peak=1.0)
    d8 = np.abs(u8.cpu().numpy().astype(int) - numpy_to_uint8(ref).astype(int))
    report(f"{arch} vae image PSNR {p:.1f} dB, uint8 max-abs {d8.max()}, mean-abs {d8.mean():.3f}, "
          f"dynamic range [{ref.min():.2f},{ref.max():.2f}] std {ref.std():.3f}")
    assert got.shape == ref.shape == (2, 64, 64, 3)
    assert p >= (45.5 if arch == "tiny" else 46.5) and d8.max() <= 10
    assert np.array_equal(u8.cpu().numpy(), (got * 255).round().astype("uint8"))


def test_vae_attention_score_chunks_are_exact(hip, dev):
    """The VAE mid-block attention materialises its scores a few images at a time (engine.score_chunk_bytes): any chunking
    gives the same bits."""
    from stable_diffusion_videos_amd import config as cfgs
    _, engine = vae_pair(cfgs.tiny_vae(), dev)
    lat = (torch.randn((5, 8, 8, 4), generator=torch.Generator().manual_seed(9)) * 0.1).to(dev)
    ref, _ = engine.decode(lat)
    for chunk_images in (1, 2, 4):
        engine.score_chunk_bytes = chunk_images * 6 * 64 * 64      # fp32 scores + bf16 probabilities of one 64-pixel image
        got, _ = engine.decode(lat)
        assert torch.equal(got, ref), chunk_images


def _tiny_pipeline(dev, **kw):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    return StableDiffusionWalkPipeline.from_pretrained("tiny", **kw).to(dev)


def _oracle_for(pipe_cpu_state):
    from helpers import make_oracle_unet, make_oracle_vae
    u, v = pipe_cpu_state
    return make_oracle_unet(u.config, u.state_dict), make_oracle_vae(v.config, v.state_dict)


def test_pipeline_call_matches_oracle(hip, dev):
    """__call__ with latents= and text_embeddings= (how make_clip_frames invokes it) vs the oracle's
    restatement of stable_diffusion_pipeline.py:308-438, 10 DDIM steps, CFG 7.5, with and without graphs."""
    from oracle.pipeline import denoise_and_decode, numpy_to_uint8
    from oracle.scheduler import DDIMScheduler as OracleDDIM
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    o_unet, o_vae = _oracle_for((pipe.unet, pipe.vae))
    pipe.to(dev)
    emb = pipe.embed_text(["a cat", "a dog"]).cpu()
    uncond = pipe.embed_text("").cpu()
    lat = torch.cat([pipe.init_noise(42, (1, 4, 8, 8)), pipe.init_noise(1337, (1, 4, 8, 8))]).cpu()
    ref = denoise_and_decode(o_unet, o_vae, OracleDDIM(), emb, uncond, lat, num_inference_steps=10, guidance_scale=7.5)
    ref8 = numpy_to_uint8(ref)
    outs = {}
    for graphs in (True, False):
        pipe.use_graphs = graphs
        pipe._graphs.clear()
        out = pipe(latents=lat, text_embeddings=emb, height=64, width=64, num_inference_steps=10, guidance_scale=7.5,
                   output_type="numpy")["images"]
        outs[graphs] = out
        p = psnr(torch.from_numpy(out), torch.from_numpy(ref), peak=1.0)
        d8 = np.abs((out * 255).round().astype(int) - ref8.astype(int))
        report(f"pipeline (graphs={graphs}) frame PSNR {p:.1f} dB, uint8 max-abs {d8.max()} mean-abs {d8.mean():.3f}")
        assert out.shape == (2, 64, 64, 3) and p >= 40.0
    assert np.array_equal(outs[True], outs[False]), "hipGraph replay must equal eager launches bit-for-bit"
    # latents after the loop (before the VAE), which is where chained-step error shows
    lat_ref = denoise_and_decode(o_unet, o_vae, OracleDDIM(), emb, uncond, lat, 10, 7.5, return_latents=True)
    lat_got = pipe(latents=lat, text_embeddings=emb, height=64, width=64, num_inference_steps=10, guidance_scale=7.5,
                   return_latents=True).cpu()
    report(f"latents after 10 steps: PSNR {psnr(lat_got, lat_ref):.1f} dB")
    assert psnr(lat_got, lat_ref) >= 40.5
    # PIL output type and no-CFG path
    ims = pipe(latents=lat[:1], text_embeddings=emb[:1], height=64, width=64, num_inference_steps=3, guidance_scale=1.0).images
    assert len(ims) == 1 and ims[0].size == (64, 64)


@pytest.mark.parametrize("name", ["PNDMScheduler", "LMSDiscreteScheduler", "EulerDiscreteScheduler", "DPMSolverMultistepScheduler",
                                  "EulerAncestralDiscreteScheduler"])
def test_pipeline_with_the_other_schedulers(hip, dev, name):
    """The reference's constructor accepts six schedulers (stable_diffusion_pipeline.py:71-78; SD-v1 checkpoints ship PNDM,
    examples/make_music_video.py:15 passes LMSDiscrete): __call__ with each of them - hipGraph replay of UNet +
    ``sdv_cfg_multistep_step`` per evaluation - against the oracle's restated loop (:412-430) with the oracle's classic
    scheduler of the same name, 8 steps, CFG 7.5.  Same gates as the DDIM test (frame >= 40 dB); graphs == eager bit for bit."""
    from oracle import scheduler as O
    from oracle.pipeline import denoise_and_decode
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd import scheduler as P
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny", scheduler=getattr(P, name)())
    o_unet, o_vae = _oracle_for((pipe.unet, pipe.vae))
    pipe.to(dev)
    emb = pipe.embed_text(["a cat", "a dog"]).cpu()
    uncond = pipe.embed_text("").cpu()
    lat = torch.cat([pipe.init_noise(42, (1, 4, 8, 8)), pipe.init_noise(1337, (1, 4, 8, 8))]).cpu()
    steps = 8
    osch = getattr(O, name)()
    osch.set_timesteps(steps)
    noise = None
    kw = {}
    if pipe.scheduler.stochastic:
        gen = torch.Generator().manual_seed(5)
        noise = torch.randn((steps, 2, 8, 8, 4), generator=gen)            # [evaluation, B, h, w, C] as the pipeline draws it
        kw["generator"] = torch.Generator().manual_seed(5)
    ref = denoise_and_decode(o_unet, o_vae, osch, emb, uncond, lat, num_inference_steps=steps, guidance_scale=7.5,
                             variance_noise=[z.permute(0, 3, 1, 2) for z in noise] if noise is not None else None)
    outs = {}
    for graphs in (True, False):
        pipe.use_graphs = graphs
        pipe._graphs.clear()
        if "generator" in kw:
            kw["generator"] = torch.Generator().manual_seed(5)
        outs[graphs] = pipe(latents=lat, text_embeddings=emb, height=64, width=64, num_inference_steps=steps, guidance_scale=7.5,
                            output_type="numpy", **kw)["images"]
    p = psnr(torch.from_numpy(outs[True]), torch.from_numpy(ref), peak=1.0)
    report(f"pipeline with {name}: {len(osch.timesteps)} UNet evaluations, frame PSNR {p:.1f} dB vs the oracle loop")
    # What this test guards is the WIRING of the scheduler into the loop (timesteps, init_noise_sigma, scale_model_input, history,
    # PLMS's repeated evaluation): any mistake there lands below 25 dB.  The step arithmetic itself is gated at 2e-5 in
    # test_cfg_multistep_step_matches_oracle, the UNet / VAE precision block by block in test_blockwise_gpu.py.  Measured
    # 39.9 (EulerAncestral, which re-injects noise every step) ... 43 dB.
    assert outs[True].shape == (2, 64, 64, 3) and p >= 35.0
    assert np.array_equal(outs[True], outs[False])
    seen = []
    pipe(latents=lat[:1], text_embeddings=emb[:1], height=64, width=64, num_inference_steps=steps,
         callback=lambda i, t, l: seen.append((i, float(t))), **({"generator": torch.Generator().manual_seed(5)} if kw else {}))
    assert [t for _, t in seen] == [float(t) for t in osch.timesteps]      # callback(i, t, latents) per evaluation, :429-430


def test_generate_inputs_matches_reference_semantics(hip, dev):
    """lerp on embeddings, whole-tensor slerp on noise, batches of batch_size with a short last batch
    (stable_diffusion_pipeline.py:464-479), against the oracle restatement."""
    from oracle import interp
    pipe = _tiny_pipeline(dev)
    T = np.linspace(0.0, 1.0, 5)
    ea, eb = pipe.embed_text("a cat").cpu(), pipe.embed_text("a dog").cpu()
    la, lb = interp.init_noise(42, (1, 4, 8, 8)), interp.init_noise(1337, (1, 4, 8, 8))
    ref = list(interp.generate_inputs(ea, eb, la, lb, T, 2))
    got = list(pipe.generate_inputs("a cat", "a dog", 42, 1337, (1, 4, 8, 8), T, 2))
    assert [g[0] for g in got] == [r[0] for r in ref] == [0, 1, 2]
    assert [tuple(g[1].shape) for g in got] == [tuple(r[1].shape) for r in ref]
    for (_, e, n), (_, er, nr) in zip(got, ref):
        assert float((e.cpu() - er).abs().max()) < 1e-5
        assert float((n.cpu() - nr).abs().max()) < 2e-5
    assert torch.equal(got[0][2][0].cpu(), la[0]) and torch.equal(got[2][2][0].cpu(), lb[0])   # t=0 / t=1 exact


def test_walk_basic_layout(hip, dev, tmp_path):
    """Mirror of the reference's test_walk_basic (tests/test_pipeline.py:41-50) plus the on-disk contract
    of walk's docstring (:648-666) and prompt_config.json (:694-714)."""
    pipe = _tiny_pipeline(dev)
    ret = pipe.walk(["a cat", "a dog", "a horse"], seeds=[42, 1337, 2022], num_interpolation_steps=[3, 3],
                    output_dir=str(tmp_path), name="basic", fps=3, num_inference_steps=4, height=64, width=64,
                    make_video=False)
    assert ret is None
    root = tmp_path / "basic"
    cfg = json.loads((root / "prompt_config.json").read_text())
    assert list(cfg) == ["prompts", "seeds", "num_interpolation_steps", "fps", "num_inference_steps", "guidance_scale",
                         "eta", "upsample", "height", "width", "audio_filepath", "audio_start_sec", "negative_prompt"]
    assert cfg["num_interpolation_steps"] == [3, 3] and cfg["audio_start_sec"] == 0
    from PIL import Image
    for i in range(2):
        frames = sorted((root / f"basic_{i:06d}").glob("*.png"))
        assert [f.name for f in frames] == [f"frame{k:06d}.png" for k in range(3)]
        assert Image.open(frames[0]).size == (64, 64)
    # T = linspace(0,1,n) has inclusive endpoints: last frame of clip 0 == first frame of clip 1
    a = np.asarray(Image.open(root / "basic_000000" / "frame000002.png"))
    b = np.asarray(Image.open(root / "basic_000001" / "frame000000.png"))
    assert np.array_equal(a, b)


def test_walk_resume_and_batching(hip, dev, tmp_path):
    """resume=True reloads prompt_config.json and continues after the last frame on disk (:741-753), and a
    batched run writes the same frames as batch_size=1."""
    from PIL import Image
    pipe = _tiny_pipeline(dev)
    kw = dict(output_dir=str(tmp_path), fps=3, num_inference_steps=3, height=64, width=64, make_video=False)
    pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=5, name="full", batch_size=1, **kw)
    pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=5, name="batched", batch_size=4, **kw)
    for k in range(5):
        a = np.asarray(Image.open(tmp_path / "full" / "full_000000" / f"frame{k:06d}.png")).astype(int)
        b = np.asarray(Image.open(tmp_path / "batched" / "batched_000000" / f"frame{k:06d}.png")).astype(int)
        assert np.abs(a - b).max() <= 2, k       # different GEMM tile shapes at different batch sizes
    # knock out the last three frames and resume
    for k in (2, 3, 4):
        (tmp_path / "full" / "full_000000" / f"frame{k:06d}.png").rename(tmp_path / f"keep{k}.png")
    pipe.walk(name="full", resume=True, batch_size=1, **kw)
    for k in (2, 3, 4):
        a = np.asarray(Image.open(tmp_path / "full" / "full_000000" / f"frame{k:06d}.png"))
        b = np.asarray(Image.open(tmp_path / f"keep{k}.png"))
        assert np.array_equal(a, b), k


def test_call_argument_errors(hip, dev):
    """Error behaviour of the reference __call__ / make_clip_frames (SURVEY.md 8b 'Errors')."""
    pipe = _tiny_pipeline(dev)
    emb = pipe.embed_text("a cat")
    with pytest.raises(ValueError, match="divisible by 8"):
        pipe(text_embeddings=emb, height=60, width=64)
    with pytest.raises(ValueError, match="callback_steps"):
        pipe(text_embeddings=emb, height=64, width=64, callback_steps=0)
    with pytest.raises(ValueError, match="`prompt` has to be of type"):
        pipe(prompt=3, height=64, width=64)
    with pytest.raises(ValueError, match="Unexpected latents shape"):
        pipe(text_embeddings=emb, latents=torch.zeros(1, 4, 9, 8), height=64, width=64)
    with pytest.raises(ValueError, match="Unexpected T shape"):
        pipe.make_clip_frames("a", "b", 0, 1, num_interpolation_steps=4, T=np.linspace(0, 1, 3), height=64, width=64)
    with pytest.raises(TypeError):
        pipe(prompt="a cat", negative_prompt=["x"], height=64, width=64)
    seen = []
    pipe(text_embeddings=emb, height=64, width=64, num_inference_steps=4, callback=lambda i, t, l: seen.append((i, t, tuple(l.shape))),
         callback_steps=2)
    assert seen == [(0, 751, (1, 4, 8, 8)), (2, 251, (1, 4, 8, 8))]


def test_sd14_full_size_two_steps(hip, dev):
    """BASELINE config geometry - SD-v1-4 architecture at 512x512 (64x64 latent, 4096-token attention), CFG 7.5 -
    for one frame and 2 DDIM steps, against the CPU oracle (~15 s of oracle time)."""
    from oracle.pipeline import denoise_and_decode, numpy_to_uint8
    from oracle.scheduler import DDIMScheduler as OracleDDIM
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("CompVis/stable-diffusion-v1-4", arch="sd14")
    o_unet, o_vae = _oracle_for((pipe.unet, pipe.vae))
    pipe.to(dev)
    emb = pipe.embed_text("a cat").cpu()
    uncond = pipe.embed_text("").cpu()
    lat = pipe.init_noise(42, (1, 4, 64, 64)).cpu()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = denoise_and_decode(o_unet, o_vae, OracleDDIM(), emb, uncond, lat, num_inference_steps=2, guidance_scale=7.5)
    out = pipe(latents=lat, text_embeddings=emb, num_inference_steps=2, guidance_scale=7.5, output_type="numpy")["images"]
    p = psnr(torch.from_numpy(out), torch.from_numpy(ref), peak=1.0)
    d8 = np.abs((out * 255).round().astype(int) - numpy_to_uint8(ref).astype(int))
    report(f"SD-1.4 512x512, 2 steps, CFG: frame PSNR {p:.1f} dB, uint8 max-abs {d8.max()} mean-abs {d8.mean():.3f}")
    assert out.shape == (1, 512, 512, 3) and p >= 39.0


def test_baseline_config1_50_steps_vs_golden(hip, dev, tmp_path):
    """BASELINE.json configs[0] through the HIP path, against the committed CPU-oracle fixture
    tests/golden/config1_sd14_50steps.npz (tests/golden/make_golden_config1.py: 22 minutes of fp32 PyTorch-eager):

        walk(['a cat', 'a dog'], seeds=[42, 1337], num_interpolation_steps=3, 512x512, 50 DDIM steps, CFG 7.5)
            /root/reference/stable_diffusion_videos/stable_diffusion_pipeline.py:556 -> :481 -> :457-479 -> :412-438

    Three granularities, each with its stated tolerance (bf16 HIP path vs fp32 oracle; with seeded random-init weights the
    guided loop AMPLIFIES - the latents grow from std 1 to std 18 over the 50 steps - so this is a harsher chain than a
    trained UNet, whose iterates contract towards the data manifold):
      1. the two prompt embeddings (native CLIP engine)                                  PSNR >= CLIP_DB
      2. the 50-step loop on the fixture's own interpolated inputs: latents after steps 1 / 10 / 25 / 50
      3. the full walk() (HIP text encoder, lerp / slerp kernels, loop, VAE, PNG files): uint8 frames, PSNR + max/mean |d|"""
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    d = np.load(Path(__file__).resolve().parent / "golden" / "config1_sd14_50steps.npz")
    pipe = StableDiffusionWalkPipeline.from_pretrained("CompVis/stable-diffusion-v1-4", arch="sd14").to(dev)
    # 1. endpoints
    emb = pipe.embed_text(["a cat", "a dog"]).cpu()
    p_emb = psnr(emb, torch.from_numpy(d["prompt_embeds"]))
    report(f"config1: prompt embeddings PSNR {p_emb:.1f} dB")
    assert p_emb >= CONFIG1_MIN["embeds_db"]
    # 2. the chained loop on the oracle's own inputs
    snaps = {}
    lat = pipe(latents=torch.from_numpy(d["noise"]), text_embeddings=torch.from_numpy(d["embeds"]), num_inference_steps=50,
               guidance_scale=7.5, return_latents=True,
               callback=lambda i, t, l: snaps.__setitem__(i + 1, l.cpu()) if i + 1 in (1, 10, 25) else None).cpu()
    snaps[50] = lat
    for k in (1, 10, 25, 50):
        ref = torch.from_numpy(d[f"latents_step{k}"])
        pk = psnr(snaps[k], ref)
        report(f"config1: latents after step {k:2d}: PSNR {pk:.1f} dB (peak {float(ref.abs().max()):.1f}), "
               f"rel-L2 {rel_l2(snaps[k], ref):.2e}")
        assert pk >= CONFIG1_MIN[f"lat{k}_db"], k
    # 3. the walk itself, files and all
    pipe.walk(["a cat", "a dog"], seeds=[42, 1337], num_interpolation_steps=3, output_dir=str(tmp_path), name="c1",
              batch_size=3, make_video=False)
    got = np.stack([np.asarray(Image.open(tmp_path / "c1" / "c1_000000" / f"frame{k:06d}.png")) for k in range(3)])
    ref8 = d["frames_u8"]
    assert got.shape == ref8.shape == (3, 512, 512, 3)
    diff = np.abs(got.astype(np.int32) - ref8.astype(np.int32))
    mse = float((diff.astype(np.float64) ** 2).mean())
    p_img = 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))
    report(f"config1: walk() frames vs oracle: PSNR {p_img:.1f} dB, uint8 max|d| {int(diff.max())}, mean|d| {diff.mean():.3f}, "
           f"p99|d| {int(np.percentile(diff, 99))}; per frame " + ", ".join(f"{10 * np.log10(255.0 ** 2 / max(float((diff[k].astype(np.float64) ** 2).mean()), 1e-12)):.1f}" for k in range(3)))
    assert p_img >= CONFIG1_MIN["frames_db"]
    assert diff.mean() <= CONFIG1_MIN["frames_mean_abs"]


# thresholds = measured - 3 dB (profiles/round2_parity_report.txt: embeddings 53.7 dB; latents 57.2 / 52.0 / 51.6 / 51.8 dB after
# steps 1 / 10 / 25 / 50; frames 47.4 dB, uint8 max |d| 7, mean |d| 0.75)
CONFIG1_MIN = {"embeds_db": 50.5, "lat1_db": 54.0, "lat10_db": 49.0, "lat25_db": 48.5, "lat50_db": 48.5, "frames_db": 44.0,
               "frames_mean_abs": 1.5}


def test_baseline_config5_fp8_50_steps_vs_golden(hip, dev, tmp_path):
    """BASELINE.json configs[4] ("SD-v1-4 fp8 (CDNA4 fp8 MFMA)") on the config-1 fixture: ``from_pretrained(fp8=True)`` through
    walk() - pilot calibration of the e4m3 activation scales, hipGraph capture, 50 steps, VAE, PNG files - against the fp32
    oracle's frames.  Acceptance (stated before measuring, SURVEY.md 8c ladder step 4): frame PSNR >= 30 dB against the fp32
    oracle; the measured PSNR, max / mean / p99 |d| on the uint8 image and the distance to the bf16 path's frames are reported.
    Also the ADVICE r2 regression: the scales must come from the pilot run (identical for a second pipeline object, finite,
    non-zero), not from the zero-filled graph warm-up."""
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    d = np.load(Path(__file__).resolve().parent / "golden" / "config1_sd14_50steps.npz")
    ref8 = d["frames_u8"]
    frames = {}
    for mode in ("fp8", "bf16"):
        pipe = StableDiffusionWalkPipeline.from_pretrained("CompVis/stable-diffusion-v1-4", arch="sd14", fp8=mode == "fp8").to(dev)
        assert pipe.use_graphs
        if mode == "fp8":
            pipe.enable_fp8_saturation_check()       # count what the e4m3 conversions clamp
        pipe.walk(["a cat", "a dog"], seeds=[42, 1337], num_interpolation_steps=3, output_dir=str(tmp_path), name=mode,
                  batch_size=3, make_video=False)
        frames[mode] = np.stack([np.asarray(Image.open(tmp_path / mode / f"{mode}_000000" / f"frame{k:06d}.png")) for k in range(3)])
        if mode == "fp8":
            scales = pipe.unet.fp8_scales()
            assert pipe.unet.fp8_calibrated and len(scales) == 22
            assert all(np.isfinite(a) and np.isfinite(b) and a > 1e-4 and b > 1e-4 for a, b in scales)
            # the pilot ran under (empty prompt, the walk's first prompt) with 2 x head-room: nothing was clamped at +-448 in the
            # pilot itself or in the 3 x 50 captured steps of the walk (hash-tokenised random-init weights: this guards the plumbing -
            # counter wired into eager AND captured launches, scales cover both guidance halves - not a trained model's outliers)
            assert pipe.fp8_saturated() == 0
            # the pilot is batch- / rank-independent: a direct call on different inputs leaves the scales alone
            pipe(prompt="a horse", num_inference_steps=50, height=512, width=512, output_type="numpy_u8")
            assert pipe.unet.fp8_scales() == scales
            assert pipe.fp8_saturated() == 0
            # ... and the counter does count: the same call with every activation scale cut to a fiftieth (2 x head-room gone 25 times over) clamps plenty
            pipe.unet.set_fp8_scales([(a * 0.02, b * 0.02) for a, b in scales])
            pipe._graphs.clear()                      # (captured launches bake alpha = sx * sw in)
            pipe(prompt="a horse", num_inference_steps=2, height=512, width=512, output_type="numpy_u8")
            assert pipe.fp8_saturated() > 0
            pipe.enable_fp8_saturation_check(False)
        del pipe
        torch.cuda.empty_cache()

    def stats(a, b):
        diff = np.abs(a.astype(np.int32) - b.astype(np.int32))
        mse = float((diff.astype(np.float64) ** 2).mean())
        return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12)), int(diff.max()), float(diff.mean()), int(np.percentile(diff, 99))

    p8, mx8, mean8, p99_8 = stats(frames["fp8"], ref8)
    p16, mx16, mean16, _ = stats(frames["bf16"], ref8)
    p816, mx816, mean816, _ = stats(frames["fp8"], frames["bf16"])
    report(f"config5 (fp8 ResBlock convs, 50 steps, 512x512, walk()): frames vs fp32 oracle PSNR {p8:.1f} dB, uint8 max|d| {mx8}, "
           f"mean|d| {mean8:.3f}, p99|d| {p99_8}  (bf16 path: {p16:.1f} dB, max {mx16}, mean {mean16:.3f}); "
           f"fp8 vs bf16 path {p816:.1f} dB, max {mx816}, mean {mean816:.3f}")
    assert p8 >= 30.0


def test_sd21_768_two_steps_with_audio_schedule(hip, dev):
    """BASELINE config 4 geometry (examples/make_music_video.py:43-55 call shape): SD-2.1 architecture at 768x768 (96x96
    latent, 9216-token self-attention with 64-wide heads, v-prediction, 1024-d text context), two interpolated frames whose
    T comes from the audio (get_timesteps_arr on the reference's tests/samples/choice.wav), 2 DDIM steps, CFG 7.5 - against
    the CPU oracle (about a minute of oracle time)."""
    from oracle import interp
    from oracle.pipeline import denoise_and_decode, numpy_to_uint8
    from oracle.scheduler import DDIMScheduler as OracleDDIM
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, get_timesteps_arr
    pipe = StableDiffusionWalkPipeline.from_pretrained("stabilityai/stable-diffusion-2-1", arch="sd21")
    assert pipe.scheduler.config.prediction_type == "v_prediction"
    o_unet, o_vae = _oracle_for((pipe.unet, pipe.vae))
    pipe.to(dev)
    wav = Path(__file__).parent / "samples" / "choice.wav"
    T = get_timesteps_arr(str(wav), offset=2.0, duration=1.0, fps=2, margin=1.0, smooth=0.0)          # 2 audio-driven positions
    assert T.shape == (2,) and 0.0 <= T[0] <= T[1] <= 1.0
    batches = list(pipe.generate_inputs("a cat", "a dog", 42, 1337, (1, 4, 96, 96), T, 2))
    _, emb, lat = batches[0]
    ea, eb = pipe.embed_text("a cat").cpu(), pipe.embed_text("a dog").cpu()
    ref_in = list(interp.generate_inputs(ea, eb, interp.init_noise(42, (1, 4, 96, 96)), interp.init_noise(1337, (1, 4, 96, 96)), T, 2))[0]
    assert float((emb.cpu() - ref_in[1]).abs().max()) < 1e-5 and float((lat.cpu() - ref_in[2]).abs().max()) < 2e-5
    uncond = pipe.embed_text("").cpu()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    ref = denoise_and_decode(o_unet, o_vae, OracleDDIM(prediction_type="v_prediction"), ref_in[1], uncond, ref_in[2],
                             num_inference_steps=2, guidance_scale=7.5)
    out = pipe(latents=lat, text_embeddings=emb, height=768, width=768, num_inference_steps=2, guidance_scale=7.5,
               output_type="numpy")["images"]
    p = psnr(torch.from_numpy(out), torch.from_numpy(ref), peak=1.0)
    d8 = np.abs((out * 255).round().astype(int) - numpy_to_uint8(ref).astype(int))
    report(f"SD-2.1 768x768 (config 4), audio T {T.round(3).tolist()}, 2 steps, CFG: frame PSNR {p:.1f} dB, uint8 max-abs {d8.max()} "
           f"mean-abs {d8.mean():.3f}")
    assert out.shape == (2, 768, 768, 3) and p >= 36.5        # measured 39.6 dB


def test_pipeline_variants(hip, dev):
    """eta > 0 (DDIM variance noise), negative prompt, num_images_per_prompt, prompt= entry, v-prediction."""
    from oracle.pipeline import denoise_and_decode
    from oracle.scheduler import DDIMScheduler as OracleDDIM
    from stable_diffusion_videos_amd import DDIMScheduler, StableDiffusionWalkPipeline
    for ptype in ("epsilon", "v_prediction"):
        pipe = StableDiffusionWalkPipeline.from_pretrained("tiny", scheduler=DDIMScheduler(prediction_type=ptype))
        o_unet, o_vae = _oracle_for((pipe.unet, pipe.vae))
        pipe.to(dev)
        emb = pipe.embed_text("a cat").cpu()
        neg = pipe.embed_text("blurry").cpu()
        lat = pipe.init_noise(7, (1, 4, 8, 8)).cpu()
        steps = 6
        g = torch.Generator().manual_seed(3)
        out = pipe(latents=lat, text_embeddings=emb, height=64, width=64, num_inference_steps=steps, guidance_scale=5.0,
                   eta=0.5, negative_prompt="blurry", generator=g, output_type="numpy")["images"]
        # the pipeline draws (steps, B, h, w, C) NHWC variance noise from the generator; mirror it for the oracle
        noise = torch.randn((steps, 1, 8, 8, 4), generator=torch.Generator().manual_seed(3)).permute(0, 1, 4, 2, 3)
        ref = denoise_and_decode(o_unet, o_vae, OracleDDIM(prediction_type=ptype), emb, neg, lat, steps, 5.0, eta=0.5,
                                 variance_noise=list(noise))
        p = psnr(torch.from_numpy(out), torch.from_numpy(ref), peak=1.0)
        report(f"tiny pipeline {ptype} eta=0.5 negative prompt: frame PSNR {p:.1f} dB")
        assert p >= 39.0
    ims = pipe(prompt=["a cat", "a dog"], height=64, width=64, num_inference_steps=2, num_images_per_prompt=2,
               generator=torch.Generator().manual_seed(0)).images
    assert len(ims) == 4
    with pytest.raises(ValueError, match="negative_prompt"):
        pipe(prompt=["a cat", "a dog"], negative_prompt=["x"], height=64, width=64, num_inference_steps=1)


def test_cfg_shared_prefix_is_exact(hip, dev):
    """Classifier-free guidance feeds the same latents twice (stable_diffusion_pipeline.py:414).  Computing the
    context-free prefix of the UNet once (cfg_shared=True) must give the same eps as computing it twice."""
    from stable_diffusion_videos_amd import config as cfgs
    for c in (cfgs.tiny_unet(), cfgs.sd14_unet()):
        _, engine = unet_pair(c, dev, seed=4)
        g = torch.Generator().manual_seed(9)
        x1 = bf16_round(torch.randn((2, c.in_channels, 16, 16), generator=g))
        x = torch.cat([x1, x1])
        ctx = bf16_round(torch.randn((4, 77, c.cross_attention_dim), generator=g))
        engine.prepare_timesteps([981, 961])
        engine.prepare_context(ctx.to(dev))
        step = torch.tensor([1], dtype=torch.int32, device=dev)
        x2 = x.permute(0, 2, 3, 1).reshape(-1, c.in_channels).to(dev, BF16).contiguous()
        a = engine.forward(x2, 4, 16, 16, step, cfg_shared=False)
        b = engine.forward(x2, 4, 16, 16, step, cfg_shared=True)
        torch.cuda.synchronize()
        d = float((a - b).abs().max())
        report(f"cfg_shared vs full ({'sd14' if c.cross_attention_dim == 768 else 'tiny'}): max |d eps| = {d:.3e}")
        assert d <= 1e-3 * float(a.abs().max())
        assert float((a[:2] - a[2:]).abs().max()) > 1e-3      # the two halves really differ (different text context)


@pytest.mark.parametrize("arch", ["tiny", "sd14"])
def test_unet_launch_trace_on_the_device(hip, dev, arch):
    """What the GPU is handed is what tests/test_launch_trace_cpu.py pins on the meta device: the same recorder around a real
    forward - real pointers in ``hip.gn_epilogue_ok``, live version counters - gives the golden trace of the same case."""
    import launch_trace as lt
    size = (4, 16, True, 0)
    want = json.loads(lt.GOLDEN_FILE.read_text())["unet/" + lt.engine_case_name(arch, size)]
    trace = lt.trace_engine(lt.build_engine(arch, dev), *size)
    torch.cuda.synchronize()
    diff = lt.first_difference(trace, want)
    assert diff is None, diff


def test_vae_launch_trace_on_the_device(hip, dev):
    """A real tiny_vae decode of one image of 8 x 8 latents launches what the meta device's ``vae/*`` case pins."""
    import launch_trace as lt
    nimg, side, want_float, per_chunk, tiled = lt.VAE_CASES["n1_s8"]
    want = json.loads(lt.GOLDEN_FILE.read_text())["vae/tiny_vae_n1_s8"]
    trace = lt.trace_vae(lt.build_vae("tiny_vae", dev, tiled=tiled), nimg, side, want_float, per_chunk)
    torch.cuda.synchronize()
    diff = lt.first_difference(trace, want)
    assert diff is None, diff


@pytest.mark.parametrize("name", ["tiny_text_b2", "tiny_vision_n2"])
def test_clip_call_launch_trace_on_the_device(hip, dev, name):
    """The whole ``text_encoder(ids)`` / ``vision(patches, n)`` call, host-side checks included, is the recorded ``clip_call/*``."""
    import launch_trace as lt
    want = json.loads(lt.GOLDEN_FILE.read_text())["clip_call/" + name]
    trace = lt.trace_clip_call(name, dev)
    torch.cuda.synchronize()
    diff = lt.first_difference(trace, want)
    assert diff is None, diff


@pytest.mark.parametrize("fp8", [False, True])
def test_cache_blocked_forward(hip, dev, fp8, monkeypatch):
    """UNetEngine._segment walks a ResBlock (+ transformer) over the batch in cache-sized chunks of images.  Every op of those
    blocks is local to one image, so the chunked forward must reproduce the whole-batch forward - same kernels, same per-row
    arithmetic; only the row statistics behind the folded LayerNorms may be summed over differently shaped tiles.  Different
    latents AND different contexts per image, ragged last chunk (5 images in chunks of 2), with and without the shared CFG prefix."""
    from stable_diffusion_videos_amd import config as cfgs
    # (split-K off: whether a launch is split along K depends on its row count, so a 2-image chunk and the 5-image batch would be
    #  two fp32 summation orders of the low-resolution convs - measured 6e-3 - and this test is about the chunk loop, not about that)
    monkeypatch.setattr(hip, "SPLIT_K", False)
    for c in (cfgs.tiny_unet(), cfgs.sd14_unet()):
        name = "sd14" if c.cross_attention_dim == 768 else "tiny"
        if fp8 and name == "tiny":
            continue
        _, engine = unet_pair(c, dev, seed=4, fp8=fp8)
        for nimg, shared in ((5, False), (6, True)):
            g = torch.Generator().manual_seed(9 + nimg)
            x = bf16_round(torch.randn((nimg, c.in_channels, 16, 16), generator=g))
            if shared:
                x = torch.cat([x[: nimg // 2]] * 2)
            ctx = bf16_round(torch.randn((nimg, 77, c.cross_attention_dim), generator=g))
            engine.prepare_timesteps([981, 961])
            engine.prepare_context(ctx.to(dev))
            step = torch.tensor([1], dtype=torch.int32, device=dev)
            x2 = x.permute(0, 2, 3, 1).reshape(-1, c.in_channels).to(dev, BF16).contiguous()
            monkeypatch.setenv("SDV_CHUNK_ROWS", "0")
            if fp8:
                engine.forward(x2, nimg, 16, 16, step, cfg_shared=shared)       # (the first eager forward calibrates the scales)
            a = engine.forward(x2, nimg, 16, 16, step, cfg_shared=shared)
            # chunk = 2 images of the 16 x 16 level (the smaller levels would take more images per chunk: they stay whole)
            monkeypatch.setenv("SDV_CHUNK_ROWS", "512")
            assert engine._chunk_images(256, nimg) == 2 and engine._chunk_images(64, nimg) == 0
            launches = []
            hip.LAUNCH_HOOK = lambda kind, info, fn: (launches.append(kind), fn())
            b = engine.forward(x2, nimg, 16, 16, step, cfg_shared=shared)
            hip.LAUNCH_HOOK = None
            launches_b = len(launches)
            monkeypatch.setenv("SDV_CHUNK_ROWS", "0")
            hip.LAUNCH_HOOK = lambda kind, info, fn: (launches.append(kind), fn())
            engine.forward(x2, nimg, 16, 16, step, cfg_shared=shared)
            hip.LAUNCH_HOOK = None
            torch.cuda.synchronize()
            d = float((a - b).abs().max()) / float(a.abs().max())
            report(f"cache-blocked vs whole-batch forward ({name}, fp8={fp8}, nimg={nimg}, shared={shared}): max |d eps| / max |eps| "
                   f"= {d:.3e}, bit-identical: {torch.equal(a, b)}, launches {len(launches) - launches_b} -> {launches_b}")
            assert launches_b > len(launches) - launches_b          # the chunk loop really ran
            assert d <= 2e-3


def _run_ranks(world, backend, args, extra_env=None, timeout=600):
    """Launch ``world`` ranks of tests/dist_walk_worker.py (all on cuda:0) and wait for them."""
    import os
    import socket
    import subprocess
    import sys
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SDV_DIST_BACKEND=backend, SDV_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0",
                   **(extra_env or {}))
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).parent / "dist_walk_worker.py"), *args], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=timeout)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    return outs


def _frames_of(root):
    return {str(f.relative_to(root)): f.read_bytes() for f in sorted(Path(root).rglob("frame*.png"))}


def test_two_rank_walk_writes_the_same_frames_as_one_rank(hip, dev, tmp_path):
    """Frame-sharded data parallelism (the reference's only multi-device strategy is
    flax_stable_diffusion_pipeline.py:568-597): 2 ranks on ONE GPU (gloo control plane, every rank's kernels on cuda:0)
    write exactly the frame files a 1-rank walk writes, byte for byte - including the auto-generated run name (broadcast
    from rank 0) and a resume after a crash that left HOLES in both ranks' blocks."""
    one = tmp_path / "one"
    two = tmp_path / "two"
    _run_ranks(1, "gloo", [str(one), "w"])
    outs = _run_ranks(2, "gloo", [str(two), "w"])
    assert all("backend gloo done" in o for o in outs)
    a, b = _frames_of(one / "w"), _frames_of(two / "w")
    assert sorted(a) == sorted(b) and len(a) == 9
    assert a == b, "2-rank frames differ from the 1-rank frames"
    assert (two / "w" / "prompt_config.json").exists()
    # auto name: both ranks must land in ONE directory
    auto = tmp_path / "auto"
    _run_ranks(2, "gloo", [str(auto), "-"])
    dirs = [d for d in auto.iterdir() if d.is_dir()]
    assert len(dirs) == 1 and len(_frames_of(dirs[0])) == 9
    # crash with holes: rank 0's block lost frames 1-2 of clip 0, rank 1's block lost frame 1 of clip 1, plus a truncated
    # (zero-byte) frame and a stale .part file
    for rel in ("w_000000/frame000001.png", "w_000000/frame000002.png", "w_000001/frame000001.png"):
        (two / "w" / rel).unlink()
    (two / "w" / "w_000001" / "frame000003.png").write_bytes(b"")
    (two / "w" / "w_000000" / "frame000004.png.part").write_bytes(b"junk")
    _run_ranks(2, "gloo", [str(two), "w", "resume"])
    c = _frames_of(two / "w")
    assert c == a, "resume after a crash with holes did not restore every frame"


def test_rccl_weight_broadcast_path_runs_with_one_rank(hip, dev, tmp_path):
    """The RCCL (backend "nccl") code path - process-group init with a device id, the two packed weight broadcasts, the
    device-side re-layout of the received buffers, barriers - executed with world_size 1 (the pool has 1-GPU boxes); the
    frames equal those of a run without any process group."""
    plain = tmp_path / "plain"
    rccl = tmp_path / "rccl"
    _run_ranks(1, "gloo", [str(plain), "w"])
    outs = _run_ranks(1, "nccl", [str(rccl), "w"], extra_env={"SDV_DIST_INIT": "1"})
    assert "backend nccl done" in outs[0]
    assert _frames_of(plain / "w") == _frames_of(rccl / "w")


def test_bench_launches_its_own_ranks(hip, dev):
    """``python bench.py --gpus 2`` with no torchrun environment spawns two ranks itself and reports the group that formed
    (here both on this box's one GPU, SDV_FORCE_DEVICE=0, so the collectives run over gloo - RCCL refuses two ranks on one
    device); ``--gpus 8`` on this 1-GPU box must fail loudly instead of printing a 1-GPU line."""
    import os
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "2", "--arch", "tiny", "--steps", "1", "--warmup", "1",
                        "--batch-size", "4", "--full", "--no-cpu-baseline", "--no-walk-pass", "--no-kernel-pass"],
                       capture_output=True, text=True, env=dict(env, SDV_FORCE_DEVICE="0"), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["dist_backend"] == "gloo" and d["config"]["frames"] == 2 * 4 and d["value"] > 0
    if torch.cuda.device_count() < 8:
        r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "8"], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode != 0 and not r.stdout.strip() and "refusing" in r.stderr


def test_plain_bench_times_its_steps_and_dumps_the_last_frames(hip, dev, tmp_path):
    """A plain ``bench.py`` run (no --full) times exactly --steps steps, carries none of the --full extras, and
    ``--dump-outputs`` writes the last timed step's frames (float32 copies of the uint8 values)."""
    import os
    import subprocess
    import sys
    root = Path(__file__).resolve().parent.parent
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(root / "bench.py"), "--gpus", "1", "--arch", "tiny", "--steps", "3", "--warmup", "1",
                        "--batch-size", "4", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["config"]["frames"] == 12 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "bf16" and "metric" in d
    assert not {"parity_check", "cpu_baseline", "walk_60_frames", "other_configs", "png_frames_per_sec_per_core"} & set(d)
    frames = np.load(tmp_path / "out" / "frames.npy")
    assert frames.dtype == np.float32 and frames.shape == (4, 128, 128, 3)
    assert np.array_equal(frames, np.round(frames)) and frames.min() >= 0 and frames.max() <= 255 and frames.std() > 0
    assert np.array_equal(np.load(tmp_path / "out" / "frame_index.npy"), np.arange(4))


def test_ragged_last_batch_reuses_the_captured_graph(hip, dev, tmp_path):
    """7 frames at batch_size 4: the 3-frame tail is padded and replays the 4-frame graph (one captured step, one private
    pool) and still writes the frames a batch_size-1 walk writes.  A tail that would be MOSTLY padding (1 frame of 4 - or the
    literal 60-frame config on a 128-frame graph) gets its own graph instead of paying for the big batch."""
    from PIL import Image
    pipe = _tiny_pipeline(dev)
    kw = dict(output_dir=str(tmp_path), fps=3, num_inference_steps=3, height=64, width=64, make_video=False)
    pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=7, name="b4", batch_size=4, **kw)
    assert len(pipe._graphs) == 1
    pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=7, name="b1", batch_size=1, **kw)
    for k in range(7):
        a = np.asarray(Image.open(tmp_path / "b4" / "b4_000000" / f"frame{k:06d}.png")).astype(int)
        b = np.asarray(Image.open(tmp_path / "b1" / "b1_000000" / f"frame{k:06d}.png")).astype(int)
        assert np.abs(a - b).max() <= 2, k
    pipe2 = _tiny_pipeline(dev)
    pipe2.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=5, name="c4", batch_size=4, **kw)
    assert len(pipe2._graphs) == 2                    # 4 frames + a 1-frame tail with its own captured step


def test_graph_cache_evicts_releases_and_recaptures(hip, dev):
    """The step cache beyond its happy path, with room for 2 steps: batch sizes 1, 2, 3, 1 - the third call evicts the 1-frame
    step and releases its cross-attention K / V^T buffers, the fourth captures again at that size into fresh ones - and a step
    first run with graphs off that is captured once they are on.  Every call equals the same call of an eager pipeline bit for
    bit (tiny arch, 64 x 64, 3 DDIM steps, CFG 7.5)."""
    pipe, eager = _tiny_pipeline(dev), _tiny_pipeline(dev)
    eager.use_graphs = False
    pipe.max_cached_graphs = 2
    emb = pipe.embed_text(["a cat", "a dog", "a horse", "a cow"]).cpu()
    lat = torch.cat([pipe.init_noise(s, (1, 4, 8, 8)) for s in (42, 1337, 7, 11)]).cpu()

    def run(p, B):
        return p(latents=lat[:B], text_embeddings=emb[:B], height=64, width=64, num_inference_steps=3, guidance_scale=7.5,
                 output_type="numpy_u8")["images"]

    def newest(p):
        return list(p._graphs)[-1]

    for call, B in enumerate((1, 2, 3, 1)):
        assert np.array_equal(run(pipe, B), run(eager, B)), (call, B)
        assert newest(pipe).graph is not None and len(pipe._graphs) == min(call + 1, 2)
        if call == 2:       # steps of 2 and 3 frames (4 and 6 samples) are cached: the 2-sample buffers of the first call are gone
            assert {k[0] for k in pipe.unet.tfm[0].ctx_by_len} <= {4, 6}
    pipe.use_graphs = False
    off = run(pipe, 4)
    assert newest(pipe).graph is None and np.array_equal(off, run(eager, 4))
    pipe.use_graphs = True
    on = run(pipe, 4)
    assert np.array_equal(on, off) and newest(pipe).graph is not None


def test_walk_with_audio_and_video(hip, dev, tmp_path):
    """Mirror of the reference's test_walk_with_audio (tests/test_pipeline.py:53-68): audio-driven T per clip,
    batch_size 16, and the mp4 files of the documented layout (:648-666) exist."""
    wav = Path(__file__).parent / "samples" / "choice.wav"
    pipe = _tiny_pipeline(dev)
    fps = 6
    offsets = [2, 4, 5, 8]
    steps = [(b - a) * fps for a, b in zip(offsets, offsets[1:])]
    ret = pipe.walk(["a cat", "a dog", "a horse", "a cow"], seeds=[42, 1337, 4321, 1234], num_interpolation_steps=steps,
                    output_dir=str(tmp_path), name="audio", fps=fps, audio_filepath=str(wav), audio_start_sec=offsets[0],
                    batch_size=16, num_inference_steps=2, height=64, width=64)
    root = tmp_path / "audio"
    assert ret == str(root / "audio.mp4") and Path(ret).exists() and Path(ret).stat().st_size > 1000
    for i, n in enumerate(steps):
        clip = root / f"audio_{i:06d}"
        assert len(list(clip.glob("frame*.png"))) == n
        assert (clip / f"audio_{i:06d}.mp4").exists()
    cfg = json.loads((root / "prompt_config.json").read_text())
    assert cfg["audio_filepath"] == str(wav) and cfg["audio_start_sec"] == 2 and cfg["num_interpolation_steps"] == steps


# ------------------------------------------------------------------------------------------------
# Real-ESRGAN x4: RRDBNet on the HIP kernels vs the fp32 oracle restatement
# ------------------------------------------------------------------------------------------------
def _esrgan_pair(dev, num_block, probe, seed=0):
    """Engine + oracle on the same bf16-exact synthetic weights.  Random weights make the un-normalised generator's
    output far wider than [0, 1] (everything would clamp and the comparison would be vacuous), so conv_last is scaled by
    a power of two (exact in bf16) that brings the oracle's output on ``probe`` to a standard deviation of ~0.15 around
    0.5."""
    import math
    from oracle.esrgan import RRDBNet, RRDBNetConfig as OCfg
    from stable_diffusion_videos_amd.config import RRDBNetConfig
    from stable_diffusion_videos_amd.esrgan import RRDBNetEngine
    from stable_diffusion_videos_amd.weights import rrdbnet_shapes, synthetic_state_dict
    cfg = RRDBNetConfig(num_block=num_block)
    sd = synthetic_state_dict(rrdbnet_shapes(cfg), seed=seed)
    sd["conv_last.bias"] = torch.full_like(sd["conv_last.bias"], 0.5)
    oracle = RRDBNet(OCfg(num_block=num_block)).eval()
    oracle.load_state_dict(sd)
    with torch.no_grad():
        std = float((oracle(probe) - 0.5).std())
    sd["conv_last.weight"] = sd["conv_last.weight"] * 2.0 ** math.floor(math.log2(0.15 / std))
    oracle.load_state_dict(sd)
    return RRDBNetEngine(cfg, sd, dev), oracle


@pytest.mark.parametrize("num_block,n,H,W", [(2, 2, 24, 40), (23, 1, 64, 64)])
def test_esrgan_matches_oracle(hip, dev, num_block, n, H, W):
    """Stated tolerance: PSNR >= 57 dB (measured 60.0 / 66.4) on the clamped [0,1] output (bf16 storage through up to 345 convs vs fp32),
    uint8 frames within a few grey levels.  **parity unpinned** (oracle/esrgan.py)."""
    from oracle.esrgan import enhance_rgb_u8
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
    engine, oracle = _esrgan_pair(dev, num_block, img.float().div(255).permute(0, 3, 1, 2))
    u8, f32 = engine(img.to(dev), want_float=True)
    torch.cuda.synchronize()
    assert u8.shape == (n, 4 * H, 4 * W, 3) and u8.dtype == torch.uint8
    with torch.no_grad():
        ref = oracle(img.float().div(255).permute(0, 3, 1, 2)).clamp(0, 1).permute(0, 2, 3, 1)
    p = psnr(f32.cpu(), ref, peak=1.0)
    ref_u8 = np.stack([enhance_rgb_u8(oracle, im.numpy()) for im in img])
    d = np.abs(u8.cpu().numpy().astype(np.int32) - ref_u8.astype(np.int32))
    frac_mid = float(((ref > 0.02) & (ref < 0.98)).float().mean())
    report(f"esrgan blocks={num_block} {n}x{H}x{W}: PSNR {p:.1f} dB, uint8 max|d| {int(d.max())}, mean|d| {d.mean():.3f}, "
           f"unclamped fraction {frac_mid:.2f}")
    assert frac_mid > 0.9, "synthetic output saturates: the comparison would be vacuous"
    assert p >= 57.0
    assert d.mean() < 1.5
    # chunked execution (several frames per call, one frame per chunk) is bit-identical
    engine.max_chunk_pixels = H * W
    u8b, _ = engine(img.to(dev))
    assert torch.equal(u8, u8b)


def test_walk_upsample_layout(hip, dev, tmp_path):
    """walk(upsample=True): same file layout as without, frames 4x larger (reference :513-516, :552)."""
    from PIL import Image
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    pipe = _tiny_pipeline(dev)
    up = RealESRGANModel(None)
    up.cfg.num_block = 1                                            # keep the test light: rebuild a 1-block generator
    from stable_diffusion_videos_amd.weights import rrdbnet_shapes, synthetic_state_dict
    up.state_dict_ = synthetic_state_dict(rrdbnet_shapes(up.cfg), seed=1)
    pipe.upsampler = up
    out = pipe.walk(prompts=["a", "b"], seeds=[1, 2], num_interpolation_steps=3, output_dir=str(tmp_path), name="u",
                    num_inference_steps=2, height=64, width=64, batch_size=2, upsample=True, make_video=False)
    assert out is None
    frames = sorted((tmp_path / "u" / "u_000000").glob("frame*.png"))
    assert len(frames) == 3
    assert Image.open(frames[0]).size == (256, 256)
    # single-image API of the reference class (float RGB in [0,1] -> PIL, BGR ndarray with convert_to_pil=False)
    img = np.random.RandomState(0).rand(16, 24, 3).astype(np.float32)
    pil = up(img)
    assert pil.size == (96, 64)
    bgr = up(img, convert_to_pil=False)
    assert bgr.shape == (64, 96, 3) and np.array_equal(bgr[:, :, ::-1], np.asarray(pil))
    assert up(img, outscale=2).size == (48, 32)


# ------------------------------------------------------------------------------------------------
# CLIP text encoder (8a row a4): the native engine vs vectors of the REAL transformers.CLIPTextModel
# ------------------------------------------------------------------------------------------------
def _clip_golden(act):
    z = np.load(Path(__file__).resolve().parent / "golden" / f"clip_{act}.npz")
    sd = {k[4:]: (torch.from_numpy(z[k].astype(np.int32)) << 16).view(torch.float32) for k in z.files if k.startswith("sd::")}
    return z, sd


@pytest.mark.parametrize("act", ["quick_gelu", "gelu"])
def test_clip_text_engine_matches_transformers_golden(hip, dev, act):
    """Stated tolerance: PSNR >= 47.5 dB (measured 50.7 / 51.4) against last_hidden_state of transformers.CLIPTextModel (tests/golden/clip_*.npz,
    generated by tests/golden/make_golden_clip.py; weights are bf16-exact so both sides share them bit for bit)."""
    from stable_diffusion_videos_amd.config import TextConfig
    from stable_diffusion_videos_amd.text import CLIPTextEngine
    z, sd = _clip_golden(act)
    D = sd["final_layer_norm.weight"].numel()
    nl = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
    cfg = TextConfig(vocab_size=sd["embeddings.token_embedding.weight"].shape[0], hidden_size=D,
                     intermediate_size=sd["encoder.layers.0.mlp.fc1.weight"].shape[0], num_hidden_layers=nl,
                     num_attention_heads=int(z["num_heads"]), hidden_act=act, bos_token_id=209, eos_token_id=210)
    eng = CLIPTextEngine(cfg, sd).to(dev)
    ids = torch.from_numpy(z["ids"]).to(dev)
    out = eng(ids)[0]
    torch.cuda.synchronize()
    ref = torch.from_numpy(z["last_hidden_state"])
    assert out.shape == ref.shape and out.dtype == torch.float32
    p = psnr(out.cpu(), ref)
    report(f"clip text engine ({act}, {nl} layers) vs transformers {str(z['transformers_version'])}: PSNR {p:.1f} dB, "
           f"rel-L2 {rel_l2(out.cpu(), ref):.2e}")
    assert p >= 47.5
    # batch independence and determinism: one row alone reproduces its slice bit for bit
    assert torch.equal(eng(ids[1:2])[0], out[1:2])
    with pytest.raises(IndexError):
        eng(torch.full((1, 77), 100000, device=dev))


def test_clip_text_engine_full_size_vs_oracle(hip, dev):
    """SD-v1-4 text encoder size (12 layers x 768, 12 heads, quick_gelu) on synthetic weights vs the pinned oracle."""
    from oracle.clip import clip_text_forward
    from stable_diffusion_videos_amd import config as cfgs
    from stable_diffusion_videos_amd.text import build_text_encoder
    eng = build_text_encoder(cfgs.sd14_text(), None, seed=3)
    sd = eng.state_dict()
    eng.to(dev)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, 49406, (2, 77), generator=g)
    ids[:, 0] = 49406
    ids[0, 12:] = 49407
    out = eng(ids.to(dev))[0].cpu()
    ref = clip_text_forward(sd, ids, 12, "quick_gelu")
    p = psnr(out, ref)
    report(f"clip text engine sd14 size vs oracle: PSNR {p:.1f} dB")
    assert p >= 52.0


def test_generate_images_on_the_hip_path(hip, dev, tmp_path):
    """generate_images (reference image_generation.py:108-215) end to end on the tiny pipeline, with and without the x4
    generator; the same seed gives the same image as a direct __call__."""
    from PIL import Image
    from stable_diffusion_videos_amd import generate_images
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    from stable_diffusion_videos_amd.weights import rrdbnet_shapes, synthetic_state_dict
    pipe = _tiny_pipeline(dev)
    files = generate_images(pipe, "a cat", batch_size=2, num_batches=2, seeds=[3, 4, 5, 6], output_dir=tmp_path, name="g",
                            height=64, width=64, num_inference_steps=2, image_file_ext=".png")
    assert [Path(f).name for f in files] == ["3.png", "4.png", "5.png", "6.png"]
    direct = pipe(text_embeddings=pipe.embed_text("a cat"), latents=pipe.init_noise(5, (1, 4, 8, 8)), height=64, width=64,
                  num_inference_steps=2, output_type="numpy_u8")["images"][0]
    assert np.array_equal(np.asarray(Image.open(files[2])), direct)
    up = RealESRGANModel(None)
    up.cfg.num_block = 1
    up.state_dict_ = synthetic_state_dict(rrdbnet_shapes(up.cfg), seed=1)
    pipe.upsampler = up
    big = generate_images(pipe, "a cat", seeds=[9], output_dir=tmp_path, name="u", height=64, width=64, num_inference_steps=2,
                          image_file_ext=".png", upsample=True)
    assert Image.open(big[0]).size == (256, 256)
