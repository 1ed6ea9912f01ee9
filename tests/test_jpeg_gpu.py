"""The JPEG encoder on the GPU (csrc/sdv_jpeg.hip behind jpeg.JpegEncoder) against tests/jpeg_ref.py (float64 restatement, sequential
packer) and PIL (libjpeg) as the independent decoder.  The shapes are the smallest that reach every branch: one MCU; ragged on both
axes with a batch of 2; tall and ragged; 78 blocks per restart interval (two wave passes); 10 intervals (RSTm wraps past 7)."""
import functools
import io
import struct

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as R

pytestmark = pytest.mark.gpu

CASES = [(shape, kind) for shape in R.SHAPES for kind in R.KINDS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in CASES]


@functools.lru_cache(maxsize=None)
def _encoder(quality):
    from stable_diffusion_videos_amd.jpeg import JpegEncoder
    return JpegEncoder(quality, torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def _run(shape, kind, quality):
    """One encode per case, shared by the tests: (frames, files, coefficients as numpy)."""
    frames = R.make_frames(kind, *shape)
    files, coef = _encoder(quality).encode(torch.from_numpy(frames).cuda(), return_coefficients=True)
    return frames, files, coef.cpu().numpy()


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_coefficients_equal_the_float64_restatement(hip, shape, kind):
    """(a) equal, except where the restatement's value / q lies within DELTA of a half-integer: there +-1; the excused share is capped."""
    for q in R.gpu_qualities(kind, shape):
        frames, _, coef = _run(shape, kind, q)
        real = R.transform_real(frames, q)
        ref = R.round_half_away(real)
        assert coef.shape == ref.shape and coef.dtype == np.int16
        window = np.abs(np.abs(real - np.floor(real)) - 0.5) < R.DELTA
        diff = np.abs(coef.astype(np.int64) - ref)
        print(f"jpeg coefficients {shape} {kind} q{q}: {int((diff != 0).sum())} of {diff.size} differ, excused share {window.mean():.4f}")
        assert window.mean() <= R.MAX_EXCUSED_SHARE
        assert not (diff[~window] != 0).any(), (q, np.argwhere((diff != 0) & ~window)[:5])
        assert diff[window].max(initial=0) <= 1


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_entropy_stage_is_exact(hip, shape, kind):
    """(b) the file bytes equal the sequential packer run on the GPU's own coefficient buffer, header included."""
    for q in R.gpu_qualities(kind, shape):
        _, files, coef = _run(shape, kind, q)
        want = R.pack(coef, shape[1], shape[2], q)
        assert len(files) == shape[0]
        for k in range(shape[0]):
            assert files[k] == want[k], (q, k, len(files[k]), len(want[k]))


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_files_decode_in_pil_as_well_as_pils_own(hip, shape, kind):
    """(c) every file loads in PIL; PSNR against the source >= PIL's own at the same quality - the restatement's margin - the tie flips."""
    for q in R.gpu_qualities(kind, shape):
        frames, files, _ = _run(shape, kind, q)
        for k, data in enumerate(files):
            got = R.decode(data)
            assert got.shape == frames[k].shape
            ours, pil = R.psnr(got, frames[k]), R.psnr(R.decode(R.pil_encode(frames[k], q)), frames[k])
            assert ours >= pil - R.PSNR_MARGIN_DB - R.TIE_FLIP_DB, (q, k, ours, pil)


def test_determinism_and_batch_independence(hip, dev):
    """(d) two runs are bit-identical; frame k of a batch equals the same frame encoded alone."""
    for kind, q in (("smooth", 75), ("noise", 100)):
        frames, files, _ = _run((2, 40, 56), kind, q)
        t = torch.from_numpy(frames).to(dev)
        assert _encoder(q).encode(t) == files
        for k in range(2):
            assert _encoder(q).encode(t[k:k + 1]) == [files[k]]


def test_memory_bounds_and_small_capacity(hip, dev):
    """(e) guard regions behind out_cap, the scratch buffer and offsets stay 0xA5; a capacity that is too small returns the needed size,
    writes nothing, and leaves the guards intact."""
    from stable_diffusion_videos_amd import jpeg
    G = 4096
    for shape, kind, q in (((1, 32, 208), "noise", 100), ((2, 40, 56), "smooth", 95), ((1, 160, 16), "checker", 95)):
        n, H, W = shape
        frames, files, coef = _run(shape, kind, q)
        total = sum(len(f) for f in files)
        header = torch.frombuffer(bytearray(jpeg.jfif_header(H, W, q)), dtype=torch.uint8).to(dev)
        coef_d = torch.from_numpy(coef).to(dev)
        sbytes = hip.jpeg_scratch_bytes(n, H)
        for cap in (total, total - 1, total // 2, 1):
            out = torch.full((cap + G,), 0xA5, dtype=torch.uint8, device=dev)
            scratch = torch.full((sbytes + G,), 0xA5, dtype=torch.uint8, device=dev)
            meta = torch.full((n + 2 + G // 8,), 0xA5A5A5A5A5A5A5A5 - (1 << 64), dtype=torch.int64, device=dev)
            hip.jpeg_entropy_pack(coef_d, H, W, header, scratch[:sbytes], out[:cap], meta[:n + 1], meta[n + 1:n + 2])
            torch.cuda.synchronize()
            assert int(meta[n + 1]) == total == int(meta[n])
            assert bool((out[cap:] == 0xA5).all()) and bool((scratch[sbytes:] == 0xA5).all())
            assert bool((meta[n + 2:].view(torch.uint8) == 0xA5).all())
            if cap >= total:
                offs = meta[:n + 1].tolist()
                host = out[:cap].cpu().numpy()
                assert [host[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == files
            else:
                assert bool((out[:cap] == 0xA5).all())
    # the encoder's own retry: uniform noise at quality 100 outgrows the first payload buffer (half the raw size)
    enc = jpeg.JpegEncoder(100, dev)
    noise = R.make_frames("noise", 1, 64, 64)
    data = enc.encode(torch.from_numpy(noise).to(dev))
    assert enc.retries == 1 and R.decode(data[0]).shape == (64, 64, 3)
    assert enc.encode(torch.from_numpy(noise).to(dev)) == data and enc.retries == 1          # the grown buffer is kept


def test_aligned_rows_take_the_vector_loads(hip, dev):
    """W % 16 == 0 stages the strip with 16-byte loads, a frame wider than one 256-pixel chunk spans two workgroups per MCU row."""
    frames = R.make_frames("smooth", 1, 32, 272)
    files, coef = _encoder(75).encode(torch.from_numpy(frames).to(dev), return_coefficients=True)
    real = R.transform_real(frames, 75)
    window = np.abs(np.abs(real - np.floor(real)) - 0.5) < R.DELTA
    diff = np.abs(coef.cpu().numpy().astype(np.int64) - R.round_half_away(real))
    assert window.mean() <= R.MAX_EXCUSED_SHARE and not (diff[~window] != 0).any() and diff.max() <= 1
    assert files == R.pack(coef.cpu().numpy(), 32, 272, 75)
    ragged = R.make_frames("smooth", 1, 24, 267)                                 # byte loads, two chunks, the second one ragged
    files, coef = _encoder(75).encode(torch.from_numpy(ragged).to(dev), return_coefficients=True)
    real = R.transform_real(ragged, 75)
    window = np.abs(np.abs(real - np.floor(real)) - 0.5) < R.DELTA
    diff = np.abs(coef.cpu().numpy().astype(np.int64) - R.round_half_away(real))
    assert window.mean() <= R.MAX_EXCUSED_SHARE and not (diff[~window] != 0).any() and diff.max() <= 1
    assert files == R.pack(coef.cpu().numpy(), 24, 267, 75) and R.decode(files[0]).shape == (24, 267, 3)


# ---- (f) public surface ------------------------------------------------------------------------------------------------------
def _tiny_pipeline(dev):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    return StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)


def _bound_ok(data, frame, q):
    got = R.decode(data)
    assert got.shape == frame.shape
    return R.psnr(got, frame) >= R.psnr(R.decode(R.pil_encode(frame, q)), frame) - R.PSNR_MARGIN_DB - R.TIE_FLIP_DB


def test_output_type_jpeg(hip, dev):
    pipe = _tiny_pipeline(dev)
    assert pipe.jpeg_quality == 75
    batches = list(pipe.generate_inputs("a cat", "a dog", 42, 1337, (1, 4, 8, 8), np.linspace(0.0, 1.0, 2), 2))
    _, embeds, noise = batches[0]
    kw = dict(latents=noise, text_embeddings=embeds, height=64, width=64, num_inference_steps=2)
    u8 = pipe(output_type="numpy_u8", **kw)["images"]
    for q in (75, 90):
        pipe.jpeg_quality = q
        images = pipe(output_type="jpeg", **kw)["images"]
        assert isinstance(images, list) and len(images) == 2 and all(isinstance(b, bytes) for b in images)
        assert all(_bound_ok(b, f, q) for b, f in zip(images, u8))
        assert images[0][:2] == b"\xff\xd8" and images[0][-2:] == b"\xff\xd9"


def test_walk_writes_jpg_frames_on_the_gpu(hip, dev, tmp_path, monkeypatch, capsys):
    pipe = _tiny_pipeline(dev)
    kw = dict(output_dir=str(tmp_path), fps=3, num_inference_steps=2, height=64, width=64, make_video=False, image_file_ext=".jpg")
    monkeypatch.delenv("SDV_JPEG", raising=False)
    pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=3, name="g", batch_size=2, **kw)
    clip = tmp_path / "g" / "g_000000"
    files = sorted(clip.glob("*"))
    assert [f.name for f in files] == [f"frame{k:06d}.jpg" for k in range(3)]
    header = R.jfif_header(64, 64, 75)
    for f in files:
        data = f.read_bytes()
        assert data.startswith(header)                                            # this package's stream, quality 75 tables
        im = Image.open(f)
        im.load()
        assert im.size == (64, 64) and im.mode == "RGB"
    stamps = [(f.stat().st_mtime_ns, f.read_bytes()) for f in files]
    assert pipe.resume_todo(clip, clip / "g_000000.mp4", 3, ".jpg") is None
    pipe.walk(name="g", resume=True, batch_size=2, **kw)
    assert "Skipping" in capsys.readouterr().out
    assert [(f.stat().st_mtime_ns, f.read_bytes()) for f in sorted(clip.glob("*"))] == stamps
    # SDV_JPEG=pil: the host-side encode, byte for byte what Image.save writes for the frames of the same walk
    monkeypatch.setenv("SDV_JPEG", "pil")
    pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=3, name="p", batch_size=2, **kw)
    monkeypatch.delenv("SDV_JPEG")
    pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=3, name="q", batch_size=2, **dict(kw, image_file_ext=".png"))
    for k in range(3):
        png = Image.open(tmp_path / "q" / "q_000000" / f"frame{k:06d}.png")
        buf = io.BytesIO()
        png.save(buf, format="JPEG")
        assert (tmp_path / "p" / "p_000000" / f"frame{k:06d}.jpg").read_bytes() == buf.getvalue()
        assert _bound_ok(files[k].read_bytes(), np.asarray(png), 75)             # the GPU's file shows the same frame


def test_make_video_mjpeg_from_a_cuda_tensor(hip, dev, tmp_path, monkeypatch):
    from test_video import find, parse_boxes
    from stable_diffusion_videos_amd import video
    monkeypatch.setenv("SDV_VIDEO_CODEC", "mjpeg")
    frames = R.make_frames("smooth", 3, 40, 56)
    t = torch.from_numpy(frames).to(dev).permute(0, 3, 1, 2)                     # (T, C, H, W), as the reference takes it
    out = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "clip.mp4")
    assert video.LAST_CODEC["video"] == "mjpeg"
    buf = open(out, "rb").read()
    assert [b[0] for b in parse_boxes(buf)] == ["ftyp", "mdat", "moov"]
    stbl = ("moov", "trak", "mdia", "minf", "stbl")
    lo, _ = find(buf, stbl + ("stsz",))
    _, _, n = struct.unpack(">III", buf[lo:lo + 12])
    sizes = struct.unpack(f">{n}I", buf[lo + 12:lo + 12 + 4 * n])
    lo, _ = find(buf, stbl + ("stco",))
    pos = struct.unpack(">III", buf[lo:lo + 12])[2]
    assert n == 3
    header = R.jfif_header(40, 56, 95)
    for k, sz in enumerate(sizes):
        sample = buf[pos:pos + sz]
        assert sample.startswith(header) and sample.endswith(b"\xff\xd9")        # compressed on the GPU at quality 95
        assert _bound_ok(sample, frames[k], 95)
        pos += sz
