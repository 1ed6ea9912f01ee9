"""The PNG encoder on the GPU (csrc/sdv_png.hip behind png.PngEncoder) against tests/png_ref.py (numpy restatement, sequential packer)
and zlib / PIL (libpng) as the independent decoders.  Lossless: every comparison is exact.  The shapes are the smallest that reach
every branch: one pixel; a batch with a ragged last stripe and odd row bytes; three stripes; a row longer than one workgroup pass;
more than 64 stripes (the scan beyond one wave); a plain batch with the default stripes."""
import functools
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as R

pytestmark = pytest.mark.gpu

CASES = [(shape, sr, kind) for shape, sr in R.CASES for kind in R.KINDS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-sr{sr}-{k}" for s, sr, k in CASES]


@functools.lru_cache(maxsize=None)
def _encoder(stripe_rows):
    from stable_diffusion_videos_amd.png import PngEncoder
    return PngEncoder(torch.device("cuda", 0), stripe_rows=stripe_rows)


@functools.lru_cache(maxsize=None)
def _run(shape, sr, kind):
    """One encode per case, shared by the tests: (frames, files, filtered rows, code lengths, rows per stripe), arrays as numpy."""
    frames = R.make_frames(kind, *shape)
    files, filtered, lengths = _encoder(sr).encode(torch.from_numpy(frames).cuda(), return_tables=True)
    return frames, files, filtered.cpu().numpy(), lengths.cpu().numpy(), sr or R.default_stripe_rows(shape[1], shape[2])


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_filter_stage_is_exact(hip, shape, sr, kind):
    """(1) the filtered buffer equals the restatement's, byte for byte: the same filter type per row, the same bytes."""
    frames, _, filtered, _, _ = _run(shape, sr, kind)
    want = R.filter_rows(frames)
    assert filtered.shape == want.shape and filtered.dtype == np.uint8
    assert np.array_equal(filtered[:, :, 0], want[:, :, 0]), np.argwhere(filtered[:, :, 0] != want[:, :, 0])[:5]
    assert np.array_equal(filtered, want)


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_tables_are_valid_and_optimal(hip, shape, sr, kind):
    """(2) per stripe: length 0 exactly for unused symbols, at most 15, Kraft sum exactly 1, and the cost of a Huffman code - the heap's
    code is at most 15 deep for every case here."""
    _, _, filtered, lengths, rows = _run(shape, sr, kind)
    n, H, _ = shape
    assert lengths.shape == (n, -(-H // rows), 257)
    for k in range(n):
        for s, hist in enumerate(R.stripe_histograms(filtered[k], rows)):
            assert R.optimal_depth(hist) <= 15
            R.check_lengths(lengths[k, s], hist, optimal=True)


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_entropy_stage_is_exact(hip, shape, sr, kind):
    """(3) the file bytes equal the sequential packer run on the GPU's own filtered rows and code lengths, from signature to IEND."""
    _, files, filtered, lengths, rows = _run(shape, sr, kind)
    want = R.pack(filtered, lengths, shape[1], shape[2], rows)
    assert len(files) == shape[0]
    for k in range(shape[0]):
        assert files[k] == want[k], (k, len(files[k]), len(want[k]))


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_independent_decoders(hip, shape, sr, kind):
    """(4) zlib inflates the IDAT payload to the filtered bytes (it checks the Adler-32 and the completeness of every table), PIL
    decodes the file to exactly the frame, every chunk CRC is right (png_ref.chunks asserts each)."""
    frames, files, filtered, _, _ = _run(shape, sr, kind)
    from stable_diffusion_videos_amd.png import png_header
    for k, data in enumerate(files):
        assert data.startswith(png_header(shape[1], shape[2])) and data[37:43] == b"IDAT\x78\x01"
        assert zlib.decompress(R.idat(data)) == filtered[k].tobytes()
        got = R.decode(data)
        assert got.shape == frames[k].shape and np.array_equal(got, frames[k])


def _pack_direct(hip, dev, buf, stripe_rows):
    """sdv_png_deflate_pack on a hand-made filtered buffer: (file bytes with the CRC hole still zero, lengths [stripes, 257])."""
    n, H, Rb = buf.shape
    assert n == 1
    stripes = -(-H // stripe_rows)
    from stable_diffusion_videos_amd.png import png_header
    header = torch.frombuffer(bytearray(png_header(H, (Rb - 1) // 3)), dtype=torch.uint8).to(dev)
    scratch = torch.empty((hip.png_scratch_bytes(1, H, stripe_rows),), dtype=torch.uint8, device=dev)
    out = torch.zeros((2 * buf.size + 1024,), dtype=torch.uint8, device=dev)
    meta = torch.zeros((3,), dtype=torch.int64, device=dev)
    lengths = torch.zeros((1, stripes, 257), dtype=torch.uint8, device=dev)
    hip.png_deflate_pack(torch.from_numpy(buf).to(dev), torch.from_numpy(R.adler_partials(buf)).to(dev), stripe_rows, header, scratch, out,
                         meta[:2], meta[2:], lengths)
    torch.cuda.synchronize()
    offs = meta.tolist()
    assert offs[0] == 0 and offs[1] == offs[2] <= out.numel()
    return out[:offs[1]].cpu().numpy().tobytes(), lengths.cpu().numpy()[0]


def test_length_limiting(hip, dev):
    """(5) hand-made filtered buffers whose unrestricted Huffman code is deeper than 15 (asserted on the restatement alone): the lengths
    are valid (no cost clause), and the stream inflates to the buffer.  First the 4181 bytes of 17 values with the Fibonacci counts
    1, 1, 2, ..., 1597 - where the depth beyond 15 hangs on the tie-break (png_ref.fibonacci_buffer) -, then counts that force it."""
    for buf, stripe_rows in ((R.fibonacci_buffer(), 113), (R.forced_deep_buffer(), 1)):
        hist = R.stripe_histograms(buf[0], stripe_rows)
        assert hist.shape[0] == 1 and R.optimal_depth(hist[0]) > 15
        data, lengths = _pack_direct(hip, dev, buf, stripe_rows)
        R.check_lengths(lengths[0], hist[0], optimal=False)
        idat = data[41:-16]                                                       # (the CRC hole is still zero: no chunk parser here)
        assert int.from_bytes(data[33:37], "big") == len(idat) and data[37:41] == b"IDAT" and data[-12:] == R.chunk(b"IEND", b"")
        assert zlib.decompress(idat) == buf.tobytes()
    hist = R.stripe_histograms(R.forced_deep_buffer()[0], 1)[0]
    assert R.optimal_depth(hist, shallow=True) > 15 and int(lengths[0].max()) == 15   # no tie-break escapes: the limiter ran
    assert sum(int(c) * int(l) for c, l in zip(hist, lengths[0])) > R.optimal_cost(hist)


def test_determinism_and_batch_independence(hip, dev):
    """(6) two runs are bit-identical; frame k of a batch equals the same frame encoded alone."""
    for shape, sr, kind in (((3, 40, 56), None, "smooth"), ((2, 5, 7), 2, "noise")):
        frames, files, _, _, _ = _run(shape, sr, kind)
        t = torch.from_numpy(frames).to(dev)
        assert _encoder(sr).encode(t) == files
        for k in range(shape[0]):
            assert _encoder(sr).encode(t[k:k + 1]) == [files[k]]


def test_memory_bounds_and_small_capacity(hip, dev):
    """(7) guard regions behind out, the scratch, the offsets and the lengths buffer stay 0xA5 at cap = total, total - 1, total / 2
    and 1; a capacity that is too small reports the needed size, writes nothing and leaves the guards; noise outgrows the encoder's
    first buffer exactly once."""
    from stable_diffusion_videos_amd import png
    G = 4096
    for shape, sr, kind in (((2, 5, 7), 2, "noise"), ((1, 70, 24), 1, "smooth"), ((3, 40, 56), None, "noise")):
        n, H, W = shape
        frames, files, filtered, lengths, rows = _run(shape, sr, kind)
        stripes = -(-H // rows)
        total = sum(len(f) for f in files)
        header = torch.frombuffer(bytearray(png.png_header(H, W)), dtype=torch.uint8).to(dev)
        filt_d = torch.from_numpy(filtered).to(dev)
        adler_d = torch.from_numpy(R.adler_partials(filtered)).to(dev)
        sbytes = hip.png_scratch_bytes(n, H, rows)
        for cap in (total, total - 1, total // 2, 1):
            out = torch.full((cap + G,), 0xA5, dtype=torch.uint8, device=dev)
            scratch = torch.full((sbytes + G,), 0xA5, dtype=torch.uint8, device=dev)
            meta = torch.full((n + 2 + G // 8,), 0xA5A5A5A5A5A5A5A5 - (1 << 64), dtype=torch.int64, device=dev)
            lens = torch.full((n * stripes * 257 + G,), 0xA5, dtype=torch.uint8, device=dev)
            hip.png_deflate_pack(filt_d, adler_d, rows, header, scratch[:sbytes], out[:cap], meta[:n + 1], meta[n + 1:n + 2],
                                 lens[:n * stripes * 257].view(n, stripes, 257))
            torch.cuda.synchronize()
            assert int(meta[n + 1]) == total == int(meta[n])
            assert bool((out[cap:] == 0xA5).all()) and bool((scratch[sbytes:] == 0xA5).all()) and bool((lens[n * stripes * 257:] == 0xA5).all())
            assert bool((meta[n + 2:].view(torch.uint8) == 0xA5).all())
            assert np.array_equal(lens[:n * stripes * 257].view(n, stripes, 257).cpu().numpy(), lengths)
            if cap >= total:
                offs = meta[:n + 1].tolist()
                host = out[:cap].cpu().numpy()
                for k in range(n):                                                # (the CRC is the host's: the hole is still zero here)
                    got = host[offs[k]:offs[k + 1]].tobytes()
                    assert got[:-16] == files[k][:-16] and got[-16:-12] == bytes(4) and got[-12:] == files[k][-12:]
            else:
                assert bool((out[:cap] == 0xA5).all())
    enc = png.PngEncoder(dev)
    noise = R.make_frames("noise", 1, 64, 64)
    data = enc.encode(torch.from_numpy(noise).to(dev))
    assert enc.retries == 1 and np.array_equal(R.decode(data[0]), noise[0])
    assert enc.encode(torch.from_numpy(noise).to(dev)) == data and enc.retries == 1          # the grown buffer is kept
    assert enc.last_bytes_to_host == len(data[0]) + 8 * 3


def test_encoder_refuses_what_it_cannot_encode(hip, dev):
    from stable_diffusion_videos_amd.png import PngEncoder
    enc = PngEncoder(dev)
    with pytest.raises(hip.SdvHipError, match="uint8"):
        enc.encode(torch.zeros((1, 4, 4, 3), device=dev))
    with pytest.raises(hip.SdvHipError, match="uint8"):
        enc.encode(torch.zeros((1, 4, 4, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(hip.SdvHipError, match="frame size"):
        enc.encode(torch.zeros((1, 1, 16385, 3), dtype=torch.uint8, device=dev))
    assert enc.encode(torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device=dev)) == []


# ---- (8) public surface ------------------------------------------------------------------------------------------------------
def _tiny_pipeline(dev):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    return StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)


def test_output_type_png(hip, dev):
    pipe = _tiny_pipeline(dev)
    batches = list(pipe.generate_inputs("a cat", "a dog", 42, 1337, (1, 4, 8, 8), np.linspace(0.0, 1.0, 2), 2))
    _, embeds, noise = batches[0]
    kw = dict(latents=noise, text_embeddings=embeds, height=64, width=64, num_inference_steps=2)
    u8 = pipe(output_type="numpy_u8", **kw)["images"]
    images = pipe(output_type="png", **kw)["images"]
    assert isinstance(images, list) and len(images) == 2 and all(isinstance(b, bytes) for b in images)
    for data, frame in zip(images, u8):
        assert np.array_equal(R.decode(data), frame)
        R.chunks(data)


def test_walk_writes_png_frames_on_the_gpu(hip, dev, tmp_path, monkeypatch, capsys):
    from stable_diffusion_videos_amd.png import png_header
    from stable_diffusion_videos_amd.video import make_video_pyav
    pipe = _tiny_pipeline(dev)
    kw = dict(output_dir=str(tmp_path), fps=3, num_inference_steps=2, height=64, width=64, make_video=False, image_file_ext=".png")
    walk = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=3, batch_size=2)
    monkeypatch.delenv("SDV_PNG", raising=False)
    assert pipe.png_encoder == "pil"
    pipe.walk(name="p", **walk, **kw)                                            # the default: Image.save in the writer's threads
    monkeypatch.setenv("SDV_PNG", "hip")
    pipe.walk(name="g", **walk, **kw)
    clip, ref = tmp_path / "g" / "g_000000", tmp_path / "p" / "p_000000"
    files = sorted(clip.glob("*"))
    assert [f.name for f in files] == [f"frame{k:06d}.png" for k in range(3)] == [f.name for f in sorted(ref.glob("*"))]
    for f in files:
        data = f.read_bytes()
        assert data.startswith(png_header(64, 64)) and data[37:41] == b"IDAT"     # this package's stream
        R.chunks(data)
        assert np.array_equal(R.decode(data), np.asarray(Image.open(ref / f.name).convert("RGB")))
    stamps = [(f.stat().st_mtime_ns, f.read_bytes()) for f in files]
    assert pipe.resume_todo(clip, clip / "g_000000.mp4", 3, ".png") is None
    pipe.walk(name="g", resume=True, batch_size=2, **kw)
    assert "Skipping" in capsys.readouterr().out
    assert [(f.stat().st_mtime_ns, f.read_bytes()) for f in sorted(clip.glob("*"))] == stamps
    # the video mux sees complete PNG files either way: the same pixels give the same video bytes
    va = make_video_pyav(clip, fps=3, output_filepath=tmp_path / "g.mp4")
    vb = make_video_pyav(ref, fps=3, output_filepath=tmp_path / "p.mp4")
    assert open(va, "rb").read() == open(vb, "rb").read()
    # without the variable the files are byte for byte what Image.save writes for the frames of the same walk
    monkeypatch.delenv("SDV_PNG")
    import io
    for f in sorted(ref.glob("*")):
        buf = io.BytesIO()
        Image.fromarray(R.decode((clip / f.name).read_bytes())).save(buf, format="PNG")
        assert f.read_bytes() == buf.getvalue()
