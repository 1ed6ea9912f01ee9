"""The PNG encoder's matching mode and GPU-side CRC-32 on the GPU (png.PngEncoder(matches=True), csrc/sdv_png.hip) against
tests/png_lz_ref.py (the stream rule in plain Python, a sequential packer, a bitwise CRC) and zlib / PIL as the independent decoders.
Lossless: every comparison is exact.  The shapes are png_ref.CASES (one pixel: L < 3; odd row bytes and a ragged last stripe; rows of
more than 258 zeros: the length cap and a match that runs to the stripe's end; more than 64 stripes; candidates R - 3 / R / R + 3 on
the first rows) and hand-made filtered buffers for what no frame reaches."""
import functools
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_lz_ref as Z
import png_ref as R

pytestmark = pytest.mark.gpu

CASES = [(shape, sr, kind) for shape, sr in R.CASES for kind in Z.KINDS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-sr{sr}-{k}" for s, sr, k in CASES]


@functools.lru_cache(maxsize=None)
def _encoder(stripe_rows, matches=True, gpu_crc=None):
    from stable_diffusion_videos_amd.png import PngEncoder
    return PngEncoder(torch.device("cuda", 0), stripe_rows=stripe_rows, matches=matches, gpu_crc=gpu_crc)


def _token_lists(words, counts, H, Rb, rows):
    """tokens[k][s] from the encoder's int32 [n, H R] words and [n, stripes] counts."""
    return [[Z.unpack_tokens(words[k, r0 * Rb:], int(counts[k, s])) for s, r0 in enumerate(range(0, H, rows))] for k in range(words.shape[0])]


@functools.lru_cache(maxsize=None)
def _run(shape, sr, kind):
    """One encode per case, shared by the tests; arrays as numpy, tokens as lists."""
    frames = Z.make_frames(kind, *shape)
    files, filtered, l0, words, counts, ll, dl = _encoder(sr).encode(torch.from_numpy(frames).cuda(), return_tables=True)
    rows = sr or R.default_stripe_rows(shape[1], shape[2])
    filtered, words, counts = filtered.cpu().numpy(), words.cpu().numpy().view(np.uint32), counts.cpu().numpy()
    tokens = _token_lists(words, counts, shape[1], filtered.shape[2], rows)
    return dict(frames=frames, files=files, filtered=filtered, l0=l0.cpu().numpy(), tokens=tokens, ll=ll.cpu().numpy(), dl=dl.cpu().numpy(), rows=rows)


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_tokens_equal_the_restatement(hip, shape, sr, kind):
    """(1) token for token, the restatement run on the GPU's own filtered rows and literal prices; the filtered rows and the prices are
    what the Huffman-only encoder gives."""
    r = _run(shape, sr, kind)
    _, filtered, l0 = _encoder(sr, False).encode(torch.from_numpy(r["frames"]).cuda(), return_tables=True)
    assert np.array_equal(filtered.cpu().numpy(), r["filtered"]) and np.array_equal(l0.cpu().numpy(), r["l0"])
    want = Z.tokenize_frames(r["filtered"], r["l0"], r["rows"])
    for k in range(shape[0]):
        for s, r0 in enumerate(range(0, shape[1], r["rows"])):
            got = r["tokens"][k][s]
            assert got == want[k][s], (k, s, len(got), len(want[k][s]), next((i for i, (a, b) in enumerate(zip(got, want[k][s])) if a != b), None))
            Z.check_tokens(got, r["filtered"][k, r0:r0 + r["rows"]].reshape(-1))


def _check_code(lengths, hist):
    """Valid: 0 exactly for unused symbols, at most 15, Kraft sum exactly 1 - or the single code of length 1, or no code at all;
    optimal where the heap's code is at most 15 deep."""
    lengths = [int(l) for l in lengths]
    used = [s for s, c in enumerate(hist) if c]
    assert len(lengths) == len(hist)
    for s, c in enumerate(hist):
        assert (lengths[s] == 0) == (c == 0) and 0 <= lengths[s] <= 15, (s, lengths[s], c)
    if len(used) == 1:
        assert lengths[used[0]] == 1
    elif used:
        assert sum(1 << (15 - l) for l in lengths if l) == 1 << 15
    if used and R.optimal_depth(hist) <= 15:
        assert sum(c * l for c, l in zip(hist, lengths)) == R.optimal_cost(hist)


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_final_code_lengths_are_valid_and_optimal(hip, shape, sr, kind):
    """(3) per stripe, both codes; a stripe without a match carries the literal prices and no distance code."""
    r = _run(shape, sr, kind)
    for k in range(shape[0]):
        for s, tokens in enumerate(r["tokens"][k]):
            ll, dd = Z.histograms(tokens)
            if not any(dd):
                assert list(r["ll"][k, s][:257]) == list(r["l0"][k, s]) and not r["ll"][k, s][257:].any() and not r["dl"][k, s].any()
            _check_code(r["ll"][k, s], ll)
            _check_code(r["dl"][k, s], dd)


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_file_bytes_equal_the_sequential_packer(hip, shape, sr, kind):
    """(4) from signature to IEND, the four CRC bytes included (the packer's CRC is the bitwise one)."""
    r = _run(shape, sr, kind)
    want = Z.pack(r["filtered"], r["tokens"], r["l0"], r["ll"], r["dl"], shape[1], shape[2], r["rows"])
    assert len(r["files"]) == shape[0]
    for k in range(shape[0]):
        assert r["files"][k] == want[k], (k, len(r["files"][k]), len(want[k]))


@pytest.mark.parametrize("shape,sr,kind", CASES, ids=IDS)
def test_independent_decoders(hip, shape, sr, kind):
    """(5) zlib inflates every IDAT payload to the filtered bytes, PIL decodes every file to the frame, png_ref.chunks accepts every
    CRC; with gpu_crc=True and matches=False the files are today's byte for byte."""
    r = _run(shape, sr, kind)
    for k, data in enumerate(r["files"]):
        assert zlib.decompress(R.idat(data)) == r["filtered"][k].tobytes()
        assert np.array_equal(R.decode(data), r["frames"][k])
    t = torch.from_numpy(r["frames"]).cuda()
    assert _encoder(sr, False, True).encode(t) == _encoder(sr, False).encode(t)


# ---- (2) hand-made filtered buffers straight through k_png_deflate_lz_pack -----------------------------------------------------
def _lz_direct(hip, dev, buf, stripe_rows, lz=True, cap=None, guard=0):
    """sdv_png_deflate_lz_pack (or sdv_png_deflate_pack) + sdv_png_crc32 on a filtered buffer [n, H, R]: dict of files, tables, tokens."""
    from stable_diffusion_videos_amd.png import png_header
    n, H, Rb = buf.shape
    W = (Rb - 1) // 3
    stripes = -(-H // stripe_rows)
    header = torch.frombuffer(bytearray(png_header(H, W)), dtype=torch.uint8).to(dev)
    scratch = torch.empty((hip.png_scratch_bytes(n, H, stripe_rows),), dtype=torch.uint8, device=dev)
    lzb = hip.png_lz_scratch_bytes(n, H, W, stripe_rows)
    cap = 2 * buf.size + 1024 * n * stripes if cap is None else cap
    fill = lambda numel, dtype=torch.uint8: torch.full((numel,), 0xA5 if dtype == torch.uint8 else -1515870811, dtype=dtype, device=dev)
    out, lzs, meta, acc = fill(cap + guard), fill(lzb + guard), fill(2 * (n + 2 + guard // 8), torch.int32).view(torch.int64), fill(n + guard // 4, torch.int32)
    l0, ll, dl = fill(n * stripes * 257 + guard), fill(n * stripes * 286 + guard), fill(n * stripes * 30 + guard)
    args = (torch.from_numpy(buf).to(dev), torch.from_numpy(R.adler_partials(buf)).to(dev), stripe_rows, header, scratch, out[:cap], meta[:n + 1],
            meta[n + 1:n + 2])
    if lz:
        hip.png_deflate_lz_pack(*args, lzs[:lzb], l0[:n * stripes * 257].view(n, stripes, 257), ll[:n * stripes * 286].view(n, stripes, 286),
                                dl[:n * stripes * 30].view(n, stripes, 30))
    else:
        hip.png_deflate_pack(*args, l0[:n * stripes * 257].view(n, stripes, 257))
    hip.png_crc32(out[:cap], meta[:n + 1], meta[n + 1:n + 2], acc[:n])
    torch.cuda.synchronize()
    offs = meta[:n + 2].tolist()
    res = dict(needed=offs[n + 1], out=out.cpu().numpy(), guards=[t[k:] for t, k in ((out, cap), (lzs, lzb), (l0, n * stripes * 257),
                                                                                       (ll, n * stripes * 286), (dl, n * stripes * 30))] +
               [meta[n + 2:].view(torch.uint8), acc[n:].view(torch.uint8)])
    assert offs[n] == offs[n + 1]
    if offs[n + 1] <= cap:
        res["files"] = [res["out"][offs[k]:offs[k + 1]].tobytes() for k in range(n)]
    res["l0"] = l0[:n * stripes * 257].view(n, stripes, 257).cpu().numpy()
    if lz:
        words = lzs[:lzb].view(torch.int32).cpu().numpy().view(np.uint32)
        res["tokens"] = _token_lists(words[:buf.size].reshape(n, -1), words[buf.size:buf.size + n * stripes].reshape(n, stripes), H, Rb, stripe_rows)
        res["ll"], res["dl"] = ll[:n * stripes * 286].view(n, stripes, 286).cpu().numpy(), dl[:n * stripes * 30].view(n, stripes, 30).cpu().numpy()
    return res


def _check_direct(res, buf, stripe_rows):
    """tokens = the restatement's on the kernel's prices; every file inflates to its rows; every CRC holds"""
    want = Z.tokenize_frames(buf, res["l0"], stripe_rows)
    assert res["tokens"] == want
    for k, data in enumerate(res["files"]):
        assert zlib.decompress(R.idat(data)) == buf[k].tobytes()
    return want


@pytest.mark.parametrize("period", (28, 27))
def test_repeat_beyond_and_inside_the_window(hip, dev, period):
    """[1, 56, 1201] in one stripe (L = 67 256), rows without any repeated 3 bytes, repeating with period 28: the only repeat lies
    33 628 back, beyond 32 768 - refused, the stripe is the Huffman-only stripe byte for byte.  Period 27: 32 427 back - taken, with
    distance symbol 29 and its 13 extra bits."""
    buf = Z.periodic_rows(period)
    res = _lz_direct(hip, dev, buf, 56)
    tokens = _check_direct(res, buf, 56)[0][0]
    matches = [t for t in tokens if isinstance(t, tuple)]
    if period == 28:
        assert not matches and res["files"] == _lz_direct(hip, dev, buf, 56, lz=False)["files"]
    else:
        assert matches and {d for _, d in matches} == {27 * 1201} and Z.dist_symbol(27 * 1201)[:2] == (29, 13)
        assert res["dl"][0, 0, 29] == 1 and not res["dl"][0, 0, :29].any()
        assert len(res["files"][0]) < len(_lz_direct(hip, dev, buf, 56, lz=False)["files"][0])


def test_hand_made_buffers(hip, dev):
    """Two identical stripes: nothing reaches across the stripe start.  A period-5 pattern: 5 is no fixed distance and is found only
    through the hash, from position 64 on (one match to the stripe's end: one distance symbol, the code of length 1).  A period-70
    pattern: found at position 70, once the source lies in an earlier group, capped at 258.  The two Fibonacci buffers: the limiter
    and the Kraft sum on 286 symbols."""
    row = Z.periodic_rows(1)[:, :1, :94]
    twice = np.concatenate([row, row], axis=1)                                   # [1, 2, 94], stripe_rows = 1
    res = _lz_direct(hip, dev, twice, 1)
    tokens = _check_direct(res, twice, 1)[0]
    assert tokens[0] == tokens[1] == row.reshape(-1).tolist()
    p5 = (np.arange(8 * 31) % 5 + 1).astype(np.uint8).reshape(1, 8, 31)
    res = _lz_direct(hip, dev, p5, 8)
    tokens = _check_direct(res, p5, 8)[0][0]
    assert tokens == p5.reshape(-1)[:64].tolist() + [(8 * 31 - 64, 5)]
    assert res["dl"][0, 0].tolist() == [0, 0, 0, 0, 1] + [0] * 25
    p70 = (np.arange(12 * 31) % 70 + 1).astype(np.uint8).reshape(1, 12, 31)
    res = _lz_direct(hip, dev, p70, 12)
    tokens = _check_direct(res, p70, 12)[0][0]
    assert tokens == p70.reshape(-1)[:70].tolist() + [(258, 70), (12 * 31 - 328, 70)]
    for buf, stripe_rows in ((R.fibonacci_buffer(), 113), (R.forced_deep_buffer(), 1)):
        res = _lz_direct(hip, dev, buf, stripe_rows)
        tokens = _check_direct(res, buf, stripe_rows)[0][0]
        ll, dd = Z.histograms(tokens)
        _check_code(res["ll"][0, 0], ll)
        _check_code(res["dl"][0, 0], dd)
        assert any(dd) and R.optimal_depth(R.stripe_histograms(buf[0], stripe_rows)[0]) > 15
        assert res["files"] == Z.pack(buf, res["tokens"], res["l0"], res["ll"], res["dl"], buf.shape[1], (buf.shape[2] - 1) // 3, stripe_rows)


def test_determinism_and_batch_independence(hip, dev):
    """(6) two encodes are bit-identical; frame k of a batch equals the same frame encoded alone."""
    for shape, sr, kind in (((3, 40, 56), None, "smooth"), ((2, 5, 7), 2, "glyphs")):
        r = _run(shape, sr, kind)
        t = torch.from_numpy(r["frames"]).to(dev)
        assert _encoder(sr).encode(t) == r["files"]
        for k in range(shape[0]):
            assert _encoder(sr).encode(t[k:k + 1]) == [r["files"][k]]


def test_memory_bounds_and_small_capacity(hip, dev):
    """(7), (8) 0xA5 guards behind out, the token scratch, offsets, the CRC workspace and every returned table stay; a capacity that
    is too small reports the needed size and nothing is written - by the packer or by the CRC launches -, the encoder retries once."""
    from stable_diffusion_videos_amd import png
    G = 4096
    for shape, sr, kind in (((2, 5, 7), 2, "glyphs"), ((1, 70, 24), 1, "smooth"), ((3, 40, 56), None, "plateaus")):
        r = _run(shape, sr, kind)
        total = sum(len(f) for f in r["files"])
        for cap in (total, total - 1, total // 2, 1):
            res = _lz_direct(hip, dev, r["filtered"], r["rows"], cap=cap, guard=G)
            assert res["needed"] == total
            for g in res["guards"]:
                assert g.numel() >= G // 8 and bool((g == 0xA5).all())
            assert res["tokens"] == r["tokens"] and np.array_equal(res["ll"], r["ll"]) and np.array_equal(res["dl"], r["dl"])
            if cap >= total:
                assert res["files"] == r["files"]
            else:
                assert (res["out"][:cap] == 0xA5).all()
    enc = png.PngEncoder(dev, matches=True)
    noise = R.make_frames("noise", 1, 64, 64)
    data = enc.encode(torch.from_numpy(noise).to(dev))
    assert enc.retries == 1 and np.array_equal(R.decode(data[0]), noise[0])
    R.chunks(data[0])
    assert enc.encode(torch.from_numpy(noise).to(dev)) == data and enc.retries == 1


# ---- (9) public surface ------------------------------------------------------------------------------------------------------
def _tiny_pipeline(dev):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    return StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)


def test_output_type_png_with_matches(hip, dev, monkeypatch):
    pipe = _tiny_pipeline(dev)
    batches = list(pipe.generate_inputs("a cat", "a dog", 42, 1337, (1, 4, 8, 8), np.linspace(0.0, 1.0, 2), 2))
    _, embeds, noise = batches[0]
    kw = dict(latents=noise, text_embeddings=embeds, height=64, width=64, num_inference_steps=2)
    monkeypatch.delenv("SDV_PNG_MATCHES", raising=False)
    plain = pipe(output_type="png", **kw)["images"]
    monkeypatch.setenv("SDV_PNG_MATCHES", "1")
    images = pipe(output_type="png", **kw)["images"]
    from stable_diffusion_videos_amd import png
    assert len(images) == len(plain) == 2 and any(enc.matches and enc.gpu_crc and enc._ws for enc in png._encoders.values())
    for data, ref in zip(images, plain):
        R.chunks(data)
        assert np.array_equal(R.decode(data), R.decode(ref))
    monkeypatch.setenv("SDV_PNG_MATCHES", "0")
    pipe.png_matches = True
    assert pipe(output_type="png", **kw)["images"] == plain


def test_walk_writes_png_frames_with_matches(hip, dev, tmp_path, monkeypatch):
    pipe = _tiny_pipeline(dev)
    kw = dict(output_dir=str(tmp_path), fps=3, num_inference_steps=2, height=64, width=64, make_video=False, image_file_ext=".png")
    walk = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=3, batch_size=2)
    monkeypatch.delenv("SDV_PNG", raising=False)
    monkeypatch.delenv("SDV_PNG_MATCHES", raising=False)
    pipe.walk(name="p", **walk, **kw)                                            # the default path: Image.save
    monkeypatch.setenv("SDV_PNG", "hip")
    pipe.walk(name="h", **walk, **kw)                                            # today's HIP path
    monkeypatch.setenv("SDV_PNG_MATCHES", "1")
    pipe.walk(name="m", **walk, **kw)
    monkeypatch.delenv("SDV_PNG_MATCHES")
    pipe.walk(name="h2", **walk, **kw)
    names = [f"frame{k:06d}.png" for k in range(3)]
    for name in names:
        ref = np.asarray(Image.open(tmp_path / "p" / "p_000000" / name).convert("RGB"))
        data = (tmp_path / "m" / "m_000000" / name).read_bytes()
        R.chunks(data)
        assert np.array_equal(R.decode(data), ref)
        plain = (tmp_path / "h" / "h_000000" / name).read_bytes()
        assert (tmp_path / "h2" / "h2_000000" / name).read_bytes() == plain and np.array_equal(R.decode(plain), ref)
