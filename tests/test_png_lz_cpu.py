"""The PNG encoder's matching mode without a GPU: the restatement of the stream rule (tests/png_lz_ref.py) is held against zlib and PIL
as independent, strict decoders and against the size conditions the rule was designed for; the bitwise CRC against zlib's; the C ABI
and the wrappers of the two new entry points validate their arguments before any launch."""
import ctypes
import functools
import os
import re
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import png_lz_ref as Z
import png_ref as R

ROOT = Path(__file__).resolve().parent.parent
SHAPES = R.CASES + (((1, 96, 96), None),)


@functools.lru_cache(maxsize=None)
def _encode(shape, sr, kind):
    frames = Z.make_frames(kind, *shape)
    return (frames,) + Z.encode(frames, sr)


def test_restatement_decodes_exactly_in_zlib_and_pil():
    """(1) every file of the restatement inflates to the filtered bytes (zlib checks the Adler-32, both tables and every distance)
    and decodes in PIL to the frame."""
    for shape, sr in R.CASES:
        for kind in Z.KINDS:
            frames, files, _, filtered, _ = _encode(shape, sr, kind)
            assert len(files) == shape[0]
            for k, data in enumerate(files):
                assert zlib.decompress(R.idat(data)) == filtered[k].tobytes()
                assert np.array_equal(R.decode(data), frames[k])


def test_tokens_are_legal_and_reproduce_the_stripe():
    """(2) 3 <= len <= 258, 1 <= d <= min(i, 32768), the bytes equal; the cases hold matches at the cap, matches to the stripe's end,
    the row distances and stripes too short for any candidate."""
    seen_len, seen_dist = set(), set()
    for shape, sr in R.CASES:
        rows = sr or R.default_stripe_rows(shape[1], shape[2])
        for kind in Z.KINDS:
            _, _, _, filtered, tokens = _encode(shape, sr, kind)
            for k in range(shape[0]):
                for s, r0 in enumerate(range(0, shape[1], rows)):
                    Z.check_tokens(tokens[k][s], filtered[k, r0:r0 + rows].reshape(-1))
                    seen_len |= {t[0] for t in tokens[k][s] if isinstance(t, tuple)}
                    seen_dist |= {(t[1], filtered.shape[2]) for t in tokens[k][s] if isinstance(t, tuple)}
    assert 258 in seen_len and 3 in seen_len
    assert any(d == Rb for d, Rb in seen_dist) and any(d in (Rb - 3, Rb + 3) for d, Rb in seen_dist) and any(d == 1 for d, _ in seen_dist)
    for buf, period in ((Z.periodic_rows(28), 28), (Z.periodic_rows(27), 27)):      # the premises of the GPU suite's window test
        l0 = R.heap_lengths(R.stripe_histograms(buf[0], 56)[0])
        matches = [t for t in Z.tokenize(buf.reshape(-1), l0, 1201) if isinstance(t, tuple)]
        assert (not matches) if period == 28 else (matches and {d for _, d in matches} == {32427})


def test_size_conditions_of_the_rule():
    """(3) a file with matches is never more than the larger table (29 bytes; 30 allowed) per stripe above the Huffman-only file; the
    zlib streams of flat and quantised frames shrink to the pinned ratios (measured on this restatement: 0.0578, 0.1234, 0.9555;
    pinned at + 10 %)."""
    for shape, sr in SHAPES:
        stripes = -(-shape[1] // (sr or R.default_stripe_rows(shape[1], shape[2])))
        for kind in Z.KINDS:
            _, files, plain, _, _ = _encode(shape, sr, kind)
            for a, b in zip(files, plain):
                assert len(a) <= len(b) + 30 * stripes, (shape, kind, len(a), len(b))
    ratio = {}
    for kind in ("zeros", "glyphs", "plateaus"):
        _, files, plain, _, _ = _encode((1, 96, 96), None, kind)
        ratio[kind] = len(R.idat(files[0])) / len(R.idat(plain[0]))
    print(ratio)
    assert ratio["zeros"] <= 0.0578 * 1.1 and ratio["glyphs"] <= 0.1234 * 1.1 and ratio["plateaus"] <= 0.9555 * 1.1, ratio


def test_bitwise_crc_equals_zlib():
    """(4)"""
    rng = np.random.default_rng(3)
    for size in (0, 1, 4, 255, 256, 257, 5000):
        data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        assert Z.crc32_bitwise(data) == zlib.crc32(data)
    assert Z.crc32_bitwise(b"IEND") == 0xAE426082


def test_header_library_and_binding_agree_on_the_new_entry_points(hip):
    """(5)"""
    header = (ROOT / "include" / "sdv_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in (("sdv_png_deflate_lz_pack", "k_png_deflate_lz_pack"), ("sdv_png_crc32", "k_png_crc32")):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(lib, name) and name in hip.EXPORTED_SYMBOLS
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._SIGNATURES[name][1]), name
    assert "Matching mode" in header and "0x9E3779B1" in header
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    assert hip.png_lz_scratch_bytes(2, 5, 7, 2) == 4 * 2 * 5 * 22 + 8 * 3 + 1280 * 6
    src = (ROOT / "stable_diffusion_videos_amd" / "png.py").read_text()
    assert "import ctypes" not in src and "lib.sdv_" not in src


def test_wrappers_refuse_cpu_tensors_wrong_dtypes_shapes_and_capacities(hip):
    """(6) the binding's checks"""
    from stable_diffusion_videos_amd.png import PngEncoder, encoder_for
    enc = PngEncoder(matches=True)
    assert enc.matches and enc.gpu_crc and not PngEncoder().gpu_crc and not PngEncoder(matches=True, gpu_crc=False).gpu_crc
    assert PngEncoder(gpu_crc=True).gpu_crc and not PngEncoder(gpu_crc=True).matches
    assert encoder_for("cuda:0", matches=True) is encoder_for("cuda:0", True) is not encoder_for("cuda:0")
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        enc.encode(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    i64 = lambda k: torch.zeros((k,), dtype=torch.int64)
    pack = torch.ops.sdv.k_png_deflate_lz_pack
    sb, lzb = hip.png_scratch_bytes(1, 4, 2), hip.png_lz_scratch_bytes(1, 4, 4, 2)
    ok = dict(filtered=u8(1, 4, 13), adler_rows=i32(1, 4, 2), stripe_rows=2, header=u8(33), scratch=u8(sb), out=u8(100), offsets=i64(2),
              needed=i64(1), lz_scratch=u8(lzb), lengths=u8(1, 2, 257), ll_lengths=u8(1, 2, 286), d_lengths=u8(1, 2, 30))
    for key, val, word in (("filtered", u8(1, 4, 12), "filtered must be"), ("adler_rows", i32(1, 3, 2), "adler_rows must be"),
                           ("stripe_rows", 0, "stripe_rows"), ("stripe_rows", 5, "stripe_rows"), ("header", u8(32), "33 bytes"),
                           ("scratch", u8(sb - 1), "scratch holds"), ("out", u8(10, 10), "out must be"), ("offsets", i64(1), "offsets must be"),
                           ("needed", i64(2), "needed must be"), ("lz_scratch", u8(lzb - 1), "lz_scratch holds"),
                           ("lz_scratch", i32(lzb), "lz_scratch must be"), ("lengths", u8(1, 2, 256), "lengths must be"),
                           ("ll_lengths", u8(1, 2, 285), "ll_lengths must be"), ("d_lengths", u8(1, 2, 31), "d_lengths must be"),
                           ("d_lengths", None, "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            pack(*dict(ok, **{key: val}).values())
    crc = torch.ops.sdv.k_png_crc32
    ok = dict(out=u8(100), offsets=i64(3), needed=i64(1), acc=i32(2))
    for key, val, word in (("out", u8(10, 10), "out must be"), ("out", i32(100), "out must be"), ("offsets", i64(1), "offsets must be"),
                           ("offsets", i32(3), "offsets must be"), ("needed", i64(2), "needed must be"), ("acc", i32(3), "acc must be"),
                           ("acc", i64(2), "acc must be"), ("acc", i32(2), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            crc(*dict(ok, **{key: val}).values())


def test_c_abi_validates_before_any_launch(hip):
    """(6) the library's checks"""
    lib = hip.load()
    stripes = 2 * 3                                                             # n = 2 frames x ceil(40 / 16) stripes
    want = 16 * stripes + 8 + 1040 * stripes
    lz_want = 4 * 2 * 40 * 169 + 8 * 3 + 1280 * stripes
    ok = [16, 32, 2, 40, 56, 16, 48, 33, 64, want, 128, 1000, 256, 512, None, 1024, lz_want, None, None, None]
    for pos, val, word in ((0, None, b"null"), (1, None, b"null"), (6, None, b"null"), (8, None, b"null"), (10, None, b"null"),
                           (12, None, b"null"), (13, None, b"null"), (15, None, b"null"), (2, 0, b"frame count"), (3, 0, b"frame size"),
                           (4, 16385, b"frame size"), (5, 0, b"stripe_rows"), (5, 41, b"stripe_rows"), (7, 32, b"header length"),
                           (9, want - 1, b"scratch buffer too small"), (11, -1, b"capacity"), (8, 68, b"aligned"), (0, 18, b"aligned"),
                           (12, 260, b"aligned"), (16, lz_want - 1, b"token scratch too small"), (15, 1028, b"token scratch must be 8-byte")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_png_deflate_lz_pack(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_png_deflate_lz_pack")
    ok = [64, 1000, 128, 256, 2, 512, None]
    for pos, val, word in ((0, None, b"null"), (2, None, b"null"), (3, None, b"null"), (5, None, b"null"), (4, 0, b"frame count"),
                           (4, 65536, b"frame count"), (1, -1, b"capacity"), (2, 132, b"aligned"), (3, 260, b"aligned"), (5, 514, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_png_crc32(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())


def test_sdv_png_matches_selects_the_mode_and_refuses_other_values(monkeypatch):
    """(7) the default, the precedence of the variable, bad values; the encoder choice is untouched."""
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_PNG_MATCHES", raising=False)
    monkeypatch.delenv("SDV_PNG", raising=False)
    assert pipe.png_matches is False and pipe.png_matches_choice() is False and pipe.png_encoder_choice() == "pil"
    pipe.png_matches = True
    assert pipe.png_matches_choice() is True and pipe.png_encoder_choice() == "pil"
    monkeypatch.setenv("SDV_PNG_MATCHES", "0")                                   # the variable wins when it is set
    assert pipe.png_matches_choice() is False
    pipe.png_matches = False
    monkeypatch.setenv("SDV_PNG_MATCHES", "1")
    assert pipe.png_matches_choice() is True
    for bad in ("true", "yes", "2", "hip", " 1"):
        monkeypatch.setenv("SDV_PNG_MATCHES", bad)
        with pytest.raises(ValueError, match="SDV_PNG_MATCHES"):
            pipe.png_matches_choice()
    assert "SDV_PNG_MATCHES" in os.environ
