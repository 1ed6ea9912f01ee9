"""Host side of the PNG encoder (png.py, the two C entry points) without a GPU: the restatement of the stream format (tests/png_ref.py)
is held against zlib and PIL (libpng) as independent, strict decoders, and the C ABI and the wrappers validate their arguments before
any launch."""
import ctypes
import re
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

import png_ref as R

ROOT = Path(__file__).resolve().parent.parent


def test_restatement_decodes_exactly_in_zlib_and_pil():
    """pack(filter_rows(f), heap lengths) inflates to the filtered bytes (zlib checks the Adler-32 and every table) and decodes in PIL
    to f, for every shape and kind of the GPU suite; every heap code is at most 15 deep there, the premise of the GPU suite's cost
    check."""
    for (n, H, W), sr in R.CASES:
        sr = sr or R.default_stripe_rows(H, W)
        for kind in R.KINDS:
            frames = R.make_frames(kind, n, H, W)
            files, filtered = R.encode(frames, sr)
            assert len(files) == n
            for k in range(n):
                assert zlib.decompress(R.idat(files[k])) == filtered[k].tobytes()
                assert np.array_equal(R.decode(files[k]), frames[k])
                assert files[k].startswith(R.png_header(H, W)) and files[k][37:43] == b"IDAT\x78\x01"
                for h in R.stripe_histograms(filtered[k], sr):
                    assert R.optimal_depth(h) <= 15
                    R.check_lengths(R.heap_lengths(h), h, optimal=True)


def test_filter_choice_of_the_restatement():
    """Noise picks all five filter types, zeros pick None everywhere; the filtered rows are what libpng's own defiltering inverts
    (the PIL decode above), and ties go to the lowest type: a constant frame costs the same under Sub and Paeth from row 1 on."""
    kinds = set()
    for (n, H, W), _ in R.CASES:
        kinds |= set(R.filter_rows(R.make_frames("noise", n, H, W))[:, :, 0].reshape(-1).tolist())
        assert not R.filter_rows(R.make_frames("zeros", n, H, W))[:, :, 0].any()
    assert kinds == {0, 1, 2, 3, 4}
    const = R.filter_rows(R.make_frames("const255", 1, 5, 7))[0]
    assert const[0, 0] == 1 and (const[1:, 0] == 2).all()                       # Sub for row 0 (Paeth ties), Up below (cost 0, before Paeth)


def test_length_limit_case_is_deeper_than_15_by_the_restatement():
    """The hand-made buffers of the GPU suite's length-limiting test.  17 values with the Fibonacci counts 1, 1, 2, ..., 1597 behind a
    type byte: with end-of-block an unrestricted Huffman code of it is 17 deep - with the heap's tie-break; a leaf-first tie-break
    finds an equally cheap code that is 10 deep.  The second buffer leaves no ties: every Huffman code of it is 17 deep."""
    buf = R.fibonacci_buffer()
    assert buf.size == 4181 and sorted(np.bincount(buf.reshape(-1)[1:])) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
    hist = R.stripe_histograms(buf[0], buf.shape[1])[0]
    assert R.optimal_depth(hist) == 17 > 15 and R.optimal_depth(hist, shallow=True) == 10
    assert sum(c * l for c, l in zip(hist, R.heap_lengths(hist, shallow=True))) == R.optimal_cost(hist)
    forced = R.forced_deep_buffer()
    hist = R.stripe_histograms(forced[0], 1)[0]
    assert sorted(hist[hist > 0]) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584]
    assert R.optimal_depth(hist) == 17 == R.optimal_depth(hist, shallow=True)


def test_product_header_and_stripes_equal_the_restatement():
    from stable_diffusion_videos_amd import hip, png
    for H, W in ((1, 1), (64, 64), (512, 512), (2048, 2048), (16384, 16384), (5, 7)):
        assert png.png_header(H, W) == R.png_header(H, W) and len(png.png_header(H, W)) == 33
        assert png.default_stripe_rows(H, W) == R.default_stripe_rows(H, W)
        assert hip.png_stripes(H, W, None) == -(-H // R.default_stripe_rows(H, W))
    assert png.default_stripe_rows(512, 512) == 21 and png.default_stripe_rows(2048, 2048) == 5
    assert png.default_stripe_rows(16384, 16384) == 1 and png.default_stripe_rows(3, 8) == 3
    assert hip.png_stripes(33, 19, 16) == 3 and hip.png_scratch_bytes(2, 5, 2) == 16 * 6 + 8 + 1040 * 6
    for bad in ((0, 4), (4, 0), (16385, 4), (4, 16385)):
        with pytest.raises(ValueError, match="frame size"):
            png.png_header(*bad)
    with pytest.raises(hip.SdvHipError, match="stripe_rows"):
        hip.png_stripes(4, 4, 5)
    with pytest.raises(ValueError, match="stripe_rows"):
        png.PngEncoder(stripe_rows=0)


def test_header_library_and_binding_agree_on_the_png_entry_points(hip):
    header = (ROOT / "include" / "sdv_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in (("sdv_png_filter_u8", "k_png_filter"), ("sdv_png_deflate_pack", "k_png_deflate_pack")):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(lib, name) and name in hip.EXPORTED_SYMBOLS
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._SIGNATURES[name][1]), name
    assert "PNG encoder" in header
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    src = (ROOT / "stable_diffusion_videos_amd" / "png.py").read_text()
    assert "import ctypes" not in src and "lib.sdv_" not in src


def test_wrappers_refuse_cpu_tensors_wrong_dtypes_shapes_and_capacities(hip):
    from stable_diffusion_videos_amd.png import PngEncoder
    enc = PngEncoder()
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        enc.encode(torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)
    i64 = lambda k: torch.zeros((k,), dtype=torch.int64)
    flt = torch.ops.sdv.k_png_filter
    with pytest.raises(hip.SdvHipError, match="GPU memory"):
        flt(u8(1, 4, 4, 3), u8(1, 4, 13), i32(1, 4, 2))
    with pytest.raises(hip.SdvHipError, match="frames must be"):
        flt(torch.zeros((1, 4, 4, 3)), u8(1, 4, 13), i32(1, 4, 2))
    with pytest.raises(hip.SdvHipError, match="frames must be"):
        flt(u8(1, 4, 4, 4), u8(1, 4, 13), i32(1, 4, 2))
    with pytest.raises(hip.SdvHipError, match="frame size"):
        flt(u8(1, 1, 16385, 3), u8(1, 1, 49156), i32(1, 1, 2))
    with pytest.raises(hip.SdvHipError, match="filtered must be"):
        flt(u8(1, 4, 4, 3), u8(1, 4, 12), i32(1, 4, 2))
    with pytest.raises(hip.SdvHipError, match="adler_rows must be"):
        flt(u8(1, 4, 4, 3), u8(1, 4, 13), i64(8).view(1, 4, 2))
    pack = torch.ops.sdv.k_png_deflate_pack
    sb = hip.png_scratch_bytes(1, 4, 2)
    ok = dict(filtered=u8(1, 4, 13), adler_rows=i32(1, 4, 2), stripe_rows=2, header=u8(33), scratch=u8(sb), out=u8(100), offsets=i64(2),
              needed=i64(1), lengths=u8(1, 2, 257))
    for key, val, word in (("filtered", u8(1, 4, 12), "filtered must be"), ("filtered", i32(1, 4, 13), "filtered must be"),
                           ("adler_rows", i32(1, 3, 2), "adler_rows must be"), ("stripe_rows", 0, "stripe_rows"),
                           ("stripe_rows", 5, "stripe_rows"), ("header", u8(32), "33 bytes"), ("scratch", u8(sb - 1), "scratch holds"),
                           ("out", u8(10, 10), "out must be"), ("offsets", i64(1), "offsets must be"), ("needed", i64(2), "needed must be"),
                           ("lengths", u8(1, 2, 256), "lengths must be"), ("lengths", None, "GPU memory"), ("out", u8(1), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            pack(*dict(ok, **{key: val}).values())


def test_c_abi_validates_before_any_launch(hip):
    lib = hip.load()
    ok = [16, 2, 40, 56, 32, 64, None]
    for pos, val, word in ((0, None, b"null"), (4, None, b"null"), (5, None, b"null"), (1, 0, b"frame count"), (1, 65536, b"frame count"),
                           (2, 0, b"frame size"), (2, 16385, b"frame size"), (3, 0, b"frame size"), (3, 16385, b"frame size"),
                           (5, 66, b"4-byte aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_png_filter_u8(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    stripes = 2 * 3                                                             # n = 2 frames x ceil(40 / 16) stripes
    want = 16 * stripes + 8 + 1040 * stripes
    ok = [16, 32, 2, 40, 56, 16, 48, 33, 64, want, 128, 1000, 256, 512, None, None]
    for pos, val, word in ((0, None, b"null"), (1, None, b"null"), (6, None, b"null"), (8, None, b"null"), (10, None, b"null"),
                           (12, None, b"null"), (13, None, b"null"), (2, 0, b"frame count"), (3, 0, b"frame size"),
                           (4, 16385, b"frame size"), (5, 0, b"stripe_rows"), (5, 41, b"stripe_rows"), (7, 32, b"header length"),
                           (9, want - 1, b"scratch buffer too small"), (11, -1, b"capacity"), (8, 68, b"aligned"), (0, 18, b"aligned"),
                           (12, 260, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_png_deflate_pack(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())


def test_sdv_png_selects_the_encoder_and_refuses_other_values(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_PNG", raising=False)
    assert pipe.png_encoder == "pil" == pipe.png_encoder_choice()
    pipe.png_encoder = "hip"
    assert pipe.png_encoder_choice() == "hip"
    monkeypatch.setenv("SDV_PNG", "pil")                                         # the variable wins when it is set
    assert pipe.png_encoder_choice() == "pil"
    monkeypatch.setenv("SDV_PNG", "HIP")
    pipe.png_encoder = "pil"
    assert pipe.png_encoder_choice() == "hip"
    for bad in ("zlib", "gpu", "1"):
        monkeypatch.setenv("SDV_PNG", bad)
        with pytest.raises(ValueError, match="SDV_PNG"):
            pipe.png_encoder_choice()
    monkeypatch.delenv("SDV_PNG")
    pipe.png_encoder = "libpng"
    with pytest.raises(ValueError, match="png_encoder"):
        pipe.png_encoder_choice()


def test_output_type_png_on_a_cpu_pipeline_raises(hip):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    with pytest.raises(hip.SdvHipError):
        pipe("a cat", height=64, width=64, num_inference_steps=1, output_type="png")
