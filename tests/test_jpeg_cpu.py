"""Host side of the JPEG encoder (jpeg.py, the two C entry points) without a GPU: the float64 restatement of the stream format
(tests/jpeg_ref.py) is held against PIL (libjpeg) as decoder and as encoder, the product's tables and header against the
restatement's and against the tables PIL writes, and the C ABI validates its arguments before any launch."""
import ctypes
import io
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_ref as R

ROOT = Path(__file__).resolve().parent.parent


def test_restatement_against_pil():
    """Every file of the restatement opens in PIL with the right size and mode; PSNR against the source and file size stay within the
    margins recorded in jpeg_ref.py of PIL's own save(quality=q, subsampling=2) on the same image.  The GPU thresholds derive from these."""
    worst_gap, worst_ratio = 0.0, 0.0
    for n, H, W in R.SHAPES:
        for kind in R.KINDS:
            frames = R.make_frames(kind, n, H, W)
            for q in (1, 75, 95, 100):
                for k, data in enumerate(R.encode(frames, q)):
                    got = R.decode(data)
                    assert got.shape == (H, W, 3)
                    pil = R.pil_encode(frames[k], q)
                    worst_gap = max(worst_gap, R.psnr(R.decode(pil), frames[k]) - R.psnr(got, frames[k]))
                    worst_ratio = max(worst_ratio, len(data) / len(pil))
    print(f"restatement vs PIL: worst PSNR gap {worst_gap:.3f} dB, worst size ratio {worst_ratio:.3f}")
    assert worst_gap <= R.PSNR_MARGIN_DB and worst_ratio <= R.SIZE_RATIO_MAX


def test_stream_layout_of_the_restatement():
    """Marker order, restart interval, RST numbering (wraps past 7 with 10 intervals) and the end of the file."""
    frames = R.make_frames("smooth", 1, 160, 16)
    data = R.encode(frames, 75)[0]
    markers, pos = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[pos] == 0xFF
        m, length = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        markers.append(m)
        if m == 0xDD:
            assert int.from_bytes(data[pos + 4:pos + 6], "big") == 1           # one MCU per MCU row at W = 16
        pos += 2 + length
        if m == 0xDA:
            break
    assert markers == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert pos == len(R.jfif_header(160, 16, 75))
    body = data[pos:]
    rst = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and 0xD0 <= body[i + 1] <= 0xD7]
    assert rst == [0xD0 + (k & 7) for k in range(9)] and body[-2:] == b"\xff\xd9"
    stray = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] not in (0, 0xD9) and not 0xD0 <= body[i + 1] <= 0xD7]
    assert not stray                                                             # every other 0xFF is stuffed


def test_excused_share_of_the_gpu_cases_stays_under_the_cap():
    """Test (a) of the GPU suite excuses coefficients whose float64 value / q lies within DELTA of a half-integer; the cases it runs
    keep that share under the cap by the restatement alone (the 0 / 255 checkerboard at quality 100 does not: 4.2 %, so it is run
    at 75 and 95 only)."""
    for n, H, W in R.SHAPES:
        for kind in R.KINDS:
            for q in R.gpu_qualities(kind, (n, H, W)):
                real = R.transform_real(R.make_frames(kind, n, H, W), q)
                share = float((np.abs(np.abs(real - np.floor(real)) - 0.5) < R.DELTA).mean())
                assert share <= R.MAX_EXCUSED_SHARE, (kind, H, W, q, share)


def test_product_tables_and_header_equal_the_restatement_and_pil():
    from stable_diffusion_videos_amd import jpeg
    assert tuple(jpeg.ZIGZAG) == tuple(int(v) for v in R.ZZ)
    for q in (1, 10, 49, 50, 75, 95, 100):
        for a, b in zip(jpeg.quant_tables(q), R.quant_tables(q)):
            assert np.array_equal(a, b) and a.min() >= 1 and a.max() <= 255
        for H, W in ((16, 16), (40, 56), (2048, 2048), (1, 65535)):
            assert jpeg.jfif_header(H, W, q) == R.jfif_header(H, W, q)
    img = R.make_frames("smooth", 1, 40, 56)[0]
    for q in (75, 95):
        written = Image.open(io.BytesIO(R.pil_encode(img, q))).quantization
        ql, qc = jpeg.quant_tables(q)
        assert list(written[0]) == ql.tolist() and list(written[1]) == qc.tolist()
    # the Huffman tables are the ones libjpeg writes without `optimize`
    data, pos, dht = R.pil_encode(img, 75), 2, {}
    while data[pos + 1] != 0xDA:
        length = int.from_bytes(data[pos + 2:pos + 4], "big")
        if data[pos + 1] == 0xC4:
            p = data[pos + 4:pos + 2 + length]
            while p:
                nv = sum(p[1:17])
                dht[p[0]] = (bytes(p[1:17]), bytes(p[17:17 + nv]))
                p = p[17 + nv:]
        pos += 2 + length
    assert {t: (b, v) for t, b, v in jpeg.HUFFMAN_TABLES} == dht
    for bad in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            jpeg.quant_tables(bad)
    with pytest.raises(ValueError, match="frame size"):
        jpeg.jfif_header(0, 16, 75)


def test_encoder_refuses_cpu_tensors(hip):
    from stable_diffusion_videos_amd.jpeg import JpegEncoder
    enc = JpegEncoder()
    assert enc.quality == 75
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        enc.encode(torch.zeros((1, 16, 16, 3), dtype=torch.uint8))
    coef = torch.zeros((1, 1, 1, 6, 64), dtype=torch.int16)
    with pytest.raises(hip.SdvHipError, match="GPU memory"):
        torch.ops.sdv.k_jpeg_transform(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), [1] * 64, [1] * 64, coef)
    with pytest.raises(hip.SdvHipError, match="coef must be"):
        torch.ops.sdv.k_jpeg_transform(torch.zeros((1, 16, 17, 3), dtype=torch.uint8), [1] * 64, [1] * 64, coef)
    with pytest.raises(hip.SdvHipError, match="64 entries"):
        torch.ops.sdv.k_jpeg_transform(torch.zeros((1, 16, 16, 3), dtype=torch.uint8), [1] * 63, [1] * 64, coef)
    u8 = lambda k: torch.zeros((k,), dtype=torch.uint8)
    i64 = lambda k: torch.zeros((k,), dtype=torch.int64)
    with pytest.raises(hip.SdvHipError, match="GPU memory"):
        torch.ops.sdv.k_jpeg_entropy_pack(coef, 16, 16, u8(600), u8(12), u8(100), i64(2), i64(1))
    with pytest.raises(hip.SdvHipError, match="scratch holds"):
        torch.ops.sdv.k_jpeg_entropy_pack(coef, 16, 16, u8(600), u8(11), u8(100), i64(2), i64(1))
    with pytest.raises(hip.SdvHipError, match="offsets must be"):
        torch.ops.sdv.k_jpeg_entropy_pack(coef, 16, 16, u8(600), u8(12), u8(100), i64(1), i64(1))
    with pytest.raises(hip.SdvHipError, match="coef must be"):
        torch.ops.sdv.k_jpeg_entropy_pack(coef, 32, 16, u8(600), u8(24), u8(100), i64(2), i64(1))


def test_c_abi_validates_before_any_launch(hip):
    lib = hip.load()
    good = (ctypes.c_uint16 * 64)(*([16] * 64))
    zero = (ctypes.c_uint16 * 64)(*([16] * 63 + [0]))
    big = (ctypes.c_uint16 * 64)(*([256] + [16] * 63))
    ok = [16, 2, 40, 56, good, good, 32, None]
    for pos, val, word in ((0, None, b"null"), (6, None, b"null"), (1, 0, b"frame count"), (1, -3, b"frame count"), (2, 0, b"frame size"),
                           (2, 65536, b"frame size"), (3, 0, b"frame size"), (3, 70000, b"frame size"), (4, zero, b"outside 1 .. 255"),
                           (5, big, b"outside 1 .. 255"), (6, 40, b"16-byte aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_jpeg_transform_u8(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    intervals = 2 * 3                                                            # n = 2 frames x ceil(40 / 16) MCU rows
    ok = [32, 2, 40, 56, 16, 623, 64, 12 * intervals, 128, 1000, 256, 512, None]
    for pos, val, word in ((0, None, b"null"), (4, None, b"null"), (6, None, b"null"), (8, None, b"null"), (10, None, b"null"),
                           (11, None, b"null"), (1, 0, b"frame count"), (2, 0, b"frame size"), (3, 65536, b"frame size"),
                           (5, 0, b"header length"), (7, 12 * intervals - 1, b"scratch buffer too small"), (9, -1, b"capacity"),
                           (6, 68, b"aligned"), (0, 40, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_jpeg_entropy_pack(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())


def test_header_library_and_binding_agree_on_the_jpeg_entry_points(hip):
    header = (ROOT / "include" / "sdv_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in (("sdv_jpeg_transform_u8", "k_jpeg_transform"), ("sdv_jpeg_entropy_pack", "k_jpeg_entropy_pack")):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(lib, name) and name in hip.EXPORTED_SYMBOLS
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._SIGNATURES[name][1]), name
    doc = header[header.index("JPEG encoder"):header.index("int sdv_jpeg_transform_u8(")]
    assert "stable_diffusion_pipeline.py:553" in doc and "make_video_pyav" in doc
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    for mod in ("jpeg.py", "video.py", "utils.py"):
        src = (ROOT / "stable_diffusion_videos_amd" / mod).read_text()
        assert "import ctypes" not in src and "lib.sdv_" not in src


def test_frame_writer_submit_bytes_part_then_rename(tmp_path):
    from stable_diffusion_videos_amd.utils import FrameWriter
    w = FrameWriter(workers=2)
    data = R.encode(R.make_frames("smooth", 1, 16, 16), 75)[0]
    w.submit_bytes(data, tmp_path / "frame000000.jpg")
    w.close()
    assert (tmp_path / "frame000000.jpg").read_bytes() == data and not list(tmp_path.glob("*.part"))
    assert Image.open(tmp_path / "frame000000.jpg").size == (16, 16)
