"""The H.264 CAVLC intra encoder without a GPU: the VLC tables (the decoder's bit strings against the kernel's words from the host-only
entry point, and against pinned code words of the Recommendation), the restatement of the stream rule (tests/h264_ref.py) round-tripped
through the separately written decoder, the coverage the case set has to reach, sizes, the colour rule, the C ABI and the wrappers'
argument checks, the codec choice of video.py / pipeline.py, and the unchanged default file."""
import ctypes
import functools
import hashlib
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

import h264_ref as R

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((1, 16, 16), (2, 32, 48), (1, 36, 50), (3, 64, 64), (1, 96, 128))
QPS = (0, 10, 16, 28, 51)


@functools.lru_cache(maxsize=None)
def _encode(shape, kind, qp):
    planes = R.make_planes(kind, *shape)
    stats = R.new_stats()
    samples, ry, rcb, rcr = R.encode_planes(*planes, qp=qp, first_index=1, stats=stats)
    return planes, samples, (ry, rcb, rcr), stats


def _all_tables():
    for t, table in enumerate(R.COEFF_TOKEN):
        yield f"coeff_token {t}", list(table.values())
    for name, rows in (("total_zeros", R.TOTAL_ZEROS), ("total_zeros chroma DC", R.TOTAL_ZEROS_CHROMA_DC), ("run_before", R.RUN_BEFORE)):
        for k, row in enumerate(rows):
            yield f"{name} {k + 1}", list(row)


def test_vlc_tables_are_prefix_free_with_the_entry_counts_of_the_clause():
    """Every table: distinct code words, none a prefix of another, the number of entries the clause gives (62 coeff_token entries per nC
    class, 14 for chroma DC; 17 - tzVlcIndex total_zeros entries; zerosLeft + 1 run_before entries, 15 from 7 on) and a Kraft sum of at
    most 1 (exactly 1 for the complete codes)."""
    counts = {f"coeff_token {t}": 62 for t in range(4)}
    counts["coeff_token 4"] = 14
    counts.update({f"total_zeros {k}": 17 - k for k in range(1, 16)})
    counts.update({f"total_zeros chroma DC {k}": 5 - k for k in range(1, 4)})
    counts.update({f"run_before {k}": k + 1 for k in range(1, 7)})
    counts["run_before 7"] = 15
    seen = 0
    for name, codes in _all_tables():
        assert len(codes) == counts[name] and len(set(codes)) == len(codes), name
        for a in codes:
            assert set(a) <= {"0", "1"} and a
            assert not any(b != a and b.startswith(a) for b in codes), (name, a)
        kraft = sum(Fraction(1, 2 ** len(c)) for c in codes)
        assert kraft <= 1, name
        if name.startswith("total_zeros") and name != "total_zeros 1" or (name.startswith("run_before") and name != "run_before 7"):
            assert kraft == 1, name
        seen += 1
    assert seen == len(counts) == 5 + 15 + 3 + 7


def test_pinned_code_words():
    """Code words of Tables 9-5, 9-7, 9-9 and 9-10 written out bit for bit."""
    t0 = R.COEFF_TOKEN[0]
    assert (t0[0, 0], t0[1, 1], t0[3, 3], t0[0, 1], t0[2, 2]) == ("1", "01", "00011", "000101", "001")
    assert R.COEFF_TOKEN[1][0, 0] == "11" and R.COEFF_TOKEN[2][0, 0] == "1111" and R.COEFF_TOKEN[3][0, 0] == "000011"
    assert R.COEFF_TOKEN[3][3, 16] == "111111" and R.COEFF_TOKEN[4][0, 0] == "01" and R.COEFF_TOKEN[4][1, 1] == "1"
    assert R.COEFF_TOKEN[4][3, 4] == "0000000"
    assert R.TOTAL_ZEROS[0][:3] == ("1", "011", "010") and R.TOTAL_ZEROS[0][15] == "000000001"
    assert R.TOTAL_ZEROS[14] == ("0", "1") and R.TOTAL_ZEROS_CHROMA_DC[0] == ("1", "01", "001", "000")
    assert R.RUN_BEFORE[0] == ("1", "0") and R.RUN_BEFORE[6][7] == "0001" and R.RUN_BEFORE[6][14] == "00000000001"
    assert R.RUN_BEFORE[2] == ("11", "10", "01", "00")
    assert R.ue(0) == "1" and R.ue(25) == "000011010" and R.se(-10) == "000010101" and R.se(1) == "010"


def test_kernel_tables_equal_the_decoder_tables(hip):
    """The words the GPU codes with (host-only entry point, no GPU work) against the decoder's bit strings, entry by entry; every word
    the layout leaves unused is empty."""
    words = hip.h264_vlc_tables()
    assert len(words) == hip.H264_VLC_WORDS == 656
    want = {}
    for t, table in enumerate(R.COEFF_TOKEN):
        for (t1, total), code in table.items():
            want[(68 * t if t < 4 else 272) + 4 * total + t1] = code
    for k, row in enumerate(R.TOTAL_ZEROS):
        for z, code in enumerate(row):
            want[292 + 16 * k + z] = code
    for k, row in enumerate(R.TOTAL_ZEROS_CHROMA_DC):
        for z, code in enumerate(row):
            want[532 + 4 * k + z] = code
    for k, row in enumerate(R.RUN_BEFORE):
        for z, code in enumerate(row):
            want[544 + 16 * k + z] = code
    for i, (length, code) in enumerate(words):
        if i in want:
            assert length == len(want[i]) and code == int(want[i], 2), (i, length, code, want[i])
        else:
            assert length == 0 and code == 0, i
    assert len(want) == 4 * 62 + 14 + sum(17 - k for k in range(1, 16)) + 9 + sum(range(2, 8)) + 15


def test_round_trip_decodes_to_the_encoders_own_reconstruction():
    """The closed loop: for every case the separately written decoder recovers, sample for sample, the pictures the restatement
    reconstructed while it predicted; slice headers read back as specified; no 00 00 0x inside a NAL unit (the decoder's unescape
    asserts it) and none ends in a zero byte."""
    for shape in SHAPES:
        n, h, w = shape
        mbw, mbh = (w + 15) // 16, (h + 15) // 16
        for kind in R.KINDS:
            for qp in QPS:
                _, samples, (ry, rcb, rcr), _ = _encode(shape, kind, qp)
                assert len(samples) == n
                for k, s in enumerate(samples):
                    d = R.decode_sample(s, w, h)
                    assert np.array_equal(d["y"], ry[k, :h, :w]), (shape, kind, qp)
                    assert np.array_equal(d["cb"], rcb[k, :h // 2, :w // 2]) and np.array_equal(d["cr"], rcr[k, :h // 2, :w // 2]), (shape, kind, qp)
                    assert len(d["headers"]) == mbh
                    for r, hd in enumerate(d["headers"]):
                        assert hd == dict(first_mb=r * mbw, slice_type=7, pps_id=0, frame_num=0, idr_pic_id=(1 + k) & 1, no_output=0, long_term=0,
                                          qp_delta=qp - 26, deblock_idc=1, nal_bytes=hd["nal_bytes"])
                        assert 4 + hd["nal_bytes"] <= R.slot_bytes(mbw)
                    assert sum(4 + hd["nal_bytes"] for hd in d["headers"]) == len(s)


def test_case_set_reaches_every_path_of_the_rule():
    """Asserted on the restatement alone: every nC class of coeff_token, level escapes with level_prefix 14 and 15, every suffixLength
    0 .. 6, cbp_luma 0 / 15, cbp_chroma 0 / 1 / 2, both I_PCM triggers, an I_PCM left neighbour feeding nC, a cropped size, a
    single-macroblock picture, and emulation-prevention bytes inside I_PCM samples."""
    tot = R.new_stats()
    for shape in SHAPES:
        for kind in R.KINDS:
            for qp in QPS:
                st = _encode(shape, kind, qp)[3]
                for key in ("nc_class", "suffix_length", "level_prefix", "cbp_luma", "cbp_chroma", "pcm"):
                    tot[key] |= st[key]
                tot["pcm_left"] |= st["pcm_left"]
    assert tot["nc_class"] == {0, 1, 2, 3, 4}
    assert {14, 15} <= tot["level_prefix"] and tot["suffix_length"] == set(range(7))
    assert tot["cbp_luma"] == {0, 15} and tot["cbp_chroma"] == {0, 1, 2}
    assert tot["pcm"] == {"bits", "level"} and tot["pcm_left"]
    assert any(h % 16 or w % 16 for _, h, w in SHAPES) and (1, 16, 16) in SHAPES
    planes, samples, _, st = _encode((1, 16, 16), "zeros_pcm", 0)
    assert st["n_pcm"] == 1 and len(samples[0]) > 4 + 1 + 3 + 384 + 50          # the hostile samples grew by emulation-prevention bytes
    assert int(planes[0].max()) <= 3


def test_sizes():
    """No macroblock above 3200 bits, every slice inside the documented capacity (checked in the round trip as well), flat frames at a
    few bytes per macroblock, and bytes per frame next to I_PCM.  Pinned at + 10 % of what this restatement measured at qp 16 on
    (1, 96, 128): flat 172, ramp 4888, glyphs 1706, noise 14490, zeros_pcm 459 bytes (I_PCM: 18536)."""
    from stable_diffusion_videos_amd import h264
    for shape in SHAPES:
        for kind in R.KINDS:
            for qp in QPS:
                assert max(_encode(shape, kind, qp)[3]["mb_bits"]) <= R.MAX_MB_BITS, (shape, kind, qp)
    measured = dict(flat=172, ramp=4888, glyphs=1706, noise=14490, zeros_pcm=459)
    shape = (1, 96, 128)
    y, cb, cr = R.make_planes("flat", *shape)
    pcm = 4 + len(h264.idr_picture_yuv(y[0], cb[0], cr[0], 0))
    for kind in R.KINDS:
        size = len(_encode(shape, kind, 16)[1][0])
        print(f"{kind}: {size} bytes per frame, I_PCM {pcm}")
        assert size <= measured[kind] * 1.1, (kind, size)
    for qp in QPS:
        assert len(_encode(shape, "flat", qp)[1][0]) <= 4 * 48, qp                # 48 macroblocks, 6 slices


def test_integer_colour_rule_is_within_one_of_the_float_rule():
    """Random frames, all (R, G) pairs at four B values, the 0 / 1 / 127 / 128 / 254 / 255 corner colours: every plane within 1 of
    h264.rgb_to_yuv420, every value inside 16 .. 240."""
    from stable_diffusion_videos_amd import h264
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (32, 48, 3), dtype=np.uint8) for _ in range(3)]
    rr, gg = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for b in (0, 85, 170, 255):
        frames.append(np.stack([rr, gg, np.full_like(rr, b)], axis=-1).astype(np.uint8))
    c = np.array([0, 1, 127, 128, 254, 255])
    corners = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    frames.append(np.repeat(np.repeat(corners.reshape(6, 36, 3), 2, axis=0), 2, axis=1).astype(np.uint8))
    for f in frames:
        h, w = f.shape[:2]
        y, cb, cr = R.rgb_to_planes(f[None])
        want = h264.rgb_to_yuv420(f)
        for got, ref in zip((y[0, :h, :w], cb[0, :h // 2, :w // 2], cr[0, :h // 2, :w // 2]), want):
            assert np.abs(got.astype(int) - ref.astype(int)).max() <= 1
            assert 16 <= got.min() and got.max() <= 240


def test_header_library_and_binding_agree_on_the_new_entry_points(hip):
    header = (ROOT / "include" / "sdv_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in (("sdv_h264_planes_u8", "k_h264_planes"), ("sdv_h264_encode_rows", "k_h264_encode_rows"), ("sdv_h264_pack", "k_h264_pack"),
                     ("sdv_h264_vlc_tables", None)):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert hasattr(lib, name) and name in hip.EXPORTED_SYMBOLS
        if op is not None:
            assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._SIGNATURES[name][1]), name
    assert "H.264 CAVLC intra encoder" in header and "600 mbw + 17" in header
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    assert hip.h264_slice_bytes(3) == R.slot_bytes(3) == 600 * 3 + 17
    assert hip.h264_out_bytes(2, 5, 3) == 10 * 1817 and hip.h264_scratch_bytes(2, 5, 3) == 10 * (1824 + 12)
    src = (ROOT / "stable_diffusion_videos_amd" / "h264_cavlc.py").read_text()
    assert "import ctypes" not in src and "lib.sdv_" not in src


def test_wrappers_refuse_cpu_tensors_wrong_dtypes_qp_and_capacities(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, encoder_for
    assert H264Encoder().qp == 16 and encoder_for(20, "cuda:0") is encoder_for(20, "cuda:0") is not encoder_for(21, "cuda:0")
    for bad in (-1, 52, 16.0, "16", True, None):
        with pytest.raises(ValueError, match="0 .. 51"):
            H264Encoder(qp=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder().encode(torch.zeros((1, 16, 16, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    i64 = lambda k: torch.zeros((k,), dtype=torch.int64)
    planes = torch.ops.sdv.k_h264_planes
    ok = dict(frames=u8(1, 20, 36, 3), y=u8(1, 32, 48), cb=u8(1, 16, 24), cr=u8(1, 16, 24))
    for key, val, word in (("frames", u8(1, 20, 36, 4), "frames must be"), ("frames", torch.zeros((1, 20, 36, 3)), "frames must be"),
                           ("frames", u8(1, 21, 36, 3), "even"), ("y", u8(1, 20, 36), "y must be"), ("cb", u8(1, 10, 18), "cb must be"),
                           ("cr", torch.zeros((1, 16, 24), dtype=torch.int8), "cr must be"), ("cr", u8(1, 16, 24), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            planes(*dict(ok, **{key: val}).values())
    rows = torch.ops.sdv.k_h264_encode_rows
    sb = hip.h264_scratch_bytes(1, 2, 3)
    ok = dict(y=u8(1, 32, 48), cb=u8(1, 16, 24), cr=u8(1, 16, 24), qp=16, first_index=0, scratch=u8(sb))
    for key, val, word in (("y", u8(1, 32, 40), "y must be"), ("y", u8(32, 48), "y must be"), ("cb", u8(1, 16, 16), "cb must be"),
                           ("qp", -1, "qp must be"), ("qp", 52, "qp must be"), ("first_index", -1, "first_index"),
                           ("scratch", u8(sb - 1), "scratch holds"), ("scratch", torch.zeros((sb,), dtype=torch.int8), "scratch must be"),
                           ("scratch", u8(sb), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            rows(*dict(ok, **{key: val}).values())
    pack = torch.ops.sdv.k_h264_pack
    ob = hip.h264_out_bytes(1, 2, 3)
    ok = dict(scratch=u8(sb), n=1, mbh=2, mbw=3, out=u8(ob), offsets=i64(2))
    for key, val, word in (("scratch", u8(sb - 1), "scratch holds"), ("n", 0, "macroblock grid"), ("mbw", 1025, "macroblock grid"),
                           ("out", u8(ob - 1), "capacity bound"), ("out", u8(2, ob), "out holds"), ("offsets", i64(3), "offsets must be"),
                           ("offsets", torch.zeros((2,), dtype=torch.int32), "offsets must be"), ("offsets", i64(2), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            pack(*dict(ok, **{key: val}).values())


def test_c_abi_validates_before_any_launch(hip):
    lib = hip.load()
    ok = [16, 1, 20, 36, 32, 48, 64, None]
    for pos, val, word in ((0, None, b"null"), (4, None, b"null"), (6, None, b"null"), (1, 0, b"frame count"), (2, 21, b"frame size"),
                           (3, 0, b"frame size"), (3, 16386, b"frame size")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_planes_u8(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_planes_u8")
    sb = hip.h264_scratch_bytes(2, 3, 4)
    ok = [16, 32, 48, 2, 3, 4, 16, 0, 64, sb, None]
    for pos, val, word in ((0, None, b"null"), (2, None, b"null"), (8, None, b"null"), (3, 0, b"frame count"), (4, 0, b"macroblock grid"),
                           (5, 1025, b"macroblock grid"), (6, -1, b"qp="), (6, 52, b"qp="), (7, -1, b"first_index"),
                           (9, sb - 1, b"scratch buffer too small"), (0, 8, b"aligned"), (1, 36, b"aligned"), (8, 68, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_rows(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    ob = hip.h264_out_bytes(2, 3, 4)
    ok = [64, sb, 2, 3, 4, 128, ob, 256, None]
    for pos, val, word in ((0, None, b"null"), (5, None, b"null"), (7, None, b"null"), (2, 0, b"frame count"), (3, 1025, b"macroblock grid"),
                           (1, sb - 1, b"scratch buffer too small"), (6, ob - 1, b"output capacity"), (0, 68, b"aligned"), (7, 260, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_pack(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    lengths, codes = (ctypes.c_uint8 * 656)(), (ctypes.c_uint16 * 656)()
    assert lib.sdv_h264_vlc_tables(lengths, codes, 655) == -1 and b"656" in lib.sdv_last_error()
    assert lib.sdv_h264_vlc_tables(None, codes, 656) == -1 and b"null" in lib.sdv_last_error()


def _frames(n=3, h=20, w=36):
    return torch.from_numpy(np.random.default_rng(7).integers(0, 256, (n, h, w, 3), dtype=np.uint8))


def test_default_call_writes_the_parent_commits_bytes(tmp_path, monkeypatch):
    """The container writer was factored to accept ready-made samples: the default (I_PCM) call still writes the file it wrote before
    (SHA-256 of this input's file computed with the parent commit's writer)."""
    pytest.importorskip("PIL")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    out = video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "d.mp4")
    if video.LAST_CODEC["video"] == "h264 (libx264)":
        pytest.skip("torchvision / pyav present: the dependency-free writer is not in use")
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and video.LAST_CODEC["why"] == "default"
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "0f64cec489154862ffc374f5923ae007157d27738c3d6e89dc650859ff0b04f5"
    same = video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "e.mp4", codec="h264")
    assert open(same, "rb").read() == open(out, "rb").read() and video.LAST_CODEC["why"] == "codec argument"


def test_codec_choice_variable_wins_and_bad_values_are_refused(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.setenv("SDV_VIDEO_CODEC", "h264")
    video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "a.mp4", codec="mjpeg")
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and video.LAST_CODEC["why"] == "SDV_VIDEO_CODEC"
    monkeypatch.delenv("SDV_VIDEO_CODEC")
    video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "b.mp4", codec="mjpeg")
    assert video.LAST_CODEC["video"] == "mjpeg"
    for bad in ("h265", "cavlc", "h264_cavlc"):
        with pytest.raises(ValueError, match="SDV_VIDEO_CODEC"):
            video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "c.mp4", codec=bad)
    with pytest.raises(ValueError, match="0 .. 51"):
        video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "c.mp4", codec="h264-cavlc", h264_qp=52)
    odd = torch.zeros((2, 21, 36, 3), dtype=torch.uint8)
    video.make_video_pyav(odd, fps=5, output_filepath=tmp_path / "o.mp4", codec="h264-cavlc")
    assert video.LAST_CODEC["video"] == "mjpeg" and "odd frame size" in video.LAST_CODEC["why"]


def test_h264_cavlc_without_a_gpu_falls_back_to_i_pcm_with_a_reason(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc")
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"]
    monkeypatch.setenv("SDV_VIDEO_CODEC", "h264-cavlc")
    b = video.make_video_pyav(_frames(), fps=5, output_filepath=tmp_path / "b.mp4")
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"]
    assert hashlib.sha256(open(a, "rb").read()).hexdigest() == hashlib.sha256(open(b, "rb").read()).hexdigest() \
        == "0f64cec489154862ffc374f5923ae007157d27738c3d6e89dc650859ff0b04f5"


def test_pipeline_attributes_and_sdv_h264_qp(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_QP", raising=False)
    assert pipe.video_codec is None and pipe.h264_qp == 16 and pipe.h264_qp_choice() == 16
    pipe.h264_qp = 22
    assert pipe.h264_qp_choice() == 22
    monkeypatch.setenv("SDV_H264_QP", "10")                                       # the variable wins when it is set
    assert pipe.h264_qp_choice() == 10
    for bad in ("52", "-1", "ten", " 10", "1.5"):
        monkeypatch.setenv("SDV_H264_QP", bad)
        with pytest.raises(ValueError, match="SDV_H264_QP"):
            pipe.h264_qp_choice()
    monkeypatch.delenv("SDV_H264_QP")
    pipe.h264_qp = 99
    with pytest.raises(ValueError, match="h264_qp"):
        pipe.h264_qp_choice()


def test_third_party_decoder_agrees(tmp_path):
    """Where pyav exists: the mp4 of the restatement's samples decodes there to exactly this file's decoder's Y'CbCr."""
    av = pytest.importorskip("av")
    from stable_diffusion_videos_amd import video
    shape = (3, 64, 64)
    n, h, w = shape
    for kind in ("ramp", "noise", "glyphs"):
        _, samples, (ry, rcb, rcr), _ = _encode(shape, kind, 16)
        path = video.write_h264_mp4(None, w, h, 5, tmp_path / f"{kind}.mp4", samples=samples)
        with av.open(str(path)) as container:
            frames = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
        assert len(frames) == n
        for k, f in enumerate(frames):
            assert np.array_equal(f[:h], ry[k, :h, :w])
            assert np.array_equal(f[h:h + h // 4].reshape(h // 2, w // 2), rcb[k, :h // 2, :w // 2])
            assert np.array_equal(f[h + h // 4:].reshape(h // 2, w // 2), rcr[k, :h // 2, :w // 2])
