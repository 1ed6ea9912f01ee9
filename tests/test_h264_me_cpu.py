"""Motion-compensated P pictures of the H.264 GOP stream (include/sdv_hip_ext.h "H.264 motion search") without a GPU:
tests/h264_me_ref.py's restatement against the separately written decoder of tests/h264_p_ref.py, the coverage of searched and injected
vectors, the conditions of the rule (still = search 0, search 0 = the GOP stream, pan2 / drift shrink), argument checks and plumbing, and
the host build of csrc/sdv_h264_core.h's motion pieces under AddressSanitizer / UBSan against the restatement."""
import ctypes
import hashlib
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import h264_me_ref as M
import h264_p_ref as P
import h264_ref as R

ROOT = Path(__file__).resolve().parent.parent
CORE = ROOT / "stable_diffusion_videos_amd" / "csrc" / "sdv_h264_core.h"
# injected-vector cases: (shape, qp, search, kind of h264_me_ref.inject) on planes planted with those vectors
INJECTED = [((7, 64, 64, 3), 16, 8, "random"), ((7, 64, 64, 3), 0, 16, "extreme"), ((5, 32, 48, 5), 28, 2, "random"),
            ((6, 96, 128, 2), 28, 16, "random"), ((5, 32, 48, 5), 51, 16, "invalid"), ((4, 16, 16, 4), 16, 16, "invalid"),
            ((3, 36, 50, 3), 16, 2, "extreme")]


def _check_round_trip(shape, kind, qp, search, injected=None):
    n, h, w, gop = shape
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    _, samples, (ry, rcb, rcr), _, used = M.reference(shape, kind, qp, search, injected)
    d = P.decode_stream(samples, w, h)                                              # raises NotWholeSample for a vector it cannot copy
    assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr), (shape, kind, qp, search)
    assert d["sync"] == list(range(0, n, gop))
    for k in range(n):
        for r in range(mbh):
            for m in range(mbw):
                vx, vy = (int(c) for c in used[k, r, m])
                assert M.admitted(vx, vy, search, m, r, mbw, mbh) and (k % gop or (vx, vy) == (0, 0))
    for k, headers in enumerate(d["headers"]):
        assert len(headers) == mbh
        for r, hd in enumerate(headers):
            assert hd["first_mb"] == r * mbw and hd["qp_delta"] == qp - 26 and 4 + hd["nal_bytes"] <= P.slot_bytes(mbw)
            assert hd["frame_num"] == (k % gop) & 15


@pytest.mark.parametrize("shape", M.SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-gop{s[3]}" for s in M.SHAPES])
def test_round_trip_decodes_to_the_encoders_own_reconstruction(shape):
    """Every case of the grid (kinds x qp x search for this shape): the independent decoder recovers, sample for sample, the pictures the
    restatement reconstructed, with no vector it would have to interpolate for; every coded vector is one the rule admits."""
    assert len(M.SHAPES) == 5
    for kind in M.KINDS:
        for qp in M.QPS:
            for search in M.SEARCHES:
                _check_round_trip(shape, kind, qp, search)


def test_injected_vectors_round_trip_and_reach_every_path_of_the_rule():
    """Asserted on the restatement's statistics, summed over the injected cases."""
    mvd_x, mvd_y, after = set(), set(), set()
    cbp0 = skip_after = invalid = 0
    edges = set()
    for shape, qp, search, kind in INJECTED:
        _check_round_trip(shape, "planted", qp, search, kind)
        st, used = M.reference(shape, "planted", qp, search, kind)[3:]
        mvd_x |= st["mvd_x"]
        mvd_y |= st["mvd_y"]
        after |= st["nonzero_after"]
        cbp0 += st["nonzero_cbp0"]
        skip_after += st["skip_after_nonzero"]
        invalid += st["invalid_as_zero"]
        if kind == "extreme" and search == 16:
            assert {-128, 128} <= st["mvd_x"] and {-128, 128} <= st["mvd_y"]       # |mvd| = 8 search: left neighbour at -search, this one at +search
        assert not st["p_mb_bits"] or max(st["p_mb_bits"]) <= R.MAX_MB_BITS
        n, mbh, mbw = used.shape[:3]
        for k in range(n):                                                          # a nonzero (so inward-pointing) vector at every edge
            if used[k, :, 0, 0].max() > 0:
                edges.add("left")
            if used[k, :, mbw - 1, 0].min() < 0:
                edges.add("right")
            if used[k, 0, :, 1].max() > 0:
                edges.add("top")
            if used[k, mbh - 1, :, 1].min() < 0:
                edges.add("bottom")
    assert min(mvd_x) < 0 < max(mvd_x) and min(mvd_y) < 0 < max(mvd_y)
    assert cbp0 and skip_after and invalid
    assert after == {"intra", "pcm", "skip"}
    assert edges == {"left", "right", "top", "bottom"}


def test_candidate_sets_are_clipped_at_the_picture_edges():
    assert M.candidates(16, 0, 0, 1, 1) == [(0, 0)]                                 # the one-macroblock picture
    assert len(M.candidates(16, 1, 1, 3, 3)) == 289 and len(M.candidates(2, 1, 1, 3, 3)) == 9
    assert all(vx >= 0 for vx, _ in M.candidates(8, 0, 1, 3, 3)) and all(vx <= 0 for vx, _ in M.candidates(8, 2, 1, 3, 3))
    assert all(vy >= 0 for _, vy in M.candidates(8, 1, 0, 3, 3)) and all(vy <= 0 for _, vy in M.candidates(8, 1, 2, 3, 3))
    assert len(M.candidates(8, 0, 0, 3, 3)) == 25 and (8, 8) in M.candidates(8, 0, 0, 3, 3)
    st = M.reference((4, 16, 16, 4), "noise", 16, 16)[3]
    assert st["vectors"] <= {(0, 0)} and st["invalid_as_zero"] == 0
    y = np.full((3, 48, 64), 77, dtype=np.uint8)                                    # all candidates tie: the order picks (0, 0)
    mv, sad = M.search_planes(y, 16, 3, 16)
    assert not mv.any() and not sad.any()
    y[:, ::2] = 200                                                                 # repeated with period 2: every even shift ties again
    assert not M.search_planes(y, 16, 3, 8)[0].any()


def test_search_finds_the_shift_of_pan2_and_drift():
    for kind, want in (("pan2", (-2, 0)), ("drift", (-2, 2))):
        y = M.make_planes(kind, 3, 96, 128)[0]
        mv, sad = M.search_planes(y, 16, 3, 8)
        inner = mv[1:, 1:-1, 1:-1].reshape(-1, 2)                                   # (a block that is flat along an axis ties, and takes the shorter vector)
        assert not sad[1:, 1:-1, 1:-1].any() and not mv[0].any() and sad[1:].any()
        assert 2 * sum(tuple(v) == want for v in inner) > len(inner), (kind, inner.tolist())


def test_still_and_search_0_write_the_bytes_of_the_gop_stream():
    for shape in ((5, 32, 48, 5), (3, 36, 50, 3)):
        for qp in M.QPS:
            zero = P.reference(shape, "still", qp)[1]
            for search in M.SEARCHES:
                assert M.reference(shape, "still", qp, search)[1] == zero          # ``still`` with any search is search 0
    for shape, kind, qp in (((5, 32, 48, 5), "pan", 16), ((7, 64, 64, 3), "cut", 0), ((3, 36, 50, 3), "fade", 28), ((6, 96, 128, 2), "noise", 51),
                            ((4, 16, 16, 4), "zeros_pcm", 0)):
        planes = P.make_planes(kind, *shape[:3])
        got = M.encode_planes(*planes, qp=qp, gop=shape[3], first_index=P.FIRST, search=0)
        want = P.encode_planes(*planes, qp=qp, gop=shape[3], first_index=P.FIRST)
        assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:4], want[1:])) and not got[4].any()


def test_pan2_and_drift_shrink_at_every_qp():
    """With search >= the shift (2 samples a picture) the stream is strictly smaller than with zero vectors.  The ratios are printed, not
    asserted (DESIGN.md "H.264 motion search" records them)."""
    shape = (6, 96, 128, 6)
    for kind in ("pan2", "drift"):
        planes = M.make_planes(kind, *shape[:3])
        for qp in M.QPS:
            zero = sum(len(s) for s in P.encode_planes(*planes, qp=qp, gop=6)[0])
            for search in M.SEARCHES:
                size = sum(len(s) for s in M.encode_planes(*planes, qp=qp, gop=6, search=search)[0])
                print(f"{kind} qp {qp} search {search}: {size} bytes, search 0 {zero} bytes, ratio {size / zero:.3f}")
                assert size < zero, (kind, qp, search, size, zero)


def test_lambda_table_equals_its_formula():
    body = CORE.read_text()
    body = body[body.index("h264_me_lambda"):]
    table = [int(v) for v in re.search(r"t\[52\] = \{([^}]*)\}", body).group(1).split(",")]
    assert table == list(M.LAMBDA) == [max(1, round(2 ** ((qp - 12) / 6))) for qp in range(52)]
    assert table[0] == table[15] == 1 and table[16] == 2 and table[51] == 91
    assert 65280 + 91 * 2 * max(M.vector_bits(c) for c in range(-16, 17, 2)) < 1 << 17    # the packed order's cost field


def test_counted_bits_are_the_written_bits_and_stay_within_3200():
    """The bits the restatement counts for a coded inter macroblock (mvd included) are the bits it writes: the P slices' lengths add up to
    headers, runs and the counted macroblocks; and no coded macroblock exceeds 3200 bits."""
    for shape, kind, qp, search, inj in (((5, 32, 48, 5), "pan2", 16, 8, None), ((7, 64, 64, 3), "planted", 16, 8, "random"),
                                         ((6, 96, 128, 2), "pan1", 0, 16, None)):
        st = M.reference(shape, kind, qp, search, inj)[3]
        assert st["counted"] and all(c in st["p_mb_bits"] for c in st["counted"]) and max(st["p_mb_bits"]) <= R.MAX_MB_BITS
        assert len(st["counted"]) == st["modes"].count("inter")


def test_default_files_are_the_parent_commits_bytes(tmp_path, monkeypatch):
    """SHA-256 computed with the parent commit's writer, as in test_h264_p_cpu.py: ``h264_search`` unset changes no byte."""
    pytest.importorskip("PIL")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = R.make_frames("ramp", 3, 36, 50)
    out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "d.mp4")
    if video.LAST_CODEC["video"] == "h264 (libx264)":
        pytest.skip("torchvision / pyav present: the dependency-free writer is not in use")
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"
    out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", h264_search=8)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"
    assert "search" not in video.LAST_CODEC


def test_extension_header_library_and_binding_agree(hip):
    header = (ROOT / "include" / "sdv_hip_ext.h").read_text()
    declared = set(re.findall(r"\b(sdv_[a-z0-9_]+)\s*\(", header)) - {"sdv_abi_version", "sdv_last_error", "sdv_h264_pack"}
    assert declared == set(hip.EXTENSION_SYMBOLS) == {"sdv_h264_motion_search", "sdv_h264_encode_gop_step"}
    assert not set(hip.EXTENSION_SYMBOLS) & set(hip.EXPORTED_SYMBOLS)
    base = (ROOT / "include" / "sdv_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in (("sdv_h264_motion_search", "k_h264_motion_search"), ("sdv_h264_encode_gop_step", "k_h264_encode_gop_step")):
        assert hasattr(lib, name) and name not in base
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._EXT_SIGNATURES[name][1]), name
        assert getattr(hip.load(), name).argtypes == hip._EXT_SIGNATURES[name][1]
    assert "H.264 motion search" in header and "additive codec extensions of ABI 12" in header
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12 and hip.H264_SEARCH_MAX == M.SEARCH_MAX == 16


def test_argument_checks_at_both_layers(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, check_search, encoder_for
    assert H264Encoder().search == 0 and H264Encoder(gop=4, search=8).search == 8 and H264Encoder(search=16).gop == 1
    assert encoder_for(20, "cuda:0", 4) is encoder_for(20, "cuda:0", 4, 0) is not encoder_for(20, "cuda:0", 4, 2)
    for bad in (-2, 1, 3, 18, 8.0, "8", True, None):
        with pytest.raises(ValueError, match="even integer in 0 .. 16"):
            check_search(bad)
        with pytest.raises(ValueError, match="even integer in 0 .. 16"):
            H264Encoder(gop=4, search=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder(gop=4, search=8).encode(torch.zeros((2, 16, 16, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    i16 = lambda *s: torch.zeros(s, dtype=torch.int16)
    op = torch.ops.sdv.k_h264_motion_search
    ok = dict(y=u8(2, 32, 48), qp=16, gop=4, search=8, mv=i16(2, 2, 3, 2), sad=None)
    for key, val, word in (("y", u8(2, 32, 40), "y must be"), ("qp", 52, "qp must be"), ("gop", 0, "gop must be"), ("search", 0, "search must be"),
                           ("search", 3, "search must be"), ("search", 18, "search must be"), ("mv", i16(2, 2, 3), "mv must be"),
                           ("mv", torch.zeros((2, 2, 3, 2), dtype=torch.int32), "mv must be"), ("sad", torch.zeros((2, 2, 3), dtype=torch.int16), "sad must be"),
                           ("sad", torch.zeros((2, 2, 2), dtype=torch.int32), "sad must be"), ("mv", i16(2, 2, 3, 2), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            op(*dict(ok, **{key: val}).values())
    op = torch.ops.sdv.k_h264_encode_gop_step
    sb = hip.h264_gop_scratch_bytes(2, 2, 3)
    ok = dict(y=u8(2, 32, 48), cb=u8(2, 16, 24), cr=u8(2, 16, 24), qp=16, gop=4, k=1, search=8, first_index=0, mv=i16(2, 2, 3, 2), ry=u8(2, 32, 48),
              rcb=u8(2, 16, 24), rcr=u8(2, 16, 24), scratch=u8(sb))
    for key, val, word in (("y", u8(2, 32, 40), "y must be"), ("cb", u8(2, 16, 16), "cb must be"), ("qp", -1, "qp must be"), ("gop", 257, "gop must be"),
                           ("k", 2, "position k"), ("k", -1, "position k"), ("search", 0, "search must be"), ("search", 5, "search must be"),
                           ("first_index", -1, "first_index"), ("mv", i16(2, 2, 3, 1), "mv must be"), ("ry", u8(2, 32, 32), "ry must be"),
                           ("rcr", u8(2, 8, 24), "rcr must be"), ("scratch", u8(sb - 1), "scratch holds"), ("scratch", u8(sb), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            op(*dict(ok, **{key: val}).values())
    with pytest.raises(hip.SdvHipError, match="position k"):
        op(*dict(ok, gop=1, k=1).values())
    lib = hip.load()
    ok = [16, 2, 3, 4, 16, 4, 8, 64, 128, None]                                     # y, n, mbh, mbw, qp, gop, search, mv, sad, stream
    for pos, val, word in ((0, None, b"null"), (7, None, b"null"), (1, 0, b"frame count"), (2, 0, b"macroblock grid"), (4, 52, b"qp="), (5, 0, b"gop="),
                           (6, 0, b"search="), (6, 7, b"search="), (6, 18, b"search="), (0, 8, b"aligned"), (7, 66, b"aligned"), (8, 130, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_motion_search(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_motion_search")
    sb = hip.h264_gop_scratch_bytes(2, 3, 4)
    ok = [16, 32, 48, 2, 3, 4, 16, 4, 1, 8, 0, 256, 64, 80, 96, 128, sb, None]     # y cb cr | n mbh mbw qp gop k search first | mv ry rcb rcr scratch | bytes
    for pos, val, word in ((0, None, b"null"), (11, None, b"null"), (12, None, b"null"), (15, None, b"null"), (3, 0, b"frame count"),
                           (4, 0, b"macroblock grid"), (5, 1009, b"above 1008"), (6, 52, b"qp="), (7, 0, b"gop="), (8, 2, b"position k"),
                           (8, -1, b"position k"), (9, 0, b"search="), (9, 3, b"search="), (10, -1, b"first_index"),
                           (16, sb - 1, b"scratch buffer too small"), (0, 8, b"aligned"), (11, 258, b"aligned"), (12, 72, b"aligned"), (15, 132, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_gop_step(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_encode_gop_step")


def test_pipeline_attribute_and_sdv_h264_search(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_SEARCH", raising=False)
    assert pipe.h264_search == 0 and pipe.h264_search_choice() == 0
    pipe.h264_search = 8
    assert pipe.h264_search_choice() == 8
    monkeypatch.setenv("SDV_H264_SEARCH", "16")                                     # the variable wins when it is set
    assert pipe.h264_search_choice() == 16
    for bad in ("3", "18", "-2", "eight", " 8", "2.0"):
        monkeypatch.setenv("SDV_H264_SEARCH", bad)
        with pytest.raises(ValueError, match="SDV_H264_SEARCH"):
            pipe.h264_search_choice()
    monkeypatch.delenv("SDV_H264_SEARCH")
    pipe.h264_search = 7
    with pytest.raises(ValueError, match="h264_search"):
        pipe.h264_search_choice()


def test_make_video_pyav_checks_search_and_falls_back_without_a_gpu(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import utils, video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = torch.from_numpy(R.make_frames("ramp", 3, 20, 36))
    for bad in (1, 18, -2, "8", 2.0):
        with pytest.raises(ValueError, match="even integer in 0 .. 16"):
            video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "x.mp4", codec="h264-cavlc", h264_gop=4, h264_search=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=4, h264_search=8)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"]
    b = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "b.mp4")
    c = utils.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "c.mp4", h264_gop=4, h264_search=8)      # ignored by the other codecs
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def test_host_build_of_the_motion_pieces_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/sdv_h264_core.h's fetch-address function and macroblock step with a vector compiled for the host with
    -fsanitize=address,undefined into a stand-alone program (tests/h264_me_host_main.cpp) and run as a subprocess on exact-size buffers with
    valid, extreme and invalid vectors: samples, reconstruction and the vectors that were coded equal the restatement's."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "h264_me_host"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "stable_diffusion_videos_amd" / "csrc"), str(ROOT / "tests" / "h264_me_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    for shape, qp, search, kind in (((7, 64, 64, 3), 16, 8, "random"), ((7, 64, 64, 3), 0, 16, "extreme"), ((5, 32, 48, 5), 51, 16, "invalid")):
        (y, cb, cr), samples, recon, _, used = M.reference(shape, "planted", qp, search, kind)
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        mv = M.inject(kind, n, mbh, mbw, search)
        (tmp_path / "in.bin").write_bytes(np.array([n, mbh, mbw, qp, shape[3], M.FIRST, search], dtype="<i4").tobytes() + y.tobytes() + cb.tobytes()
                                          + cr.tobytes() + mv.astype("<i2").tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        data, at, got = (tmp_path / "out.bin").read_bytes(), 0, []
        for _ in range(n):
            size = int.from_bytes(data[at:at + 4], "little")
            got.append(data[at + 4:at + 4 + size])
            at += 4 + size
        assert got == samples, (shape, qp, search, kind)
        for want in recon:
            assert np.array_equal(np.frombuffer(data[at:at + want.size], dtype=np.uint8).reshape(want.shape), want), (shape, qp, search, kind)
            at += want.size
        assert np.array_equal(np.frombuffer(data[at:at + 2 * used.size], dtype="<i2").reshape(used.shape), used)
        assert at + 2 * used.size == len(data)
