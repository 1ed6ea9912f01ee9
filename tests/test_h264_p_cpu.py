"""The H.264 GOP stream (P pictures with zero-motion inter prediction) without a GPU: tests/h264_p_ref.py's restatement against its
separately written decoder, the coverage of the case set, sizes, the container's ``stss`` box, argument checks and plumbing, and the
host build of csrc/sdv_h264_core.h under AddressSanitizer / UBSan against the restatement."""
import ctypes
import hashlib
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import h264_p_ref as P
import h264_ref as R

ROOT = Path(__file__).resolve().parent.parent
KINDS = P.KINDS + P.EXTRA_KINDS
CASES = [(s, k, q) for s in P.SHAPES for k in KINDS for q in P.QPS]


def test_inter_cbp_table_structure_and_pinned_words():
    """Typed from memory of Table 9-4 (not compared with a copy of the standard, no third-party decoder met): a permutation of 0 .. 47, the first
    13 entries pinned, and the kernel's inverse table (csrc/sdv_h264_core.h) agrees with it."""
    assert sorted(P.CBP_INTER) == list(range(48))
    assert P.CBP_INTER[:13] == (0, 16, 1, 2, 4, 8, 32, 3, 5, 10, 12, 15, 47)
    core = (ROOT / "stable_diffusion_videos_amd" / "csrc" / "sdv_h264_core.h").read_text()
    body = core[core.index("h264_cbp_inter_code"):]
    inverse = [int(v) for v in re.search(r"t\[48\] = \{([^}]*)\}", body).group(1).split(",")]
    assert inverse == [P.CBP_INTER.index(c) for c in range(48)]
    header = (ROOT / "include" / "sdv_hip.h").read_text()
    assert " ".join(map(str, P.CBP_INTER)) in " ".join(header.replace(" *", " ").split())


def test_round_trip_decodes_to_the_encoders_own_reconstruction():
    """For every case the decoder recovers, sample for sample (the cropped-away border included), the pictures the restatement
    reconstructed while it predicted; IDR pictures sit where the rule puts them; slice headers read back as specified."""
    for shape, kind, qp in CASES:
        n, h, w, gop = shape
        mbw, mbh = (w + 15) // 16, (h + 15) // 16
        _, samples, (ry, rcb, rcr), _ = P.reference(shape, kind, qp)
        d = P.decode_stream(samples, w, h)
        assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr), (shape, kind, qp)
        assert d["sync"] == P.sync_samples(n, gop) == list(range(0, n, gop))
        for k, (s, headers) in enumerate(zip(samples, d["headers"])):
            assert len(headers) == mbh and sum(4 + hd["nal_bytes"] for hd in headers) == len(s)
            for r, hd in enumerate(headers):
                assert hd["first_mb"] == r * mbw and hd["qp_delta"] == qp - 26 and hd["pps_id"] == 0 and 4 + hd["nal_bytes"] <= P.slot_bytes(mbw)
                if k % gop == 0:
                    assert (hd["nal_unit_type"], hd["nal_ref_idc"], hd["slice_type"], hd["frame_num"]) == (5, 3, 7, 0)
                    assert hd["idr_pic_id"] == (P.FIRST + k) & 1
                else:
                    assert (hd["nal_unit_type"], hd["nal_ref_idc"], hd["slice_type"], hd["frame_num"]) == (1, 2, 5, (k % gop) & 15)


def test_gop_1_is_the_intra_stream():
    for shape, kind, qp in (((3, 36, 50), "pan", 16), ((2, 32, 48), "noise", 0), ((2, 16, 16), "zeros_pcm", 0), ((3, 64, 64), "fade", 28)):
        planes = P.make_planes(kind, *shape)
        got = P.encode_planes(*planes, qp=qp, gop=1, first_index=P.FIRST)
        want = R.encode_planes(*planes, qp=qp, first_index=P.FIRST)
        assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))


def test_case_set_reaches_every_path_of_the_rule():
    """Asserted on the restatement's statistics, summed over the case set."""
    modes, runs, luma, chroma, pcm = set(), set(), set(), set(), set()
    only_run = trailing = intra_after_inter = inter_after_intra = inter_after_pcm = 0
    wrap = short = False
    for shape, kind, qp in CASES:
        st = P.reference(shape, kind, qp)[3]
        modes |= set(st["modes"])
        runs |= st["skip_runs"]
        luma |= st["inter_cbp_luma"]
        chroma |= st["inter_cbp_chroma"]
        pcm |= st["pcm_in_p"]
        only_run += st["only_run_slices"]
        trailing += st["trailing_runs"]
        intra_after_inter += st["intra_after_inter"]
        inter_after_intra += st["inter_after_intra"]
        inter_after_pcm += st["inter_after_pcm"]
        wrap |= any(a == 15 and b == 0 for a, b in zip(st["frame_nums"], st["frame_nums"][1:]) if shape[3] > 16)
        short |= st["short_gop"]
    assert modes == {"skip", "inter", "intra", "pcm"}
    assert 0 in runs and any(r >= 2 for r in runs) and only_run and trailing
    assert {0, 15} <= luma and luma - {0, 15} and chroma == {0, 1, 2}
    assert intra_after_inter and inter_after_intra
    assert pcm == {"bits", "level"} and inter_after_pcm
    assert wrap and short


def test_sizes():
    """No P macroblock above 3200 bits; every slice inside the documented capacity (asserted in the restatement and in the round trip); the
    two inequalities at every qp; bytes per picture pinned at + 10 % of what this restatement measured at qp 16 on (6, 96, 128), gop 6
    (IDR + 5 P pictures), bytes of the six samples together: still 2067, fade 7991 (11875 all intra), pan 11088, cut 45150, noise 86563, zeros_pcm 1986."""
    for shape, kind, qp in CASES:
        st = P.reference(shape, kind, qp)[3]
        assert not st["p_mb_bits"] or max(st["p_mb_bits"]) <= R.MAX_MB_BITS
    shape = (6, 96, 128)
    measured = dict(still=2067, fade=7991, pan=11088, cut=45150, noise=86563, zeros_pcm=1986)
    for qp in P.QPS:
        sizes = {}
        for kind in P.KINDS:
            planes = P.make_planes(kind, *shape)
            sizes[kind] = [len(s) for s in P.encode_planes(*planes, qp=qp, gop=6)[0]]
            if kind == "fade":
                intra = sum(len(s) for s in P.encode_planes(*planes, qp=qp, gop=1)[0])
                print(f"qp {qp} fade: gop 6 {sum(sizes[kind])} bytes, gop 1 {intra} bytes, ratio {sum(sizes[kind]) / intra:.3f}")
                assert sum(sizes[kind]) < intra, (qp, sizes[kind], intra)
        assert all(p < sizes["still"][0] for p in sizes["still"][1:]), (qp, sizes["still"])
        print(f"qp {qp}: " + ", ".join(f"{k} {sum(v)}" for k, v in sizes.items()))
        if qp == 16:
            for kind in P.KINDS:
                assert sum(sizes[kind]) <= measured[kind] * 1.1, (kind, sum(sizes[kind]))


def test_capacity_bound_of_the_gop_path(hip):
    """The derivation of sdv_hip.h in numbers: the P slice's bound fits the slot of the wider picture for every admitted width, and the
    size functions of the binding are those of the restatement."""
    for mbw in range(1, hip.H264_GOP_MAX_MBW + 1):
        rbsp = P.p_rbsp_bound(mbw)
        assert rbsp <= 403 * mbw + 13 and 5 + rbsp + rbsp // 2 <= P.slot_bytes(mbw) == hip.h264_slice_bytes(hip.h264_gop_slot_mbw(mbw))
        assert 400 * mbw + 10 <= rbsp                                               # an IDR slice of the GOP path: 72 bits of header + stop bit
    assert hip.h264_gop_slot_mbw(hip.H264_GOP_MAX_MBW) == 1024 and hip.h264_gop_slot_mbw(3) == P.slot_mbw(3) == 4
    assert hip.h264_gop_out_bytes(2, 5, 3) == hip.h264_out_bytes(2, 5, 4) and hip.h264_gop_scratch_bytes(2, 5, 3) == hip.h264_scratch_bytes(2, 5, 4)
    assert hip.h264_out_bytes(2, 5, 3) == 10 * 1817                                # (the intra path's functions are untouched)


def _stss(path):
    data = open(path, "rb").read()
    ftyp = int.from_bytes(data[:4], "big")
    moov = ftyp + int.from_bytes(data[ftyp + 8:ftyp + 16], "big")                  # behind the mdat box (64-bit size)
    assert data[moov + 4:moov + 8] == b"moov"
    at = data.find(b"stss", moov)
    if at < 0:
        return None
    count = struct.unpack(">I", data[at + 8:at + 12])[0]
    return [v - 1 for v in struct.unpack(f">{count}I", data[at + 12:at + 12 + 4 * count])]


def test_stss_box_names_the_idr_pictures_and_is_absent_by_default(tmp_path):
    from stable_diffusion_videos_amd import video
    planes = P.make_planes("fade", 7, 32, 32)
    samples = P.encode_planes(*planes, qp=16, gop=3)[0]
    a = video.write_h264_mp4(None, 32, 32, 5, tmp_path / "a.mp4", samples=samples, sync_samples=P.sync_samples(7, 3))
    assert _stss(a) == [0, 3, 6]
    assert R.mp4_samples(a)[3] == samples
    intra = R.encode_planes(*planes, qp=16)[0]
    b = video.write_h264_mp4(None, 32, 32, 5, tmp_path / "b.mp4", samples=intra)
    c = video.write_h264_mp4(None, 32, 32, 5, tmp_path / "c.mp4", samples=intra, sync_samples=list(range(7)))
    assert _stss(b) is None and open(b, "rb").read() == open(c, "rb").read()
    filled = []                                                                   # a list the sample generator fills, as video.py does

    def gen():
        for k, s in enumerate(samples):
            yield s
            if k % 3 == 0:
                filled.append(k)
    d = video.write_h264_mp4(None, 32, 32, 5, tmp_path / "d.mp4", samples=gen(), sync_samples=filled)
    assert open(d, "rb").read() == open(a, "rb").read()


def test_default_files_are_the_parent_commits_bytes(tmp_path, monkeypatch):
    """SHA-256 computed with the parent commit's writer: the default (I_PCM) call with ``h264_gop`` unset, and the container around
    ready-made intra samples without a sync list."""
    pytest.importorskip("PIL")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = R.make_frames("ramp", 3, 36, 50)
    out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "d.mp4")
    if video.LAST_CODEC["video"] == "h264 (libx264)":
        pytest.skip("torchvision / pyav present: the dependency-free writer is not in use")
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"
    out = video.write_h264_mp4(None, 50, 36, 5, tmp_path / "e.mp4", samples=R.encode_frames(frames, qp=16)[0])
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == "5bf50cbeeb9dda546140fd1011954c74b1ef51807992483f3aef21f2e3a5a7d6"


def test_header_library_and_binding_agree_on_the_new_entry_point(hip):
    header = (ROOT / "include" / "sdv_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    name = "sdv_h264_encode_gops"
    assert re.search(rf"\bint {name}\s*\(", header) and hasattr(lib, name) and name in hip.EXPORTED_SYMBOLS
    assert "k_h264_encode_gops" in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key("sdv::k_h264_encode_gops", "Meta")
    decl = header[header.index(f"int {name}("):]
    assert len(decl[:decl.index(");")].split(",")) == len(hip._SIGNATURES[name][1])
    assert "H.264 P pictures" in header and "mbw' = mbw + 1 + mbw / 64" in header
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12 and len(hip.EXPORTED_SYMBOLS) == 51


def test_argument_checks_at_both_layers(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, check_gop, encoder_for
    assert H264Encoder().gop == 1 and H264Encoder(gop=12).gop == 12 and H264Encoder().last_sync == []
    assert encoder_for(20, "cuda:0") is encoder_for(20, "cuda:0", 1) is not encoder_for(20, "cuda:0", 2)
    for bad in (0, -1, 257, 12.0, "12", True, None):
        with pytest.raises(ValueError, match="1 .. 256"):
            check_gop(bad)
        with pytest.raises(ValueError, match="1 .. 256"):
            H264Encoder(gop=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder(gop=4).encode(torch.zeros((1, 16, 16, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    op = torch.ops.sdv.k_h264_encode_gops
    sb = hip.h264_gop_scratch_bytes(1, 2, 3)
    ok = dict(y=u8(1, 32, 48), cb=u8(1, 16, 24), cr=u8(1, 16, 24), qp=16, gop=4, first_index=0, ry=u8(1, 32, 48), rcb=u8(1, 16, 24), rcr=u8(1, 16, 24),
              scratch=u8(sb))
    for key, val, word in (("y", u8(1, 32, 40), "y must be"), ("cb", u8(1, 16, 16), "cb must be"), ("qp", 52, "qp must be"), ("gop", 0, "gop must be"),
                           ("gop", 257, "gop must be"), ("first_index", -1, "first_index"), ("ry", u8(1, 32, 32), "ry must be"),
                           ("rcb", u8(1, 8, 24), "rcb must be"), ("rcr", torch.zeros((1, 16, 24), dtype=torch.int8), "rcr must be"),
                           ("scratch", u8(sb - 1), "scratch holds"), ("scratch", u8(hip.h264_scratch_bytes(1, 2, 3)), "scratch holds"),
                           ("scratch", u8(sb), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            op(*dict(ok, **{key: val}).values())
    wide = 16 * (hip.H264_GOP_MAX_MBW + 1)
    with pytest.raises(hip.SdvHipError, match="wider than"):
        op(u8(1, 16, wide), u8(1, 8, wide // 2), u8(1, 8, wide // 2), 16, 2, 0, u8(1, 16, wide), u8(1, 8, wide // 2), u8(1, 8, wide // 2), u8(8))
    lib = hip.load()
    sb = hip.h264_gop_scratch_bytes(2, 3, 4)
    ok = [16, 32, 48, 2, 3, 4, 16, 2, 0, 64, 80, 96, 128, sb, None]
    for pos, val, word in ((0, None, b"null"), (9, None, b"null"), (11, None, b"null"), (12, None, b"null"), (3, 0, b"frame count"),
                           (4, 0, b"macroblock grid"), (5, 1009, b"above 1008"), (6, 52, b"qp="), (7, 0, b"gop="), (7, 257, b"gop="),
                           (8, -1, b"first_index"), (13, sb - 1, b"scratch buffer too small"), (0, 8, b"aligned"), (9, 72, b"aligned"),
                           (10, 84, b"aligned"), (12, 132, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_gops(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_encode_gops")


def test_pipeline_attribute_and_sdv_h264_gop(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_GOP", raising=False)
    assert pipe.h264_gop == 1 and pipe.h264_gop_choice() == 1
    pipe.h264_gop = 12
    assert pipe.h264_gop_choice() == 12
    monkeypatch.setenv("SDV_H264_GOP", "4")                                        # the variable wins when it is set
    assert pipe.h264_gop_choice() == 4
    for bad in ("0", "257", "-1", "four", " 4", "1.5"):
        monkeypatch.setenv("SDV_H264_GOP", bad)
        with pytest.raises(ValueError, match="SDV_H264_GOP"):
            pipe.h264_gop_choice()
    monkeypatch.delenv("SDV_H264_GOP")
    pipe.h264_gop = 300
    with pytest.raises(ValueError, match="h264_gop"):
        pipe.h264_gop_choice()


def test_make_video_pyav_checks_gop_and_falls_back_without_a_gpu(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = torch.from_numpy(R.make_frames("ramp", 3, 20, 36))
    for bad in (0, 257, "4", 2.0):
        with pytest.raises(ValueError, match="1 .. 256"):
            video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "x.mp4", codec="h264-cavlc", h264_gop=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=4)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"]
    b = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "b.mp4")
    assert open(a, "rb").read() == open(b, "rb").read() and _stss(a) is None
    c = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "c.mp4", h264_gop=4)           # ignored by the other codecs
    assert open(c, "rb").read() == open(b, "rb").read()


def test_decoder_refuses_a_vector_that_is_not_whole_sample():
    """Patch mvd_l0 of the first P_L0_16x16 macroblock of a one-macroblock picture from se(0) se(0) to se(1) se(0) (a quarter sample): the
    decoder must refuse it instead of assuming zero; se(8), two whole luma samples, decodes (edge-clamped copy)."""
    planes = P.make_planes("fade", 2, 16, 16)
    samples, ry, _, _ = P.encode_planes(*planes, qp=16, gop=2)
    s = samples[1]
    bits = np.unpackbits(np.frombuffer(R.unescape(s[5:]), dtype=np.uint8)).tolist()
    head = len(P.p_slice_header(0, 1, 16)) + 1 + 1                                  # header, mb_skip_run ue(0), mb_type ue(0)
    assert bits[head:head + 2] == [1, 1]                                            # mvd_l0: se(0) se(0)

    def patched(mvd_bits):
        b = bits[:head] + mvd_bits + bits[head + 1:]
        b = b[:len(b) - b[::-1].index(1) - 1] + [1]
        b += [0] * (-len(b) % 8)
        nal = bytes([0x41]) + R.escape(np.packbits(np.array(b, dtype=np.uint8)).tobytes())
        return len(nal).to_bytes(4, "big") + nal
    with pytest.raises(P.NotWholeSample):
        P.decode_stream([samples[0], patched([int(c) for c in R.se(1)])], 16, 16)
    with pytest.raises(P.NotWholeSample):
        P.decode_stream([samples[0], patched([int(c) for c in R.se(4)])], 16, 16)    # whole in luma, half a sample in chroma
    d = P.decode_stream([samples[0], patched([int(c) for c in R.se(8)])], 16, 16)
    assert d["n_inter"] == 1 and not np.array_equal(d["y"][1], ry[1])
    assert np.array_equal(P.decode_stream(samples, 16, 16)["y"], ry)


def test_host_build_of_the_core_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/sdv_h264_core.h's GOP path compiled for the host with -fsanitize=address,undefined into a stand-alone program
    (tests/h264_p_host_main.cpp) and run as a subprocess: samples and reconstruction equal the restatement's on three cases."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "h264_p_host"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "stable_diffusion_videos_amd" / "csrc"), str(ROOT / "tests" / "h264_p_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    for shape, kind, qp in (((7, 64, 64, 3), "cut", 0), ((3, 36, 50, 3), "pan", 16), ((5, 32, 48, 5), "flash_pcm", 0)):
        (y, cb, cr), samples, recon, _ = P.reference(shape, kind, qp)
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        (tmp_path / "in.bin").write_bytes(np.array([n, mbh, mbw, qp, shape[3], P.FIRST], dtype="<i4").tobytes() + y.tobytes() + cb.tobytes() + cr.tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        data, at, got = (tmp_path / "out.bin").read_bytes(), 0, []
        for _ in range(n):
            size = int.from_bytes(data[at:at + 4], "little")
            got.append(data[at + 4:at + 4 + size])
            at += 4 + size
        assert got == samples, (shape, kind, qp)
        for want in recon:
            assert np.array_equal(np.frombuffer(data[at:at + want.size], dtype=np.uint8).reshape(want.shape), want), (shape, kind, qp)
            at += want.size
        assert at == len(data)
