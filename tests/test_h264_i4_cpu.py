"""Intra4x4 prediction of the H.264 IDR pictures (include/sdv_hip_h264_i4.h "H.264 Intra4x4") without a GPU: the two predictors of
tests/h264_i4_ref.py pinned on their own and against each other, the intra column of Table 9-4, the restatement against the decoder,
coverage read from the statistics, sizes against ``intra4`` 0, argument checks and plumbing, and the host build of csrc/sdv_h264_core.h's
Intra4x4 pieces under AddressSanitizer / UBSan against the restatement."""
import ctypes
import hashlib
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import h264_i4_ref as I
import h264_ref as R

ROOT = Path(__file__).resolve().parent.parent
SHA_DEFAULT = "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"
ALL = I.TOP | I.LEFT | I.CORNER | I.TOPRIGHT
CASES = [(s, k, g) for s in I.SHAPES for k in I.KINDS for g in I.SETTINGS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}-gop{g[0]}-search{g[1]}-subpel{g[2]}" for s, k, g in CASES]
SIZE_SHAPE = (2, 96, 128)                        # the largest shape of the set: most blocks have all their neighbours


def _edge(fn):
    """Edge vector (L3 L2 L1 L0 C T0 .. T7) and the clause form's dict, both sampled from fn(x, y)."""
    p = {(x, -1): fn(x, -1) for x in range(8)}
    p.update({(-1, y): fn(-1, y) for y in range(-1, 4)})
    e = np.array([p[(-1, 3)], p[(-1, 2)], p[(-1, 1)], p[(-1, 0)], p[(-1, -1)]] + [p[(x, -1)] for x in range(8)], dtype=np.int64)
    return e, p


# ------------------------------------------------------------------------------------------------------------------------------------
# the predictors alone
# ------------------------------------------------------------------------------------------------------------------------------------
def test_constant_neighbours_give_a_constant_prediction_in_every_mode():
    for value in (0, 77, 255):
        e, p = _edge(lambda x, y: value)
        for mode in range(9):
            assert (I.pred4(e, ALL, mode) == value).all(), (value, mode)
            assert (np.array(I.pred4_clauses(p, mode)) == value).all(), (value, mode)


def test_a_ramp_that_is_constant_along_a_modes_direction_is_reproduced_within_1():
    """v = 100 + 2 u with u = a x + b y constant along the direction of the mode: every mode's taps interpolate linearly between
    neighbours that lie on the line through the sample, so the prediction is v(x, y) up to the rounding - for HU only where it still
    interpolates (x + 2 y < 5; beyond it repeats p[-1,3])."""
    for mode, (a, b) in I._DIRECTION.items():
        v = lambda x, y: 100 + 2 * (a * x + b * y)
        e, p = _edge(v)
        want = np.array([[v(x, y) for x in range(4)] for y in range(4)])
        keep = np.array([[mode != I.HU or x + 2 * y < 5 for x in range(4)] for y in range(4)])
        for got in (I.pred4(e, ALL, mode), np.array(I.pred4_clauses(p, mode))):
            assert (np.abs(got - want)[keep] <= 1).all(), (mode, got, want)
    e, p = _edge(lambda x, y: 100 + 2 * (x + 2 * y))
    assert (I.pred4(e, ALL, I.HU)[~np.array([[x + 2 * y <= 5 for x in range(4)] for y in range(4)])] == p[(-1, 3)]).all()


def test_the_transpose_maps_v_to_h_vr_to_hd_and_ddr_to_itself():
    rng = np.random.default_rng(3)
    for _ in range(20):
        e = rng.integers(0, 256, 13)
        t = e.copy()
        t[0:9] = e[0:9][::-1]                                                       # left column <-> top row, the corner stays
        for mode, other in ((I.V, I.H), (I.H, I.V), (I.VR, I.HD), (I.HD, I.VR), (I.DDR, I.DDR), (I.DC, I.DC)):
            assert np.array_equal(I.pred4(e, ALL, mode), I.pred4(t, ALL, other).T), (mode, other)


def test_the_table_form_equals_the_clause_form_on_random_neighbours():
    rng = np.random.default_rng(4)
    for _ in range(50):
        vals = rng.integers(0, 256, (5, 9))
        e, p = _edge(lambda x, y: int(vals[y + 1, x + 1]))
        for mode in range(9):
            assert np.array_equal(I.pred4(e, ALL, mode), np.array(I.pred4_clauses(p, mode))), mode


def test_top_right_substitution():
    """Without top-right samples p[4..7,-1] = p[3,-1]: edge_of says so, and DDL / VL then read T3 where they would read T4 .. T7."""
    rng = np.random.default_rng(5)
    ry = rng.integers(0, 256, (16, 16))
    for bx, by in ((1, 1), (1, 3), (3, 1), (3, 2), (3, 3)):
        av = I.avail4(bx, by, True)
        assert av & I.TOP and not av & I.TOPRIGHT
        e = I.edge_of(ry, rng.integers(0, 256, 16), bx, by, av)
        assert (e[9:13] == e[8]).all() and np.array_equal(e[5:9], ry[4 * by - 1, 4 * bx:4 * bx + 4])
        p = {(x, -1): int(ry[4 * by - 1, 4 * bx + min(x, 3)]) for x in range(8)}
        for mode in (I.DDL, I.VL):
            assert np.array_equal(I.pred4(e, av, mode), np.array(I.pred4_clauses(p, mode)))
        assert (I.pred4(e, av, I.DDL)[3, :] == e[8]).all() and I.pred4(e, av, I.VL)[3, 3] == e[8]
    for bx, by in ((0, 1), (2, 1), (0, 2), (1, 2), (2, 2), (0, 3), (2, 3)):
        av = I.avail4(bx, by, False)
        assert av & I.TOPRIGHT and np.array_equal(I.edge_of(ry, None, bx, by, av)[9:13], ry[4 * by - 1, 4 * bx + 4:4 * bx + 8])
    assert all(not I.avail4(bx, 0, True) & (I.TOP | I.TOPRIGHT | I.CORNER) for bx in range(4))
    assert I.avail4(0, 2, False) == I.TOP | I.TOPRIGHT and I.avail4(0, 0, False) == 0 and I.avail4(0, 0, True) == I.LEFT


def test_the_three_dc_fallbacks():
    e, p = _edge(lambda x, y: 10 * (x + 1) if y < 0 else 200 + y)
    st, sl = 10 + 20 + 30 + 40, 200 + 201 + 202 + 203
    top_only = {k: v for k, v in p.items() if k[1] == -1 and k[0] >= 0}
    left_only = {k: v for k, v in p.items() if k[0] == -1 and k[1] >= 0}
    for avail, sub, want in ((I.TOP | I.LEFT | I.CORNER, p, (st + sl + 4) >> 3), (I.TOP, top_only, (st + 2) >> 2), (I.LEFT, left_only, (sl + 2) >> 2),
                             (0, {}, 128)):
        assert (I.pred4(e, avail, I.DC) == want).all() and (np.array(I.pred4_clauses(sub, I.DC)) == want).all()
    for mode in range(9):                                                           # a mode that reads a missing sample is refused
        if mode != I.DC:
            with pytest.raises(KeyError):
                I.pred4_clauses({}, mode)
            with pytest.raises(AssertionError):
                I.pred4(e, 0, mode)


# ------------------------------------------------------------------------------------------------------------------------------------
# Table 9-4, intra column
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_intra_cbp_column():
    assert sorted(I.CBP_INTRA) == list(range(48))
    assert I.CBP_INTRA[:16] == (47, 31, 15, 0, 23, 27, 29, 30, 7, 11, 13, 14, 39, 43, 45, 46)
    core = (ROOT / "stable_diffusion_videos_amd" / "csrc" / "sdv_h264_core.h").read_text()
    body = core[core.index("H264_HD int h264_cbp_intra_code(int cbp)"):]
    table = [int(v) for v in re.findall(r"\d+", body[body.index("{", body.index("t[48]")) + 1:body.index("};")])]
    assert len(table) == 48 and all(I.CBP_INTRA[table[cbp]] == cbp for cbp in range(48))
    import h264_p_ref as P
    assert tuple(I.CBP_INTRA) != tuple(P.CBP_INTER)


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement against the decoder
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind,setting", CASES, ids=IDS)
def test_the_decoder_gives_the_restatements_reconstruction(shape, kind, setting):
    n, h, w = shape
    for qp in I.QPS:
        _, samples, recon, stats = I.reference(shape, kind, qp, setting)
        d = I.decode_stream(samples, w, h)
        assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon)), qp
        assert d["sync"] == list(range(0, n, setting[0])) and d["p_i4"] == 0
        assert d["n_i4"] == stats["i4"]["mbs"] and d["i4_modes"] == stats["i4"]["modes"]


def test_coverage_of_the_case_set():
    """Read from the statistics of the round-trip cases (all intra: every picture an IDR picture)."""
    total = I.new_stats()["i4"]
    for shape in I.SHAPES:
        for kind in I.KINDS + (I.EXTRA_KINDS if shape == SIZE_SHAPE else ()):
            for qp in I.QPS:
                _, samples, recon, stats = I.reference(shape, kind, qp, (1, 0, 0))
                st = stats["i4"]
                if kind in I.EXTRA_KINDS:                                          # (the others: the round trips above)
                    d = I.decode_stream(samples, shape[2], shape[1])
                    assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon)) and d["n_i4"] == st["mbs"] > 0
                for key, v in st.items():
                    if isinstance(v, set):
                        total[key] |= v
                    elif key == "modes":
                        total[key] = [a + b for a, b in zip(total[key], v)]
                    else:
                        total[key] += v
    assert all(c > 0 for c in total["modes"]), total["modes"]                      # every mode 0 .. 8 chosen
    assert total["flags"] == {0, 1} and total["rem_below"] > 0 and total["rem_above"] > 0
    classes = {I.avail4(bx, by, left) for bx in range(4) for by in range(4) for left in (False, True)}
    assert total["avail"] == classes == {0, I.LEFT, I.TOP | I.TOPRIGHT, I.TOP | I.LEFT | I.CORNER, ALL}    # each availability class
    assert total["substituted"] > 0
    kinds = ("i4", "i16", "pcm")
    assert {(a, b) for a in kinds for b in kinds} <= total["after"], total["after"]
    assert {(None, b) for b in kinds} <= total["after"]
    assert total["cbp0"] > 0 and total["cbp_chroma"] == {0, 1, 2} and len(total["cbp_codes"]) >= 20, sorted(total["cbp_codes"])
    assert total["pcm_from_i4"] > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# size
# ------------------------------------------------------------------------------------------------------------------------------------
def _size(kind, qp):
    (y, _, _), a, (ry, _, _), _ = I.reference(SIZE_SHAPE, kind, qp, (1, 0, 0), 1)
    _, b, (ry0, _, _), _ = I.reference(SIZE_SHAPE, kind, qp, (1, 0, 0), 0)
    psnr = lambda r: 10 * np.log10(255.0 ** 2 / max(float(((r.astype(np.float64) - y) ** 2).mean()), 1e-9))
    return sum(map(len, a)), sum(map(len, b)), psnr(ry), psnr(ry0)


@pytest.mark.parametrize("kind", I.GRATINGS + ("glyphs", "vramp"))
def test_intra4_takes_fewer_bytes_on_directional_content(kind):
    for qp in (16, 28):
        a, b, pa, pb = _size(kind, qp)
        print(f"{kind} qp {qp}: {a} bytes with intra4 1, {b} with 0, ratio {a / b:.3f}; Y-PSNR {pa:.2f} dB against {pb:.2f} dB")
        assert a < b, (kind, qp, a, b)


def test_noise_and_zeros_pcm_sizes_are_reported():
    for kind in ("noise", "zeros_pcm"):
        for qp in (16, 28):
            a, b, pa, pb = _size(kind, qp)
            print(f"{kind} qp {qp}: {a} bytes with intra4 1, {b} with 0, ratio {a / b:.3f}; Y-PSNR {pa:.2f} dB against {pb:.2f} dB")


def test_flat_macroblocks_stay_intra16x16():
    """DC16 of the decision is the macroblock's own DC, so sum |src - DC16| is 0 on a flat macroblock and no sum of costs is below it:
    with or without a left neighbour (the first macroblock of a row is predicted from 128 against luma 129 of this picture)."""
    for qp in I.QPS:
        st = I.reference(SIZE_SHAPE, "flat", qp, (1, 0, 0))[3]["i4"]
        assert st["kinds"] and all(k == "i16" for k in st["kinds"]), qp


def test_flat_takes_the_bytes_of_intra4_0():
    for qp in I.QPS:
        a, b, _, _ = _size("flat", qp)
        assert a == b, (qp, a, b)


# ------------------------------------------------------------------------------------------------------------------------------------
# everything else
# ------------------------------------------------------------------------------------------------------------------------------------
def test_default_files_are_the_parent_commits_bytes(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = R.make_frames("ramp", 3, 36, 50)
    out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "d.mp4")
    if video.LAST_CODEC["video"] == "h264 (libx264)":
        pytest.skip("torchvision / pyav present: the dependency-free writer is not in use")
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == SHA_DEFAULT
    for value in (0, 1):                                                            # the default codec is not this track: no effect
        out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", h264_intra4=value)
        assert hashlib.sha256(open(out, "rb").read()).hexdigest() == SHA_DEFAULT
        assert "intra4" not in video.LAST_CODEC


def test_i4_header_library_and_binding_agree(hip):
    header = (ROOT / "include" / "sdv_hip_h264_i4.h").read_text()
    names = {"sdv_h264_encode_idr4": "k_h264_encode_idr4"}
    declared = set(re.findall(r"\bint (sdv_[a-z0-9_]+)\s*\(", header))
    assert declared == set(hip.H264_I4_SYMBOLS) == set(names)
    assert not set(hip.H264_I4_SYMBOLS) & (set(hip.EXPORTED_SYMBOLS) | set(hip.EXTENSION_SYMBOLS) | set(hip.H264_SUB_SYMBOLS))
    others = [(ROOT / "include" / f).read_text() for f in ("sdv_hip.h", "sdv_hip_ext.h", "sdv_hip_h264_sub.h")]
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in names.items():
        assert hasattr(lib, name) and not any(name in text for text in others)
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._H264_I4_SIGNATURES[name][1]), name
        assert getattr(hip.load(), name).argtypes == hip._H264_I4_SIGNATURES[name][1]
    assert "H.264 Intra4x4" in header and "8.3.1.2" in header and " ".join(map(str, I.CBP_INTRA[:20])) in " ".join(header.split()).replace("* ", "")
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="meta")                # the Meta kernel accepts the schema and does nothing
    torch.ops.sdv.k_h264_encode_idr4(u8(2, 32, 48), u8(2, 16, 24), u8(2, 16, 24), 16, 1, 0, u8(2, 32, 48), u8(2, 16, 24), u8(2, 16, 24), u8(64))


def test_argument_checks_at_both_layers(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, check_intra4, encoder_for
    assert H264Encoder().intra4 == 0 and H264Encoder(gop=4, search=8, subpel=4, intra4=1).intra4 == 1 and H264Encoder(intra4=1).gop == 1
    assert [check_intra4(v) for v in (0, 1)] == [0, 1]
    assert encoder_for(20, "cuda:0", 4, 8, 4) is encoder_for(20, "cuda:0", 4, 8, 4, 0) is encoder_for(20, "cuda:0", 4, 8, 4, intra4=0)
    assert encoder_for(20, "cuda:0", 4, 8, 4, 1) is not encoder_for(20, "cuda:0", 4, 8, 4)
    for bad in (2, -1, True, False, "1", 1.0, None):
        with pytest.raises(ValueError, match="one of the integers 0, 1"):
            check_intra4(bad)
        with pytest.raises(ValueError, match="one of the integers 0, 1"):
            H264Encoder(intra4=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder(intra4=1).encode(torch.zeros((2, 16, 16, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    op = torch.ops.sdv.k_h264_encode_idr4
    sb = hip.h264_gop_scratch_bytes(2, 2, 3)
    ok = dict(y=u8(2, 32, 48), cb=u8(2, 16, 24), cr=u8(2, 16, 24), qp=16, gop=4, first_index=0, ry=u8(2, 32, 48), rcb=u8(2, 16, 24),
              rcr=u8(2, 16, 24), scratch=u8(sb))
    for key, val, word in (("y", u8(2, 32, 40), "y must be"), ("cb", u8(2, 16, 16), "cb must be"), ("qp", -1, "qp must be"), ("qp", 52, "qp must be"),
                           ("gop", 0, "gop must be"), ("gop", 257, "gop must be"), ("first_index", -1, "first_index"), ("ry", u8(2, 32, 32), "ry must be"),
                           ("rcr", u8(2, 8, 24), "rcr must be"), ("scratch", u8(sb - 1), "scratch holds"),
                           ("scratch", u8(hip.h264_scratch_bytes(2, 2, 3)), "scratch holds"), ("scratch", u8(sb), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            op(*dict(ok, **{key: val}).values())
    lib = hip.load()
    sb = hip.h264_gop_scratch_bytes(2, 3, 4)
    ok = [16, 32, 48, 2, 3, 4, 16, 4, 0, 64, 80, 96, 128, sb, None]                 # y cb cr | n mbh mbw qp gop first | ry rcb rcr scratch | bytes
    for pos, val, word in ((0, None, b"null"), (9, None, b"null"), (12, None, b"null"), (3, 0, b"frame count"), (4, 0, b"macroblock grid"),
                           (5, 1009, b"above 1008"), (6, 52, b"qp="), (6, -1, b"qp="), (7, 0, b"gop="), (7, 257, b"gop="), (8, -1, b"first_index"),
                           (13, sb - 1, b"scratch buffer too small"), (0, 8, b"aligned"), (9, 72, b"aligned"), (10, 84, b"aligned"), (12, 132, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_idr4(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_encode_idr4")


def test_pipeline_attribute_and_sdv_h264_intra4(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_INTRA4", raising=False)
    assert pipe.h264_intra4 == 0 and pipe.h264_intra4_choice() == 0
    pipe.h264_intra4 = 1
    assert pipe.h264_intra4_choice() == 1
    monkeypatch.setenv("SDV_H264_INTRA4", "0")                                      # the variable wins when it is set
    assert pipe.h264_intra4_choice() == 0
    monkeypatch.setenv("SDV_H264_INTRA4", "")
    assert pipe.h264_intra4_choice() == 1
    for bad in ("2", "-1", "one", " 1", "1.0", "true"):
        monkeypatch.setenv("SDV_H264_INTRA4", bad)
        with pytest.raises(ValueError, match="SDV_H264_INTRA4"):
            pipe.h264_intra4_choice()
    monkeypatch.delenv("SDV_H264_INTRA4")
    for bad in (2, True, "1"):
        pipe.h264_intra4 = bad
        with pytest.raises(ValueError, match="h264_intra4"):
            pipe.h264_intra4_choice()


def test_make_video_pyav_checks_intra4_and_falls_back_without_a_gpu(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import utils, video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = torch.from_numpy(R.make_frames("ramp", 3, 20, 36))
    for bad in (2, -1, "1", 1.0, True):
        with pytest.raises(ValueError, match="one of the integers 0, 1"):
            video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "x.mp4", codec="h264-cavlc", h264_intra4=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=4, h264_intra4=1)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"] and "intra4" not in video.LAST_CODEC
    b = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "b.mp4")
    c = utils.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "c.mp4", h264_gop=4, h264_intra4=1)   # ignored by the other codecs
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def test_host_build_of_the_intra4x4_pieces_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/sdv_h264_core.h's Intra4x4 macroblock step (edges, predictor, block chain, I_NxN coder, the Intra16x16 and I_PCM ways out)
    compiled for the host with -fsanitize=address,undefined into a stand-alone program (tests/h264_i4_host_main.cpp) and run as a
    subprocess on exact-size buffers: samples, reconstruction, macroblock kinds and the nine predictions of a full edge vector equal the
    restatement's on four cases."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "h264_i4_host"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "stable_diffusion_videos_amd" / "csrc"), str(ROOT / "tests" / "h264_i4_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    code = {"i16": 0, "pcm": 3, "i4": 4}                                            # kH264ModeIntra, kH264ModePcm, kH264ModeI4
    for shape, kind, qp in (((3, 36, 50), "glyphs", 16), ((2, 96, 128), "noise", 0), ((3, 32, 48), "grat6", 28), ((2, 96, 128), "zeros_pcm", 51)):
        (y, cb, cr), samples, recon, stats = I.reference(shape, kind, qp)
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        (tmp_path / "in.bin").write_bytes(np.array([n, mbh, mbw, qp, I.FIRST], dtype="<i4").tobytes() + y.tobytes() + cb.tobytes() + cr.tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        data, at, got = (tmp_path / "out.bin").read_bytes(), 0, []
        for _ in range(n):
            size = int.from_bytes(data[at:at + 4], "little")
            got.append(data[at + 4:at + 4 + size])
            at += 4 + size
        assert got == samples, (shape, kind, qp)
        for want in recon:
            assert np.array_equal(np.frombuffer(data[at:at + want.size], dtype=np.uint8).reshape(want.shape), want), (shape, kind, qp)
            at += want.size
        assert list(data[at:at + n * mbh * mbw]) == [code[k] for k in stats["i4"]["kinds"]]
        at += n * mbh * mbw
        for f in range(n):
            e = y[f].reshape(-1)[:13].astype(np.int64)                              # corner, top 0 .. 7, left 0 .. 3
            want = I.pred4_all(np.concatenate([e[9:13][::-1], e[0:1], e[1:9]]), ALL)
            assert np.array_equal(np.frombuffer(data[at:at + 144], dtype=np.uint8).reshape(9, 16), want)
            at += 144
        assert at == len(data)
