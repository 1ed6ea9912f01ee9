"""The in-loop deblocking filter of the H.264 track (include/sdv_hip_h264_lf.h "H.264 deblocking") without a GPU: the two filters of
tests/h264_lf_ref.py pinned on their own and against each other, the tables, the restatement against the decoder (exact equality, no
tolerance anywhere), coverage read from the decoder's statistics, argument checks and plumbing, and the host build of
csrc/sdv_h264_core.h's filter pieces under AddressSanitizer / UBSan against the restatement.

The rule, restated: slice headers write disable_deblocking_filter_idc 0 and two zero offsets; every reconstructed picture is filtered by 8.7
(bS 4 / 3 at intra edges, 2 at coded blocks, 1 where vectors differ by >= 4 quarter samples; qP 0 for I_PCM; chroma through QPc; indexA =
indexB = (qPp + qPq + 1) >> 1) on the whole macroblock grid, slice boundaries included and picture edges excluded, before it is shown and
before the next picture predicts from it; intra prediction reads unfiltered samples.

One item of the coverage list, an I_PCM-sided filtered edge at indexA >= 16, needs an I_PCM macroblock at qp >= 31 (the I_PCM side counts as
qP 0).  The track's own I_PCM triggers (more than 3200 bits, level_prefix > 15) cannot fire there: at qp >= 31 the largest level any
residual of 8-bit samples gives is below 256, far from the 2063 that level_prefix 15 still codes, and 384 such levels stay below 3200 bits
(measured: no I_PCM macroblock on uniform or binary noise from qp 28 up).  So the case set has one more kind, ``forced_pcm``, whose
restatement codes every third macroblock as I_PCM - a choice every encoder is free to make - at qp 40 and 51; the GPU meets such words
through sdv_h264_deblock alone (tests/test_h264_lf_gpu.py)."""
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
import h264_lf_ref as L
import h264_ref as R

ROOT = Path(__file__).resolve().parent.parent
SHA_DEFAULT = "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"
CASES, IDS, _planes, _info = L.CASES, L.IDS, L.random_planes, L.random_info
FORCED = [(s, L.FORCED_KIND, g) for s in ((3, 36, 50), (3, 48, 80)) for g in L.SETTINGS]
TOTAL = L.new_lf_stats()                         # what the decoder's filter met over the whole case set (filled by the round trips)
COUNTED = set()                                  # the (shape, kind, qp, setting) that are in TOTAL


class _Pic:
    """What deblock_picture reads of a decoded picture, made from the encoder side's information."""

    def __init__(self, planes, info):
        self.mbh, self.mbw = info["intra"].shape
        self.Y, self.C = planes[0].astype(np.int64).copy(), np.stack([planes[1], planes[2]]).astype(np.int64)
        self.ref = [-1 if v else 0 for v in info["intra"].reshape(-1)]
        self.pcm = {i for i, v in enumerate(info["pcm"].reshape(-1)) if v}
        self.nz_y = info["nz"].astype(np.int64) * 3
        self.mv = [tuple(int(c) for c in v) for v in info["mv"].reshape(-1, 2)]
        self.slice_of = [i // self.mbw for i in range(self.mbh * self.mbw)]


def _both(planes, info, qp):
    """The planes through the diagonal / vectorised filter and through the clause filter -> (diagonal's, clauses', the clause statistics)."""
    a = [p.astype(np.int64).copy() for p in planes]
    L.filter_diagonals(a[0], a[1], a[2], qp, info)
    pic, st = _Pic(planes, info), L.new_lf_stats()
    L.deblock_picture(pic, qp, st)
    return a, [pic.Y, pic.C[0], pic.C[1]], st


# ------------------------------------------------------------------------------------------------------------------------------------
# the filter alone
# ------------------------------------------------------------------------------------------------------------------------------------
def test_the_tables():
    assert len(L.ALPHA) == len(L.BETA) == len(L.TC0) == 52
    for t in (L.ALPHA, L.BETA, [v[0] for v in L.TC0], [v[1] for v in L.TC0], [v[2] for v in L.TC0]):
        assert all(a <= b for a, b in zip(t, t[1:])), "non-decreasing"
    assert all(v == 0 for v in L.ALPHA[:16] + L.BETA[:16]) and L.ALPHA[16] == 4 and L.BETA[16] == 2 and all(v == (0, 0, 0) for v in L.TC0[:17])
    assert all(a <= b <= c for a, b, c in L.TC0)
    assert L.ALPHA[51] == 255 and L.BETA[51] == 18 and L.TC0[51] == (13, 17, 25) and L.TC0[17] == (0, 0, 1) and L.TC0[23] == (1, 1, 1)
    header = " ".join((ROOT / "include" / "sdv_hip_h264_lf.h").read_text().replace("*", " ").split())
    assert " ".join(map(str, L.ALPHA[16:])) in header and " ".join(map(str, L.BETA[16:])) in header
    for (lo, hi), v in L._TC0_RUNS:                                                 # the header's tc0 runs are the table's
        assert (f"{lo} - {hi} " if hi > lo else f"{lo} ") + "(%d,%d,%d)" % v in header, (lo, hi, v)


def test_a_flat_picture_is_a_fixed_point_at_every_bs():
    rng = np.random.default_rng(1)
    for qp in (16, 28, 51):
        for p_intra in (0.0, 0.5, 1.0):
            info = _info(rng, 3, 4, p_intra)
            planes = tuple(np.full(s, 77, dtype=np.int64) for s in ((48, 64), (24, 32), (24, 32)))
            a, b, st = _both(planes, info, qp)
            assert all((x == 77).all() and (y == 77).all() for x, y in zip(a, b))
    assert {bs for (_, _, bs) in st["bs"]} >= {3, 4}


def test_a_step_below_and_above_alpha_against_hand_computed_lines():
    """qp 28 on both sides: index 28, alpha 20, beta 7, tc0 (1, 1, 2).  A step p = 100 | q = 100 + s between flat halves."""
    assert (L.ALPHA[28], L.BETA[28], L.TC0[28]) == (20, 7, (1, 1, 2))
    line = lambda s: np.array([100] * 4 + [100 + s] * 4)
    # step 8 < alpha: ap = aq = 0 < beta.  bS 1, 2: tc = 1 + 2 = 3, delta = (4 * 8 + (100 - 108) + 4) >> 3 = 3; p1 += clip((100 + 104 - 200) >> 1 = 2, 1) = 1,
    # q1 += clip((108 + 104 - 216) >> 1 = -2, -1) = -1
    for bs in (1, 2):
        assert list(L.filter_lines(line(8), bs, 28, False)) == [100, 100, 101, 103, 105, 107, 108, 108]
    # bS 3: tc0 2, tc 4, delta 3; p1 + clip(2, 2) = 102, q1 + clip(-2, -2) = 106
    assert list(L.filter_lines(line(8), 3, 28, False)) == [100, 100, 102, 103, 105, 106, 108, 108]
    # bS 4: |p0 - q0| = 8 >= (20 >> 2) + 2 = 7: the weak form (2 p1 + p0 + q1 + 2) >> 2 = (200 + 100 + 108 + 2) >> 2 = 102, q0 = (216 + 108 + 100 + 2) >> 2 = 106
    assert list(L.filter_lines(line(8), 4, 28, False)) == [100, 100, 100, 102, 106, 108, 108, 108]
    # step 6 < 7: the strong form: p0 = (100 + 200 + 200 + 212 + 106 + 4) >> 3 = 102, p1 = (300 + 106 + 2) >> 2 = 102, p2 = (200 + 300 + 100 + 100 + 106 + 4) >> 3 = 101;
    # q0 = (100 + 200 + 212 + 212 + 106 + 4) >> 3 = 104, q1 = (100 + 318 + 2) >> 2 = 105, q2 = (212 + 318 + 106 + 106 + 100 + 4) >> 3 = 105
    assert list(L.filter_lines(line(6), 4, 28, False)) == [100, 101, 102, 102, 104, 105, 105, 106]
    # chroma: bS 1: tc = tc0 + 1 = 2, delta = clip(3) = 2; bS 4: the weak form
    assert list(L.filter_lines(line(8), 1, 28, True)) == [100, 100, 100, 102, 106, 108, 108, 108]
    assert list(L.filter_lines(line(8), 4, 28, True)) == [100, 100, 100, 102, 106, 108, 108, 108]
    for bs in (1, 2, 3, 4):                                                         # a step of alpha or more is an edge of the picture's content
        for chroma in (False, True):
            assert list(L.filter_lines(line(20), bs, 28, chroma)) == list(line(20))
            assert list(L.filter_lines(line(-25), bs, 28, chroma)) == list(line(-25))
    assert list(L.filter_lines(line(8), 0, 28, False)) == list(line(8))
    st = L.new_lf_stats()                                                           # the clause form on the same lines
    for s, bs, chroma in ((8, 1, False), (8, 3, False), (8, 4, False), (6, 4, False), (8, 1, True), (8, 4, True), (20, 4, False)):
        want = L.filter_lines(line(s), bs, 28, chroma)
        r = 2 if chroma else 4
        pp, qq, _ = L._line_clauses([100] * r, [100 + s] * r, bs, 28, 28, chroma, st)
        assert pp == list(want[3::-1][:r]) and qq == list(want[4:4 + r]), (s, bs, chroma)
    assert st["strong_taken"] == 2 and st["strong_refused"] == 2


def test_the_two_filters_agree_on_random_pictures_and_random_side_information():
    """The diagonal order with whole edges as arrays against raster order with loops over lines: every bS, I_PCM sides, vectors."""
    rng = np.random.default_rng(2)
    seen = set()
    for mbh, mbw, qp, lo, hi in ((1, 1, 30, 0, 256), (1, 5, 36, 100, 130), (5, 1, 36, 100, 130), (3, 5, 28, 90, 120), (6, 8, 40, 0, 256), (4, 3, 51, 60, 200),
                                 (3, 4, 17, 120, 126)):
        info = _info(rng, mbh, mbw)
        a, b, st = _both(_planes(rng, mbh, mbw, lo, hi), info, qp)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (mbh, mbw, qp)
        seen |= {bs for (_, _, bs), n in st["bs"].items() if n}
    assert seen == {0, 1, 2, 3, 4}


def test_the_transpose_of_vertical_only_is_horizontal_only_of_the_transpose():
    rng = np.random.default_rng(3)
    mbh, mbw, qp = 3, 4, 34
    info = _info(rng, mbh, mbw)
    planes = _planes(rng, mbh, mbw, 100, 140)
    tinfo = dict(intra=info["intra"].T.copy(), pcm=info["pcm"].T.copy(), nz=info["nz"].T.copy(), mv=info["mv"].transpose(1, 0, 2)[..., ::-1].copy())

    def one_direction(planes, info, dirn):
        pic = _Pic(planes, info)
        L.deblock_picture(pic, qp, L.new_lf_stats(), directions=(dirn,))
        return [pic.Y, pic.C[0], pic.C[1]]

    v = one_direction(planes, info, 0)
    h = one_direction(tuple(p.T.copy() for p in planes), tinfo, 1)
    assert all(np.array_equal(a.T, b) for a, b in zip(v, h))
    assert not np.array_equal(v[0], planes[0])


def test_qp_up_to_15_without_i_pcm_and_with_it_leaves_the_planes_untouched():
    rng = np.random.default_rng(4)
    for qp in (0, 12, 15):
        info = _info(rng, 3, 5, p_pcm=0.2 if qp == 15 else 0.0)
        planes = _planes(rng, 3, 5, 100, 104)
        a, b, _ = _both(planes, info, qp)
        assert all(np.array_equal(x, p) and np.array_equal(y, p) for x, y, p in zip(a, b, planes))
    info = _info(rng, 3, 5, p_pcm=0.0)
    a, _, _ = _both(_planes(rng, 3, 5, 100, 104), info, 16)                         # and 16 is the first quantiser that filters
    assert L.ALPHA[16] > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# round trips: the decoder's output of the restatement's bytes is its (filtered) reconstruction
# ------------------------------------------------------------------------------------------------------------------------------------
def _round_trip(shape, kind, qp, setting):
    (y, cb, cr), samples, recon, used, infos = L.reference(shape, kind, qp, setting)
    st = L.new_lf_stats()
    out = L.decode_stream(samples, shape[2], shape[1], stats=st)
    for name, want in zip(("y", "cb", "cr"), recon):
        assert np.array_equal(out[name], want), (shape, kind, qp, setting, name)
    assert out["sync"] == list(range(0, shape[0], setting[0]))
    assert all(h["deblock_idc"] == 0 for hs in out["headers"] for h in hs)
    if (shape, kind, qp, setting) in COUNTED:
        return out, st
    COUNTED.add((shape, kind, qp, setting))
    for key, val in st.items():
        if key == "bs":
            for k2, v2 in val.items():
                TOTAL["bs"][k2] = TOTAL["bs"].get(k2, 0) + v2
        else:
            TOTAL[key] += val
    return out, st


@pytest.mark.parametrize("shape,kind,setting", CASES + FORCED, ids=IDS + [f"{s[0]}x{s[1]}x{s[2]}-{k}-gop{g[0]}-search{g[1]}-subpel{g[2]}-intra4{g[3]}"
                                                                         for s, k, g in FORCED])
def test_round_trip(shape, kind, setting):
    for qp in (L.FORCED_QPS if kind == L.FORCED_KIND else L.QPS):
        out, st = _round_trip(shape, kind, qp, setting)
        if kind == L.FORCED_KIND:
            assert out["n_pcm"] > 0
        if qp <= 15:
            assert st["lines_changed"] == 0, "below index 16 nothing may change"


def test_coverage_of_the_case_set():
    """Read from the statistics the decoder's filter gathered over the round trips above (it runs after them, in this file's order).  Run
    without them, or after a selection of them, it first makes the round trips of a thinned case set that meets the list too."""
    for shape, kind, setting in CASES[::7] + FORCED[:2]:
        for qp in (L.FORCED_QPS if kind == L.FORCED_KIND else L.QPS):
            if (shape, kind, qp, setting) not in COUNTED:
                _round_trip(shape, kind, qp, setting)
    seen = lambda plane, d: {bs for (p, dd, bs), n in TOTAL["bs"].items() if p == plane and dd == d and n}
    assert seen("y", "v") == seen("y", "h") == {0, 1, 2, 3, 4}, TOTAL["bs"]
    assert (seen("cb", "v") | seen("cb", "h")) == (seen("cr", "v") | seen("cr", "h")) == {0, 1, 2, 3, 4}
    assert TOTAL["pcm_filtered"] > 0, "no filtered edge with an I_PCM side at indexA >= 16"
    assert TOTAL["strong_taken"] > 0 and TOTAL["strong_refused"] > 0
    assert TOTAL["slice_edge_changed"] > 0, "no top macroblock edge across a slice boundary changed a sample"


def test_deblock_1_changes_the_bytes_of_a_p_picture_on_a_blocky_kind():
    """The reference picture really is the filtered one: at qp 28 the P pictures of ``fade`` are coded differently with and without."""
    shape, setting = (3, 48, 80), (3, 0, 0, 0)
    on = L.reference(shape, "fade", 28, setting)
    off = L.reference(shape, "fade", 28, setting, deblock=0)
    assert len(on[1]) == len(off[1]) == 3
    assert not np.array_equal(on[2][0][0], off[2][0][0]), "the IDR picture's reconstruction is filtered"
    assert any(len(a) != len(b) for a, b in zip(on[1][1:], off[1][1:])) or any(a[8:] != b[8:] for a, b in zip(on[1][1:], off[1][1:]))
    dec_on, dec_off = L.decode_stream(on[1], 80, 48), I.decode_stream(off[1], 80, 48)
    assert not np.array_equal(dec_on["y"][1], dec_off["y"][1])
    assert np.array_equal(dec_off["y"], off[2][0])


def test_deblock_0_is_the_other_modules_restatement():
    for setting in ((1, 0, 0, 0), (3, 8, 4, 1)):
        a = L.reference((3, 36, 50), "glyphs", 28, setting, deblock=0)
        b = I.reference((3, 36, 50), "glyphs", 28, setting[:3], setting[3])
        assert a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def test_only_three_header_bits_differ_in_an_all_skip_picture():
    """``flat`` at gop 3: the P pictures are one skip run per slice; with the filter on the slice differs in the three header bits only."""
    on, off = L.reference((3, 36, 50), "flat", 28, (3, 0, 0, 0)), L.reference((3, 36, 50), "flat", 28, (3, 0, 0, 0), deblock=0)
    for a, b in zip(on[1][1:], off[1][1:]):
        assert len(a) == len(b)
        diff = [i for i in range(len(a)) if a[i] != b[i]]
        assert diff and all(bin(a[i] ^ b[i]).count("1") <= 3 for i in diff) and len(diff) <= 2 * 3


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
        out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", h264_deblock=value)
        assert hashlib.sha256(open(out, "rb").read()).hexdigest() == SHA_DEFAULT
        assert "deblock" not in video.LAST_CODEC


LF_OPS = {"sdv_h264_encode_gop_step_lf": "k_h264_encode_gop_step_lf", "sdv_h264_encode_gop_step_sub_lf": "k_h264_encode_gop_step_sub_lf",
          "sdv_h264_encode_idr4_lf": "k_h264_encode_idr4_lf", "sdv_h264_deblock": "k_h264_deblock"}


def test_lf_header_library_and_binding_agree(hip):
    header = (ROOT / "include" / "sdv_hip_h264_lf.h").read_text()
    declared = set(re.findall(r"\bint (sdv_[a-z0-9_]+)\s*\(", header))
    assert declared == set(hip.H264_LF_SYMBOLS) == set(LF_OPS)
    assert not set(hip.H264_LF_SYMBOLS) & (set(hip.EXPORTED_SYMBOLS) | set(hip.EXTENSION_SYMBOLS) | set(hip.H264_SUB_SYMBOLS) | set(hip.H264_I4_SYMBOLS))
    others = [(ROOT / "include" / f).read_text() for f in ("sdv_hip.h", "sdv_hip_ext.h", "sdv_hip_h264_sub.h", "sdv_hip_h264_i4.h")]
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in LF_OPS.items():
        assert hasattr(lib, name) and not any(name in text for text in others)
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._H264_LF_SIGNATURES[name][1]), name
        assert getattr(hip.load(), name).argtypes == hip._H264_LF_SIGNATURES[name][1]
    assert "H.264 deblocking" in header and "8.7" in header and "bits 0 .. 15" in header
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="meta")                # the Meta kernels accept the schemas and do nothing
    i16, i32 = torch.zeros((2, 2, 3, 2), dtype=torch.int16, device="meta"), torch.zeros((2, 2, 3), dtype=torch.int32, device="meta")
    planes = (u8(2, 32, 48), u8(2, 16, 24), u8(2, 16, 24))
    torch.ops.sdv.k_h264_deblock(*planes, 28, 2, 0, 0, i32, i16, 0)
    torch.ops.sdv.k_h264_encode_idr4_lf(*planes, 16, 1, 0, *planes, u8(64), i32)
    torch.ops.sdv.k_h264_encode_gop_step_lf(*planes, 16, 2, 1, 2, 0, i16, *planes, u8(64), i32)
    torch.ops.sdv.k_h264_encode_gop_step_sub_lf(*planes, 16, 2, 1, 2, 4, 0, i16, *planes, u8(64), i32)


def test_argument_checks_at_both_layers(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, check_deblock, encoder_for
    assert H264Encoder().deblock == 0 and H264Encoder(gop=4, search=8, subpel=4, intra4=1, deblock=1).deblock == 1 and H264Encoder(deblock=1).gop == 1
    assert [check_deblock(v) for v in (0, 1)] == [0, 1]
    assert encoder_for(21, "cuda:0", 4, 8, 4, 1) is encoder_for(21, "cuda:0", 4, 8, 4, 1, 0) is encoder_for(21, "cuda:0", 4, 8, 4, 1, deblock=0)
    assert encoder_for(21, "cuda:0", 4, 8, 4, 1, 1) is not encoder_for(21, "cuda:0", 4, 8, 4, 1)
    for bad in (2, -1, True, False, "1", 1.0, None):
        with pytest.raises(ValueError, match="one of the integers 0, 1"):
            check_deblock(bad)
        with pytest.raises(ValueError, match="one of the integers 0, 1"):
            H264Encoder(deblock=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder(deblock=1).encode(torch.zeros((2, 16, 16, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    mvt, info = torch.zeros((2, 2, 3, 2), dtype=torch.int16), torch.zeros((2, 2, 3), dtype=torch.int32)
    ok = dict(ry=u8(2, 32, 48), rcb=u8(2, 16, 24), rcr=u8(2, 16, 24), qp=28, gop=2, k=1, subpel=0, mbinfo=info, mv=mvt, waves=0)
    for key, val, word in (("ry", u8(2, 32, 40), "y must be"), ("rcb", u8(2, 16, 16), "cb must be"), ("qp", 52, "qp must be"), ("gop", 0, "gop must be"),
                           ("k", 2, "position k"), ("k", -1, "position k"), ("subpel", 3, "subpel must be"), ("waves", 17, "waves must be"),
                           ("waves", -1, "waves must be"), ("mbinfo", torch.zeros((2, 2, 4), dtype=torch.int32), "mbinfo must be"),
                           ("mbinfo", torch.zeros((2, 2, 3), dtype=torch.int64), "mbinfo must be"), ("mv", torch.zeros((2, 2, 3, 2)), "mv must be"),
                           ("mv", mvt, "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_deblock(*dict(ok, **{key: val}).values())
    sb = hip.h264_gop_scratch_bytes(2, 2, 3)
    step = dict(y=u8(2, 32, 48), cb=u8(2, 16, 24), cr=u8(2, 16, 24), qp=16, gop=2, k=1, search=2, first_index=0, mv=mvt, ry=u8(2, 32, 48),
                rcb=u8(2, 16, 24), rcr=u8(2, 16, 24), scratch=u8(sb), mbinfo=info)
    for key, val, word in (("mbinfo", torch.zeros((2, 3, 3), dtype=torch.int32), "mbinfo must be"), ("mbinfo", u8(2, 2, 3), "mbinfo must be"),
                           ("qp", 52, "h264_encode_gop_step_lf: qp"), ("scratch", u8(sb - 1), "scratch holds"), ("mbinfo", info, "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_encode_gop_step_lf(*dict(step, **{key: val}).values())
    sub = {k: v for k, v in list(step.items())[:7]} | dict(subpel=4) | {k: v for k, v in list(step.items())[7:]}
    with pytest.raises(hip.SdvHipError, match="mbinfo must be"):
        torch.ops.sdv.k_h264_encode_gop_step_sub_lf(*dict(sub, mbinfo=u8(12)).values())
    idr = {k: v for k, v in step.items() if k not in ("k", "search", "mv")}
    with pytest.raises(hip.SdvHipError, match="mbinfo must be"):
        torch.ops.sdv.k_h264_encode_idr4_lf(*dict(idr, mbinfo=torch.zeros((2, 2, 3), dtype=torch.int16)).values())
    lib = hip.load()
    # ry rcb rcr | n mbh mbw qp gop k subpel | mbinfo count mv | waves stream
    ok = [64, 80, 96, 2, 3, 4, 28, 2, 1, 0, 128, 24, 256, 0, None]
    for pos, val, word in ((0, None, b"null"), (2, None, b"null"), (10, None, b"null"), (12, None, b"null"), (3, 0, b"mbinfo holds"), (4, 0, b"mbinfo holds"),
                           (11, 23, b"mbinfo holds"), (11, 25, b"mbinfo holds"), (6, 52, b"qp="), (6, -1, b"qp="), (7, 0, b"gop="), (7, 257, b"gop="),
                           (8, 2, b"position k"), (8, -1, b"position k"), (9, 3, b"subpel="), (9, -1, b"subpel="), (13, 17, b"waves="), (13, -1, b"waves="),
                           (0, 72, b"aligned"), (1, 84, b"aligned"), (10, 130, b"aligned"), (12, 258, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_deblock(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_deblock")
    sb = hip.h264_gop_scratch_bytes(2, 3, 4)
    # y cb cr | n mbh mbw qp gop k search first | mv ry rcb rcr scratch | bytes | mbinfo count | stream
    ok = [16, 32, 48, 2, 3, 4, 16, 2, 1, 2, 0, 256, 64, 80, 96, 128, sb, 512, 24, None]
    for pos, val, word in ((17, None, b"null"), (17, 514, b"aligned"), (18, 23, b"mbinfo holds"), (6, 52, b"qp="), (16, sb - 1, b"scratch buffer too small")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_gop_step_lf(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    a = ok[:10] + [4] + ok[10:]                                                     # ... search subpel first ...
    a[18] = None
    assert lib.sdv_h264_encode_gop_step_sub_lf(*a) == -1 and b"sdv_h264_encode_gop_step_sub_lf: null" in lib.sdv_last_error()
    a = ok[:8] + [0] + ok[12:]                                                      # y cb cr | n mbh mbw qp gop first | ry rcb rcr scratch | bytes | mbinfo count
    a[15] = 25
    assert lib.sdv_h264_encode_idr4_lf(*a) == -1 and b"sdv_h264_encode_idr4_lf: mbinfo holds" in lib.sdv_last_error()


def test_pipeline_attribute_and_sdv_h264_deblock(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_DEBLOCK", raising=False)
    assert pipe.h264_deblock == 0 and pipe.h264_deblock_choice() == 0
    pipe.h264_deblock = 1
    assert pipe.h264_deblock_choice() == 1
    monkeypatch.setenv("SDV_H264_DEBLOCK", "0")                                     # the variable wins when it is set
    assert pipe.h264_deblock_choice() == 0
    monkeypatch.setenv("SDV_H264_DEBLOCK", "")
    assert pipe.h264_deblock_choice() == 1
    for bad in ("2", "-1", "one", " 1", "1.0", "true"):
        monkeypatch.setenv("SDV_H264_DEBLOCK", bad)
        with pytest.raises(ValueError, match="SDV_H264_DEBLOCK"):
            pipe.h264_deblock_choice()
    monkeypatch.delenv("SDV_H264_DEBLOCK")
    for bad in (2, True, "1"):
        pipe.h264_deblock = bad
        with pytest.raises(ValueError, match="h264_deblock"):
            pipe.h264_deblock_choice()


def test_make_video_pyav_checks_deblock_and_falls_back_without_a_gpu(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import utils, video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = torch.from_numpy(R.make_frames("ramp", 3, 20, 36))
    for bad in (2, -1, "1", 1.0, True):
        with pytest.raises(ValueError, match="one of the integers 0, 1"):
            video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "x.mp4", codec="h264-cavlc", h264_deblock=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=4, h264_deblock=1)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"] and "deblock" not in video.LAST_CODEC
    b = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "b.mp4")
    c = utils.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "c.mp4", h264_gop=4, h264_deblock=1)   # ignored by the other codecs
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def test_host_build_of_the_filter_pieces_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/sdv_h264_core.h's loop filter (side information word, bS, index, line filter, the raster-order picture walk) and the slice
    headers with the filter on, compiled for the host with -fsanitize=address,undefined into a stand-alone program
    (tests/h264_lf_host_main.cpp) and run as a subprocess on exact-size buffers: samples, filtered reconstruction, side information words
    and the three tables equal the restatement's on four cases, a one-row and a one-column picture among them."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "h264_lf_host"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "stable_diffusion_videos_amd" / "csrc"), str(ROOT / "tests" / "h264_lf_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    for shape, kind, qp, setting in (((3, 16, 64), "glyphs", 28, (3, 8, 4, 1)), ((3, 64, 16), "pan2", 40, (3, 8, 0, 0)), ((3, 36, 50), "mosaic_pcm", 16, (3, 0, 0, 1)),
                                     ((2, 96, 128), "noise", 51, (1, 0, 0, 0))):
        (y, cb, cr), samples, recon, used, infos = L.reference(shape, kind, qp, setting)
        gop, search, subpel, intra4 = setting
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        mv = used if subpel else used // 4
        (tmp_path / "in.bin").write_bytes(np.array([n, mbh, mbw, qp, gop, L.FIRST, search, subpel, intra4], dtype="<i4").tobytes() + y.tobytes() +
                                          cb.tobytes() + cr.tobytes() + mv.astype("<i2").tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        data, at, got = (tmp_path / "out.bin").read_bytes(), 0, []
        for _ in range(n):
            size = int.from_bytes(data[at:at + 4], "little")
            got.append(data[at + 4:at + 4 + size])
            at += 4 + size
        assert got == samples, (shape, kind, qp, setting)
        for want in recon:
            assert np.array_equal(np.frombuffer(data[at:at + want.size], dtype=np.uint8).reshape(want.shape), want), (shape, kind, qp, setting)
            at += want.size
        words = np.frombuffer(data[at:at + 4 * n * mbh * mbw], dtype="<u4").reshape(n, mbh, mbw)
        assert np.array_equal(words.astype(np.int64), L.mbinfo_words(infos).astype(np.int64)), (shape, kind, qp, setting)
        at += 4 * n * mbh * mbw
        tables = list(data[at:at + 260])
        assert tables[:52] == list(L.ALPHA) and tables[52:104] == list(L.BETA) and tables[104:] == [v for row in L.TC0 for v in row]
        assert at + 260 == len(data)
