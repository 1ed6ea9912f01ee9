"""Several slices per macroblock row of the H.264 track (include/sdv_hip_h264_seg.h "H.264 row slices") without a GPU: the restatement of
tests/h264_seg_ref.py against its separately written decoder (exact equality, no tolerance anywhere), coverage read from the decoder's
statistics, geometry and capacity in numbers, argument checks and plumbing, and the host build of csrc/sdv_h264_core.h's row-slice pieces
under AddressSanitizer / UBSan against the restatement.

The rule, restated: row_slices S (1 .. 16, with every other setting) writes segs = max(1, min(S, mbw, 1024 // mbh)) slices per macroblock
row; slice s covers macroblocks s * mbw // segs .. (s + 1) * mbw // segs - 1 and carries first_mb_in_slice = r * mbw + m0; the slices stand
in the sample in that order.  A slice start is a row start (no neighbour A: 128 / nC 0 / mvp (0, 0) / mb_skip_run from zero / no left
samples in I_NxN); vectors, the loop filter and the search do not stop there.  A slice of at most W = ceil(mbw / segs) macroblocks lies in a
slot of 600 (W + 1 + W // 64) + 17 bytes, slot index (f * mbh + r) * segs + s."""
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
import h264_me_ref as M
import h264_part_ref as PT
import h264_ref as R
import h264_seg_ref as G
import h264_sub_ref as S

ROOT = Path(__file__).resolve().parent.parent
SHA_DEFAULT = "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"     # the parent commit's default file (test_h264_part_cpu.py)
TOTAL = G.new_seg_stats()                        # what the decoder met over the whole case set (filled by the round trips)
COUNTED = set()


CASES, IDS = G.CASES, G.IDS


def _round_trip(shape, kind, setting, qp, row_slices, injected):
    planes, samples, recon, used, infos, segs, stats = G.reference(shape, kind, qp, setting, row_slices, injected)
    n, h, w = shape
    mbh, mbw = (h + 15) // 16, (w + 15) // 16
    assert segs == max(1, min(row_slices, mbw, 1024 // mbh))
    st = G.new_seg_stats()
    out = G.decode_stream(samples, w, h, stats=st)
    for name, want in zip(("y", "cb", "cr"), recon):
        assert np.array_equal(out[name], want), (shape, kind, setting, qp, row_slices, injected, name)
    gop, deblock = setting[1], setting[5]
    assert out["sync"] == list(range(0, n, gop))
    want_first = [r * mbw + s * mbw // segs for r in range(mbh) for s in range(segs)]       # the rule, restated here
    for hs in out["headers"]:                                                               # per picture: mbh * segs slices, exactly these
        assert [h_["first_mb"] for h_ in hs] == want_first == G.first_mbs(mbh, mbw, segs)
        assert all(h_["deblock_idc"] == 1 - deblock for h_ in hs)
    assert st["slices"] == n * mbh * segs
    assert st["widths"] == {m1 - m0 + 1 for m0, m1 in G.bounds(mbw, segs)}
    key = (shape, kind, setting, qp, row_slices, injected)
    if key not in COUNTED:
        COUNTED.add(key)
        for k, v in st.items():
            TOTAL[k] = TOTAL[k] | v if isinstance(v, set) else TOTAL[k] + v
    return out, st, stats


@pytest.mark.parametrize("shape,kind,setting,qp,row_slices,injected", CASES, ids=IDS)
def test_round_trip(shape, kind, setting, qp, row_slices, injected):
    out, st, stats = _round_trip(shape, kind, setting, qp, row_slices, injected)
    if shape[1:] == (16, 16):
        assert G.reference(shape, kind, qp, setting, row_slices, injected)[5] == 1          # a one-macroblock picture has one slice a row


def test_coverage_of_the_case_set():
    """Read from the statistics the decoder gathered over the round trips above (it runs after them, in this file's order).  Run without
    them it first makes the round trips of the whole case set."""
    for case in CASES:
        if case not in COUNTED:
            _round_trip(*case)
    t = TOTAL
    # a slice start whose left macroblock is inter (with a nonzero vector), intra, I_PCM or skipped ...
    assert t["start_left"] >= {"inter", "intra", "pcm", "skip"}, t["start_left"]
    assert t["start_left_nonzero_mv"] > 0
    # ... with the consequence in the bits: the decoder asserts mvp == (0, 0) at every slice start; here a start whose vector is not zero
    # beside a left macroblock whose vector is not zero (mvd carries the whole vector), Intra16x16 / I_NxN starts beside decoded samples
    assert t["start_mvd_is_v"] > 0 and t["start_intra16_dc128"] > 0
    assert t["p8x8_start"] > 0 and t["p8x8_start_part2_a"] == {"absent"}
    assert t["i4_start"] > 0 and t["i4_start_block0_dc"] == t["i4_start"] and t["i4_start_top_mode"] > 0
    assert t["only_run"] > 0 and t["begins_in_run"] > 0 and t["ends_in_run"] > 0 and t["begins_and_ends_in_run"] > 0
    assert t["pcm_first"] > 0 and t["pcm_last"] > 0
    assert t["boundary_bs"] == {0, 1, 2, 4}, t["boundary_bs"]
    assert t["start_kinds"] >= {"skip", "l16", "p8x8", "intra", "pcm"}
    assert 1 in t["widths"] and {2, 3} <= t["widths"]                                       # one-macroblock slices; unequal widths 2 + 3 (+ 3)
    assert [m1 - m0 + 1 for m0, m1 in G.bounds(5, 2)] == [2, 3] and [m1 - m0 + 1 for m0, m1 in G.bounds(8, 3)] == [2, 3, 3]
    assert G.bounds(3, 3) == [(0, 0), (1, 1), (2, 2)]


def test_the_decoder_refuses_slices_out_of_order_overlapping_or_missing():
    shape, setting = (4, 32, 48), G.SETTINGS[1]
    samples = G.reference(shape, "pan2", 28, setting, 3)[1]

    def nals(sample):
        out, at = [], 0
        while at < len(sample):
            size = int.from_bytes(sample[at:at + 4], "big")
            out.append(sample[at:at + 4 + size])
            at += 4 + size
        return out

    first = nals(samples[0])
    assert len(first) == 2 * 3
    G.decode_stream(samples[:1], 48, 32)
    for bad, word in ((first[:1] + [first[2], first[1]] + first[3:], "out of order"), (first[:2] + first[3:], "never coded"),
                      (first[:5], "never coded")):
        with pytest.raises(AssertionError, match=word):
            G.decode_stream([b"".join(bad)], 48, 32)
    wide = G.reference(shape, "pan2", 28, setting, 2)[1]                           # a slice of two macroblocks over a one-macroblock slice's ground
    mixed = first[:1] + nals(wide[0])[1:2] + first[2:]                             # macroblocks 1 .. 2, then a slice that starts at 2
    with pytest.raises(AssertionError, match="overlap"):
        G.decode_stream([b"".join(mixed)], 48, 32)


def test_row_slices_1_is_the_other_modules_stream():
    """The restatement's own loop in the four-vector layout at row_slices 1 (and at any S on a picture one macroblock wide): the bytes and
    planes of h264_part_ref, and with part 0 those of the one-vector modules."""
    planes = L.make_planes("glyphs", 3, 36, 50)
    moving = M.make_planes("pan2", 4, 32, 48)
    for gop, search, subpel, intra4, deblock in ((1, 0, 0, 0, 0), (1, 0, 0, 1, 1), (3, 0, 0, 0, 1), (3, 8, 0, 0, 0), (3, 8, 4, 1, 1), (3, 8, 2, 0, 1)):
        for src in (planes, moving):
            for part in (0, 1):
                a = G.encode_planes(*src, qp=28, gop=gop, first_index=3, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part, row_slices=1)
                b = PT.encode_planes(*src, qp=28, gop=gop, first_index=3, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part)
                assert a[6] == 1 and a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4])), (gop, search, subpel, intra4, deblock, part)
    c = G.encode_planes(*moving, qp=16, gop=4, first_index=3, search=8, subpel=4, row_slices=1)
    d = S.encode_planes(*moving, qp=16, gop=4, first_index=3, search=8, subpel=4)
    assert c[0] == d[0]
    e = G.encode_planes(*moving, qp=16, gop=4, first_index=3, search=8, row_slices=1)
    f = M.encode_planes(*moving, qp=16, gop=4, first_index=3, search=8)
    assert e[0] == f[0] and e[4].any()
    g = G.encode_planes(*moving, qp=16, gop=1, first_index=3, row_slices=1)
    assert g[0] == R.encode_planes(*moving, qp=16, first_index=3)[0]
    one = M.make_planes("noise", 3, 16, 16)
    assert G.encode_planes(*one, qp=28, gop=3, row_slices=4)[0] == G.encode_planes(*one, qp=28, gop=3, row_slices=1)[0]
    two = G.encode_planes(*moving, qp=16, gop=4, first_index=3, search=8, row_slices=2)
    assert two[0] != e[0] and [len(s) for s in two[0]] > [len(s) for s in e[0]]             # more slices, more bytes


def test_row_segments_table(hip):
    table = ((1, 1, 1, 1), (1, 1, 16, 1), (2, 3, 4, 3), (3, 5, 2, 2), (3, 8, 3, 3), (128, 128, 8, 8), (128, 128, 16, 8), (300, 20, 8, 3), (300, 20, 2, 2),
             (513, 40, 4, 1), (1024, 1008, 16, 1), (64, 1008, 16, 16), (65, 1008, 16, 15), (32, 2, 16, 2), (4, 7, 16, 7))
    for mbh, mbw, s, want in table:
        assert G.row_segments(mbh, mbw, s) == hip.h264_row_segments(mbh, mbw, s) == want == max(1, min(s, mbw, 1024 // mbh)), (mbh, mbw, s)
        segs = want
        b = G.bounds(mbw, segs)
        assert b[0][0] == 0 and b[-1][1] == mbw - 1 and all(b[i][1] + 1 == b[i + 1][0] for i in range(segs - 1))
        widths = [m1 - m0 + 1 for m0, m1 in b]
        assert min(widths) >= 1 and max(widths) - min(widths) <= 1 and max(widths) == -(-mbw // segs)
        assert mbh * segs <= 1024


def test_capacity_in_numbers(hip):
    """For every mbw 1 .. 1008 and segs 1 .. 16 (segs <= mbw): the slot of the widest slice is above the GOP path's bound for it, the
    layout is the intra layout at (n, mbh segs, w'), and first_mb_in_slice stays below 2^20."""
    for mbw in range(1, 1009):
        for segs in range(1, min(mbw, 16) + 1):
            wmax = -(-mbw // segs)
            slot_mbw = wmax + 1 + wmax // 64
            assert G.seg_slot_mbw(mbw, segs) == hip.h264_seg_slot_mbw(mbw, segs) == slot_mbw <= 1024
            slot = 600 * slot_mbw + 17
            assert 2 * slot >= 2 * 5 + 3 * (403 * wmax + 13) and slot >= G.slice_bound(wmax)         # 604.5 w + 25 (sdv_hip.h) and its integer form
            assert slot == hip.h264_slice_bytes(slot_mbw) == G.seg_slot_bytes(mbw, segs)
    assert 1024 * 1008 < 1 << 20
    for n, mbh, mbw, segs in ((1, 1, 1, 1), (3, 2, 3, 3), (5, 3, 5, 2), (8, 128, 128, 8), (2, 64, 1008, 16)):
        assert hip.h264_seg_scratch_bytes(n, mbh, mbw, segs) == G.seg_scratch_bytes(n, mbh, mbw, segs) == hip.h264_scratch_bytes(n, mbh * segs, hip.h264_seg_slot_mbw(mbw, segs))
        assert hip.h264_seg_out_bytes(n, mbh, mbw, segs) == G.seg_out_bytes(n, mbh, mbw, segs) == hip.h264_out_bytes(n, mbh * segs, hip.h264_seg_slot_mbw(mbw, segs))
    assert hip.h264_seg_scratch_bytes(2, 3, 5, 1) == hip.h264_gop_scratch_bytes(2, 3, 5) and hip.h264_seg_out_bytes(2, 3, 5, 1) == hip.h264_gop_out_bytes(2, 3, 5)
    assert (hip.h264_seg_slot_mbw(128, 8), hip.h264_seg_slot_mbw(5, 2), hip.h264_seg_slot_mbw(3, 3), hip.h264_seg_slot_mbw(1008, 16)) == (17, 4, 2, 64)


def test_default_files_are_the_parent_commits_bytes(tmp_path, monkeypatch):
    pytest.importorskip("PIL")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = R.make_frames("ramp", 3, 36, 50)
    out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "d.mp4")
    if video.LAST_CODEC["video"] == "h264 (libx264)":
        pytest.skip("torchvision / pyav present: the dependency-free writer is not in use")
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == SHA_DEFAULT
    for value in (1, 2, 16):                                                        # the default codec is not this track: no effect
        out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", h264_row_slices=value)
        assert hashlib.sha256(open(out, "rb").read()).hexdigest() == SHA_DEFAULT
        assert "row_slices" not in video.LAST_CODEC


SEG_OPS = {"sdv_h264_encode_gop_step_seg": "k_h264_encode_gop_step_seg", "sdv_h264_encode_gop_step_seg_lf": "k_h264_encode_gop_step_seg_lf",
           "sdv_h264_encode_idr4_seg": "k_h264_encode_idr4_seg", "sdv_h264_encode_idr4_seg_lf": "k_h264_encode_idr4_seg_lf"}


def test_seg_header_library_and_binding_agree(hip):
    header = (ROOT / "include" / "sdv_hip_h264_seg.h").read_text()
    declared = set(re.findall(r"\bint (sdv_[a-z0-9_]+)\s*\(", header))
    assert declared == set(hip.H264_SEG_SYMBOLS) == set(SEG_OPS)
    assert not set(hip.H264_SEG_SYMBOLS) & (set(hip.EXPORTED_SYMBOLS) | set(hip.EXTENSION_SYMBOLS) | set(hip.H264_SUB_SYMBOLS) | set(hip.H264_I4_SYMBOLS) |
                                            set(hip.H264_LF_SYMBOLS) | set(hip.H264_PART_SYMBOLS))
    others = [(ROOT / "include" / f).read_text() for f in ("sdv_hip.h", "sdv_hip_ext.h", "sdv_hip_h264_sub.h", "sdv_hip_h264_i4.h", "sdv_hip_h264_lf.h",
                                                           "sdv_hip_h264_part.h")]
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in SEG_OPS.items():
        assert hasattr(lib, name) and not any(name in text for text in others)
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._H264_SEG_SIGNATURES[name][1]), name
        assert getattr(hip.load(), name).argtypes == hip._H264_SEG_SIGNATURES[name][1]
        assert "int32_t segs, void* stream" in " ".join(decl[:decl.index(");")].split())
    text = " ".join(header.replace("*", " ").split())
    for phrase in ("H.264 row slices", "segs = max(1, min(S, mbw, 1024 / mbh))", "m0 = s mbw / segs", "first_mb_in_slice = r mbw + m0", "A slice start is a row start",
                   "What does not stop at a slice start", "(f mbh + r) segs + s", "600 w' + 17", "w' = W + 1 + W / 64", "no arbitrary slice order",
                   "int16 [n][mbh][mbw][4][2]", "A setting, not a measured optimum", "no third-party decoder", "segs outside 1 .. min(mbw, 16)", "mbh segs > 1024"):
        assert phrase in text, phrase
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="meta")                # the Meta kernels accept the schemas and do nothing
    i16, i32 = torch.zeros((2, 2, 3, 4, 2), dtype=torch.int16, device="meta"), torch.zeros((2, 2, 3), dtype=torch.int32, device="meta")
    planes = (u8(2, 32, 48), u8(2, 16, 24), u8(2, 16, 24))
    torch.ops.sdv.k_h264_encode_gop_step_seg(*planes, 16, 2, 1, 2, 4, 0, i16, *planes, u8(64), 2)
    torch.ops.sdv.k_h264_encode_gop_step_seg_lf(*planes, 16, 2, 1, 2, 0, 0, i16, *planes, u8(64), i32, 3)
    torch.ops.sdv.k_h264_encode_idr4_seg(*planes, 16, 2, 0, *planes, u8(64), 2)
    torch.ops.sdv.k_h264_encode_idr4_seg_lf(*planes, 16, 2, 0, *planes, u8(64), i32, 2)


def test_argument_checks_at_both_layers(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, check_row_slices, encoder_for
    assert H264Encoder().row_slices == 1 and H264Encoder(gop=1, row_slices=16).row_slices == 16
    assert H264Encoder(gop=4, search=8, subpel=4, intra4=1, deblock=1, part=1, row_slices=8).row_slices == 8       # valid with every other setting
    assert [check_row_slices(v) for v in (1, 2, 16)] == [1, 2, 16]
    assert encoder_for(22, "cuda:0", 4, 8, 4, 1, 1, 1) is encoder_for(22, "cuda:0", 4, 8, 4, 1, 1, 1, 1) is encoder_for(22, "cuda:0", 4, 8, 4, 1, 1, 1, row_slices=1)
    assert encoder_for(22, "cuda:0", 4, 8, 4, 1, 1, 1, 2) is not encoder_for(22, "cuda:0", 4, 8, 4, 1, 1, 1)
    for bad in (0, 17, -1, True, False, "2", 2.0, None):
        with pytest.raises(ValueError, match="h264 row_slices must be an integer in 1 .. 16"):
            check_row_slices(bad)
        with pytest.raises(ValueError, match="an integer in 1 .. 16"):
            H264Encoder(row_slices=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder(gop=1, row_slices=2).encode(torch.zeros((2, 16, 32, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    mvt, info = torch.zeros((2, 2, 3, 4, 2), dtype=torch.int16), torch.zeros((2, 2, 3), dtype=torch.int32)
    sb = hip.h264_seg_scratch_bytes(2, 2, 3, 3)
    assert sb > hip.h264_seg_scratch_bytes(2, 2, 3, 1) == hip.h264_gop_scratch_bytes(2, 2, 3)
    step = dict(y=u8(2, 32, 48), cb=u8(2, 16, 24), cr=u8(2, 16, 24), qp=16, gop=2, k=1, search=2, subpel=0, first_index=0, mv=mvt, ry=u8(2, 32, 48),
                rcb=u8(2, 16, 24), rcr=u8(2, 16, 24), scratch=u8(sb), segs=3)
    for key, val, word in (("mv", torch.zeros((2, 2, 3, 2), dtype=torch.int16), "mv must be"), ("qp", 52, "h264_encode_gop_step_seg: qp"), ("k", 2, "position k"),
                           ("search", 3, "search must be"), ("subpel", 8, "subpel must be"), ("scratch", u8(sb - 1), "scratch holds"), ("ry", u8(2, 32, 32), "ry must be"),
                           ("segs", 0, "segs must be 1 .. min"), ("segs", 4, "segs must be 1 .. min"), ("segs", 17, "segs must be"), ("mv", mvt, "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_encode_gop_step_seg(*dict(step, **{key: val}).values())
    lf = dict(step)
    segs = lf.pop("segs")
    for key, val, word in (("mbinfo", torch.zeros((2, 3, 3), dtype=torch.int32), "mbinfo must be"), ("qp", -1, "h264_encode_gop_step_seg_lf: qp"), ("segs", 4, "segs must be")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_encode_gop_step_seg_lf(*dict(dict(lf, mbinfo=info, segs=segs), **{key: val}).values())
    idr = dict(y=u8(2, 32, 48), cb=u8(2, 16, 24), cr=u8(2, 16, 24), qp=16, gop=2, first_index=0, ry=u8(2, 32, 48), rcb=u8(2, 16, 24), rcr=u8(2, 16, 24),
               scratch=u8(sb), segs=3)
    for key, val, word in (("qp", 52, "h264_encode_idr4_seg: qp"), ("gop", 0, "gop must be"), ("scratch", u8(sb - 1), "scratch holds"), ("segs", 4, "segs must be"),
                           ("segs", -1, "segs must be"), ("first_index", -1, "first_index"), ("y", u8(2, 32, 48), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_encode_idr4_seg(*dict(idr, **{key: val}).values())
    tall = dict(idr, y=u8(1, 16 * 600, 32), cb=u8(1, 8 * 600, 16), cr=u8(1, 8 * 600, 16), ry=u8(1, 16 * 600, 32), rcb=u8(1, 8 * 600, 16), rcr=u8(1, 8 * 600, 16), segs=2)
    with pytest.raises(hip.SdvHipError, match="slot rows"):
        torch.ops.sdv.k_h264_encode_idr4_seg(*tall.values())
    lib = hip.load()
    sb = hip.h264_seg_scratch_bytes(2, 3, 4, 4)
    # y cb cr | n mbh mbw qp gop k search subpel first | mv count | ry rcb rcr scratch | bytes | (mbinfo count) | segs stream
    ok = [16, 32, 48, 2, 3, 4, 16, 2, 1, 2, 0, 0, 256, 192, 64, 80, 96, 128, sb]
    for pos, val, segs, word in ((12, None, 4, b"null"), (12, 258, 4, b"aligned"), (13, 48, 4, b"mv holds"), (6, 52, 4, b"qp="), (8, 2, 4, b"position k"),
                                 (9, 5, 4, b"search="), (10, 3, 4, b"subpel="), (18, sb - 1, 4, b"scratch buffer too small"), (14, 72, 4, b"aligned"),
                                 (0, None, 4, b"null"), (18, sb, 0, b"segs=0 outside"), (18, sb, 5, b"segs=5 outside"), (18, sb, 17, b"segs=17 outside"),
                                 (18, sb, -1, b"segs=-1 outside"), (18, hip.h264_seg_scratch_bytes(2, 3, 4, 2), 4, b"scratch buffer too small")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_gop_step_seg(*a, segs, None) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_encode_gop_step_seg:")
        assert lib.sdv_h264_encode_gop_step_seg_lf(*a, 512, 24, segs, None) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    assert lib.sdv_h264_encode_gop_step_seg_lf(*ok, None, 24, 4, None) == -1 and b"sdv_h264_encode_gop_step_seg_lf: null" in lib.sdv_last_error()
    assert lib.sdv_h264_encode_gop_step_seg_lf(*ok, 512, 23, 4, None) == -1 and b"mbinfo holds" in lib.sdv_last_error()
    # y cb cr | n mbh mbw qp gop first | ry rcb rcr scratch | bytes | (mbinfo count) | segs stream
    ok = [16, 32, 48, 2, 3, 4, 16, 2, 0, 64, 80, 96, 128, sb]
    for pos, val, segs, word in ((0, None, 4, b"null"), (12, None, 4, b"null"), (6, 52, 4, b"qp="), (7, 0, 4, b"gop="), (8, -1, 4, b"first_index"),
                                 (13, sb - 1, 4, b"scratch buffer too small"), (9, 72, 4, b"aligned"), (13, sb, 5, b"segs=5 outside"), (13, sb, 0, b"segs=0 outside")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_idr4_seg(*a, segs, None) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_encode_idr4_seg:")
        assert lib.sdv_h264_encode_idr4_seg_lf(*a, 512, 24, segs, None) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    assert lib.sdv_h264_encode_idr4_seg_lf(*ok, 512, 25, 4, None) == -1 and b"mbinfo holds" in lib.sdv_last_error()
    tall = [16, 32, 48, 1, 600, 4, 16, 2, 0, 64, 80, 96, 128, 1 << 40]
    assert lib.sdv_h264_encode_idr4_seg(*tall, 2, None) == -1 and b"slot rows" in lib.sdv_last_error()


def test_pipeline_attribute_and_sdv_h264_row_slices(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_ROW_SLICES", raising=False)
    assert pipe.h264_row_slices == 1 and pipe.h264_row_slices_choice() == 1
    pipe.h264_row_slices = 4
    assert pipe.h264_row_slices_choice() == 4
    monkeypatch.setenv("SDV_H264_ROW_SLICES", "2")                                  # the variable wins when it is set
    assert pipe.h264_row_slices_choice() == 2
    monkeypatch.setenv("SDV_H264_ROW_SLICES", "16")
    assert pipe.h264_row_slices_choice() == 16
    monkeypatch.setenv("SDV_H264_ROW_SLICES", "")
    assert pipe.h264_row_slices_choice() == 4
    for bad in ("0", "17", "-1", "two", " 2", "2.0", "true"):
        monkeypatch.setenv("SDV_H264_ROW_SLICES", bad)
        with pytest.raises(ValueError, match="SDV_H264_ROW_SLICES"):
            pipe.h264_row_slices_choice()
    monkeypatch.delenv("SDV_H264_ROW_SLICES")
    for bad in (0, 17, True, "2"):
        pipe.h264_row_slices = bad
        with pytest.raises(ValueError, match="h264_row_slices"):
            pipe.h264_row_slices_choice()


def test_make_video_pyav_checks_row_slices_and_falls_back_without_a_gpu(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import utils, video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = torch.from_numpy(R.make_frames("ramp", 3, 20, 36))
    for bad in (0, 17, -1, "2", 2.0, True):
        with pytest.raises(ValueError, match="h264 row_slices must be an integer in 1 .. 16"):
            video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "x.mp4", codec="h264-cavlc", h264_row_slices=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=3, h264_row_slices=2)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"] and "row_slices" not in video.LAST_CODEC
    b = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "b.mp4")
    c = utils.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "c.mp4", h264_gop=3, h264_row_slices=2)    # ignored by the other codecs
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def _host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "h264_seg_host"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "stable_diffusion_videos_amd" / "csrc"), str(ROOT / "tests" / "h264_seg_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    return exe


def test_host_build_of_the_row_slice_pieces_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/sdv_h264_core.h's row-slice pieces (the slice count, bounds, slot index and layout) around the macroblock coders, compiled for the
    host with -fsanitize=address,undefined into a stand-alone program (tests/h264_seg_host_main.cpp) and run as a subprocess on exact-size
    buffers, walking every picture slice by slice: bytes, reconstruction and side information equal the restatement's on three cases."""
    exe = _host_program(tmp_path)
    for shape, kind, setting, qp, row_slices, injected in (((5, 40, 72), "split8", G.SETTINGS[4], 28, 2, None), ((4, 32, 48), "planted", G.SETTINGS[2], 16, 4, "invalid"),
                                                           ((3, 48, 128), "noise", G.SETTINGS[5], 0, 3, None)):
        (y, cb, cr), samples, recon, used, infos, segs, _ = G.reference(shape, kind, qp, setting, row_slices, injected)
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        _, gop, search, subpel, intra4, deblock, part = setting
        mv = used if injected is None else G.injected_case(shape, injected, search, subpel)[1]     # the program validates the vectors itself
        hd = np.array([n, mbh, mbw, qp, gop, G.FIRST, search or 2, subpel if search else 0, intra4, deblock, row_slices], dtype="<i4")
        (tmp_path / "in.bin").write_bytes(hd.tobytes() + y.tobytes() + cb.tobytes() + cr.tobytes() + mv.astype("<i2").tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        data, got = (tmp_path / "out.bin").read_bytes(), []
        assert int.from_bytes(data[:4], "little") == segs > 1
        at = 4
        for _ in range(n):
            size = int.from_bytes(data[at:at + 4], "little")
            got.append(data[at + 4:at + 4 + size])
            at += 4 + size
        assert got == samples, (shape, kind, injected, qp)
        for want in recon:
            assert np.array_equal(np.frombuffer(data[at:at + want.size], dtype=np.uint8).reshape(want.shape), want), (shape, kind, injected)
            at += want.size
        words = np.frombuffer(data[at:at + 4 * n * mbh * mbw], dtype="<u4").reshape(n, mbh, mbw)
        if deblock:
            assert np.array_equal(words.astype(np.int64), PT.mbinfo_words(infos).astype(np.int64)), (shape, kind, injected)
        assert at + 4 * n * mbh * mbw == len(data)
