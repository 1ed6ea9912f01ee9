"""Macroblock partitions of the H.264 track (include/sdv_hip_h264_part.h "H.264 partitions") without a GPU: the restatement of
tests/h264_part_ref.py against its separately written decoder (exact equality, no tolerance anywhere), coverage read from the decoder's
statistics, the search's decision rule, argument checks and plumbing, and the host build of csrc/sdv_h264_core.h's partition pieces under
AddressSanitizer / UBSan against the restatement.

The rule, restated: with part 1, gop > 1 and search > 0 every inter macroblock has four quarter-sample vectors, one per 8x8 quadrant; four
equal vectors are coded as before (P_Skip / P_L0_16x16), others as P_8x8 with four P_L0_8x8 sub types and four mvd pairs predicted by
8.4.1.3 (the row above is another slice); prediction per partition; the search takes the four quadrant winners iff
sum cost8 + 8 lambda < cost16; the loop filter compares vectors per partition.

One item of the coverage list, a refused vector in exactly one partition, cannot be seen by a decoder (a refused vector is coded as (0, 0),
which is a legal vector): it is read from the restatement's own statistics."""
import ctypes
import hashlib
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import h264_lf_ref as L
import h264_part_ref as Q
import h264_ref as R
import h264_sub_ref as S

ROOT = Path(__file__).resolve().parent.parent
SHA_DEFAULT = "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"
TOTAL = Q.new_part_stats()                       # what the decoder met over the whole case set (filled by the round trips)
ENC = dict(refused_one=0, p8x8=0)
COUNTED = set()


def _round_trip(shape, kind, injected, qp, subpel, filters):
    planes, samples, recon, used, infos, stats = Q.reference(shape, kind, qp, subpel, filters, injected=injected)
    st = Q.new_part_stats()
    out = Q.decode_stream(samples, shape[2], shape[1], stats=st)
    for name, want in zip(("y", "cb", "cr"), recon):
        assert np.array_equal(out[name], want), (shape, kind, injected, qp, subpel, filters, name)
    assert out["sync"] == [0] and all(h["deblock_idc"] == 1 - filters[1] for hs in out["headers"] for h in hs)
    assert st["p8x8"] == stats["p8x8"]
    key = (shape, kind, injected, qp, subpel, filters)
    if key not in COUNTED:
        COUNTED.add(key)
        for k, v in st.items():
            TOTAL[k] = TOTAL[k] | v if isinstance(v, set) else TOTAL[k] + v
        ENC["refused_one"] += stats["refused_one"]
        ENC["p8x8"] += stats["p8x8"]
    return out, st, stats


def used_any(*case):
    """Whether any coded vector of the case is not (0, 0)."""
    return bool(Q.reference(*case[:2], *case[3:], injected=case[2])[3].any())


@pytest.mark.parametrize("shape,kind,injected", Q.CASES, ids=Q.IDS)
def test_round_trip(shape, kind, injected):
    for qp in Q.QPS:
        for subpel in Q.SUBPELS:
            for filters in Q.FILTERS:
                out, st, stats = _round_trip(shape, kind, injected, qp, subpel, filters)
                if shape[1:] == (16, 16):
                    assert st["p8x8"] == 0, "a one-macroblock picture admits only (0, 0)"
                if kind == "still":
                    assert st["p8x8"] == 0 and not used_any(shape, kind, injected, qp, subpel, filters)


def test_coverage_of_the_case_set():
    """Read from the statistics the decoder gathered over the round trips above (it runs after them, in this file's order).  Run without
    them it first makes the round trips of a thinned case set that meets the list too."""
    for shape, kind, injected in Q.CASES:
        if shape in ((4, 48, 64), (3, 36, 50), (3, 16, 64)) and kind != "still":
            for qp, subpel, filters in ((0, 4, (0, 0)), (28, 4, (1, 1)), (28, 0, (1, 1)), (40, 2, (1, 1))):
                if (shape, kind, injected, qp, subpel, filters) not in COUNTED:
                    _round_trip(shape, kind, injected, qp, subpel, filters)
    assert TOTAL["p8x8_cbp0"] > 0 and TOTAL["p8x8_cbp"] > 0
    assert TOTAL["p8x8_first"] > 0
    assert TOTAL["p8x8_after"] >= {"p8x8", "l16", "skip", "intra", "pcm", None}, TOTAL["p8x8_after"]
    assert TOTAL["l16_after_split"] > 0
    assert TOTAL["part2_a"] == {"absent", "intra", "inter"}
    assert TOTAL["part3_mixed"] > 0, "no partition-3 median that is none of its inputs"
    assert ENC["refused_one"] > 0
    assert TOTAL["lf_inner8"] == {0, 1}
    assert TOTAL["lf_half"] > 0, "no macroblock edge with bS 1 on one half and 0 on the other"
    assert TOTAL["lf_inner8_bs2"] > 0
    assert TOTAL["kinds"] >= {"p8x8", "l16", "skip", "intra", "pcm"}


# ------------------------------------------------------------------------------------------------------------------------------------
# the decision rule
# ------------------------------------------------------------------------------------------------------------------------------------
def _two_motions(n, h, w, top, bottom, subpel):
    """Planted content whose upper partitions move by ``top`` and whose lower ones by ``bottom`` in every macroblock that admits both."""
    mbh, mbw = (h + 15) // 16, (w + 15) // 16
    mv = np.zeros((n, mbh, mbw, 4, 2), dtype=np.int16)
    mv[1:, :, :, :2], mv[1:, :, :, 2:] = top, bottom
    return mv, Q.plant(n, h, w, mv, Q.SEARCH, subpel, fresh=lambda k, r, m: False)


def test_two_planted_motions_inside_a_macroblock_are_found_at_every_subpel_that_can_represent_them():
    for top, bottom, subpels in (((8, 0), (-8, 8), (0, 1, 2, 4)), ((4, 0), (0, -4), (1, 2, 4)), ((2, 0), (-6, 2), (2, 4)), ((3, 1), (-1, 2), (4,))):
        for subpel in subpels:
            mv, planes = _two_motions(3, 64, 80, top, bottom, subpel)
            got, sad, taken = Q.search_planes(planes[0], 16, 3, Q.SEARCH, subpel)
            inner = (slice(1, None), slice(1, 3), slice(1, 4))                      # macroblocks that admit both vectors
            assert taken[inner].all(), (top, bottom, subpel)
            assert np.array_equal(got[inner], mv[inner]), (top, bottom, subpel)
            assert (sad[inner][..., :4] == 0).all() and (sad[inner][..., 4] > 0).all()
            samples = Q.encode_planes(*planes, qp=16, gop=3, first_index=0, search=Q.SEARCH, subpel=subpel)[0]
            assert Q.decode_stream(samples, 80, 64)["part"]["p8x8"] >= 12


def test_still_flat_uniform_pan_and_one_macroblock_pictures_yield_four_equal_vectors():
    pan = np.zeros((3, 4, 5, 4, 2), dtype=np.int16)
    pan[1:] = (8, -8)
    cases = [Q.make_planes("still", 3, 64, 80)[0], Q.make_planes("flat", 3, 64, 80)[0], Q.plant(3, 64, 80, pan, Q.SEARCH, 4, fresh=lambda k, r, m: False)[0],
             Q.make_planes("split8", 3, 16, 16)[0], Q.make_planes("noise", 3, 16, 16)[0]]
    for i, y in enumerate(cases):
        for subpel in Q.SUBPELS:
            for qp in (0, 28, 51):
                mv, _, taken = Q.search_planes(y, qp, 3, Q.SEARCH, subpel)
                assert (mv == mv[:, :, :, :1]).all(), (i, subpel, qp)
                if i != 2:
                    assert not mv.any()
    mv = Q.search_planes(cases[2], 16, 3, Q.SEARCH, 4)[0]
    assert (mv[1:, 1:3, 1:4] == (8, -8)).all()


def test_at_the_threshold_equality_keeps_16x16(tmp_path):
    """sum cost8 + 8 lambda == cost16 keeps w16; one less takes the quadrants - in the restatement's rule and in the host build."""
    lam = 4
    rows = []
    for delta in (0, 1, -1, 100):
        q = [(10, 4, 0), (12, -4, 8), (9, 0, 0), (11, 4, 4)]
        c16 = sum(c for c, _, _ in q) + 8 * lam + delta
        rows.append([lam] + [v for t in q for v in t] + [c16, 8, -8])
    want = [[int(r[13] > sum(r[1:13:3]) + 8 * lam)] for r in rows]
    assert [w[0] for w in want] == [0, 1, 0, 1]
    exe = _host_program(tmp_path)
    hd = np.array([1, 1, 1, 28, 1, 0, 8, 4, 0, 0, len(rows)], dtype="<i4")
    (tmp_path / "in.bin").write_bytes(hd.tobytes() + bytes(256 + 128) + bytes(16) + np.array(rows, dtype="<i4").tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res = np.frombuffer((tmp_path / "out.bin").read_bytes()[-36 * len(rows):], dtype="<i4").reshape(len(rows), 9)
    for row, got in zip(rows, res):
        take = row[13] > sum(row[1:13:3]) + 8 * lam
        assert got[0] == int(take)
        assert list(got[1:]) == ([v for i in range(4) for v in row[2 + 3 * i:4 + 3 * i]] if take else [8, -8] * 4)


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
        out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", h264_part=value)
        assert hashlib.sha256(open(out, "rb").read()).hexdigest() == SHA_DEFAULT
        assert "part" not in video.LAST_CODEC


def test_part_1_without_p_pictures_or_without_a_search_is_part_0():
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    planes = L.make_planes("glyphs", 3, 36, 50)
    for gop, search, subpel, intra4, deblock in ((1, 8, 4, 0, 0), (3, 0, 0, 0, 1), (1, 0, 0, 1, 1)):
        a = Q.encode_planes(*planes, qp=28, gop=gop, first_index=3, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=1)
        b = L.encode_planes(*planes, qp=28, gop=gop, first_index=3, search=search, subpel=subpel, intra4=intra4, deblock=deblock)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))
        enc = H264Encoder(28, None, gop=gop, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=1)
        assert enc.part == 1 and not enc._parted                                     # the encoder then runs today's route
    assert H264Encoder(28, None, gop=3, search=8, part=1)._parted and not H264Encoder(28, None, gop=3, search=8)._parted
    c = Q.encode_planes(*planes, qp=28, gop=3, first_index=3, search=8, subpel=4, part=0)
    d = S.encode_planes(*planes, qp=28, gop=3, first_index=3, search=8, subpel=4)
    assert c[0] == d[0]


PART_OPS = {"sdv_h264_motion_search_part": "k_h264_motion_search_part", "sdv_h264_encode_gop_step_part": "k_h264_encode_gop_step_part",
            "sdv_h264_encode_gop_step_part_lf": "k_h264_encode_gop_step_part_lf", "sdv_h264_deblock_part": "k_h264_deblock_part"}


def test_part_header_library_and_binding_agree(hip):
    header = (ROOT / "include" / "sdv_hip_h264_part.h").read_text()
    declared = set(re.findall(r"\bint (sdv_[a-z0-9_]+)\s*\(", header))
    assert declared == set(hip.H264_PART_SYMBOLS) == set(PART_OPS)
    assert not set(hip.H264_PART_SYMBOLS) & (set(hip.EXPORTED_SYMBOLS) | set(hip.EXTENSION_SYMBOLS) | set(hip.H264_SUB_SYMBOLS) | set(hip.H264_I4_SYMBOLS) |
                                             set(hip.H264_LF_SYMBOLS))
    others = [(ROOT / "include" / f).read_text() for f in ("sdv_hip.h", "sdv_hip_ext.h", "sdv_hip_h264_sub.h", "sdv_hip_h264_i4.h", "sdv_hip_h264_lf.h")]
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in PART_OPS.items():
        assert hasattr(lib, name) and not any(name in text for text in others)
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._H264_PART_SIGNATURES[name][1]), name
        assert getattr(hip.load(), name).argtypes == hip._H264_PART_SIGNATURES[name][1]
    text = " ".join(header.replace("*", " ").split())
    for phrase in ("H.264 partitions", "mb_type ue(3)", "sub_mb_type ue(0)", "8.4.1.3", "median(v2, v1, v0)", "sum_q cost8_q + 8 lambda(qp) < cost16(w16)",
                   "bits 19 .. 22", "int16 [n][mbh][mbw][4][2]", "600 (mbw + 1 + mbw / 64) + 17", "P_8x8ref0 are never written", "A setting, not a measured optimum",
                   "no third-party decoder"):
        assert phrase in text, phrase
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="meta")                # the Meta kernels accept the schemas and do nothing
    i16, i32 = torch.zeros((2, 2, 3, 4, 2), dtype=torch.int16, device="meta"), torch.zeros((2, 2, 3), dtype=torch.int32, device="meta")
    planes = (u8(2, 32, 48), u8(2, 16, 24), u8(2, 16, 24))
    torch.ops.sdv.k_h264_motion_search_part(planes[0], 28, 2, 8, 0, i16, None)
    torch.ops.sdv.k_h264_deblock_part(*planes, 28, 2, 0, i32, i16, 0)
    torch.ops.sdv.k_h264_encode_gop_step_part(*planes, 16, 2, 1, 2, 4, 0, i16, *planes, u8(64))
    torch.ops.sdv.k_h264_encode_gop_step_part_lf(*planes, 16, 2, 1, 2, 0, 0, i16, *planes, u8(64), i32)


def test_argument_checks_at_both_layers(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, check_part, encoder_for
    assert H264Encoder().part == 0 and H264Encoder(gop=4, search=8, subpel=4, intra4=1, deblock=1, part=1).part == 1
    assert [check_part(v) for v in (0, 1)] == [0, 1]
    assert encoder_for(21, "cuda:0", 4, 8, 4, 1, 1) is encoder_for(21, "cuda:0", 4, 8, 4, 1, 1, 0) is encoder_for(21, "cuda:0", 4, 8, 4, 1, 1, part=0)
    assert encoder_for(21, "cuda:0", 4, 8, 4, 1, 1, 1) is not encoder_for(21, "cuda:0", 4, 8, 4, 1, 1)
    for bad in (2, -1, True, False, "1", 1.0, None):
        with pytest.raises(ValueError, match="h264 part must be one of the integers 0, 1"):
            check_part(bad)
        with pytest.raises(ValueError, match="one of the integers 0, 1"):
            H264Encoder(part=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder(gop=2, search=8, part=1).encode(torch.zeros((2, 16, 16, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    mvt, info = torch.zeros((2, 2, 3, 4, 2), dtype=torch.int16), torch.zeros((2, 2, 3), dtype=torch.int32)
    ok = dict(y=u8(2, 32, 48), qp=28, gop=2, search=8, subpel=0, mv=mvt, sad=None)
    for key, val, word in (("y", u8(2, 32, 40), "y must be"), ("qp", 52, "qp must be"), ("gop", 0, "gop must be"), ("search", 7, "search must be"),
                           ("search", 0, "search must be"), ("search", 18, "search must be"), ("subpel", 3, "subpel must be 0, 1, 2 or 4"),
                           ("subpel", -1, "subpel must be"), ("mv", torch.zeros((2, 2, 3, 2), dtype=torch.int16), "mv must be"),
                           ("mv", torch.zeros((2, 2, 3, 4, 2), dtype=torch.int32), "mv must be"), ("sad", torch.zeros((2, 2, 3), dtype=torch.int32), "sad must be"),
                           ("mv", mvt, "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_motion_search_part(*dict(ok, **{key: val}).values())
    sb = hip.h264_gop_scratch_bytes(2, 2, 3)
    step = dict(y=u8(2, 32, 48), cb=u8(2, 16, 24), cr=u8(2, 16, 24), qp=16, gop=2, k=1, search=2, subpel=0, first_index=0, mv=mvt, ry=u8(2, 32, 48),
                rcb=u8(2, 16, 24), rcr=u8(2, 16, 24), scratch=u8(sb))
    for key, val, word in (("mv", torch.zeros((2, 2, 3, 2), dtype=torch.int16), "mv must be"), ("qp", 52, "h264_encode_gop_step_part: qp"), ("k", 2, "position k"),
                           ("search", 3, "search must be"), ("subpel", 8, "subpel must be"), ("scratch", u8(sb - 1), "scratch holds"), ("ry", u8(2, 32, 32), "ry must be"),
                           ("mv", mvt, "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_encode_gop_step_part(*dict(step, **{key: val}).values())
    for key, val, word in (("mbinfo", torch.zeros((2, 3, 3), dtype=torch.int32), "mbinfo must be"), ("mbinfo", u8(2, 2, 3), "mbinfo must be"),
                           ("qp", -1, "h264_encode_gop_step_part_lf: qp")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_encode_gop_step_part_lf(*dict(dict(step, mbinfo=info), **{key: val}).values())
    dbl = dict(ry=u8(2, 32, 48), rcb=u8(2, 16, 24), rcr=u8(2, 16, 24), qp=28, gop=2, k=1, mbinfo=info, mv=mvt, waves=0)
    for key, val, word in (("rcb", u8(2, 16, 16), "cb must be"), ("k", 2, "position k"), ("waves", 17, "waves must be"), ("mbinfo", info[:1], "mbinfo must be"),
                           ("mv", mvt[..., :1].contiguous(), "mv must be"), ("mv", mvt, "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            torch.ops.sdv.k_h264_deblock_part(*dict(dbl, **{key: val}).values())
    lib = hip.load()
    # y | n mbh mbw qp gop search subpel | mv count sad count | stream
    ok = [16, 2, 3, 4, 28, 2, 8, 4, 256, 192, 512, 120, None]
    for pos, val, word in ((0, None, b"null"), (8, None, b"null"), (8, 258, b"aligned"), (0, 24, b"aligned"), (10, 514, b"aligned"), (9, 191, b"mv holds"),
                           (9, 48, b"mv holds"), (11, 24, b"sad holds"), (1, 0, b"mv holds"), (4, 52, b"qp="), (5, 0, b"gop="), (6, 7, b"search="), (6, 0, b"search="),
                           (6, 18, b"search="), (7, 3, b"subpel="), (7, -1, b"subpel="), (7, 8, b"subpel=")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_motion_search_part(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_motion_search_part")
    sb = hip.h264_gop_scratch_bytes(2, 3, 4)
    # y cb cr | n mbh mbw qp gop k search subpel first | mv count | ry rcb rcr scratch | bytes | (mbinfo count) | stream
    ok = [16, 32, 48, 2, 3, 4, 16, 2, 1, 2, 0, 0, 256, 192, 64, 80, 96, 128, sb]
    for pos, val, word in ((12, None, b"null"), (12, 258, b"aligned"), (13, 48, b"mv holds"), (6, 52, b"qp="), (8, 2, b"position k"), (9, 5, b"search="),
                           (10, 3, b"subpel="), (18, sb - 1, b"scratch buffer too small"), (14, 72, b"aligned"), (0, None, b"null")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_gop_step_part(*a, None) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_h264_encode_gop_step_part_lf(*a, 512, 24, None) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
    assert lib.sdv_h264_encode_gop_step_part_lf(*ok, None, 24, None) == -1 and b"sdv_h264_encode_gop_step_part_lf: null" in lib.sdv_last_error()
    assert lib.sdv_h264_encode_gop_step_part_lf(*ok, 512, 23, None) == -1 and b"mbinfo holds" in lib.sdv_last_error()
    assert lib.sdv_h264_encode_gop_step_part_lf(*ok, 514, 24, None) == -1 and b"aligned" in lib.sdv_last_error()
    # ry rcb rcr | n mbh mbw qp gop k | mbinfo count mv count | waves stream
    ok = [64, 80, 96, 2, 3, 4, 28, 2, 1, 128, 24, 256, 192, 0, None]
    for pos, val, word in ((0, None, b"null"), (9, None, b"null"), (11, None, b"null"), (10, 23, b"mbinfo holds"), (12, 48, b"mv holds"), (12, 193, b"mv holds"),
                           (6, 52, b"qp="), (7, 257, b"gop="), (8, 2, b"position k"), (13, 17, b"waves="), (13, -1, b"waves="), (0, 72, b"aligned"),
                           (9, 130, b"aligned"), (11, 258, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_deblock_part(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_deblock_part")


def test_pipeline_attribute_and_sdv_h264_part(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_PART", raising=False)
    assert pipe.h264_part == 0 and pipe.h264_part_choice() == 0
    pipe.h264_part = 1
    assert pipe.h264_part_choice() == 1
    monkeypatch.setenv("SDV_H264_PART", "0")                                        # the variable wins when it is set
    assert pipe.h264_part_choice() == 0
    monkeypatch.setenv("SDV_H264_PART", "")
    assert pipe.h264_part_choice() == 1
    for bad in ("2", "-1", "one", " 1", "1.0", "true"):
        monkeypatch.setenv("SDV_H264_PART", bad)
        with pytest.raises(ValueError, match="SDV_H264_PART"):
            pipe.h264_part_choice()
    monkeypatch.delenv("SDV_H264_PART")
    for bad in (2, True, "1"):
        pipe.h264_part = bad
        with pytest.raises(ValueError, match="h264_part"):
            pipe.h264_part_choice()


def test_make_video_pyav_checks_part_and_falls_back_without_a_gpu(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import utils, video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = torch.from_numpy(R.make_frames("ramp", 3, 20, 36))
    for bad in (2, -1, "1", 1.0, True):
        with pytest.raises(ValueError, match="h264 part must be one of the integers 0, 1"):
            video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "x.mp4", codec="h264-cavlc", h264_part=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=4, h264_search=8, h264_part=1)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"] and "part" not in video.LAST_CODEC
    b = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "b.mp4")
    c = utils.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "c.mp4", h264_gop=4, h264_search=8, h264_part=1)   # ignored by the other codecs
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def _host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "h264_part_host"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "stable_diffusion_videos_amd" / "csrc"), str(ROOT / "tests" / "h264_part_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    return exe


def test_host_build_of_the_partition_pieces_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/sdv_h264_core.h's partition pieces (admission and fetch, per-partition windows and prediction, vector prediction, the P_8x8
    writer, the side information word, bS with four vectors) compiled for the host with -fsanitize=address,undefined into a stand-alone
    program (tests/h264_part_host_main.cpp) and run as a subprocess on exact-size buffers: bytes, reconstruction, vectors and side
    information equal the restatement's on six cases, the one-row and one-column pictures and injected refused vectors among them."""
    exe = _host_program(tmp_path)
    for shape, kind, injected, qp, subpel, filters in (((3, 16, 64), "split8", None, 28, 4, (1, 1)), ((3, 64, 16), "planted", "invalid", 16, 2, (0, 1)),
                                                       ((3, 36, 50), "planted", "mixed", 0, 0, (0, 0)), ((4, 48, 64), "planted", "far", 40, 1, (1, 1)),
                                                       ((3, 36, 50), "noise", None, 28, 4, (0, 1)), ((3, 16, 16), "split8", None, 51, 4, (1, 1))):
        (y, cb, cr), samples, recon, used, infos, _ = Q.reference(shape, kind, qp, subpel, filters, injected=injected)
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        mv = used if injected is None else Q.inject(injected, n, mbh, mbw, Q.SEARCH, subpel)       # the program validates the vectors itself
        hd = np.array([n, mbh, mbw, qp, n, Q.FIRST, Q.SEARCH, subpel, filters[0], filters[1], 0], dtype="<i4")
        (tmp_path / "in.bin").write_bytes(hd.tobytes() + y.tobytes() + cb.tobytes() + cr.tobytes() + mv.astype("<i2").tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        data, at, got = (tmp_path / "out.bin").read_bytes(), 0, []
        for _ in range(n):
            size = int.from_bytes(data[at:at + 4], "little")
            got.append(data[at + 4:at + 4 + size])
            at += 4 + size
        assert got == samples, (shape, kind, injected, qp, subpel, filters)
        for want in recon:
            assert np.array_equal(np.frombuffer(data[at:at + want.size], dtype=np.uint8).reshape(want.shape), want), (shape, kind, injected)
            at += want.size
        words = np.frombuffer(data[at:at + 4 * n * mbh * mbw], dtype="<u4").reshape(n, mbh, mbw)
        if filters[1]:
            assert np.array_equal(words.astype(np.int64), Q.mbinfo_words(infos).astype(np.int64)), (shape, kind, injected)
        assert at + 4 * n * mbh * mbw == len(data)
