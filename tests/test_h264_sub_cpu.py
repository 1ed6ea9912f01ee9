"""Sub-sample motion vectors of the H.264 GOP stream (include/sdv_hip_h264_sub.h "H.264 sub-sample motion") without a GPU: the
interpolator of tests/h264_sub_ref.py pinned on its own, the restatement against h264_p_ref.py's decoder with that interpolator installed,
coverage of injected vectors, agreement with the parent rule and between the grids, argument checks and plumbing, and the host build of
csrc/sdv_h264_core.h's sub-sample pieces under AddressSanitizer / UBSan against the restatement."""
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
import h264_sub_ref as S

ROOT = Path(__file__).resolve().parent.parent
SHA_DEFAULT = "9b4ce0583c2f522b297b0f87c5cc2682f8bee02589bf61215a6e4788d93746c0"
FRACTIONS = [(xf, yf) for yf in range(4) for xf in range(4)]
# injected-vector cases: (shape, qp, search, subpel, kind of h264_sub_ref.inject) on planes planted with those vectors
INJECTED = [((5, 32, 48, 5), 28, 2, 4, "fractions"), ((3, 36, 50, 3), 16, 8, 4, "fractions"), ((6, 96, 128, 6), 51, 8, 4, "fractions"),
            ((7, 64, 64, 3), 0, 16, 4, "extreme"), ((3, 36, 50, 3), 16, 2, 1, "extreme"), ((5, 32, 48, 5), 28, 8, 2, "random"),
            ((3, 36, 50, 3), 28, 8, 4, "edges"), ((5, 32, 48, 5), 16, 2, 2, "edges"), ((4, 16, 16, 4), 16, 16, 4, "fractions"),
            ((5, 32, 48, 5), 51, 16, 1, "invalid"), ((3, 36, 50, 3), 16, 8, 2, "invalid"), ((4, 16, 16, 4), 16, 16, 4, "invalid")]


# ------------------------------------------------------------------------------------------------------------------------------------
# the interpolator on its own
# ------------------------------------------------------------------------------------------------------------------------------------
def _luma(plane, xf, yf, x0=8, y0=8, size=4):
    return S.inter_pred(np.asarray(plane, dtype=np.int64), (xf, yf), x0, y0, size, 0)


def test_a_constant_plane_stays_constant_at_all_16_positions():
    for value in (0, 77, 255):
        plane = np.full((24, 24), value)
        for xf, yf in FRACTIONS:
            assert (_luma(plane, xf, yf) == value).all(), (value, xf, yf)
            assert (_luma(plane, xf - 4 * 9, yf + 4 * 30, size=16) == value).all()   # far outside: everything is clamped
        for xf in range(8):
            for yf in range(8):
                assert (S.inter_pred(plane, (xf, yf), 4, 4, 8, 1) == value).all()


def test_a_linear_ramp_gives_exact_halves_and_rounded_quarters():
    """The 6-tap filter reproduces a linear ramp at the half positions: 32 (g + 1/2 step).  With a step of 2 the half value is a whole
    number and every quarter position is the rounded average of its two neighbours."""
    ramp_x = np.tile(40 + 2 * np.arange(24), (24, 1))
    ramp_y = ramp_x.T
    plane = 20 + 2 * np.arange(24)[None, :] + 4 * np.arange(24)[:, None]           # both at once: G = 20 + 2 x + 4 y
    G = lambda p: p[8:12, 8:12]
    assert np.array_equal(_luma(ramp_x, 2, 0), G(ramp_x) + 1) and np.array_equal(_luma(ramp_y, 0, 2), G(ramp_y) + 1)
    assert np.array_equal(_luma(plane, 2, 0), G(plane) + 1) and np.array_equal(_luma(plane, 0, 2), G(plane) + 2)      # b, h
    assert np.array_equal(_luma(plane, 2, 2), G(plane) + 3)                                                             # j
    g = G(plane)
    b, h, j, m, s = g + 1, g + 2, g + 3, g + 2 + 2, g + 1 + 4
    avg = lambda p, q: (p + q + 1) >> 1
    want = {(1, 0): avg(g, b), (3, 0): avg(g + 2, b), (0, 1): avg(g, h), (0, 3): avg(g + 4, h), (1, 1): avg(b, h), (3, 1): avg(b, m),
            (1, 3): avg(h, s), (3, 3): avg(m, s), (2, 1): avg(b, j), (2, 3): avg(j, s), (1, 2): avg(h, j), (3, 2): avg(j, m)}
    for (xf, yf), w in want.items():
        assert np.array_equal(_luma(plane, xf, yf), w), (xf, yf)


def test_an_impulse_of_32_reproduces_the_taps():
    plane = np.zeros((24, 24), dtype=np.int64)
    plane[10, 10] = 32
    taps = [1, -5, 20, 20, -5, 1]
    row = S.inter_pred(plane, (2, 0), 0, 10, 24, 0)[0]                              # b between x and x + 1: the impulse is tap x + 3 - 10 ... reversed
    col = S.inter_pred(plane, (0, 2), 10, 0, 24, 0)[:, 0]
    want = np.zeros(24, dtype=np.int64)
    for t, c in enumerate(taps):                                                    # b at x reads x - 2 .. x + 3 with taps[0 .. 5]: x = 10 + 2 - t
        want[10 + 2 - t] = np.clip((32 * c + 16) >> 5, 0, 255)
    assert np.array_equal(row, want) and np.array_equal(col, want)
    assert want[8:13].tolist() == [0, 20, 20, 0, 1] and want[7] == 1                 # -5 clips to 0
    plane[:] = 100                                                                  # on a pedestal nothing clips
    plane[10, 10] = 132
    row = S.inter_pred(plane, (2, 0), 0, 10, 24, 0)[0]
    assert (row[7:13] - 100).tolist() == taps[::-1] and (np.delete(row, range(7, 13)) == 100).all()


def test_transpose_and_mirror_symmetries():
    rng = np.random.default_rng(5)
    plane = rng.integers(0, 256, (40, 40))
    for xf, yf in FRACTIONS:
        for ix, iy in ((0, 0), (-3, 2), (5, -20)):                                  # the last one clamps at the top
            a = S.inter_pred(plane, (4 * ix + xf, 4 * iy + yf), 12, 8, 16, 0)
            b = S.inter_pred(plane.T.copy(), (4 * iy + yf, 4 * ix + xf), 8, 12, 16, 0)
            assert np.array_equal(a, b.T), (xf, yf, ix, iy)
            # mirrored plane: sample x of the block at x0 with offset v is sample (w - 1 - x) with offset -v
            c = S.inter_pred(plane[:, ::-1].copy(), (-(4 * ix + xf), 4 * iy + yf), 40 - 12 - 16, 8, 16, 0)
            assert np.array_equal(a, c[:, ::-1]), (xf, yf, ix, iy)
    chroma = rng.integers(0, 256, (20, 20))
    for xf in range(8):
        for yf in range(8):
            a = S.inter_pred(chroma, (8 + xf, -8 + yf), 4, 4, 8, 1)
            assert np.array_equal(a, S.inter_pred(chroma.T.copy(), (-8 + yf, 8 + xf), 4, 4, 8, 1).T)
            assert np.array_equal(a, S.inter_pred(chroma[:, ::-1].copy(), (-(8 + xf), -8 + yf), 20 - 4 - 8, 4, 8, 1)[:, ::-1])


def test_fraction_0_equals_the_whole_sample_copy():
    rng = np.random.default_rng(6)
    plane = rng.integers(0, 256, (32, 48)).astype(np.int64)
    for vx, vy in ((0, 0), (8, -12), (-64, 64), (4, 0), (-20, 36)):
        for x0, y0 in ((0, 0), (32, 16), (16, 0)):
            assert np.array_equal(S.inter_pred(plane, (vx, vy), x0, y0, 16, 0), P._inter_pred(plane, (vx, vy), x0, y0, 16, 0))
            assert np.array_equal(S.inter_pred(plane[::2, ::2], (2 * vx, 2 * vy), x0 // 2, y0 // 2, 8, 1),
                                  P._inter_pred(plane[::2, ::2], (2 * vx, 2 * vy), x0 // 2, y0 // 2, 8, 1))


def test_chroma_bilinear_on_a_ramp_and_a_checker():
    ramp = 16 + 8 * np.arange(20)[None, :] + 8 * np.arange(20)[:, None]             # exact at every eighth: 8 / 8 = 1 per fraction step
    for xf in range(8):
        for yf in range(8):
            assert np.array_equal(S.inter_pred(ramp, (xf, yf), 4, 4, 8, 1), ramp[4:12, 4:12] + xf + yf)
    checker = np.array([[10, 250], [90, 30]])
    for xf in range(8):
        for yf in range(8):
            want = ((8 - xf) * (8 - yf) * 10 + xf * (8 - yf) * 250 + (8 - xf) * yf * 90 + xf * yf * 30 + 32) >> 6
            assert S.inter_pred(checker, (xf, yf), 0, 0, 1, 1)[0, 0] == want


def test_taps_are_clamped_at_all_four_edges():
    rng = np.random.default_rng(7)
    plane = rng.integers(0, 256, (32, 32)).astype(np.int64)
    padded = np.pad(plane, 8, mode="edge")                                          # the clamp is edge replication
    for xf, yf in FRACTIONS:
        for x0, y0, ix, iy in ((0, 0, 0, 0), (16, 0, 0, 0), (0, 16, 0, 0), (16, 16, 0, 0), (16, 16, -1 if xf else 0, -1 if yf else 0), (0, 0, -2, -2),
                               (16, 16, 2, 2)):
            v = (4 * ix + xf, 4 * iy + yf)
            assert np.array_equal(S.inter_pred(plane, v, x0, y0, 16, 0), S.inter_pred(padded, v, x0 + 8, y0 + 8, 16, 0)), (xf, yf, x0, y0, ix, iy)
    c = plane[:16, :16]
    pc = np.pad(c, 4, mode="edge")
    for v in ((3, 5), (-3, -5), (9, 1), (-12, 15)):
        for x0, y0 in ((0, 0), (8, 0), (0, 8), (8, 8)):
            assert np.array_equal(S.inter_pred(c, v, x0, y0, 8, 1), S.inter_pred(pc, v, x0 + 4, y0 + 4, 8, 1))


# ------------------------------------------------------------------------------------------------------------------------------------
# round trips
# ------------------------------------------------------------------------------------------------------------------------------------
def _check_round_trip(shape, kind, qp, search, subpel, injected=None):
    n, h, w, gop = shape
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    _, samples, (ry, rcb, rcr), _, used = S.reference(shape, kind, qp, search, subpel, injected)
    d = S.decode_stream(samples, w, h)                                              # (P.NotWholeSample cannot occur: the interpolator is installed)
    assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr), (shape, kind, qp, search, subpel)
    assert d["sync"] == list(range(0, n, gop))
    for k in range(n):
        for r in range(mbh):
            for m in range(mbw):
                vx, vy = (int(c) for c in used[k, r, m])
                assert S.admitted(vx, vy, search, subpel, m, r, mbw, mbh) and (k % gop or (vx, vy) == (0, 0))
    for k, headers in enumerate(d["headers"]):
        assert len(headers) == mbh
        for r, hd in enumerate(headers):
            assert hd["first_mb"] == r * mbw and hd["qp_delta"] == qp - 26 and 4 + hd["nal_bytes"] <= P.slot_bytes(mbw)
            assert hd["frame_num"] == (k % gop) & 15


@pytest.mark.parametrize("subpel", S.SUBPELS)
@pytest.mark.parametrize("shape", S.SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}-gop{s[3]}" for s in S.SHAPES])
def test_round_trip_decodes_to_the_encoders_own_reconstruction(shape, subpel):
    """Every case of the grid (kinds x qp x search for this shape and grid): the decoder with the interpolator installed recovers, sample
    for sample, the pictures the restatement reconstructed; every coded vector is one the rule admits."""
    assert sorted(s[:3] for s in S.SHAPES) == sorted([(4, 16, 16), (5, 32, 48), (3, 36, 50), (6, 96, 128)])
    for kind in S.KINDS:
        for qp in S.QPS:
            for search in S.SEARCHES:
                _check_round_trip(shape, kind, qp, search, subpel)


def test_the_unpatched_decoder_refuses_a_fractional_stream():
    """The round trips above mean something only if the parent's decoder cannot read these streams."""
    shape = (5, 32, 48, 5)
    samples, used = S.reference(shape, "glide1", 16, 8, 4)[1], S.reference(shape, "glide1", 16, 8, 4)[4]
    assert (used % 4).any()
    with pytest.raises(P.NotWholeSample):
        P.decode_stream(samples, shape[2], shape[1])


def test_injected_vectors_round_trip_and_reach_every_path_of_the_rule():
    """Asserted on the restatement's statistics, summed over the injected cases."""
    mvd_x, mvd_y, after, fractions, taps = set(), set(), set(), set(), set()
    cbp0 = skip_after = skip_after_fraction = 0
    kinds = set()                                                                   # which of the three reasons made a vector invalid
    for shape, qp, search, subpel, kind in INJECTED:
        _check_round_trip(shape, "planted", qp, search, subpel, kind)
        st, used = S.reference(shape, "planted", qp, search, subpel, kind)[3:]
        mvd_x |= st["mvd_x"]
        mvd_y |= st["mvd_y"]
        after |= st["nonzero_after"]
        fractions |= st["fractions"]
        taps |= st["tap_edges"]
        cbp0 += st["nonzero_cbp0"]
        skip_after += st["skip_after_nonzero"]
        skip_after_fraction += st.get("skip_after_fraction", 0)
        if kind == "extreme" and search == 16:
            assert {-128, 128} <= st["mvd_x"] and {-128, 128} <= st["mvd_y"]       # |mvd| = 8 search: left neighbour at -4 search, this one at +4 search
        if kind == "invalid":                                                       # off-grid, out-of-range and not-admitted alike: (0, 0)
            n, mbh, mbw = used.shape[:3]
            mv = S.inject(kind, n, mbh, mbw, search, subpel)
            bad = [(k, r, m) for k in range(n) if k % shape[3] for r in range(mbh) for m in range(mbw)
                   if not S.admitted(int(mv[k, r, m, 0]), int(mv[k, r, m, 1]), search, subpel, m, r, mbw, mbh)]
            assert st["invalid_as_zero"] == len(bad) > 0 and all(not used[i].any() for i in bad)
            for k, r, m in bad:
                vx, vy = int(mv[k, r, m, 0]), int(mv[k, r, m, 1])
                kinds.add("grid" if vx % (4 // subpel) or vy % (4 // subpel) else "range" if max(abs(vx), abs(vy)) > 4 * search else "admission")
        if shape[:3] == (4, 16, 16):                                                # the one-macroblock picture has only (0, 0)
            assert not used.any()
        assert not st["p_mb_bits"] or max(st["p_mb_bits"]) <= R.MAX_MB_BITS
    assert fractions == set(FRACTIONS)
    assert kinds == {"grid", "range", "admission"}
    assert min(mvd_x) < 0 < max(mvd_x) and min(mvd_y) < 0 < max(mvd_y)
    assert any(v % 4 for v in mvd_x) and any(v % 4 for v in mvd_y)
    assert cbp0 and skip_after and skip_after_fraction
    assert after == {"intra", "pcm", "skip"}
    assert taps == {"left", "right", "top", "bottom"}


def test_invalid_vectors_are_of_all_three_kinds():
    for subpel in (1, 2):
        assert any(v[0] % (4 // subpel) or v[1] % (4 // subpel) for v in S.INVALID)                               # off the grid
    assert any(abs(v[0]) > 64 or abs(v[1]) > 64 for v in S.INVALID)                                                 # out of range
    assert not S.admitted(-64, 0, 16, 4, 0, 0, 3, 2) and not S.admitted(3, 3, 16, 4, 2, 1, 3, 2)                    # leave the picture
    assert S.admitted(3, 3, 16, 4, 1, 0, 3, 2) and not S.admitted(3, 3, 16, 2, 1, 0, 3, 2) and not S.admitted(2, 6, 16, 1, 1, 0, 3, 2)
    assert not any(S.admitted(v[0], v[1], 16, 4, 0, 0, 1, 1) for v in S.INVALID)
    assert S.candidates(16, 4, 0, 0, 1, 1) == [(0, 0)] and len(S.candidates(2, 4, 1, 1, 3, 3)) == 17 * 17
    assert len(S.candidates(16, 1, 1, 1, 3, 3)) == 33 * 33 and len(S.candidates(2, 2, 1, 1, 3, 3)) == 81
    # a fractional vector needs the whole sample beyond it: at the right edge (1, 0) is out, (-1, 0) is in
    assert not S.admitted(1, 0, 8, 4, 2, 1, 3, 3) and S.admitted(-1, 0, 8, 4, 2, 1, 3, 3) and S.admitted(0, 0, 8, 4, 2, 1, 3, 3)


# ------------------------------------------------------------------------------------------------------------------------------------
# agreement with the parent rule and between the grids
# ------------------------------------------------------------------------------------------------------------------------------------
def test_subpel_0_is_the_parents_restatement():
    for shape, kind, qp, search in (((5, 32, 48, 5), "pan2", 16, 8), ((3, 36, 50, 3), "noise", 28, 2), ((4, 16, 16, 4), "zeros_pcm", 0, 16),
                                    ((5, 32, 48, 5), "pan1", 51, 16), ((3, 36, 50, 3), "cut", 0, 8), ((5, 32, 48, 5), "still", 16, 2)):
        got = S.reference(shape, kind, qp, search, 0)
        want = M.reference(shape, kind, qp, search)
        assert got[1] == want[1] and all(np.array_equal(a, b) for a, b in zip(got[2], want[2])) and np.array_equal(got[4], 4 * want[4])
    planes = S.make_planes("glide2", 5, 32, 48)
    for gop, search, subpel in ((1, 8, 4), (5, 0, 4)):                              # accepted, and changes nothing
        got = S.encode_planes(*planes, qp=16, gop=gop, search=search, subpel=subpel)
        want = M.encode_planes(*planes, qp=16, gop=gop, search=search)
        assert got[0] == want[0]


def test_subpel_1_on_pan2_gives_the_parents_vectors():
    """Content that moves by two samples a picture: the whole-sample grid finds the parent's even vectors, times 4.  A few blocks
    (3 of 288 at 96 x 128) are flat along x where they moved, so a shift by one sample has SAD 0 as well and the order prefers the shorter
    vector; there the winner must be strictly smaller under the order, everywhere else identical."""
    for shape, qp, search in (((5, 32, 48, 5), 28, 2), ((3, 36, 50, 3), 16, 8), ((6, 96, 128, 6), 16, 8)):
        y = S.make_planes("pan2", *shape[:3])[0]
        mv1, sad1 = S.search_planes(y, qp, shape[3], search, 1)
        mv0, sad0 = M.search_planes(y, qp, shape[3], search)
        odd = (mv1 % 8 != 0).any(axis=-1)
        print(shape, qp, search, "blocks with an odd winner:", int(odd.sum()), "of", odd.size)
        assert np.array_equal(mv1[~odd], 4 * mv0[~odd]) and np.array_equal(sad1[~odd], sad0[~odd]) and mv0.any() and 10 * odd.sum() < odd.size
        for i in np.argwhere(odd):
            a, b = tuple(int(c) for c in mv1[tuple(i)]), tuple(4 * int(c) for c in mv0[tuple(i)])
            assert S._key(int(sad1[tuple(i)]), S.LAMBDA[qp], *a) < S._key(int(sad0[tuple(i)]), S.LAMBDA[qp], *b)
    y = S.make_planes("pan2", 5, 32, 48)[0]                                         # with the range 2 no block has an odd winner: plain equality
    assert np.array_equal(S.search_planes(y, 28, 5, 2, 1)[0], 4 * M.search_planes(y, 28, 5, 2)[0])


def test_flat_and_repeated_pictures_yield_zero_vectors():
    y = np.full((3, 48, 64), 77, dtype=np.uint8)
    for subpel in S.SUBPELS:
        mv, sad = S.search_planes(y, 16, 3, 8, subpel)
        assert not mv.any() and not sad.any()
    y[:, ::2] = 200
    y[:, :, ::3] = 31                                                               # periods 2 and 3: many shifts tie again
    for subpel in S.SUBPELS:
        assert not S.search_planes(y, 16, 3, 8, subpel)[0].any()


def test_finer_grids_shrink_the_stream():
    """Bytes of six pictures at 96 x 128, gop 6: strict inequalities only; the ratios are printed (DESIGN.md "H.264 sub-sample motion"
    records them)."""
    shape = (6, 96, 128)
    for kind, coarse, fine in (("pan1", 0, 1), ("glide2", 1, 2), ("glide1", 2, 4)):
        planes = S.make_planes(kind, *shape)
        for qp in (16, 28):
            a = sum(len(s) for s in S.encode_planes(*planes, qp=qp, gop=6, search=8, subpel=coarse)[0])
            b = sum(len(s) for s in S.encode_planes(*planes, qp=qp, gop=6, search=8, subpel=fine)[0])
            print(f"{kind} qp {qp}: subpel {coarse} {a} bytes, subpel {fine} {b} bytes, ratio {b / a:.3f}")
            assert b < a, (kind, qp, coarse, a, fine, b)


def test_glide_moves_by_its_quarter_samples():
    for s, subpel in ((1, 4), (2, 2), (6, 2), (2, 4)):
        y = S.make_planes(f"glide{s}", 3, 96, 128)[0]
        mv = S.search_planes(y, 16, 3, 8, subpel)[0]
        inner = mv[1:, 1:-1, 1:-1].reshape(-1, 2)
        assert 2 * sum(tuple(v) == (-s, 0) for v in inner) > len(inner), (s, subpel, inner.tolist())


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
    out = video.make_video_pyav(torch.from_numpy(frames).permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", h264_subpel=4)
    assert hashlib.sha256(open(out, "rb").read()).hexdigest() == SHA_DEFAULT
    assert "subpel" not in video.LAST_CODEC and "search" not in video.LAST_CODEC


def test_sub_header_library_and_binding_agree(hip):
    header = (ROOT / "include" / "sdv_hip_h264_sub.h").read_text()
    names = {"sdv_h264_motion_search_sub": "k_h264_motion_search_sub", "sdv_h264_encode_gop_step_sub": "k_h264_encode_gop_step_sub"}
    declared = set(re.findall(r"\b(sdv_[a-z0-9_]+)\s*\(", header)) - {"sdv_abi_version", "sdv_last_error"}
    assert declared == set(hip.H264_SUB_SYMBOLS) == set(names)
    assert not set(hip.H264_SUB_SYMBOLS) & (set(hip.EXPORTED_SYMBOLS) | set(hip.EXTENSION_SYMBOLS))
    base, ext = (ROOT / "include" / "sdv_hip.h").read_text(), (ROOT / "include" / "sdv_hip_ext.h").read_text()
    lib = ctypes.CDLL(str(hip.lib_path()))
    for name, op in names.items():
        assert hasattr(lib, name) and name not in base and not re.search(name + r"\s*\(", ext)
        assert op in hip.KERNEL_OPS and torch._C._dispatch_has_kernel_for_dispatch_key(f"sdv::{op}", "Meta")
        decl = header[header.index(f"int {name}("):]
        assert len(decl[:decl.index(");")].split(",")) == len(hip._H264_SUB_SIGNATURES[name][1]), name
        assert getattr(hip.load(), name).argtypes == hip._H264_SUB_SIGNATURES[name][1]
    assert "H.264 sub-sample motion" in header and "8.4.2.2.1" in header and "8.4.2.2.2" in header
    assert hip.load().sdv_abi_version() == hip.ABI_VERSION == 12 and hip.H264_SUBPELS == S.SUBPELS
    y = torch.zeros((2, 32, 48), dtype=torch.uint8, device="meta")                  # the Meta kernels accept the schema and do nothing
    torch.ops.sdv.k_h264_motion_search_sub(y, 16, 2, 8, 4, torch.zeros((2, 2, 3, 2), dtype=torch.int16, device="meta"), None)


def test_argument_checks_at_both_layers(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, check_subpel, encoder_for
    assert H264Encoder().subpel == 0 and H264Encoder(gop=4, search=8, subpel=4).subpel == 4 and H264Encoder(subpel=2).search == 0
    assert [check_subpel(v) for v in (0, 1, 2, 4)] == [0, 1, 2, 4]
    assert encoder_for(20, "cuda:0", 4, 8) is encoder_for(20, "cuda:0", 4, 8, 0) is not encoder_for(20, "cuda:0", 4, 8, 4)
    for bad in (3, 8, -1, True, "4", 4.0, None, 16):
        with pytest.raises(ValueError, match="one of the integers 0, 1, 2, 4"):
            check_subpel(bad)
        with pytest.raises(ValueError, match="one of the integers 0, 1, 2, 4"):
            H264Encoder(gop=4, search=8, subpel=bad)
    with pytest.raises(hip.SdvHipError, match="no CPU fallback"):
        H264Encoder(gop=4, search=8, subpel=4).encode(torch.zeros((2, 16, 16, 3), dtype=torch.uint8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    i16 = lambda *s: torch.zeros(s, dtype=torch.int16)
    op = torch.ops.sdv.k_h264_motion_search_sub
    ok = dict(y=u8(2, 32, 48), qp=16, gop=4, search=8, subpel=4, mv=i16(2, 2, 3, 2), sad=None)
    for key, val, word in (("y", u8(2, 32, 40), "y must be"), ("qp", 52, "qp must be"), ("gop", 0, "gop must be"), ("search", 0, "search must be"),
                           ("search", 3, "search must be"), ("search", 18, "search must be"), ("subpel", 0, "subpel must be"),
                           ("subpel", 3, "subpel must be"), ("subpel", 8, "subpel must be"), ("subpel", -1, "subpel must be"),
                           ("mv", i16(2, 2, 3), "mv must be"), ("mv", torch.zeros((2, 2, 3, 2), dtype=torch.int32), "mv must be"),
                           ("sad", torch.zeros((2, 2, 3), dtype=torch.int16), "sad must be"), ("sad", torch.zeros((2, 2, 2), dtype=torch.int32), "sad must be"),
                           ("mv", i16(2, 2, 3, 2), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            op(*dict(ok, **{key: val}).values())
    op = torch.ops.sdv.k_h264_encode_gop_step_sub
    sb = hip.h264_gop_scratch_bytes(2, 2, 3)
    ok = dict(y=u8(2, 32, 48), cb=u8(2, 16, 24), cr=u8(2, 16, 24), qp=16, gop=4, k=1, search=8, subpel=2, first_index=0, mv=i16(2, 2, 3, 2),
              ry=u8(2, 32, 48), rcb=u8(2, 16, 24), rcr=u8(2, 16, 24), scratch=u8(sb))
    for key, val, word in (("y", u8(2, 32, 40), "y must be"), ("cb", u8(2, 16, 16), "cb must be"), ("qp", -1, "qp must be"), ("gop", 257, "gop must be"),
                           ("k", 2, "position k"), ("k", -1, "position k"), ("search", 0, "search must be"), ("search", 5, "search must be"),
                           ("subpel", 0, "subpel must be"), ("subpel", 3, "subpel must be"), ("subpel", 8, "subpel must be"),
                           ("first_index", -1, "first_index"), ("mv", i16(2, 2, 3, 1), "mv must be"), ("ry", u8(2, 32, 32), "ry must be"),
                           ("rcr", u8(2, 8, 24), "rcr must be"), ("scratch", u8(sb - 1), "scratch holds"), ("scratch", u8(sb), "GPU memory")):
        with pytest.raises(hip.SdvHipError, match=word):
            op(*dict(ok, **{key: val}).values())
    lib = hip.load()
    ok = [16, 2, 3, 4, 16, 4, 8, 4, 64, 128, None]                                  # y, n, mbh, mbw, qp, gop, search, subpel, mv, sad, stream
    for pos, val, word in ((0, None, b"null"), (8, None, b"null"), (1, 0, b"frame count"), (2, 0, b"macroblock grid"), (4, 52, b"qp="), (5, 0, b"gop="),
                           (6, 0, b"search="), (6, 7, b"search="), (6, 18, b"search="), (7, 0, b"subpel="), (7, 3, b"subpel="), (7, 8, b"subpel="),
                           (7, -1, b"subpel="), (0, 8, b"aligned"), (8, 66, b"aligned"), (9, 130, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_motion_search_sub(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_motion_search_sub")
    sb = hip.h264_gop_scratch_bytes(2, 3, 4)
    ok = [16, 32, 48, 2, 3, 4, 16, 4, 1, 8, 4, 0, 256, 64, 80, 96, 128, sb, None]  # y cb cr | n mbh mbw qp gop k search subpel first | mv ry rcb rcr scratch | bytes
    for pos, val, word in ((0, None, b"null"), (12, None, b"null"), (13, None, b"null"), (16, None, b"null"), (3, 0, b"frame count"),
                           (4, 0, b"macroblock grid"), (5, 1009, b"above 1008"), (6, 52, b"qp="), (7, 0, b"gop="), (8, 2, b"position k"),
                           (8, -1, b"position k"), (9, 0, b"search="), (9, 3, b"search="), (10, 0, b"subpel="), (10, 3, b"subpel="), (10, 8, b"subpel="),
                           (11, -1, b"first_index"), (17, sb - 1, b"scratch buffer too small"), (0, 8, b"aligned"), (12, 258, b"aligned"),
                           (13, 72, b"aligned"), (16, 132, b"aligned")):
        a = list(ok)
        a[pos] = val
        assert lib.sdv_h264_encode_gop_step_sub(*a) == -1 and word in lib.sdv_last_error(), (pos, val, lib.sdv_last_error())
        assert lib.sdv_last_error().startswith(b"sdv_h264_encode_gop_step_sub")


def test_pipeline_attribute_and_sdv_h264_subpel(monkeypatch):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny")
    monkeypatch.delenv("SDV_H264_SUBPEL", raising=False)
    assert pipe.h264_subpel == 0 and pipe.h264_subpel_choice() == 0
    pipe.h264_subpel = 2
    assert pipe.h264_subpel_choice() == 2
    monkeypatch.setenv("SDV_H264_SUBPEL", "4")                                      # the variable wins when it is set
    assert pipe.h264_subpel_choice() == 4
    for bad in ("3", "8", "-1", "four", " 4", "2.0", "16"):
        monkeypatch.setenv("SDV_H264_SUBPEL", bad)
        with pytest.raises(ValueError, match="SDV_H264_SUBPEL"):
            pipe.h264_subpel_choice()
    monkeypatch.delenv("SDV_H264_SUBPEL")
    for bad in (3, True, "4"):
        pipe.h264_subpel = bad
        with pytest.raises(ValueError, match="h264_subpel"):
            pipe.h264_subpel_choice()


def test_make_video_pyav_checks_subpel_and_falls_back_without_a_gpu(tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import utils, video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = torch.from_numpy(R.make_frames("ramp", 3, 20, 36))
    for bad in (3, 8, -1, "4", 2.0, True):
        with pytest.raises(ValueError, match="one of the integers 0, 1, 2, 4"):
            video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "x.mp4", codec="h264-cavlc", h264_gop=4, h264_search=8, h264_subpel=bad)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    a = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=4, h264_search=8, h264_subpel=4)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)" and "no GPU" in video.LAST_CODEC["why"] and "subpel" not in video.LAST_CODEC
    b = video.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "b.mp4")
    c = utils.make_video_pyav(frames, fps=5, output_filepath=tmp_path / "c.mp4", h264_gop=4, h264_search=8, h264_subpel=4)   # ignored by the other codecs
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()


def test_host_build_of_the_sub_sample_pieces_under_sanitizers_equals_the_restatement(tmp_path):
    """csrc/sdv_h264_core.h's interpolators, window addresses and macroblock step with a quarter-sample vector compiled for the host with
    -fsanitize=address,undefined into a stand-alone program (tests/h264_sub_host_main.cpp) and run as a subprocess on exact-size buffers:
    samples, reconstruction and the coded vectors equal the restatement's on three cases, and the 16 positions at the four corners equal
    ``inter_pred``."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "h264_sub_host"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "stable_diffusion_videos_amd" / "csrc"), str(ROOT / "tests" / "h264_sub_host_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("the host compiler has no sanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr
    for shape, qp, search, subpel, kind in (((3, 36, 50, 3), 16, 8, 4, "fractions"), ((7, 64, 64, 3), 0, 16, 4, "extreme"),
                                            ((5, 32, 48, 5), 51, 16, 1, "invalid"), ((3, 36, 50, 3), 28, 8, 4, "edges")):
        (y, cb, cr), samples, recon, _, used = S.reference(shape, "planted", qp, search, subpel, kind)
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        mv = S.inject(kind, n, mbh, mbw, search, subpel)
        (tmp_path / "in.bin").write_bytes(np.array([n, mbh, mbw, qp, shape[3], S.FIRST, search, subpel], dtype="<i4").tobytes() + y.tobytes()
                                          + cb.tobytes() + cr.tobytes() + mv.astype("<i2").tobytes())
        r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        data, at, got = (tmp_path / "out.bin").read_bytes(), 0, []
        for _ in range(n):
            size = int.from_bytes(data[at:at + 4], "little")
            got.append(data[at + 4:at + 4 + size])
            at += 4 + size
        assert got == samples, (shape, qp, search, subpel, kind)
        for want in recon:
            assert np.array_equal(np.frombuffer(data[at:at + want.size], dtype=np.uint8).reshape(want.shape), want), (shape, qp, search, kind)
            at += want.size
        assert np.array_equal(np.frombuffer(data[at:at + 2 * used.size], dtype="<i2").reshape(used.shape), used)
        at += 2 * used.size
        for corner in range(4):
            for fr in range(16):
                m, row, xf, yf = (mbw - 1 if corner & 1 else 0), (mbh - 1 if corner & 2 else 0), fr & 3, fr >> 2
                v = (xf - (4 if corner & 1 and xf else 0), yf - (4 if corner & 2 and yf else 0))
                assert S.admitted(v[0], v[1], 2, 4, m, row, mbw, mbh)
                assert tuple(np.frombuffer(data[at:at + 4], dtype="<i2")) == v
                assert np.array_equal(np.frombuffer(data[at + 4:at + 260], dtype=np.uint8).reshape(16, 16), S.inter_pred(y[0], v, 16 * m, 16 * row, 16, 0))
                assert np.array_equal(np.frombuffer(data[at + 260:at + 324], dtype=np.uint8).reshape(8, 8), S.inter_pred(cb[0], v, 8 * m, 8 * row, 8, 1))
                at += 324
        assert at == len(data)
