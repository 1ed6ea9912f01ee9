"""Several slices per macroblock row of the H.264 track (include/sdv_hip_h264_seg.h, DESIGN.md "H.264 row slices") restated in plain Python /
numpy on top of h264_part_ref.py, h264_lf_ref.py, h264_i4_ref.py, h264_sub_ref.py, h264_me_ref.py, h264_p_ref.py and h264_ref.py, none of
which is edited.  Nothing here imports the package's encoder.

The rule, restated.  Setting row_slices S in 1 .. 16, with every gop, search, subpel, intra4, deblock and part.
  segs = max(1, min(S, mbw, 1024 // mbh)) slices per macroblock row; the frame size alone decides.
  Geometry.  Slice s (0 .. segs - 1) of row r covers macroblocks m0 = s * mbw // segs .. m1 = (s + 1) * mbw // segs - 1: widths differ by at
  most one, none is empty.  first_mb_in_slice = r * mbw + m0; the slices of a picture stand in the sample in increasing first_mb_in_slice
  order, each behind its 4-byte length: mbh * segs slices a sample.  Everything else in the headers, stss and the parameter sets is unchanged.
  A slice start is a row start: the macroblock at m0 has no neighbour A (and no B, C, D as before).  Intra16x16 DC and chroma DC predict 128;
  nC is 0; mvp of partition 0 or of the one vector is (0, 0), partition 2 takes the median with A = (0, 0) / refIdx -1; P_Skip infers
  (0, 0); mb_skip_run counts from zero and a trailing run ends the slice; in I_NxN the four left blocks have no left samples and
  predIntra4x4PredMode 2, block 0 admits DC (128) only; intra in a P slice does not read the left slice's reconstruction.
  What does not stop at a slice start: motion vectors (admission is the picture's), the loop filter (the left macroblock edge at m0 is
  filtered across the boundary with the usual bS), the search (on source pictures).
  Capacity: a slice of at most W = ceil(mbw / segs) macroblocks takes at most the GOP path's bound for W; its slot is 600 w' + 17 bytes with
  w' = W + 1 + W // 64.  Slot index (f * mbh + r) * segs + s.
  One vector layout for every route: int16 [n][mbh][mbw][4][2] in quarter samples; a one-vector search result is written four times (scaled
  to quarter samples), no search is zeros; four equal vectors are coded as P_L0_16x16 / P_Skip.

(a) ``row_segments`` / ``bounds`` / ``seg_slot_mbw`` / ``seg_scratch_bytes`` / ``seg_out_bytes``;
(b) ``encode_planes(..., row_slices=S, mv=None)``: always its own loop over (picture, row, slice, macroblock) in the four-vector layout - at
    S = 1 too, where its bytes must be those of the other modules;
(c) ``decode_stream``: a picture loop of its own whose neighbour availability comes from SLICE MEMBERSHIP: it reads first_mb_in_slice,
    assigns every macroblock, 8x8 partition and 4x4 block the slice it was decoded in, and derives A / B / C / D, nC, the intra sample
    availability and predIntra4x4PredMode from that alone (it knows nothing of rows); it filters across slice boundaries; it refuses a
    sample whose slices are out of order, overlap or leave a macroblock uncovered.  It counts what it meets (``new_seg_stats``).
"""
import functools
from unittest import mock

import numpy as np

import h264_i4_ref as I
import h264_lf_ref as L
import h264_me_ref as M
import h264_p_ref as P
import h264_part_ref as PT
import h264_ref as R
import h264_sub_ref as S

ROW_SLICES_MAX = 16
SLOT_ROWS = 1024
FIRST = P.FIRST
SEARCH = 8
SHAPES = ((3, 16, 16), (4, 32, 48), (5, 40, 72), (3, 48, 128))                     # 1 x 1 (segs 1) | 2 x 3 | 3 x 5 padded | 3 x 8
ROW_SLICES = (2, 3, 4)
QPS = (0, 16, 28, 51)
GOP = 3
# the named setting rows: (name, gop, search, subpel, intra4, deblock, part)
SETTINGS = (("off", GOP, 0, 0, 0, 0, 0), ("search8", GOP, 8, 0, 0, 0, 0), ("search8-subpel4-part", GOP, 8, 4, 0, 0, 1),
            ("intra4-deblock", GOP, 0, 0, 1, 1, 0), ("all", GOP, 8, 4, 1, 1, 1), ("gop1-intra4", 1, 0, 0, 1, 0, 0))
KINDS = ("still", "pan2", "split8", "cut", "noise", "zeros_pcm", "flash_pcm")
INJECTED = ("mixed", "far", "invalid")


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) geometry and capacity
# ------------------------------------------------------------------------------------------------------------------------------------
def row_segments(mbh, mbw, row_slices):
    return max(1, min(row_slices, mbw, SLOT_ROWS // mbh))


def bounds(mbw, segs):
    """[(m0, m1)] of the slices of a row, m1 inclusive."""
    return [(s * mbw // segs, (s + 1) * mbw // segs - 1) for s in range(segs)]


def first_mbs(mbh, mbw, segs):
    return [r * mbw + m0 for r in range(mbh) for m0, _ in bounds(mbw, segs)]


def seg_slot_mbw(mbw, segs):
    return P.slot_mbw(-(-mbw // segs))


def seg_slot_bytes(mbw, segs):
    return 600 * seg_slot_mbw(mbw, segs) + 17


def seg_scratch_bytes(n, mbh, mbw, segs):
    return n * mbh * segs * (((seg_slot_bytes(mbw, segs) + 7) & ~7) + 12)


def seg_out_bytes(n, mbh, mbw, segs):
    return n * mbh * segs * seg_slot_bytes(mbw, segs)


def slice_bound(w):
    """Bytes one slice of w macroblocks takes at most in a sample (sdv_hip.h "Capacity of the GOP path", as a fraction-free bound): 4-byte
    length, NAL header, an RBSP of at most (72 + 3221 w + 21 + 8 + 7) / 8 bytes, an emulation prevention byte behind every second byte."""
    rbsp = (72 + 3221 * w + 21 + 8 + 7) // 8
    return 5 + rbsp + rbsp // 2


def make_planes(kind, n, h, w, seed=0):
    if kind.startswith("split"):
        return PT.make_planes(kind, n, h, w, seed)
    if kind == "flash_pcm":
        return P.make_planes(kind, n, h, w, seed)
    return M.make_planes(kind, n, h, w, seed)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
def vectors_for(y, qp, gop, search, subpel, part):
    """The four-vector tensor of the settings, int16 [n, mbh, mbw, 4, 2] in quarter samples: the partition search with ``part``, else the
    one-vector search of the settings written four times (whole samples scaled by 4), zeros without a search or without P pictures."""
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    if gop == 1 or search == 0:
        return np.zeros((n, mbh, mbw, 4, 2), dtype=np.int16)
    if part:
        return PT.search_planes(y, qp, gop, search, subpel)[0]
    one = S.search_planes(y, qp, gop, search, subpel)[0] if subpel else 4 * M.search_planes(y, qp, gop, search)[0]
    return np.repeat(np.asarray(one)[:, :, :, None, :], 4, axis=3).astype(np.int16)


def encode_planes(y, cb, cr, qp=16, gop=1, first_index=0, stats=None, search=0, subpel=0, intra4=0, deblock=0, part=0, row_slices=1, mv=None):
    """Padded planes -> (samples, recon Y, recon Cb, recon Cr, mv used int16 [n, mbh, mbw, 4, 2] quarter samples, side information per
    picture (always; the filter runs with ``deblock`` only), segs).  ``mv`` None: the vectors of the settings (``vectors_for``); else
    injected ones, each coded as (0, 0) where the rule does not admit it.  Every slice is asserted to fit its slot."""
    stats = PT.new_stats() if stats is None else stats
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    segs = row_segments(mbh, mbw, row_slices)
    active = gop > 1 and search > 0
    if mv is None:
        mv = vectors_for(y, qp, gop, search, subpel if active else 0, part if active else 0)
    v_search, v_subpel = (search, subpel) if active else (2, 0)                    # without a search the step takes its smallest range
    used = np.zeros((n, mbh, mbw, 4, 2), dtype=np.int16)
    ry, rcb, rcr = np.empty_like(y), np.empty_like(cb), np.empty_like(cr)
    samples, infos = [], []
    cap = seg_slot_bytes(mbw, segs)
    for k in range(n):
        is_p = k % gop != 0
        info = dict(intra=np.zeros((mbh, mbw), dtype=bool), pcm=np.zeros((mbh, mbw), dtype=bool), nz=np.zeros((4 * mbh, 4 * mbw), dtype=bool),
                    mv4=np.zeros((4 * mbh, 4 * mbw, 2), dtype=np.int64), mv=np.zeros((mbh, mbw, 4, 2), dtype=np.int64))
        py_, pcb_, pcr_ = (np.empty(p.shape[1:], dtype=np.int64) for p in (y, cb, cr))
        sample = bytearray()
        for r in range(mbh):
            for m0, m1 in bounds(mbw, segs):
                hdr = P.p_slice_header(r * mbw + m0, k % gop, qp) if is_p else R.slice_header(r * mbw + m0, (first_index + k) & 1, qp)
                bits = [L.lf_header(hdr) if deblock else hdr]
                left, run, chain = None, 0, ((0, 0), (0, 0))                       # a slice start is a row start
                for m in range(m0, m1 + 1):
                    ys, xs, yc, xc = slice(16 * r, 16 * r + 16), slice(16 * m, 16 * m + 16), slice(8 * r, 8 * r + 8), slice(8 * m, 8 * m + 8)
                    sy, sc = y[k, ys, xs], np.stack([cb[k, yc, xc], cr[k, yc, xc]])
                    if is_p:
                        vs = [(int(mv[k, r, m, i, 0]), int(mv[k, r, m, i, 1])) for i in range(4)]
                        ok = [PT.admitted(v[0], v[1], v_search, v_subpel, m, r, mbw, mbh) for v in vs]
                        stats["refused"] += 4 - sum(ok)
                        stats["refused_one"] += sum(ok) == 3
                        vs = tuple(v if o else (0, 0) for v, o in zip(vs, ok))
                        fy = PT.part_pred(ry[k - 1], vs, 16 * m, 16 * r, 16, 0).astype(np.uint8)
                        fc = np.stack([PT.part_pred(p[k - 1], vs, 8 * m, 8 * r, 8, 1) for p in (rcb, rcr)]).astype(np.uint8)
                        if len(set(vs)) == 1:
                            stats["equal4"] += 1
                            mode, mb, py, pc, left, mvp = S.encode_p_mb(sy, sc, fy, fc, left, chain[0], vs[0], qp, stats)
                            chain = (mvp, mvp)
                        else:
                            mode, mb, py, pc, left, chain = PT.encode_p8x8(sy, sc, fy, fc, left, chain, vs, qp, stats)
                        stats["modes"].append(mode)
                        if mode == "skip":
                            run += 1
                        else:
                            bits.append(R.ue(run))
                            run = 0
                        if mode == "inter":
                            info["nz"][4 * r:4 * r + 4, 4 * m:4 * m + 4] = L._inter_nz(sy, fy, qp)
                            info["mv"][r, m] = used[k, r, m] = vs
                            for i in range(4):
                                info["mv4"][4 * r + 2 * (i >> 1):4 * r + 2 * (i >> 1) + 2, 4 * m + 2 * (i & 1):4 * m + 2 * (i & 1) + 2] = vs[i]
                    else:
                        if intra4:
                            mb, py, pc, left, pcm = I.encode_mb(sy, sc, left, qp, stats, R.encode_mb)
                        else:
                            mb, py, pc, left, pcm = R.encode_mb(sy, sc, left, qp, stats["intra"])
                        mode = "pcm" if pcm else "intra"
                    info["intra"][r, m], info["pcm"][r, m] = mode in ("intra", "pcm"), mode == "pcm"
                    if mode == "pcm":
                        bits.append(R.ue(30 if is_p else 25))
                        bits.append("0" * (-sum(map(len, bits)) % 8))
                        bits.append("".join(format(int(s), "08b") for s in np.concatenate([sy.reshape(-1), sc.reshape(-1)])))
                    elif mode != "skip":
                        bits.append(mb)
                        assert len(mb) <= R.MAX_MB_BITS
                    py_[ys, xs] = py
                    pcb_[yc, xc], pcr_[yc, xc] = pc[0], pc[1]
                if is_p and run:
                    bits.append(R.ue(run))
                s = "".join(bits) + "1"
                s += "0" * (-len(s) % 8)
                rbsp = int(s, 2).to_bytes(len(s) // 8, "big")
                nal = bytes([0x41 if is_p else 0x65]) + R.escape(rbsp)
                assert 4 + len(nal) <= slice_bound(m1 - m0 + 1) <= cap, "the slot bound of sdv_hip_h264_seg.h"
                sample += len(nal).to_bytes(4, "big") + nal
        samples.append(bytes(sample))
        if deblock:
            PT.filter_picture(py_, pcb_, pcr_, qp, info)                           # the filter knows nothing of slices
        ry[k], rcb[k], rcr[k] = py_, pcb_, pcr_
        infos.append(info)
    return samples, ry, rcb, rcr, used, infos, segs


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the decoder
# ------------------------------------------------------------------------------------------------------------------------------------
def new_seg_stats():
    return dict(slices=0, widths=set(), start_left=set(), start_left_nonzero_mv=0, start_mvd_is_v=0, start_kinds=set(), p8x8_start=0,
                p8x8_start_part2_a=set(), i4_start=0, i4_start_top_mode=0, i4_start_block0_dc=0, only_run=0, begins_in_run=0, ends_in_run=0,
                begins_and_ends_in_run=0, pcm_first=0, pcm_last=0, boundary_bs=set(), boundary_edges=0, start_intra16_dc128=0)


def _boundary_bs(pic, sst):
    """bS of the luma lines of every vertical macroblock edge that is a slice boundary inside a row (it depends on modes, coefficients
    and vectors only, so it can be read before the filter runs)."""
    mbw = pic.mbw
    for mb in range(mbw * pic.mbh):
        my, mx = divmod(mb, mbw)
        if mx == 0 or pic.slice_of[mb] == pic.slice_of[mb - 1]:
            continue
        sst["boundary_edges"] += 1
        for k in range(16):
            qy, qx = 16 * my + k, 16 * mx
            if pic.ref[mb] < 0 or pic.ref[mb - 1] < 0:
                bs = 4
            elif pic.nz_y[qy // 4, qx // 4] != 0 or pic.nz_y[qy // 4, (qx - 1) // 4] != 0:
                bs = 2
            elif (np.abs(pic.mv8[qy // 8, qx // 8] - pic.mv8[qy // 8, (qx - 1) // 8]) >= 4).any():
                bs = 1
            else:
                bs = 0
            sst["boundary_bs"].add(bs)


def _decode_picture(sample, mbw, mbh, ref_pic, pic_init_qp=26):
    """One mp4 sample -> (_Picture, headers).  Every slice starts where its first_mb_in_slice says; a macroblock's neighbours are
    available iff they were decoded in the SAME slice (6.4.x) - nothing here knows that slices are pieces of rows.  Refused: slices out
    of order, overlapping slices, an uncovered macroblock.  P_Skip, P_L0_16x16, P_8x8 with four P_L0_8x8, Intra16x16, I_NxN, I_PCM; loop
    filter by the slice header, across slice boundaries (disable_deblocking_filter_idc 0, not 2)."""
    pst, sst = PT.decode_stream.stats, decode_stream.stats
    pic = P._Picture(mbw, mbh)
    pic.pcm = set()
    blk, _ = I._i4_state(pic)
    PT._grid(pic)
    headers, at, slice_no = [], 0, 0
    slice_qp, idc, last_first = None, None, -1
    while at < len(sample):
        size = int.from_bytes(sample[at:at + 4], "big")
        nal = sample[at + 4:at + 4 + size]
        at += 4 + size
        assert nal[0] >> 7 == 0 and nal[-1] != 0
        ref_idc, unit_type = (nal[0] >> 5) & 3, nal[0] & 31
        assert unit_type in (1, 5) and ref_idc != 0
        rd = R.BitReader(R.unescape(nal[1:]))
        hd = dict(nal_unit_type=unit_type, nal_ref_idc=ref_idc, first_mb=rd.ue(), slice_type=rd.ue(), pps_id=rd.ue(), frame_num=rd.u(4), nal_bytes=size)
        is_p = hd["slice_type"] % 5 == 0
        assert is_p or hd["slice_type"] % 5 == 2, "P and I slices only"
        assert not (unit_type == 5 and is_p)
        if unit_type == 5:
            hd["idr_pic_id"] = rd.ue()
        if is_p:
            if rd.u(1):
                assert rd.ue() == 0, "one active reference only"
            assert rd.u(1) == 0
        if unit_type == 5:
            hd["no_output"], hd["long_term"] = rd.u(1), rd.u(1)
        else:
            assert rd.u(1) == 0
        hd["qp_delta"] = rd.se()
        hd["deblock_idc"] = rd.ue()
        if hd["deblock_idc"] != 1:
            assert hd["deblock_idc"] == 0 and rd.se() == 0 and rd.se() == 0, "idc 0 without offsets, or idc 1"
        assert idc in (None, hd["deblock_idc"])
        idc = hd["deblock_idc"]
        headers.append(hd)
        qp = pic_init_qp + hd["qp_delta"]
        assert slice_qp in (None, qp)
        slice_qp = qp
        mb = first = hd["first_mb"]
        assert first > last_first, "slices out of order (arbitrary slice order is not part of the stream)"
        assert first < mbw * mbh, "first_mb_in_slice outside the picture"
        last_first = first
        more = True
        began_in_run = False
        coded = []                                                      # the kinds of this slice's macroblocks in order

        def claim(m):
            assert m < mbw * mbh, "a slice runs past the picture"
            assert pic.slice_of[m] == -1, "slices overlap"
            pic.slice_of[m] = slice_no

        def done(m):
            y4, x4 = divmod(m, mbw)
            blk[4 * y4:4 * y4 + 4, 4 * x4:4 * x4 + 4] = slice_no

        while more:                                                     # 7.3.4
            if is_p:
                run = rd.ue()
                for _ in range(run):
                    my, mx = divmod(mb, mbw)
                    claim(mb)
                    v = PT._mv_skip(pic, mx, my, slice_no)
                    if mb == first:
                        assert v == (0, 0)                              # no neighbour A in this slice
                        if mx:
                            sst["start_left"].add("skip" if pic.kind[mb - 1] == "skip" else _left_kind(pic, mb - 1))
                            sst["start_left_nonzero_mv"] += bool(pic.mv8[2 * my:2 * my + 2, 2 * mx - 1].any())
                        sst["start_kinds"].add("skip")
                    P._decode_inter(rd, pic, ref_pic, mb, v, 0, qp, False, False)
                    PT._set(pic, mb, slice_no, [v] * 4, 0, "skip")
                    pst["kinds"].add("skip")
                    pic.n_skip += 1
                    coded.append("skip")
                    done(mb)
                    mb += 1
                if run > 0:
                    more = rd.more_rbsp_data()
                    began_in_run = began_in_run or len(coded) == run
            if more:
                my, mx = divmod(mb, mbw)
                claim(mb)
                avail_a = mx > 0 and pic.slice_of[mb - 1] == slice_no
                avail_b = my > 0 and pic.slice_of[mb - mbw] == slice_no
                left_kind = pic.kind[mb - 1] if avail_a else None
                start = mb == first
                if start and mx:
                    sst["start_left"].add(_left_kind(pic, mb - 1))
                    sst["start_left_nonzero_mv"] += bool(pic.mv8[2 * my:2 * my + 2, 2 * mx - 1].any())
                mb_type = rd.ue()
                if is_p and mb_type < 5:
                    assert mb_type in (0, 3), "P_L0_16x16 and P_8x8 only: 16x8, 8x16 and P_8x8ref0 are refused"
                    assert ref_pic is not None
                    if mb_type == 0:
                        mvp = PT._mv_pred(pic, 2 * mx, 2 * my, 2, slice_no)
                        v = (mvp[0] + rd.se(), mvp[1] + rd.se())
                        vs, kind = (v, v, v, v), "l16"
                        if start:
                            assert mvp == (0, 0)
                            sst["start_mvd_is_v"] += mx > 0 and v != (0, 0) and bool(pic.mv8[2 * my, 2 * mx - 1].any())
                        if left_kind == "p8x8" and tuple(pic.mv8[2 * my, 2 * mx - 2]) != tuple(pic.mv8[2 * my, 2 * mx - 1]):
                            pst["l16_after_split"] += 1
                    else:                                               # sub_mb_pred(): four sub_mb_type, no ref_idx, the mvd pairs
                        subs = [rd.ue() for _ in range(4)]
                        assert subs == [0, 0, 0, 0], "P_L0_8x8 only: sub-8x8 partitions are refused"
                        mvd = [(rd.se(), rd.se()) for _ in range(4)]
                        vs, kind = [], "p8x8"
                        mv8, ref8, slice8 = PT._grid(pic)
                        for i in range(4):
                            gx, gy = 2 * mx + (i & 1), 2 * my + (i >> 1)

                            def note(a, b, c, i=i):
                                if i == 2:
                                    pst["part2_a"].add("absent" if not a[0] else "intra" if a[1] < 0 else "inter")
                                    if start:
                                        assert not a[0]
                                        sst["p8x8_start_part2_a"].add("absent")
                                if i == 0 and start:
                                    assert not a[0] and not b[0] and not c[0]
                                if i == 3 and all(x[1] == 0 for x in (a, b, c)):
                                    med = (P._median(a[2][0], b[2][0], c[2][0]), P._median(a[2][1], b[2][1], c[2][1]))
                                    pst["part3_mixed"] += med not in (a[2], b[2], c[2])
                            mvp = PT._mv_pred(pic, gx, gy, 1, slice_no, note)
                            v = (mvp[0] + mvd[i][0], mvp[1] + mvd[i][1])
                            vs.append(v)
                            mv8[gy, gx], ref8[gy, gx], slice8[gy, gx] = v, 0, slice_no     # partition i is decoded: i + 1 may read it
                        vs = tuple(vs)
                        pst["p8x8"] += 1
                        pst["p8x8_first"] += mx == 0
                        pst["p8x8_after"].add(left_kind)
                        sst["p8x8_start"] += start and mx > 0
                    code = rd.ue()
                    assert code < 48
                    cbp = P.CBP_INTER[code]
                    if kind == "p8x8":
                        pst["p8x8_cbp0" if cbp == 0 else "p8x8_cbp"] += 1
                    qp = P._decode_inter(rd, pic, ref_pic, mb, vs if kind == "p8x8" else vs[0], cbp, qp, avail_a, avail_b)
                    PT._set(pic, mb, slice_no, vs, 0, kind)
                    pic.n_inter += 1
                else:
                    t = mb_type - 5 if is_p else mb_type
                    if t == 25:
                        P._decode_pcm(rd, pic, mb)
                        pic.pcm.add(mb)
                        kind = "pcm"
                    elif t == 0:
                        qp = I._decode_i4(rd, pic, mb, slice_no, qp, avail_a, avail_b)
                        hd["n_i4"] = hd.get("n_i4", 0) + 1
                        kind = "intra"
                        if start and mx:                                # the left column has no left samples: modes that need only the top
                            modes = [int(pic.i4_mode[4 * my + by, 4 * mx]) for by in range(4)]
                            assert modes[0] == I.DC and all(not I.NEED[m_] & (I.LEFT | I.CORNER) for m_ in modes)
                            sst["i4_start"] += 1
                            sst["i4_start_block0_dc"] += 1
                            sst["i4_start_top_mode"] += any(m_ != I.DC for m_ in modes[1:])
                    else:
                        assert 1 <= t <= 24
                        qp = P._decode_intra16(rd, pic, mb, t, qp, avail_a, avail_b)
                        pic.n_intra += 1
                        kind = "intra"
                        sst["start_intra16_dc128"] += start and mx > 0
                    assert pic.ref[mb] == -1
                    PT._set(pic, mb, slice_no, [(0, 0)] * 4, -1, kind)
                pst["kinds"].add(kind)
                if start:
                    sst["start_kinds"].add(kind)
                coded.append(kind)
                assert qp == slice_qp
                done(mb)
                mb += 1
                more = rd.more_rbsp_data()
        assert coded, "an empty slice"
        sst["slices"] += 1
        sst["widths"].add(len(coded))
        sst["only_run"] += all(c == "skip" for c in coded)
        sst["begins_in_run"] += began_in_run
        sst["ends_in_run"] += coded[-1] == "skip"
        sst["begins_and_ends_in_run"] += began_in_run and coded[-1] == "skip" and not all(c == "skip" for c in coded)
        sst["pcm_first"] += coded[0] == "pcm" and first % mbw > 0
        sst["pcm_last"] += coded[-1] == "pcm" and mb % mbw > 0
        slice_no += 1
    assert all(s >= 0 for s in pic.slice_of), "a macroblock was never coded"
    if idc == 0:
        _boundary_bs(pic, sst)
        PT.deblock_picture(pic, slice_qp, PT.decode_stream.lf, pst)     # every left edge with mx > 0: slice boundaries included
    I.decode_stream.pictures.append(pic)
    return pic, headers


def _left_kind(pic, mb):
    kind = pic.kind[mb]
    if kind in ("l16", "p8x8"):
        return "inter"
    if kind == "pcm":
        return "pcm"
    return kind                                                         # "skip" | "intra"


def decode_stream(samples, width, height, stats=None):
    """h264_part_ref.decode_stream's result for a stream with any number of slices a picture; ``stats`` (``new_seg_stats``) takes what the
    decoder met at slice starts and boundaries (out["seg"]), beside out["part"] and out["lf"]."""
    decode_stream.stats = new_seg_stats() if stats is None else stats
    PT.decode_stream.stats = PT.new_part_stats()
    PT.decode_stream.lf = L.new_lf_stats()
    I.decode_stream.pictures = []
    with mock.patch.object(P, "_decode_picture", _decode_picture), mock.patch.object(P, "_inter_pred", PT._pred_any):
        out = P.decode_stream(samples, width, height)
    out["seg"], out["part"], out["lf"] = decode_stream.stats, PT.decode_stream.stats, PT.decode_stream.lf
    return out


decode_stream.stats = new_seg_stats()


def injected_case(shape, injected, search, subpel, seed=0):
    """Planes planted with injected vectors (h264_part_ref.inject / plant) and the vectors."""
    n, h, w = shape
    mbh, mbw = (h + 15) // 16, (w + 15) // 16
    mv = PT.inject(injected, n, mbh, mbw, search, subpel, seed)
    return PT.plant(n, h, w, mv, search, subpel, seed), mv


@functools.lru_cache(maxsize=None)
def reference(shape, kind, qp, setting, row_slices, injected=None):
    """(planes, samples, (ry, rcb, rcr), mv used, side information, segs, stats) of one case, computed once for all the tests that read
    it.  ``setting``: a row of SETTINGS.  ``injected``: a kind of h264_part_ref.inject - the vectors are those and the planes planted
    with them (``kind`` is then only a name; the setting must search)."""
    n, h, w = shape
    _, gop, search, subpel, intra4, deblock, part = setting
    stats = PT.new_stats()
    mv = None
    if injected is None:
        planes = make_planes(kind, n, h, w)
    else:
        assert search > 0 and gop > 1
        planes, mv = injected_case(shape, injected, search, subpel)
    samples, ry, rcb, rcr, used, infos, segs = encode_planes(*planes, qp=qp, gop=gop, first_index=FIRST, stats=stats, search=search, subpel=subpel,
                                                             intra4=intra4, deblock=deblock, part=part, row_slices=row_slices, mv=mv)
    return planes, samples, (ry, rcb, rcr), used, infos, segs, stats


def cases():
    """Every shape x setting row x content kind, with qp and S cycling so that every (shape, S) and every (setting, qp) occurs; then the
    injected vectors on the rows that search with partitions."""
    out, i = [], 0
    for shape in SHAPES:
        for setting in SETTINGS:
            for kind in KINDS:
                out.append((shape, kind, setting, QPS[(i + i // 4) % 4], ROW_SLICES[i % 3], None))
                i += 1
    for shape in SHAPES[1:]:
        for setting in (SETTINGS[2], SETTINGS[4]):
            for injected in INJECTED:
                out.append((shape, "planted", setting, QPS[(i + i // 4) % 4], ROW_SLICES[i % 3], injected))
                i += 1
    return out


CASES = cases()
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{i or k}-{g[0]}-qp{q}-S{rs}" for s, k, g, q, rs, i in CASES]
