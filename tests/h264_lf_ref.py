"""The in-loop deblocking filter of the H.264 track (include/sdv_hip_h264_lf.h, DESIGN.md "H.264 deblocking") restated in plain Python /
numpy on top of h264_i4_ref.py, h264_sub_ref.py, h264_me_ref.py, h264_p_ref.py and h264_ref.py, none of which is edited.  Nothing here
imports the package's encoder.

The rule, restated.  Slice headers write disable_deblocking_filter_idc ue(0), slice_alpha_c0_offset_div2 se(0), slice_beta_offset_div2
se(0) where they wrote ue(1); nothing else in the stream's syntax, the mode decisions, the motion search or the I_PCM triggers changes.
After a picture is coded its reconstruction is filtered by 8.7 (frame macroblocks, 4:2:0, no 8x8 transform, filterOffsetA = filterOffsetB
= 0) on the whole padded macroblock grid; intra prediction inside the picture has read unfiltered samples, the P picture after it predicts
from the filtered ones.  The left and top picture edges are not filtered, slice boundaries are.  Macroblocks in raster order; per
macroblock luma vertical edges left to right, luma horizontal edges top to bottom, then the same for Cb and Cr (edges 0 and 4, bS from
luma edges 0 and 2).  bS: 4 on a macroblock edge with an intra side, 3 on an inner edge of an intra macroblock, else 2 where a 4x4 luma
block on either side has a nonzero coefficient, else 1 where the vectors differ by >= 4 quarter samples in a component, else 0.  qPp / qPq
0 for I_PCM and the slice qp otherwise, through QPc first for chroma; indexA = indexB = clip(0, 51, (qPp + qPq + 1) >> 1).  A line is
filtered when bS != 0 and |p0 - q0| < alpha and |p1 - p0| < beta and |q1 - q0| < beta; bS < 4 the clipped delta with tc = tc0 + (ap <
beta) + (aq < beta) in luma (and the p1 / q1 corrections clipped to +- tc0), tc0 + 1 in chroma; bS 4 the strong form in luma where ap <
beta and |p0 - q0| < (alpha >> 2) + 2, else and in chroma (2 p1 + p0 + q1 + 2) >> 2.

(a) ``ALPHA``, ``BETA``, ``TC0``: Tables 8-16 and 8-17.
(b) ``filter_diagonals``: the encoder side's filter - the macroblocks of one diagonal x + 2 y at a time, all their lines of one edge as
    one array, the clauses as masks.  ``filter_lines`` is its sample filter.
(c) ``encode_planes(..., deblock=1)``: the picture loop of h264_sub_ref.encode_planes around the other modules' macroblock functions, with
    the headers above, side information gathered per macroblock (kind; for inter macroblocks the nonzero 4x4 blocks, quantised again here;
    the vector) and the reference planes filtered between two pictures.
(d) ``decode_stream``: h264_i4_ref's picture loop with a slice header reader of its own, and after every picture ``deblock_picture``: the
    filter written separately, macroblock by macroblock in raster order as loops over edges, lines and samples straight from the clauses,
    bS from what was parsed (mb_type, TotalCoeff, vectors) - never from the encoder's side information.  It counts what it meets.
"""
import functools
from unittest import mock

import numpy as np

import h264_i4_ref as I
import h264_me_ref as M
import h264_p_ref as P
import h264_ref as R
import h264_sub_ref as S

ALPHA = (0,) * 16 + (4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144, 162, 182, 203,
                     226, 255, 255)
BETA = (0,) * 16 + (2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17, 18, 18)
_TC0_RUNS = (((0, 16), (0, 0, 0)), ((17, 20), (0, 0, 1)), ((21, 22), (0, 1, 1)), ((23, 26), (1, 1, 1)), ((27, 30), (1, 1, 2)), ((31, 32), (1, 2, 3)),
             ((33, 33), (2, 2, 3)), ((34, 34), (2, 2, 4)), ((35, 36), (2, 3, 4)), ((37, 37), (3, 3, 5)), ((38, 39), (3, 4, 6)), ((40, 40), (4, 5, 7)),
             ((41, 41), (4, 5, 8)), ((42, 42), (4, 6, 9)), ((43, 43), (5, 7, 10)), ((44, 44), (6, 8, 11)), ((45, 45), (6, 8, 13)), ((46, 46), (7, 10, 14)),
             ((47, 47), (8, 11, 16)), ((48, 48), (9, 12, 18)), ((49, 49), (10, 13, 20)), ((50, 50), (11, 15, 23)), ((51, 51), (13, 17, 25)))
TC0 = tuple(v for (lo, hi), v in _TC0_RUNS for _ in range(lo, hi + 1))            # [index][bS - 1]

MOVING_KINDS = tuple(k for k in M.KINDS if k not in ("noise", "zeros_pcm"))       # still fade pan2 drift pan1 cut
KINDS = I.KINDS + I.EXTRA_KINDS + MOVING_KINDS
SHAPES = ((2, 16, 16), (3, 16, 64), (3, 64, 16), (3, 36, 50), (3, 48, 80), (2, 96, 128))
QPS = (12, 16, 28, 40, 51)
SETTINGS = ((1, 0, 0, 0), (1, 0, 0, 1), (3, 0, 0, 0), (3, 8, 0, 0), (3, 8, 4, 1))  # (gop, search, subpel, intra4)
FIRST = P.FIRST
# the case set: intra kinds at every setting, moving kinds where there are P pictures; the forced I_PCM kind at its two quantisers
CASES = [(s, k, g) for s in SHAPES for k in KINDS for g in SETTINGS if k not in MOVING_KINDS or g[0] > 1]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}-gop{g[0]}-search{g[1]}-subpel{g[2]}-intra4{g[3]}" for s, k, g in CASES]
FORCED_KIND = "forced_pcm"                       # vramp planes with every third macroblock coded as I_PCM by the restatement (encode_planes)
FORCED_QPS = (40, 51)


def random_planes(rng, mbh, mbw, lo=0, hi=256):
    """One picture's planes with samples in lo .. hi - 1."""
    return (rng.integers(lo, hi, (16 * mbh, 16 * mbw)), rng.integers(lo, hi, (8 * mbh, 8 * mbw)), rng.integers(lo, hi, (8 * mbh, 8 * mbw)))


def random_info(rng, mbh, mbw, p_intra=0.3, p_pcm=0.1):
    """Side information of one picture as ``filter_diagonals`` reads it: every kind of macroblock next to every other."""
    intra = rng.random((mbh, mbw)) < p_intra
    pcm = intra & (rng.random((mbh, mbw)) < p_pcm / max(p_intra, 1e-9))
    nz = (rng.random((4 * mbh, 4 * mbw)) < 0.3) & ~np.repeat(np.repeat(intra, 4, axis=0), 4, axis=1)
    mv = rng.integers(-6, 7, (mbh, mbw, 2)) * ~intra[..., None]
    return dict(intra=intra, pcm=pcm, nz=nz, mv=mv.astype(np.int64))


def make_planes(kind, n, h, w, seed=0):
    if kind == FORCED_KIND:
        return I.make_planes("vramp", n, h, w, seed)
    if kind in MOVING_KINDS:
        return M.make_planes(kind, n, h, w, seed)
    return I.make_planes(kind, n, h, w, seed)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the encoder side's filter: one diagonal at a time, vectorised
# ------------------------------------------------------------------------------------------------------------------------------------
def filter_lines(lines, bs, index, chroma):
    """lines int64 [..., 8] = p3 p2 p1 p0 q0 q1 q2 q3 (chroma reads and writes only p1 p0 q0 q1), bs [...] 0 .. 4, index [...] -> the filtered lines."""
    lines = np.asarray(lines, dtype=np.int64)
    bs, index = np.broadcast_to(bs, lines.shape[:-1]), np.broadcast_to(index, lines.shape[:-1])
    p3, p2, p1, p0, q0, q1, q2, q3 = (lines[..., i] for i in range(8))
    alpha, beta = np.array(ALPHA)[index], np.array(BETA)[index]
    tc0 = np.array(TC0)[index, np.clip(bs, 1, 3) - 1]
    on = (bs > 0) & (np.abs(p0 - q0) < alpha) & (np.abs(p1 - p0) < beta) & (np.abs(q1 - q0) < beta)
    ap, aq = np.abs(p2 - p0) < beta, np.abs(q2 - q0) < beta
    if chroma:
        ap = aq = np.zeros_like(on)
    tc = tc0 + 1 if chroma else tc0 + ap + aq
    delta = np.clip((4 * (q0 - p0) + (p1 - q1) + 4) >> 3, -tc, tc)
    weak = on & (bs < 4)
    strong = on & (bs == 4)
    small = np.abs(p0 - q0) < (alpha >> 2) + 2
    sp, sq = strong & ap & small, strong & aq & small                            # (never in chroma: ap = aq = False)
    out = lines.copy()
    mid = (p0 + q0 + 1) >> 1
    out[..., 3] = np.where(weak, np.clip(p0 + delta, 0, 255), np.where(sp, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3,
                                                                       np.where(strong, (2 * p1 + p0 + q1 + 2) >> 2, p0)))
    out[..., 4] = np.where(weak, np.clip(q0 - delta, 0, 255), np.where(sq, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3,
                                                                       np.where(strong, (2 * q1 + q0 + p1 + 2) >> 2, q0)))
    out[..., 2] = np.where(weak & ap, p1 + np.clip((p2 + mid - 2 * p1) >> 1, -tc0, tc0), np.where(sp, (p2 + p1 + p0 + q0 + 2) >> 2, p1))
    out[..., 5] = np.where(weak & aq, q1 + np.clip((q2 + mid - 2 * q1) >> 1, -tc0, tc0), np.where(sq, (p0 + q0 + q1 + q2 + 2) >> 2, q1))
    out[..., 1] = np.where(sp, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, p2)
    out[..., 6] = np.where(sq, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3, q2)
    return out


def _edge_bs(info, ys, xs, dy, dx, e, dirn):
    """bS [M, 4] of edge ``e`` (in 4x4 blocks) of the macroblocks (ys, xs), one value per 4x4 block along it; the P side is the
    macroblock at (ys - dy, xs - dx) for e = 0 and the macroblock itself otherwise."""
    intra, nz, mv = info["intra"], info["nz"], info["mv"]
    pys, pxs = (ys - dy, xs - dx) if e == 0 else (ys, xs)
    along = np.arange(4)
    if dirn == 0:                                                                  # vertical edge: blocks (by = along, bx = e) against bx = e - 1
        qb = (4 * ys[:, None] + along, 4 * xs[:, None] + e)
        pb = (4 * ys[:, None] + along, 4 * xs[:, None] + e - 1)
    else:
        qb = (4 * ys[:, None] + e, 4 * xs[:, None] + along)
        pb = (4 * ys[:, None] + e - 1, 4 * xs[:, None] + along)
    either_intra = (intra[ys, xs] | intra[pys, pxs])[:, None]
    coded = nz[qb] | nz[pb]
    moved = (np.abs(mv[ys, xs].astype(np.int64) - mv[pys, pxs].astype(np.int64)) >= 4).any(axis=-1)[:, None]
    return np.where(either_intra, 4 if e == 0 else 3, np.where(coded, 2, np.where(moved, 1, 0)))


def filter_diagonals(ry, rcb, rcr, qp, info):
    """One picture's planes, filtered in place.  info: intra, pcm bool [mbh, mbw]; nz bool [4 mbh, 4 mbw]; mv int [mbh, mbw, 2] in quarter
    samples.  The macroblocks of a diagonal d = x + 2 y depend only on earlier diagonals, so each of their edges is one array operation."""
    mbh, mbw = info["intra"].shape
    qpy = np.where(info["pcm"], 0, qp)
    qpc = np.array(R.QPC)[qpy]
    planes = ((ry, 16, 4, qpy, False), (rcb, 8, 2, qpc, True), (rcr, 8, 2, qpc, True))
    for d in range(mbw + 2 * (mbh - 1)):
        ys = np.array([yy for yy in range(mbh) if 0 <= d - 2 * yy < mbw], dtype=np.int64)
        if not len(ys):
            continue
        xs = d - 2 * ys
        for plane, size, edges, q, chroma in planes:
            for dirn in (0, 1):
                dy, dx = (0, 1) if dirn == 0 else (1, 0)
                for e in range(edges):
                    le = e * (16 // edges) // 4                                    # the luma edge (in 4x4 blocks) that gives the bS
                    keep = (xs > 0) if (e == 0 and dirn == 0) else (ys > 0) if e == 0 else np.ones(len(ys), dtype=bool)
                    if not keep.any():
                        continue
                    y_, x_ = ys[keep], xs[keep]
                    bs = np.repeat(_edge_bs(info, y_, x_, dy, dx, le, dirn), size // 4, axis=1)          # [M, size]
                    py_, px_ = (y_ - dy, x_ - dx) if e == 0 else (y_, x_)
                    index = np.clip((q[y_, x_] + q[py_, px_] + 1) >> 1, 0, 51)[:, None]
                    across = 4 * e + np.arange(-4, 4) if not chroma else 4 * e + np.array([-2, -2, -2, -1, 0, 1, 1, 1])
                    line = np.arange(size)
                    if dirn == 0:
                        rows = (size * y_)[:, None, None] + line[None, :, None]
                        cols = (size * x_)[:, None, None] + across[None, None, :]
                    else:
                        rows = (size * y_)[:, None, None] + across[None, None, :]
                        cols = (size * x_)[:, None, None] + line[None, :, None]
                    rows, cols = np.broadcast_arrays(rows, cols)
                    rows, cols = np.clip(rows, 0, plane.shape[0] - 1), np.clip(cols, 0, plane.shape[1] - 1)
                    got = filter_lines(plane[rows, cols], bs, index, chroma)
                    w = slice(1, 7) if not chroma else slice(3, 5)                   # what the clauses may change
                    plane[rows[..., w], cols[..., w]] = got[..., w]


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
def lf_header(bits):
    """A slice header of the other modules with the loop filter switched on: the last three bits."""
    assert bits.endswith(R.ue(1))
    return bits[:-3] + R.ue(0) + R.se(0) + R.se(0)


def _inter_nz(sy, fy, qp):
    """Which 4x4 luma blocks of an inter macroblock keep a nonzero level (dead zone 1/6), [4, 4] by (by, bx)."""
    qbits = 15 + qp // 6
    mf = np.array(R.MF[qp % 6])[R.POS_CLASS]
    d = sy.astype(np.int64) - fy.astype(np.int64)
    out = np.zeros((4, 4), dtype=bool)
    for by in range(4):
        for bx in range(4):
            out[by, bx] = R._quant(R.CF @ d[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] @ R.CF.T, mf, (1 << qbits) // 6, qbits).any()
    return out


def _pcm_left(sy, sc):
    left = R._Left(sy[:, 15].astype(np.int64), sc[:, :, 7].astype(np.int64), np.full(4, 16), np.full((2, 2), 16))
    left.modes, left.kind = (I.DC,) * 4, "pcm"
    return left


def encode_planes(y, cb, cr, qp=16, gop=1, first_index=0, stats=None, search=0, subpel=0, intra4=0, deblock=1, force_pcm=None):
    """Padded planes -> (samples, recon Y, recon Cb, recon Cr (FILTERED), mv used in quarter samples, side information per picture).
    ``force_pcm(k, r, m)`` true codes that macroblock as I_PCM whatever the triggers say (any encoder may; the track's own triggers - more
    than 3200 bits or level_prefix > 15 - cannot fire at qp >= 31, where an I_PCM side still leaves indexA >= 16)."""
    stats = I.new_stats() if stats is None else stats
    if not deblock:
        return I.encode_planes(y, cb, cr, qp=qp, gop=gop, first_index=first_index, stats=stats, search=search, subpel=subpel, intra4=intra4) + (None,)
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    searched = search > 0 and gop > 1
    sub = subpel if searched else 0
    if searched and sub:
        mv = S.search_planes(y, qp, gop, search, sub)[0]
    elif searched:
        mv = 4 * M.search_planes(y, qp, gop, search)[0]
    else:
        mv = np.zeros((n, mbh, mbw, 2), dtype=np.int16)
    used = np.zeros((n, mbh, mbw, 2), dtype=np.int16)
    ry, rcb, rcr = np.empty_like(y), np.empty_like(cb), np.empty_like(cr)
    samples, infos = [], []
    for k in range(n):
        is_p = k % gop != 0
        info = dict(intra=np.zeros((mbh, mbw), dtype=bool), pcm=np.zeros((mbh, mbw), dtype=bool), nz=np.zeros((4 * mbh, 4 * mbw), dtype=bool),
                    mv=np.zeros((mbh, mbw, 2), dtype=np.int64))
        py_, pcb_, pcr_ = (np.empty(p.shape[1:], dtype=np.int64) for p in (y, cb, cr))
        sample = bytearray()
        for r in range(mbh):
            bits = [lf_header(P.p_slice_header(r * mbw, k % gop, qp) if is_p else R.slice_header(r * mbw, (first_index + k) & 1, qp))]
            left, run, mvp = None, 0, (0, 0)
            for m in range(mbw):
                ys, xs, yc, xc = slice(16 * r, 16 * r + 16), slice(16 * m, 16 * m + 16), slice(8 * r, 8 * r + 8), slice(8 * m, 8 * m + 8)
                sy, sc = y[k, ys, xs], np.stack([cb[k, yc, xc], cr[k, yc, xc]])
                if force_pcm is not None and force_pcm(k, r, m):
                    if is_p:
                        bits.append(R.ue(run))
                        run, mvp = 0, (0, 0)
                    mode, py, pc, left = "pcm", sy.astype(np.int64), sc.astype(np.int64), _pcm_left(sy, sc)
                elif is_p:
                    v = (int(mv[k, r, m, 0]), int(mv[k, r, m, 1]))
                    ok = S.admitted(v[0], v[1], search, sub, m, r, mbw, mbh) if sub else \
                        (not searched and v == (0, 0)) or (searched and v[0] % 4 == 0 and v[1] % 4 == 0 and M.admitted(v[0] // 4, v[1] // 4, search, m, r, mbw, mbh))
                    v = v if ok else (0, 0)
                    fy = S.inter_pred(ry[k - 1], v, 16 * m, 16 * r, 16, 0).astype(np.uint8)
                    fc = np.stack([S.inter_pred(p[k - 1], v, 8 * m, 8 * r, 8, 1) for p in (rcb, rcr)]).astype(np.uint8)
                    mode, mb, py, pc, left, mvp = S.encode_p_mb(sy, sc, fy, fc, left, mvp, v, qp, stats)
                    stats["modes"].append(mode)
                    if mode == "skip":
                        run += 1
                    else:
                        bits.append(R.ue(run))
                        run = 0
                    if mode == "inter":
                        info["nz"][4 * r:4 * r + 4, 4 * m:4 * m + 4] = _inter_nz(sy, fy, qp)
                        info["mv"][r, m] = used[k, r, m] = v
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
                py_[ys, xs] = py
                pcb_[yc, xc], pcr_[yc, xc] = pc[0], pc[1]
            if is_p and run:
                bits.append(R.ue(run))
            s = "".join(bits) + "1"
            s += "0" * (-len(s) % 8)
            rbsp = int(s, 2).to_bytes(len(s) // 8, "big")
            assert not is_p or len(rbsp) <= P.p_rbsp_bound(mbw)
            nal = bytes([0x41 if is_p else 0x65]) + R.escape(rbsp)
            assert 4 + len(nal) <= P.slot_bytes(mbw)
            sample += len(nal).to_bytes(4, "big") + nal
        samples.append(bytes(sample))
        filter_diagonals(py_, pcb_, pcr_, qp, info)
        ry[k], rcb[k], rcr[k] = py_, pcb_, pcr_
        infos.append(info)
    return samples, ry, rcb, rcr, used, infos


def mbinfo_words(infos):
    """The side information of ``encode_planes`` as the words of sdv_hip_h264_lf.h, int32 [n, mbh, mbw] (bit 18 wherever the vector is zero)."""
    out = []
    for info in infos:
        mbh, mbw = info["intra"].shape
        w = np.zeros((mbh, mbw), dtype=np.int64)
        for r in range(mbh):
            for m in range(mbw):
                if info["intra"][r, m]:
                    w[r, m] = (1 << 16) | (int(info["pcm"][r, m]) << 17)
                else:
                    nz = info["nz"][4 * r:4 * r + 4, 4 * m:4 * m + 4].reshape(-1)
                    w[r, m] = sum(1 << i for i in range(16) if nz[i]) | ((not info["mv"][r, m].any()) << 18)
        out.append(w)
    return np.stack(out).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) the decoder: slice header, picture loop, and the filter from the clauses
# ------------------------------------------------------------------------------------------------------------------------------------
def new_lf_stats():
    return dict(bs={}, pcm_filtered=0, strong_taken=0, strong_refused=0, slice_edge_changed=0, lines_changed=0)


def _line_clauses(p, q, bs, index_a, index_b, chroma, st):
    """8.7.2.2 - 8.7.2.4 for one line: p = [p0, p1, p2, p3], q = [q0, q1, q2, q3] (chroma: two each) -> (p', q', filterSamplesFlag)."""
    alpha, beta = ALPHA[index_a], BETA[index_b]
    flag = bs != 0 and abs(p[0] - q[0]) < alpha and abs(p[1] - p[0]) < beta and abs(q[1] - q[0]) < beta
    pp, qq = list(p), list(q)
    if not flag:
        return pp, qq, False
    clip3 = lambda lo, hi, v: lo if v < lo else hi if v > hi else v
    if bs < 4:                                                                     # 8.7.2.3
        tc0 = TC0[index_a][bs - 1]
        if chroma:
            tc = tc0 + 1
        else:
            ap, aq = abs(p[2] - p[0]), abs(q[2] - q[0])
            tc = tc0 + (1 if ap < beta else 0) + (1 if aq < beta else 0)
        delta = clip3(-tc, tc, (((q[0] - p[0]) << 2) + (p[1] - q[1]) + 4) >> 3)
        pp[0], qq[0] = clip3(0, 255, p[0] + delta), clip3(0, 255, q[0] - delta)
        if not chroma and ap < beta:
            pp[1] = p[1] + clip3(-tc0, tc0, (p[2] + ((p[0] + q[0] + 1) >> 1) - (p[1] << 1)) >> 1)
        if not chroma and aq < beta:
            qq[1] = q[1] + clip3(-tc0, tc0, (q[2] + ((p[0] + q[0] + 1) >> 1) - (q[1] << 1)) >> 1)
        return pp, qq, True
    if not chroma:                                                                 # 8.7.2.4
        ap, aq = abs(p[2] - p[0]), abs(q[2] - q[0])
        near = abs(p[0] - q[0]) < ((alpha >> 2) + 2)
        for side, a, x, y_ in (("p", ap, p, q), ("q", aq, q, p)):
            out = pp if side == "p" else qq
            if a < beta and near:
                out[0] = (x[2] + 2 * x[1] + 2 * x[0] + 2 * y_[0] + y_[1] + 4) >> 3
                out[1] = (x[2] + x[1] + x[0] + y_[0] + 2) >> 2
                out[2] = (2 * x[3] + 3 * x[2] + x[1] + x[0] + y_[0] + 4) >> 3
                st["strong_taken"] += 1
            else:
                out[0] = (2 * x[1] + x[0] + y_[1] + 2) >> 2
                st["strong_refused"] += 1
        return pp, qq, True
    pp[0], qq[0] = (2 * p[1] + p[0] + q[1] + 2) >> 2, (2 * q[1] + q[0] + p[1] + 2) >> 2
    return pp, qq, True


def deblock_picture(pic, qp, st, directions=(0, 1)):
    """8.7 on a decoded picture (h264_p_ref._Picture with ``pcm``: the set of its I_PCM macroblocks), in place, from what the decoder
    parsed: ``ref`` (-1 = intra), ``nz_y`` (TotalCoeff of every 4x4 luma block), ``mv``, ``slice_of``.  ``directions``: (0, 1) is the
    standard's filter; (0,) or (1,) leaves out the horizontal or the vertical edges (for a symmetry test)."""
    mbw, mbh = pic.mbw, pic.mbh
    intra = lambda mb: pic.ref[mb] < 0
    qpy = lambda mb: 0 if mb in pic.pcm else qp
    for mb in range(mbw * mbh):
        my, mx = divmod(mb, mbw)
        for plane_no in range(3):                                                  # luma, Cb, Cr
            chroma = plane_no > 0
            plane = pic.Y if not chroma else pic.C[plane_no - 1]
            size, n_edges, reach = (16, 4, 4) if not chroma else (8, 2, 2)
            for dirn in directions:                                                # vertical edges, then horizontal edges
                for e in range(n_edges):
                    if e == 0 and (mx == 0 if dirn == 0 else my == 0):
                        continue                                                   # filterLeftMbEdgeFlag / filterTopMbEdgeFlag = 0 at the picture edge
                    other = mb if e else (mb - 1 if dirn == 0 else mb - mbw)
                    for k in range(size):
                        # the luma samples q0 / p0 of this line (chroma sample k of chroma edge e sits over luma line 2 k of luma edge 2 e)
                        lk, le = (k, 4 * e) if not chroma else (2 * k, 8 * e)
                        qy, qx = (16 * my + lk, 16 * mx + le) if dirn == 0 else (16 * my + le, 16 * mx + lk)
                        py, px = (qy, qx - 1) if dirn == 0 else (qy - 1, qx)
                        if intra(mb) or intra(other):
                            bs = 4 if e == 0 else 3
                        elif pic.nz_y[qy // 4, qx // 4] != 0 or pic.nz_y[py // 4, px // 4] != 0:
                            bs = 2
                        elif abs(pic.mv[mb][0] - pic.mv[other][0]) >= 4 or abs(pic.mv[mb][1] - pic.mv[other][1]) >= 4:
                            bs = 1
                        else:
                            bs = 0
                        key = (("y", "cb", "cr")[plane_no], "v" if dirn == 0 else "h", bs)
                        st["bs"][key] = st["bs"].get(key, 0) + 1
                        if bs == 0:
                            continue
                        qa, qb = qpy(other), qpy(mb)
                        if chroma:
                            qa, qb = R.QPC[qa], R.QPC[qb]
                        index = min(51, max(0, (qa + qb + 1) >> 1))
                        y0, x0 = size * my, size * mx
                        if dirn == 0:
                            at_q = [(y0 + k, x0 + 4 * e + i) for i in range(reach)]
                            at_p = [(y0 + k, x0 + 4 * e - 1 - i) for i in range(reach)]
                        else:
                            at_q = [(y0 + 4 * e + i, x0 + k) for i in range(reach)]
                            at_p = [(y0 + 4 * e - 1 - i, x0 + k) for i in range(reach)]
                        p, q = [int(plane[a]) for a in at_p], [int(plane[a]) for a in at_q]
                        pp, qq, flag = _line_clauses(p, q, bs, index, index, chroma, st)
                        if flag and index >= 16 and (mb in pic.pcm or other in pic.pcm):
                            st["pcm_filtered"] += 1
                        if pp != p or qq != q:
                            st["lines_changed"] += 1
                            if e == 0 and dirn == 1 and pic.slice_of[mb] != pic.slice_of[other]:
                                st["slice_edge_changed"] += 1
                        for a, v in zip(at_p + at_q, pp + qq):
                            plane[a] = v


def _decode_picture(sample, mbw, mbh, ref_pic, pic_init_qp=26):
    """h264_i4_ref._decode_picture with a slice header reader that knows disable_deblocking_filter_idc 0 and its two offsets, the set of
    I_PCM macroblocks, and the loop filter after the last slice.  Every macroblock goes through the other modules' functions."""
    pic = P._Picture(mbw, mbh)
    pic.pcm = set()
    blk, modes = I._i4_state(pic)
    headers, at, slice_no = [], 0, 0
    slice_qp = None
    while at < len(sample):
        size = int.from_bytes(sample[at:at + 4], "big")
        nal = sample[at + 4:at + 4 + size]
        at += 4 + size
        assert nal[0] >> 7 == 0 and nal[-1] != 0
        ref_idc, unit_type = (nal[0] >> 5) & 3, nal[0] & 31
        assert unit_type in (1, 5) and ref_idc != 0, "every picture is a reference picture"
        rd = R.BitReader(R.unescape(nal[1:]))
        hd = dict(nal_unit_type=unit_type, nal_ref_idc=ref_idc, first_mb=rd.ue(), slice_type=rd.ue(), pps_id=rd.ue(), frame_num=rd.u(4), nal_bytes=size)
        is_p = hd["slice_type"] % 5 == 0
        assert is_p or hd["slice_type"] % 5 == 2, "P and I slices only"
        assert not (unit_type == 5 and is_p), "an IDR picture has I slices only"
        if unit_type == 5:
            hd["idr_pic_id"] = rd.ue()
        if is_p:
            if rd.u(1):
                assert rd.ue() == 0, "one active reference only"
            assert rd.u(1) == 0, "ref_pic_list_modification is not decoded here"
        if unit_type == 5:
            hd["no_output"], hd["long_term"] = rd.u(1), rd.u(1)
        else:
            assert rd.u(1) == 0, "adaptive_ref_pic_marking_mode_flag 1 is not decoded here"
        hd["qp_delta"] = rd.se()
        hd["deblock_idc"] = rd.ue()                                        # deblocking_filter_control_present_flag is 1
        if hd["deblock_idc"] != 1:
            hd["alpha_offset_div2"], hd["beta_offset_div2"] = rd.se(), rd.se()
        assert hd["deblock_idc"] == 0 and hd["alpha_offset_div2"] == 0 and hd["beta_offset_div2"] == 0, "this decoder filters with idc 0 and no offsets"
        headers.append(hd)
        qp = pic_init_qp + hd["qp_delta"]
        assert slice_qp in (None, qp)
        slice_qp = qp
        mb = hd["first_mb"]
        more = True

        def done(m):
            y4, x4 = divmod(m, mbw)
            blk[4 * y4:4 * y4 + 4, 4 * x4:4 * x4 + 4] = slice_no

        while more:                                                     # 7.3.4
            if is_p:
                run = rd.ue()
                hd.setdefault("skip_runs", []).append(run)
                for _ in range(run):
                    assert ref_pic is not None
                    pic.slice_of[mb] = slice_no
                    P._decode_inter(rd, pic, ref_pic, mb, P._mv_skip(pic, mb, slice_no), 0, qp, False, False)
                    pic.n_skip += 1
                    done(mb)
                    mb += 1
                if run > 0:
                    more = rd.more_rbsp_data()
            if more:
                my, mx = divmod(mb, mbw)
                pic.slice_of[mb] = slice_no
                avail_a = mx > 0 and pic.slice_of[mb - 1] == slice_no
                avail_b = my > 0 and pic.slice_of[mb - mbw] == slice_no
                mb_type = rd.ue()
                if is_p and mb_type < 5:
                    assert mb_type == 0, "only P_L0_16x16 of the inter types is decoded here"
                    assert ref_pic is not None
                    mvp = P._mv_pred_16x16(pic, mb, slice_no)
                    mv = (mvp[0] + rd.se(), mvp[1] + rd.se())
                    code = rd.ue()
                    assert code < 48
                    qp = P._decode_inter(rd, pic, ref_pic, mb, mv, P.CBP_INTER[code], qp, avail_a, avail_b)
                    pic.n_inter += 1
                else:
                    t = mb_type - 5 if is_p else mb_type
                    if t == 25:
                        P._decode_pcm(rd, pic, mb)
                        pic.pcm.add(mb)
                    elif t == 0:
                        qp = I._decode_i4(rd, pic, mb, slice_no, qp, avail_a, avail_b)
                        hd["n_i4"] = hd.get("n_i4", 0) + 1
                    else:
                        assert 1 <= t <= 24
                        qp = P._decode_intra16(rd, pic, mb, t, qp, avail_a, avail_b)
                        pic.n_intra += 1
                    assert pic.ref[mb] == -1
                assert qp == slice_qp, "the track never sends a nonzero mb_qp_delta"
                done(mb)
                mb += 1
                more = rd.more_rbsp_data()
        slice_no += 1
    assert all(s >= 0 for s in pic.slice_of), "a macroblock was never coded"
    deblock_picture(pic, slice_qp, decode_stream.stats)
    I.decode_stream.pictures.append(pic)
    return pic, headers


def decode_stream(samples, width, height, stats=None):
    """h264_i4_ref.decode_stream's result for a stream with the loop filter on: every picture filtered before it is shown and before it is
    predicted from.  ``stats`` (``new_lf_stats``) takes what the filter met."""
    decode_stream.stats = new_lf_stats() if stats is None else stats
    with mock.patch.object(I, "_decode_picture", _decode_picture):
        out = I.decode_stream(samples, width, height)
    out["lf"] = decode_stream.stats
    return out


decode_stream.stats = new_lf_stats()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, qp, setting=(1, 0, 0, 0), deblock=1):
    """(planes, samples, (ry, rcb, rcr), mv used, side information) of one case, computed once for all the tests that read it."""
    n, h, w = shape
    gop, search, subpel, intra4 = setting
    planes = make_planes(kind, n, h, w)
    force = (lambda k, r, m: (k + r + 2 * m) % 3 == 0) if kind == FORCED_KIND else None
    samples, ry, rcb, rcr, used, infos = encode_planes(*planes, qp=qp, gop=gop, first_index=FIRST, search=search, subpel=subpel, intra4=intra4,
                                                       deblock=deblock, force_pcm=force)
    return planes, samples, (ry, rcb, rcr), used, infos
