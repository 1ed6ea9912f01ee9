"""Macroblock partitions of the H.264 track (include/sdv_hip_h264_part.h, DESIGN.md "H.264 partitions") restated in plain Python / numpy on
top of h264_lf_ref.py, h264_i4_ref.py, h264_sub_ref.py, h264_me_ref.py, h264_p_ref.py and h264_ref.py, none of which is edited.  Nothing
here imports the package's encoder.

The rule, restated.  Setting part 1 on top of gop > 1 and search > 0 (otherwise the other modules' stream, byte for byte).
  Vectors.  Four per inter macroblock, one per 8x8 luma quadrant (mbPartIdx 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right), always
  in quarter luma samples, tensor int16 [n][mbh][mbw][4][2].  Grid: subpel 0 multiples of 8 quarter units, subpel 1, 2, 4 multiples of
  4 / subpel; |v| <= 4 search; admission is the macroblock's 16x16 rule for all four.
  Type.  Four equal vectors: P_Skip (cbp 0 and v = (0, 0)) or P_L0_16x16 as before.  Else P_8x8: mb_type ue(3), four sub_mb_type ue(0), no
  ref_idx, mvd_l0 x then y for partitions 0 .. 3, coded_block_pattern me(v) inter column, mb_qp_delta only with cbp != 0, the residual.
  Vector prediction (8.4.1.3), the row above being another slice: partition 0: the left macroblock's top-right 8x8 ((0, 0) when absent,
  intra or P_Skip); 1: v0; 2: median(left macroblock's bottom-right 8x8 or (0, 0), v0, v1); 3: median(v2, v1, v0).  A P_L0_16x16
  macroblock right of a P_8x8 predicts from its partition 1; P_Skip infers (0, 0).
  Prediction per partition: luma 8.4.2.2.1 on 8x8, chroma 8.4.2.2.2 on 4x4, coordinates clamped.
  Mode: sad_inter over the four displaced partitions; intra iff sad_intra < sad_inter.  The counting pass includes the real syntax bits.
  Search on source pictures: stage 1 exhaustive over the admitted whole-sample vectors (subpel 0: the even ones) keeping the quadrant SADs;
  cost8_q(v) = SAD_q(v) + lambda (B(vx) + B(vy)), order (cost, |vx| + |vy|, vy, vx); stages 2 / 3 refine each quadrant winner (and, as
  before, the 16x16 winner w16) at +- 2 and +- 1 quarter samples on its own samples.  The quadrant winners are taken iff
  sum_q cost8_q + 8 lambda < cost16(w16), else w16 four times.
  Loop filter: bS as before, the vectors compared per 4x4 block pair between the partitions the two blocks lie in.

(a) ``search_planes``; (b) ``encode_planes(..., part=1, mv=None)`` with ``inject`` / ``plant`` for vectors that are not searched;
(c) ``decode_stream``: a picture loop with its own ``sub_mb_pred`` reader, the general A / B / C / D neighbour derivation of 8.4.1.3 on the
    picture's grid of 8x8 partitions (``_mv_pred``: availability = inside the picture, already decoded, same slice - not the four cases
    above), per-partition prediction and a loop filter that reads the vectors per 4x4 block; it refuses every other inter type.  It
    counts what it meets (``new_part_stats``).
"""
import functools
from unittest import mock

import numpy as np

import h264_i4_ref as I
import h264_lf_ref as L
import h264_me_ref as M
import h264_p_ref as P
import h264_ref as R
import h264_sub_ref as S

SUBPELS = (0, 1, 2, 4)
FIRST = P.FIRST
LAMBDA = M.LAMBDA
SHAPES = ((3, 16, 16), (3, 16, 64), (3, 64, 16), (4, 48, 64), (3, 96, 128), (3, 36, 50))      # one macroblock, a row, a column, 3x4, 6x8, padded
QPS = (0, 16, 28, 40, 51)
FILTERS = ((0, 0), (1, 1))                                                         # (intra4, deblock)
SEARCH = 8
# the case set: (kind, injected) - three searched kinds and three kinds of injected vectors on planted content
KINDS = (("split8", None), ("still", None), ("noise", None), ("planted", "mixed"), ("planted", "far"), ("planted", "invalid"))
CASES = [(s, k, i) for s in SHAPES for k, i in KINDS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{i or k}" for s, k, i in CASES]


def admitted(vx, vy, search, subpel, mx, my, mbw, mbh):
    if subpel == 0:
        return vx % 8 == 0 and vy % 8 == 0 and S.admitted(vx, vy, search, 1, mx, my, mbw, mbh)
    return S.admitted(vx, vy, search, subpel, mx, my, mbw, mbh)


def median3(a, b, c):
    return sorted((a, b, c))[1]


def part_pred(ref, vs, x0, y0, size, shift):
    """The macroblock's prediction in one plane from four vectors: partition i covers the quadrant at (size / 2) (i & 1, i >> 1)."""
    h = size // 2
    out = np.empty((size, size), dtype=np.int64)
    for i, v in enumerate(vs):
        ox, oy = h * (i & 1), h * (i >> 1)
        out[oy:oy + h, ox:ox + h] = S.inter_pred(ref, v, x0 + ox, y0 + oy, h, shift)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# frame kinds
# ------------------------------------------------------------------------------------------------------------------------------------
def split_frames(s, n, h, w):
    """h264_sub_ref.glide_frames whose upper 8 rows of every macroblock row glide right by s quarter samples a picture and whose lower 8
    rows glide left: two motions inside every macroblock."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sign = np.where(yy.astype(np.int64) % 16 < 8, 1.0, -1.0)
    frames = np.empty((n, h, w, 3), dtype=np.uint8)
    for k in range(n):
        x = xx - sign * k * s / 4.0
        v = 128 + 38 * np.sin(2 * np.pi * x / 11 + 0.3) + 30 * np.sin(2 * np.pi * (x / 7.3 + yy / 19)) + 24 * np.sin(2 * np.pi * yy / 9 + 1.0) \
            + 20 * np.sin(2 * np.pi * (x / 23 - yy / 13))
        c = 128 + 50 * np.sin(2 * np.pi * (x / 29 + yy / 37) + 0.7)
        frames[k] = np.clip(np.rint(np.stack([v, 0.5 * v + 0.5 * c, c], axis=-1)), 0, 255).astype(np.uint8)
    return frames


def make_planes(kind, n, h, w, seed=0):
    if kind.startswith("split"):
        return R.rgb_to_planes(split_frames(int(kind[5:]), n, h, w))
    if kind == "flat":
        return I.make_planes("flat", n, h, w, seed)
    return S.make_planes(kind, n, h, w, seed)


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the search
# ------------------------------------------------------------------------------------------------------------------------------------
def _refine(win, block, prev, x0, y0, size, lam, search, subpel, mx, my, mbw, mbh):
    for step in (2, 1):
        if step * subpel < 4:
            continue
        cx, cy = win[3], win[2]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                vx, vy = cx + step * dx, cy + step * dy
                if (dx, dy) == (0, 0) or not admitted(vx, vy, search, subpel, mx, my, mbw, mbh):
                    continue
                s = int(np.abs(block - S._luma_pred(prev, (vx, vy), x0, y0, size)).sum())
                win = min(win, S._key(s, lam, vx, vy))
    return win


def search_planes(y, qp, gop, search, subpel):
    """Source luma -> (mv int16 [n, mbh, mbw, 4, 2] quarter samples, sad int32 [n, mbh, mbw, 5]: the quadrant winners' and w16's source SAD,
    taken bool [n, mbh, mbw]: the quadrant winners were written).  Zeros for the IDR pictures."""
    assert subpel in SUBPELS
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    mv, sad = np.zeros((n, mbh, mbw, 4, 2), dtype=np.int16), np.zeros((n, mbh, mbw, 5), dtype=np.int32)
    taken = np.zeros((n, mbh, mbw), dtype=bool)
    lam = LAMBDA[qp]
    for k in range(n):
        if k % gop == 0:
            continue
        cur, prev = y[k].astype(np.int64), y[k - 1].astype(np.int64)
        ref = np.zeros((hh + 2 * search, ww + 2 * search), dtype=np.int64)
        ref[search:search + hh, search:search + ww] = prev
        best = [[[None] * 5 for _ in range(mbw)] for _ in range(mbh)]
        for vy in range(-search, search + 1, 1 if subpel else 2):
            for vx in range(-search, search + 1, 1 if subpel else 2):
                diff = np.abs(cur - ref[search + vy:search + vy + hh, search + vx:search + vx + ww])
                q = diff.reshape(mbh, 2, 8, mbw, 2, 8).sum(axis=(2, 5))             # [mbh, qy, mbw, qx]
                for my in range(mbh):
                    for mx in range(mbw):
                        if not admitted(4 * vx, 4 * vy, search, subpel and 1, mx, my, mbw, mbh):
                            continue
                        s4 = [int(q[my, i >> 1, mx, i & 1]) for i in range(4)]
                        for i, s in enumerate(s4 + [sum(s4)]):
                            key = S._key(s, lam, 4 * vx, 4 * vy)
                            if best[my][mx][i] is None or key < best[my][mx][i]:
                                best[my][mx][i] = key
        for my in range(mbh):
            for mx in range(mbw):
                b = best[my][mx]
                block = cur[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
                w16 = _refine(b[4], block, prev, 16 * mx, 16 * my, 16, lam, search, subpel, mx, my, mbw, mbh)
                w8 = [_refine(b[i], block[8 * (i >> 1):8 * (i >> 1) + 8, 8 * (i & 1):8 * (i & 1) + 8], prev, 16 * mx + 8 * (i & 1), 16 * my + 8 * (i >> 1), 8,
                              lam, search, subpel, mx, my, mbw, mbh) for i in range(4)]
                take = sum(w[0] for w in w8) + 8 * lam < w16[0]
                taken[k, my, mx] = take
                for i in range(4):
                    w = w8[i] if take else w16
                    mv[k, my, mx, i] = (w[3], w[2])
                    sad[k, my, mx, i] = w8[i][4]
                sad[k, my, mx, 4] = w16[4]
    return mv, sad, taken


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    st = I.new_stats()
    st.update(p8x8=0, p8x8_cbp0=0, refused_one=0, refused=0, equal4=0)
    return st


def _edge_bs4(info, ys, xs, dy, dx, e, dirn):
    """h264_lf_ref._edge_bs with one vector per 4x4 block (info["mv4"] [4 mbh, 4 mbw, 2]): the blocks on either side of the edge."""
    intra, nz, mv4 = info["intra"], info["nz"], info["mv4"]
    pys, pxs = (ys - dy, xs - dx) if e == 0 else (ys, xs)
    along = np.arange(4)
    if dirn == 0:
        qb = (4 * ys[:, None] + along, 4 * xs[:, None] + e)
        pb = (4 * ys[:, None] + along, 4 * xs[:, None] + e - 1)
    else:
        qb = (4 * ys[:, None] + e, 4 * xs[:, None] + along)
        pb = (4 * ys[:, None] + e - 1, 4 * xs[:, None] + along)
    either_intra = (intra[ys, xs] | intra[pys, pxs])[:, None]
    coded = nz[qb] | nz[pb]
    moved = (np.abs(mv4[qb].astype(np.int64) - mv4[pb].astype(np.int64)) >= 4).any(axis=-1)
    return np.where(either_intra, 4 if e == 0 else 3, np.where(coded, 2, np.where(moved, 1, 0)))


def filter_picture(ry, rcb, rcr, qp, info):
    """h264_lf_ref.filter_diagonals with the bS of four vectors a macroblock."""
    with mock.patch.object(L, "_edge_bs", _edge_bs4):
        L.filter_diagonals(ry, rcb, rcr, qp, info)


def encode_p8x8(sy, sc, fy, fc, left, chain, vs, qp, stats):
    """One inter-predicted macroblock whose four vectors differ -> (mode, bits, recon Y, recon C, _Left, new chain).  chain: the vectors of the
    left macroblock's partitions 1 and 3 ((0, 0) where it is absent, intra, I_PCM or P_Skip)."""
    probe = P.new_stats()
    mode, bits, ry, rc, new_left = P.encode_p_mb(sy, sc, fy, fc, left, qp, probe)
    for key in ("inter_cbp_luma", "inter_cbp_chroma", "pcm_in_p"):
        stats[key] |= probe[key]
    if mode in ("intra", "pcm"):
        return mode, bits, ry, rc, new_left, ((0, 0), (0, 0))
    mvp = (chain[0], vs[0], tuple(median3(chain[1][c], vs[0][c], vs[1][c]) for c in range(2)), tuple(median3(vs[2][c], vs[1][c], vs[0][c]) for c in range(2)))
    head = R.ue(3) + R.ue(0) * 4 + "".join(R.se(vs[i][0] - mvp[i][0]) + R.se(vs[i][1] - mvp[i][1]) for i in range(4))
    if mode == "skip":                                                             # cbp 0: coded_block_pattern codeNum 0, no mb_qp_delta
        bits = head + R.ue(0)
        stats["p8x8_cbp0"] += 1
    else:
        assert bits[:3] == "111"
        bits = head + bits[3:]
        if len(bits) > R.MAX_MB_BITS:                                              # the counting pass includes the real syntax bits
            stats["pcm_in_p"].add("bits")
            sy, sc = sy.astype(np.int64), sc.astype(np.int64)
            return "pcm", None, sy, sc, R._Left(sy[:, 15].copy(), sc[:, :, 7].copy(), np.full(4, 16), np.full((2, 2), 16)), ((0, 0), (0, 0))
    stats["p8x8"] += 1
    return "inter", bits, ry, rc, new_left, (vs[1], vs[3])


def encode_planes(y, cb, cr, qp=16, gop=1, first_index=0, stats=None, search=0, subpel=0, intra4=0, deblock=0, part=1, mv=None):
    """Padded planes -> (samples, recon Y, recon Cb, recon Cr, mv used int16 [n, mbh, mbw, 4, 2] quarter samples, side information per
    picture or None).  ``mv`` None: the searched vectors; else injected ones, each coded as (0, 0) where the rule does not admit it."""
    stats = new_stats() if stats is None else stats
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    if not (part and gop > 1 and search > 0):
        assert mv is None
        out = L.encode_planes(y, cb, cr, qp=qp, gop=gop, first_index=first_index, stats=stats, search=search, subpel=subpel, intra4=intra4, deblock=deblock)
        used = np.repeat(np.asarray(out[4])[:, :, :, None, :], 4, axis=3).astype(np.int16)          # (every module returns quarter samples)
        return out[0], out[1], out[2], out[3], used, out[5]
    if mv is None:
        mv = search_planes(y, qp, gop, search, subpel)[0]
    used = np.zeros((n, mbh, mbw, 4, 2), dtype=np.int16)
    ry, rcb, rcr = np.empty_like(y), np.empty_like(cb), np.empty_like(cr)
    samples, infos = [], []
    for k in range(n):
        is_p = k % gop != 0
        info = dict(intra=np.zeros((mbh, mbw), dtype=bool), pcm=np.zeros((mbh, mbw), dtype=bool), nz=np.zeros((4 * mbh, 4 * mbw), dtype=bool),
                    mv4=np.zeros((4 * mbh, 4 * mbw, 2), dtype=np.int64), mv=np.zeros((mbh, mbw, 4, 2), dtype=np.int64))
        py_, pcb_, pcr_ = (np.empty(p.shape[1:], dtype=np.int64) for p in (y, cb, cr))
        sample = bytearray()
        for r in range(mbh):
            hdr = P.p_slice_header(r * mbw, k % gop, qp) if is_p else R.slice_header(r * mbw, (first_index + k) & 1, qp)
            bits = [L.lf_header(hdr) if deblock else hdr]
            left, run, chain = None, 0, ((0, 0), (0, 0))
            for m in range(mbw):
                ys, xs, yc, xc = slice(16 * r, 16 * r + 16), slice(16 * m, 16 * m + 16), slice(8 * r, 8 * r + 8), slice(8 * m, 8 * m + 8)
                sy, sc = y[k, ys, xs], np.stack([cb[k, yc, xc], cr[k, yc, xc]])
                if is_p:
                    vs = [(int(mv[k, r, m, i, 0]), int(mv[k, r, m, i, 1])) for i in range(4)]
                    ok = [admitted(v[0], v[1], search, subpel, m, r, mbw, mbh) for v in vs]
                    stats["refused"] += 4 - sum(ok)
                    stats["refused_one"] += sum(ok) == 3
                    vs = tuple(v if o else (0, 0) for v, o in zip(vs, ok))
                    fy = part_pred(ry[k - 1], vs, 16 * m, 16 * r, 16, 0).astype(np.uint8)
                    fc = np.stack([part_pred(p[k - 1], vs, 8 * m, 8 * r, 8, 1) for p in (rcb, rcr)]).astype(np.uint8)
                    if len(set(vs)) == 1:
                        stats["equal4"] += 1
                        mode, mb, py, pc, left, mvp = S.encode_p_mb(sy, sc, fy, fc, left, chain[0], vs[0], qp, stats)
                        chain = (mvp, mvp)
                    else:
                        mode, mb, py, pc, left, chain = encode_p8x8(sy, sc, fy, fc, left, chain, vs, qp, stats)
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
            assert not is_p or len(rbsp) <= P.p_rbsp_bound(mbw)
            nal = bytes([0x41 if is_p else 0x65]) + R.escape(rbsp)
            assert 4 + len(nal) <= P.slot_bytes(mbw)
            sample += len(nal).to_bytes(4, "big") + nal
        samples.append(bytes(sample))
        if deblock:
            filter_picture(py_, pcb_, pcr_, qp, info)
        ry[k], rcb[k], rcr[k] = py_, pcb_, pcr_
        infos.append(info)
    return samples, ry, rcb, rcr, used, (infos if deblock else None)


def mbinfo_words(infos):
    """The side information as the words of sdv_hip_h264_part.h, int32 [n, mbh, mbw]: bit 18 where all four vectors are zero, bits 19 .. 22
    per partition (inter and skipped macroblocks)."""
    out = []
    for info in infos:
        mbh, mbw = info["intra"].shape
        w = np.zeros((mbh, mbw), dtype=np.int64)
        for r in range(mbh):
            for m in range(mbw):
                if info["intra"][r, m]:
                    w[r, m] = (1 << 16) | (int(info["pcm"][r, m]) << 17)
                    continue
                nz = info["nz"][4 * r:4 * r + 4, 4 * m:4 * m + 4].reshape(-1)
                w[r, m] = sum(1 << i for i in range(16) if nz[i]) | ((not info["mv"][r, m].any()) << 18)
                if "mv4" in info:
                    w[r, m] |= sum(1 << (19 + i) for i in range(4) if not info["mv"][r, m, i].any())
        out.append(w)
    return np.stack(out).astype(np.int32)


INVALID = ((1, 0), (0, -3), (2, 6), (4, 2), (32767, 4), (4, -32768), (64, 64), (-64, 0), (0, 65), (3, 3), (8, 0), (0, -8))


def inject(kind, n, mbh, mbw, search, subpel, seed=0):
    """Four vectors a macroblock that are not searched, int16 [n, mbh, mbw, 4, 2].  ``mixed``: by (k + r + m) % 6 - four different admitted
    vectors | one admitted vector four times | zeros | four different | two and two (partitions 0 = 1, 2 = 3) | zeros; ``invalid``:
    admitted random vectors with, in every other macroblock, exactly one partition's replaced by one of INVALID (off grid for some subpel,
    out of range or not admitted); ``far``: partitions 0 .. 3 spread so that the median of partition 3 mixes components."""
    rng = np.random.default_rng(seed)
    step = 8 if subpel == 0 else 4 // subpel
    mv = np.zeros((n, mbh, mbw, 4, 2), dtype=np.int16)
    for k in range(n):
        for r in range(mbh):
            for m in range(mbw):
                c = [v for v in S.candidates(min(search, 2), 4, m, r, mbw, mbh) if v[0] % step == 0 and v[1] % step == 0]
                pick = lambda: c[int(rng.integers(len(c)))]
                i = (k + r + m) % 6
                if kind == "mixed":
                    vs = [pick() for _ in range(4)] if i in (0, 3) else [pick()] * 4 if i == 1 else [pick()] * 2 + [pick()] * 2 if i == 4 else [(0, 0)] * 4
                elif kind == "far":
                    a, b = pick(), pick()
                    vs = [(a[0], b[1]), (b[0], a[1]), (a[1] if (a[1], 0) in c else 0, b[0] if (0, b[0]) in c else 0), pick()]
                elif kind == "invalid":
                    vs = [pick() for _ in range(4)]
                    if (r + m) % 2 == 0:
                        vs[(k + m) % 4] = INVALID[(k + 3 * r + 5 * m) % len(INVALID)]
                else:
                    raise ValueError(kind)
                mv[k, r, m] = vs
    return mv


def plant(n, h, w, mv, search, subpel, seed=0, fresh=M.fresh):
    """h264_sub_ref.plant with four vectors a macroblock: every 8x8 quadrant of macroblock (r, m) of picture k is the PREDICTION of that
    quadrant from picture k - 1 by its vector ((0, 0) where the rule does not admit it) - except the ``fresh`` macroblocks, new noise."""
    y0, cb0, cr0 = R.rgb_to_planes(R.make_frames("noise", 1, h, w, seed))
    mbh, mbw = y0.shape[1] // 16, y0.shape[2] // 16
    noise = R.rgb_to_planes(R.make_frames("noise", n, 16 * mbh, 16 * mbw, seed + 1))
    planes = [np.repeat(p, n, axis=0) for p in (y0, cb0, cr0)]
    for k in range(1, n):
        for r in range(mbh):
            for m in range(mbw):
                vs = [(int(v[0]), int(v[1])) for v in mv[k, r, m]]
                vs = [v if admitted(v[0], v[1], search, subpel, m, r, mbw, mbh) else (0, 0) for v in vs]
                for p, q, size, shift in zip(planes, noise, (16, 8, 8), (0, 1, 1)):
                    ya, xa = size * r, size * m
                    if fresh(k, r, m):
                        p[k, ya:ya + size, xa:xa + size] = q[k, ya:ya + size, xa:xa + size]
                    else:
                        p[k, ya:ya + size, xa:xa + size] = part_pred(p[k - 1], vs, xa, ya, size, shift)
    return tuple(planes)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the decoder
# ------------------------------------------------------------------------------------------------------------------------------------
def new_part_stats():
    return dict(p8x8=0, p8x8_cbp0=0, p8x8_cbp=0, p8x8_first=0, p8x8_after=set(), l16_after_split=0, part2_a=set(), part3_mixed=0, lf_inner8=set(),
                lf_half=0, lf_inner8_bs2=0, kinds=set())


def _grid(pic):
    """Per 8x8 partition of the picture: its vector, its refIdxL0 (-1 intra) and the slice it was decoded in (-1: not yet)."""
    if not hasattr(pic, "mv8"):
        pic.mv8 = np.zeros((2 * pic.mbh, 2 * pic.mbw, 2), dtype=np.int64)
        pic.ref8 = np.full((2 * pic.mbh, 2 * pic.mbw), -1, dtype=np.int64)
        pic.slice8 = np.full((2 * pic.mbh, 2 * pic.mbw), -1, dtype=np.int64)
        pic.kind = [None] * (pic.mbw * pic.mbh)
    return pic.mv8, pic.ref8, pic.slice8


def _nb(pic, gx, gy, slice_no):
    """(available, refIdx, mv) of the 8x8 partition at grid position (gx, gy): in the picture, already decoded, in this slice (6.4.11.7)."""
    mv8, ref8, slice8 = _grid(pic)
    if not (0 <= gx < 2 * pic.mbw and 0 <= gy < 2 * pic.mbh) or slice8[gy, gx] != slice_no:
        return False, -1, (0, 0)
    return True, int(ref8[gy, gx]), (int(mv8[gy, gx, 0]), int(mv8[gy, gx, 1]))


def _mv_pred(pic, gx, gy, width, slice_no, note=None):
    """8.4.1.3 for a partition whose top-left 8x8 lies at grid (gx, gy) and that is ``width`` 8x8 units wide, refIdxL0 0."""
    a, b, c, d = _nb(pic, gx - 1, gy, slice_no), _nb(pic, gx, gy - 1, slice_no), _nb(pic, gx + width, gy - 1, slice_no), _nb(pic, gx - 1, gy - 1, slice_no)
    if not c[0]:
        c = d
    if not b[0] and not c[0] and a[0]:
        b = c = a
    if note is not None:
        note(a, b, c)
    same = [x for x in (a, b, c) if x[1] == 0]
    if len(same) == 1:
        return same[0][2]
    return P._median(a[2][0], b[2][0], c[2][0]), P._median(a[2][1], b[2][1], c[2][1])


def _mv_skip(pic, mx, my, slice_no):
    a, b = _nb(pic, 2 * mx - 1, 2 * my, slice_no), _nb(pic, 2 * mx, 2 * my - 1, slice_no)
    if not a[0] or not b[0] or (a[1] == 0 and a[2] == (0, 0)) or (b[1] == 0 and b[2] == (0, 0)):
        return 0, 0
    return _mv_pred(pic, 2 * mx, 2 * my, 2, slice_no)


def _pred_any(ref, mv, x0, y0, size, shift):
    """h264_p_ref._inter_pred for one vector or for a tuple of four: per-partition prediction."""
    if isinstance(mv[0], tuple):
        return part_pred(ref, mv, x0, y0, size, shift)
    return S.inter_pred(ref, mv, x0, y0, size, shift)


def _set(pic, mb, slice_no, vs, ref, kind):
    mv8, ref8, slice8 = _grid(pic)
    my, mx = divmod(mb, pic.mbw)
    for i in range(4):
        mv8[2 * my + (i >> 1), 2 * mx + (i & 1)] = vs[i]
    ref8[2 * my:2 * my + 2, 2 * mx:2 * mx + 2] = ref
    slice8[2 * my:2 * my + 2, 2 * mx:2 * mx + 2] = slice_no
    pic.kind[mb] = kind


def deblock_picture(pic, qp, st, pst):
    """8.7 on a decoded picture as h264_lf_ref.deblock_picture does it, with the vectors read per 4x4 block from the grid of 8x8 partitions."""
    mbw, mbh = pic.mbw, pic.mbh
    mv8 = pic.mv8
    intra = lambda mb: pic.ref[mb] < 0
    qpy = lambda mb: 0 if mb in pic.pcm else qp
    for mb in range(mbw * mbh):
        my, mx = divmod(mb, mbw)
        for plane_no in range(3):
            chroma = plane_no > 0
            plane = pic.Y if not chroma else pic.C[plane_no - 1]
            size, n_edges, reach = (16, 4, 4) if not chroma else (8, 2, 2)
            for dirn in (0, 1):
                for e in range(n_edges):
                    if e == 0 and (mx == 0 if dirn == 0 else my == 0):
                        continue
                    other = mb if e else (mb - 1 if dirn == 0 else mb - mbw)
                    halves = [set(), set()]
                    for k in range(size):
                        lk, le = (k, 4 * e) if not chroma else (2 * k, 8 * e)
                        qy, qx = (16 * my + lk, 16 * mx + le) if dirn == 0 else (16 * my + le, 16 * mx + lk)
                        py, px = (qy, qx - 1) if dirn == 0 else (qy - 1, qx)
                        if intra(mb) or intra(other):
                            bs = 4 if e == 0 else 3
                        elif pic.nz_y[qy // 4, qx // 4] != 0 or pic.nz_y[py // 4, px // 4] != 0:
                            bs = 2
                        elif (np.abs(mv8[qy // 8, qx // 8] - mv8[py // 8, px // 8]) >= 4).any():
                            bs = 1
                        else:
                            bs = 0
                        key = (("y", "cb", "cr")[plane_no], "v" if dirn == 0 else "h", bs)
                        st["bs"][key] = st["bs"].get(key, 0) + 1
                        if not chroma:
                            halves[k >> 3].add(bs)
                            if e == 2 and bs == 1:
                                pst["lf_inner8"].add(dirn)
                            if e == 2 and bs == 2 and pic.kind[mb] == "p8x8":
                                pst["lf_inner8_bs2"] += 1
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
                        pp, qq, flag = L._line_clauses(p, q, bs, index, index, chroma, st)
                        if pp != p or qq != q:
                            st["lines_changed"] += 1
                        for a, v in zip(at_p + at_q, pp + qq):
                            plane[a] = v
                    if not chroma and e == 0 and sorted(halves, key=sorted) == [{0}, {1}]:
                        pst["lf_half"] += 1


def _decode_picture(sample, mbw, mbh, ref_pic, pic_init_qp=26):
    """One mp4 sample -> (_Picture, headers): P_Skip, P_L0_16x16, P_8x8 with four P_L0_8x8, Intra16x16, I_NxN, I_PCM; loop filter by the
    slice header."""
    pst = decode_stream.stats
    pic = P._Picture(mbw, mbh)
    pic.pcm = set()
    blk, _ = I._i4_state(pic)
    _grid(pic)
    headers, at, slice_no = [], 0, 0
    slice_qp, idc = None, None
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
        mb = hd["first_mb"]
        more = True

        def done(m):
            y4, x4 = divmod(m, mbw)
            blk[4 * y4:4 * y4 + 4, 4 * x4:4 * x4 + 4] = slice_no

        while more:                                                     # 7.3.4
            if is_p:
                run = rd.ue()
                for _ in range(run):
                    my, mx = divmod(mb, mbw)
                    pic.slice_of[mb] = slice_no
                    v = _mv_skip(pic, mx, my, slice_no)
                    P._decode_inter(rd, pic, ref_pic, mb, v, 0, qp, False, False)
                    _set(pic, mb, slice_no, [v] * 4, 0, "skip")
                    pst["kinds"].add("skip")
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
                left_kind = pic.kind[mb - 1] if avail_a else None
                mb_type = rd.ue()
                if is_p and mb_type < 5:
                    assert mb_type in (0, 3), "P_L0_16x16 and P_8x8 only: 16x8, 8x16 and P_8x8ref0 are refused"
                    assert ref_pic is not None
                    if mb_type == 0:
                        mvp = _mv_pred(pic, 2 * mx, 2 * my, 2, slice_no)
                        v = (mvp[0] + rd.se(), mvp[1] + rd.se())
                        vs, kind = (v, v, v, v), "l16"
                        if left_kind == "p8x8" and tuple(pic.mv8[2 * my, 2 * mx - 2]) != tuple(pic.mv8[2 * my, 2 * mx - 1]):
                            pst["l16_after_split"] += 1
                    else:                                               # sub_mb_pred(): four sub_mb_type, no ref_idx, the mvd pairs
                        subs = [rd.ue() for _ in range(4)]
                        assert subs == [0, 0, 0, 0], "P_L0_8x8 only: sub-8x8 partitions are refused"
                        mvd = [(rd.se(), rd.se()) for _ in range(4)]
                        vs, kind = [], "p8x8"
                        mv8, ref8, slice8 = _grid(pic)
                        for i in range(4):
                            gx, gy = 2 * mx + (i & 1), 2 * my + (i >> 1)

                            def note(a, b, c, i=i):
                                if i == 2:
                                    pst["part2_a"].add("absent" if not a[0] else "intra" if a[1] < 0 else "inter")
                                if i == 3 and all(x[1] == 0 for x in (a, b, c)):
                                    med = (P._median(a[2][0], b[2][0], c[2][0]), P._median(a[2][1], b[2][1], c[2][1]))
                                    pst["part3_mixed"] += med not in (a[2], b[2], c[2])
                            mvp = _mv_pred(pic, gx, gy, 1, slice_no, note)
                            v = (mvp[0] + mvd[i][0], mvp[1] + mvd[i][1])
                            vs.append(v)
                            mv8[gy, gx], ref8[gy, gx], slice8[gy, gx] = v, 0, slice_no     # partition i is decoded: i + 1 may read it
                        vs = tuple(vs)
                        pst["p8x8"] += 1
                        pst["p8x8_first"] += mx == 0
                        pst["p8x8_after"].add(left_kind)
                    code = rd.ue()
                    assert code < 48
                    cbp = P.CBP_INTER[code]
                    if kind == "p8x8":
                        pst["p8x8_cbp0" if cbp == 0 else "p8x8_cbp"] += 1
                    qp = P._decode_inter(rd, pic, ref_pic, mb, vs if kind == "p8x8" else vs[0], cbp, qp, avail_a, avail_b)
                    _set(pic, mb, slice_no, vs, 0, kind)
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
                    else:
                        assert 1 <= t <= 24
                        qp = P._decode_intra16(rd, pic, mb, t, qp, avail_a, avail_b)
                        pic.n_intra += 1
                        kind = "intra"
                    assert pic.ref[mb] == -1
                    _set(pic, mb, slice_no, [(0, 0)] * 4, -1, kind)
                pst["kinds"].add(kind)
                assert qp == slice_qp
                done(mb)
                mb += 1
                more = rd.more_rbsp_data()
        slice_no += 1
    assert all(s >= 0 for s in pic.slice_of), "a macroblock was never coded"
    if idc == 0:
        deblock_picture(pic, slice_qp, decode_stream.lf, pst)
    I.decode_stream.pictures.append(pic)
    return pic, headers


def decode_stream(samples, width, height, stats=None):
    """h264_i4_ref.decode_stream's result for a stream that may hold P_8x8 macroblocks, with or without the loop filter; ``stats``
    (``new_part_stats``) takes what the decoder met."""
    decode_stream.stats = new_part_stats() if stats is None else stats
    decode_stream.lf = L.new_lf_stats()
    I.decode_stream.pictures = []
    with mock.patch.object(P, "_decode_picture", _decode_picture), mock.patch.object(P, "_inter_pred", _pred_any):
        out = P.decode_stream(samples, width, height)
    out["part"], out["lf"] = decode_stream.stats, decode_stream.lf
    return out


decode_stream.stats, decode_stream.lf = new_part_stats(), L.new_lf_stats()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, qp, subpel, filters=(0, 0), search=SEARCH, part=1, injected=None, gop=None):
    """(planes, samples, (ry, rcb, rcr), mv used, side information, stats) of one case, computed once for all the tests that read it.
    ``injected``: a kind of ``inject`` - the vectors are those and the planes ``plant``ed with them (``kind`` is then only a name)."""
    n, h, w = shape
    gop = n if gop is None else gop
    mbh, mbw = (h + 15) // 16, (w + 15) // 16
    stats = new_stats()
    mv = None if injected is None else inject(injected, n, mbh, mbw, search, subpel)
    planes = make_planes(kind, n, h, w) if injected is None else plant(n, h, w, mv, search, subpel)
    samples, ry, rcb, rcr, used, infos = encode_planes(*planes, qp=qp, gop=gop, first_index=FIRST, stats=stats, search=search, subpel=subpel,
                                                       intra4=filters[0], deblock=filters[1], part=part, mv=mv)
    return planes, samples, (ry, rcb, rcr), used, infos, stats


@functools.lru_cache(maxsize=None)
def searched(shape, kind, qp, search, subpel):
    n, h, w = shape
    return search_planes(make_planes(kind, n, h, w)[0], qp, n, search, subpel)
