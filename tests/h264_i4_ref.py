"""The Intra4x4 rule of the H.264 IDR pictures (include/sdv_hip_h264_i4.h, DESIGN.md "H.264 Intra4x4") restated in plain Python / numpy
on top of h264_sub_ref.py, h264_me_ref.py, h264_p_ref.py and h264_ref.py, none of which is edited, and a decoder for ``I_NxN``.  Nothing
here imports the package's encoder.

The rule, restated.  Every IDR picture chooses per macroblock between ``I_NxN`` and the Intra16x16 DC macroblock of h264_ref, I_PCM by
its two triggers; P pictures are untouched.  The row above is another slice, so for 4x4 block (bx, by) of macroblock m of a row: top iff
by >= 1; left iff bx >= 1 or m > 0; corner iff both; top-right iff by >= 1 and bx <= 2 and (bx, by) not in {(1,1), (1,3)}, else
p[4..7,-1] = p[3,-1].  V, DDL, VL need top; H, HU left; DDR, VR, HD top, left and corner; DC nothing.  Predictors: 8.3.1.2.1 - .9.
Blocks in blkIdx order, each predicted from the reconstruction; cost = SAD + lambda(qp) * (1 if mode == predicted else 4), winner the
minimum of (cost, mode); predicted = min(modeA, modeB), 2 when A or B is unavailable, an Intra16x16 / I_PCM neighbour counts as 2.  The
macroblock is I_NxN iff the sum of the costs < sum |src - DC16| (strict), DC16 = (sum of the 256 source samples + 128) >> 8.  Syntax: mb_type ue(0); per block prev_intra4x4_pred_mode_flag
and rem_intra4x4_pred_mode u(3); intra_chroma_pred_mode ue(0); coded_block_pattern by the intra column of Table 9-4; mb_qp_delta only if
cbp != 0; per coded 8x8 four 16-coefficient blocks (dead zone 1/3, no DC transform, nC from the 16-coefficient TotalCoeff); chroma as in
h264_ref.  Above 3200 bits or on level_prefix > 15 the macroblock is I_PCM and hands mode 2 to the right.  With ``gop`` > 1 and ``search``
0 the P pictures are those of h264_me_ref with zero vectors (its ``search`` 0 case).

(a) ``pred4``: the nine predictors as one table of taps over an edge vector (L3 L2 L1 L0 C T0 .. T7).
(b) ``encode_planes(..., intra4=1)``: h264_sub_ref.encode_planes with ``encode_mb`` below installed for the macroblocks of IDR pictures
    (the way h264_sub_ref installs its interpolator into the decoder), with statistics.
(c) ``decode_stream``: h264_p_ref's decoder with h264_sub_ref's interpolator and a picture loop that knows mb_type 0; its predictor
    ``pred4_clauses`` is written separately, as loops over (x, y) from the clauses, with availability taken from what has been decoded.
(d) ``make_planes``: oriented gratings in the eight mode directions (``grat0`` .. ``grat8`` without 2), ``glyphs``, ``vramp``, ``flat``,
    ``noise``, ``zeros_pcm``; and ``mosaic_pcm``, planes whose macroblock columns alternate between the three macroblock kinds.
"""
import functools
from unittest import mock

import numpy as np

import h264_me_ref as M
import h264_p_ref as P
import h264_ref as R
import h264_sub_ref as S

# Table 9-4, intra column, ChromaArrayType 1: codeNum -> coded_block_pattern
CBP_INTRA = (47, 31, 15, 0, 23, 27, 29, 30, 7, 11, 13, 14, 39, 43, 45, 46, 16, 3, 5, 10, 12, 19, 21, 26, 28, 35, 37, 42, 44, 1, 2, 4, 8, 17, 18,
             20, 24, 6, 9, 22, 25, 32, 33, 34, 36, 40, 38, 41)
V, H, DC, DDL, DDR, VR, HD, VL, HU = range(9)
TOP, LEFT, CORNER, TOPRIGHT = 1, 2, 4, 8
NEED = {V: TOP, DDL: TOP, VL: TOP, H: LEFT, HU: LEFT, DDR: TOP | LEFT | CORNER, VR: TOP | LEFT | CORNER, HD: TOP | LEFT | CORNER, DC: 0}
GRATINGS = tuple("grat%d" % m for m in (V, H, DDL, DDR, VR, HD, VL, HU))
KINDS = GRATINGS + ("glyphs", "vramp", "flat", "noise", "zeros_pcm")
EXTRA_KINDS = ("mosaic_pcm",)                    # planes whose macroblock columns cycle through flat | hostile | flat | ramp | hostile
SHAPES = ((2, 16, 16), (3, 32, 48), (3, 36, 50), (2, 96, 128))
QPS = (0, 16, 28, 51)
SETTINGS = ((1, 0, 0), (3, 0, 0), (3, 8, 0), (3, 8, 4))                          # (gop, search, subpel)
FIRST = P.FIRST
LAMBDA = M.LAMBDA


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) prediction: an edge vector E = (L3, L2, L1, L0, C, T0 .. T7) and, per mode and sample, taps (index, weight) whose weights sum to 4
# ------------------------------------------------------------------------------------------------------------------------------------
def _t(i):
    return 5 + min(i, 7)                                                         # p[i,-1], i = -1 (the corner) .. ; beyond 7 repeats T7


def _l(j):
    return 3 - min(j, 3)                                                         # p[-1,j], j = -1 (the corner) .. ; beyond 3 repeats L3


def _taps(mode, x, y):
    if mode == V:
        return [(_t(x), 4)]
    if mode == DDL:                                                              # x = y = 3 reads T6, T7, T7
        return [(_t(x + y), 1), (_t(x + y + 1), 2), (_t(x + y + 2), 1)]
    if mode == DDR:                                                              # the diagonal through E[4 + x - y]
        return [(3 + x - y, 1), (4 + x - y, 2), (5 + x - y, 1)]
    if mode == VR:
        z, i = 2 * x - y, x - (y >> 1)
        if z >= 0:
            return [(_t(i - 1), 2), (_t(i), 2)] if z % 2 == 0 else [(_t(i - 2), 1), (_t(i - 1), 2), (_t(i), 1)]
        return [(_l(0), 1), (4, 2), (_t(0), 1)] if z == -1 else [(_l(y - 1), 1), (_l(y - 2), 2), (_l(y - 3), 1)]
    if mode == VL:
        i = x + (y >> 1)
        return [(_t(i), 2), (_t(i + 1), 2)] if y % 2 == 0 else [(_t(i), 1), (_t(i + 1), 2), (_t(i + 2), 1)]
    if mode == HU:                                                               # z = 5 reads L2, L3, L3; beyond it L3 alone
        z, j = x + 2 * y, y + (x >> 1)
        return [(_l(j), 2), (_l(j + 1), 2)] if z % 2 == 0 else [(_l(j), 1), (_l(j + 1), 2), (_l(j + 2), 1)]
    if mode in (H, HD):                                                          # the transposed block reads the mirrored edge vector
        return [(8 - i, w) for i, w in _taps(V if mode == H else VR, y, x)]
    raise ValueError(mode)


def _tables():
    idx, wgt = np.zeros((9, 16, 3), dtype=np.int64), np.zeros((9, 16, 3), dtype=np.int64)
    for mode in range(9):
        if mode == DC:
            continue
        for y in range(4):
            for x in range(4):
                for k, (i, w) in enumerate(_taps(mode, x, y)):
                    idx[mode, 4 * y + x, k], wgt[mode, 4 * y + x, k] = i, w
    return idx, wgt


_IDX, _WGT = _tables()


def avail4(bx, by, have_left):
    top, left = by >= 1, bx >= 1 or have_left
    tr = top and bx <= 2 and (bx, by) not in ((1, 1), (1, 3))
    return (TOP if top else 0) | (LEFT if left else 0) | (CORNER if top and left else 0) | (TOPRIGHT if tr else 0)


def pred4_all(edge, avail):
    """``edge`` int64 [13] (missing samples hold anything) -> int64 [9, 16], the nine predictions (rows of modes that are not allowed
    hold numbers nobody reads)."""
    out = ((edge[_IDX] * _WGT).sum(axis=-1) + 2) >> 2
    st, sl = int(edge[5:9].sum()), int(edge[0:4].sum())
    top, left = avail & TOP, avail & LEFT
    out[DC] = (st + sl + 4) >> 3 if top and left else (st + 2) >> 2 if top else (sl + 2) >> 2 if left else 128
    return out


def pred4(edge, avail, mode):
    assert avail & NEED[mode] == NEED[mode]
    return pred4_all(np.asarray(edge, dtype=np.int64), avail)[mode].reshape(4, 4)


def edge_of(ry, lcol, bx, by, avail):
    """The edge vector of block (bx, by) from the macroblock's reconstruction so far and the left neighbour's right column."""
    e = np.full(13, 128, dtype=np.int64)
    x0, y0 = 4 * bx, 4 * by
    if avail & TOP:
        e[5:9] = ry[y0 - 1, x0:x0 + 4]
        e[9:13] = ry[y0 - 1, x0 + 4:x0 + 8] if avail & TOPRIGHT else e[8]
    if avail & LEFT:
        e[0:4] = (ry[y0:y0 + 4, x0 - 1] if bx else lcol[y0:y0 + 4])[::-1]
    if avail & CORNER:
        e[4] = ry[y0 - 1, x0 - 1] if bx else lcol[y0 - 1]
    return e


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) frame kinds
# ------------------------------------------------------------------------------------------------------------------------------------
_DIRECTION = {V: (1, 0), H: (0, 1), DDL: (1, 1), DDR: (1, -1), VR: (2, -1), HD: (-1, 2), VL: (2, 1), HU: (1, 2)}    # u = a x + b y is constant along it


def make_frames(kind, n, h, w, seed=0):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind.startswith("grat"):
        a, b = _DIRECTION[int(kind[4:])]
        norm = float(np.hypot(a, b))
        v = [128 + 90 * np.sin(2 * np.pi * ((a * xx + b * yy) / norm / 13.0) + 0.9 * k) for k in range(n)]
        return np.repeat(np.clip(np.rint(np.stack(v)), 0, 255).astype(np.uint8)[..., None], 3, axis=-1)
    if kind == "vramp":
        v = [np.clip(20 + 2 * yy + 3 * k, 0, 255) for k in range(n)]
        return np.repeat(np.stack(v).astype(np.uint8)[..., None], 3, axis=-1)
    return R.make_frames(kind, n, h, w, seed)


def make_planes(kind, n, h, w, seed=0):
    if kind == "zeros_pcm":
        return R.make_planes(kind, n, h, w, seed)
    if kind == "mosaic_pcm":
        # per macroblock column m % 5: flat 128 (Intra16x16: its DC predictor is exact) | samples near 0 and 255 whose right column is
        # 128 (I_PCM) | flat 128 | a vertical ramp (I_NxN) | hostile again: every kind of macroblock gets every kind of left neighbour
        rng = np.random.default_rng(seed + n + h + w)
        hostile = lambda *sh: np.where(rng.random(sh) < 0.5, rng.integers(0, 4, sh), 252 + rng.integers(0, 4, sh))
        y, cb, cr = (np.full(sh, 128, dtype=np.int64) for sh in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2)))
        for m in range((w + 15) // 16):
            xs, xc = slice(16 * m, 16 * m + 16), slice(8 * m, 8 * m + 8)
            if m % 5 in (1, 4):
                y[:, :, xs], cb[:, :, xc], cr[:, :, xc] = hostile(*y[:, :, xs].shape), hostile(*cb[:, :, xc].shape), hostile(*cr[:, :, xc].shape)
                y[:, :, 16 * m + 15:16 * m + 16], cb[:, :, 8 * m + 7:8 * m + 8], cr[:, :, 8 * m + 7:8 * m + 8] = 128, 128, 128
            elif m % 5 == 3:
                y[:, :, xs] = (40 + 11 * (np.arange(h) % 16))[None, :, None]
        return R.pad_planes(y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8))
    return R.rgb_to_planes(make_frames(kind, n, h, w, seed))


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    st = S.new_stats()
    st.update(i4=dict(kinds=[], modes=[0] * 9, flags=set(), rem_below=0, rem_above=0, avail=set(), substituted=0, after=set(), cbp0=0,
                      cbp_chroma=set(), cbp_codes=set(), pcm_from_i4=0, mbs=0))
    return st


def _chroma(sc, left, qp):
    """The chroma half of h264_ref.encode_mb: -> (cbp_chroma, dc levels [2][4], ac levels [2][4][15], recon [2, 8, 8])."""
    qpc = R.QPC[qp]
    qbc, kc, fc = 15 + qpc // 6, qpc // 6, (1 << (15 + qpc // 6)) // 3
    mfc, nvc = np.array(R.MF[qpc % 6])[R.POS_CLASS], np.array(R.NORM[qpc % 6])[R.POS_CLASS]
    zz = list(R.ZIGZAG)
    pred = np.full((2, 8, 8), 128, dtype=np.int64)
    if left is not None:
        for c in range(2):
            pred[c, :4], pred[c, 4:] = (int(left.ccol[c, :4].sum()) + 2) >> 2, (int(left.ccol[c, 4:].sum()) + 2) >> 2
    ac, dc = [[None] * 4, [None] * 4], []
    for c in range(2):
        d2 = np.zeros((2, 2), dtype=np.int64)
        for b in range(4):
            y, x = 4 * (b >> 1), 4 * (b & 1)
            w = R.CF @ (sc[c, y:y + 4, x:x + 4] - pred[c, y:y + 4, x:x + 4]) @ R.CF.T
            d2[b >> 1, b & 1] = w[0, 0]
            ac[c][b] = R._quant(w, mfc, fc, qbc).reshape(-1)[zz][1:]
        dc.append(R._quant(R.H2 @ d2 @ R.H2, R.MF[qpc % 6][0], 2 * fc, qbc + 1).reshape(-1))
    cbp = 2 if any(a.any() for cc in ac for a in cc) else 1 if any(d.any() for d in dc) else 0
    rc = np.empty((2, 8, 8), dtype=np.int64)
    for c in range(2):
        dcc = ((R.H2 @ dc[c].reshape(2, 2) @ R.H2) * R.NORM[qpc % 6][0] << kc) >> 1
        for b in range(4):
            y, x = 4 * (b >> 1), 4 * (b & 1)
            lv = np.zeros(16, dtype=np.int64)
            lv[zz[1:]] = ac[c][b]
            d = (lv.reshape(4, 4) * nvc) << kc
            d[0, 0] = dcc[b >> 1, b & 1]
            rc[c, y:y + 4, x:x + 4] = np.clip(pred[c, y:y + 4, x:x + 4] + R._inverse4x4(d), 0, 255)
    return cbp, dc, ac, rc


def _kind_of(left):
    return None if left is None else getattr(left, "kind", "i16")


def encode_mb(sy, sc, left, qp, stats, intra16):
    """One macroblock of an IDR picture, h264_ref.encode_mb's signature and results (``intra16`` is that function): I_NxN, or what
    ``intra16`` returns when sum |src - DC16| (DC16 the macroblock's own DC) is not above the sum of the block costs.  The _Left it returns carries
    ``modes`` (the four right-hand modes) and ``kind``."""
    st = stats["i4"]
    sy, sc = sy.astype(np.int64), sc.astype(np.int64)
    qbits, k = 15 + qp // 6, qp // 6
    f = (1 << qbits) // 3
    mf, nv = np.array(R.MF[qp % 6])[R.POS_CLASS], np.array(R.NORM[qp % 6])[R.POS_CLASS]
    zz = list(R.ZIGZAG)
    lam = LAMBDA[qp]
    lcol = None if left is None else np.asarray(left.ycol, dtype=np.int64)
    lmodes = None if left is None else getattr(left, "modes", (DC,) * 4)
    ry = np.zeros((16, 16), dtype=np.int64)
    modes = np.full((4, 4), DC, dtype=np.int64)
    levels, predicted, total, avails, subst = [None] * 16, [DC] * 16, 0, [], 0
    for b, (x, y) in enumerate(R.BLK_XY):
        bx, by = x // 4, y // 4
        av = avail4(bx, by, left is not None)
        a = int(modes[by, bx - 1]) if bx else (None if left is None else int(lmodes[by]))
        t = int(modes[by - 1, bx]) if by else None
        pm = DC if a is None or t is None else min(a, t)
        preds = pred4_all(edge_of(ry, lcol, bx, by, av), av)
        src = sy[y:y + 4, x:x + 4].reshape(-1)
        sads = np.abs(src[None, :] - preds).sum(axis=1)
        cost, mode = min((int(sads[m]) + lam * (1 if m == pm else 4), m) for m in range(9) if av & NEED[m] == NEED[m])
        total += cost
        w = R.CF @ (src - preds[mode]).reshape(4, 4) @ R.CF.T
        q = R._quant(w, mf, f, qbits)
        levels[b] = q.reshape(-1)[zz]
        ry[y:y + 4, x:x + 4] = np.clip(preds[mode].reshape(4, 4) + R._inverse4x4((q * nv) << k), 0, 255)
        modes[by, bx], predicted[b] = mode, pm
        avails.append(av)
        subst += 1 if (av & TOP and not av & TOPRIGHT and mode in (DDL, VL)) else 0
    dc16 = (int(sy.sum()) + 128) >> 8                                           # the macroblock's own DC, not its predictor
    if not total < int(np.abs(sy - dc16).sum()):
        bits, py, pc, new_left, pcm = intra16(sy, sc, left, qp, stats["intra"])
        new_left.modes, new_left.kind = (DC,) * 4, "pcm" if pcm else "i16"
        st["kinds"].append(new_left.kind)
        st["after"].add((_kind_of(left), new_left.kind))
        return bits, py, pc, new_left, pcm
    cbp_chroma, dc_c, ac_c, rc = _chroma(sc, left, qp)
    cbp_luma = sum(1 << i for i in range(4) if any(levels[4 * i + j].any() for j in range(4)))
    tc_y, tc_c = np.zeros((4, 4), dtype=np.int64), np.zeros((2, 2, 2), dtype=np.int64)
    flags, rems = [], []
    why = None
    try:
        out = [R.ue(0)]
        for b, (x, y) in enumerate(R.BLK_XY):
            mode, pm = int(modes[y // 4, x // 4]), predicted[b]
            flags.append(int(mode == pm))
            if mode == pm:
                out.append("1")
            else:
                rems.append((mode, pm))
                out.append("0" + format(mode if mode < pm else mode - 1, "03b"))
        out += [R.ue(0), R.ue(CBP_INTRA.index(cbp_luma + 16 * cbp_chroma))]
        if cbp_luma or cbp_chroma:
            out.append(R.se(0))
        for b, (x, y) in enumerate(R.BLK_XY):
            if not (cbp_luma >> (b >> 2)) & 1:
                continue
            bx, by = x // 4, y // 4
            a = int(tc_y[by, bx - 1]) if bx else (None if left is None else int(left.tc_y[by]))
            t = int(tc_y[by - 1, bx]) if by else None
            bits, tc_y[by, bx] = R.code_block([int(v) for v in levels[b]], R._nc(a, t), stats["intra"])
            out.append(bits)
        if cbp_chroma:
            for c in range(2):
                out.append(R.code_block([int(v) for v in dc_c[c]], -1, stats["intra"])[0])
        if cbp_chroma == 2:
            for c in range(2):
                for b in range(4):
                    by, bx = b >> 1, b & 1
                    a = int(tc_c[c, by, bx - 1]) if bx else (None if left is None else int(left.tc_c[c, by]))
                    t = int(tc_c[c, by - 1, bx]) if by else None
                    bits, tc_c[c, by, bx] = R.code_block([int(v) for v in ac_c[c][b]], R._nc(a, t), stats["intra"])
                    out.append(bits)
        bits = "".join(out)
        if len(bits) > R.MAX_MB_BITS:
            why = "bits"
    except R.Uncodable:
        why = "level"
    if why is not None:
        stats["intra"]["pcm"].add(why)
        st["pcm_from_i4"] += 1
        st["kinds"].append("pcm")
        st["after"].add((_kind_of(left), "pcm"))
        new_left = R._Left(sy[:, 15].copy(), sc[:, :, 7].copy(), np.full(4, 16), np.full((2, 2), 16))
        new_left.modes, new_left.kind = (DC,) * 4, "pcm"
        return None, sy, sc, new_left, True
    st["mbs"] += 1
    st["kinds"].append("i4")
    st["after"].add((_kind_of(left), "i4"))
    for m in modes.reshape(-1):
        st["modes"][int(m)] += 1
    st["flags"] |= set(flags)
    st["rem_below"] += sum(1 for m, p in rems if m < p)
    st["rem_above"] += sum(1 for m, p in rems if m > p)
    st["avail"] |= set(avails)
    st["substituted"] += subst
    st["cbp0"] += int(cbp_luma == 0 and cbp_chroma == 0)
    st["cbp_chroma"].add(cbp_chroma)
    st["cbp_codes"].add(cbp_luma + 16 * cbp_chroma)
    new_left = R._Left(ry[:, 15].copy(), rc[:, :, 7].copy(), tc_y[:, 3].copy(), tc_c[:, :, 1].copy())
    new_left.modes, new_left.kind = tuple(int(m) for m in modes[:, 3]), "i4"
    return bits, ry, rc, new_left, False


def encode_planes(y, cb, cr, qp=16, gop=1, first_index=0, stats=None, search=0, subpel=0, intra4=0):
    """Padded planes -> (samples, recon Y, recon Cb, recon Cr, mv used): h264_sub_ref.encode_planes, and with ``intra4`` 1 the
    macroblocks of its IDR pictures through ``encode_mb`` above.  (That function hands the statistics object ``stats["intra"]`` to the
    macroblocks of IDR pictures and a probe of its own to the intra macroblocks of P slices, which stay Intra16x16.)"""
    assert intra4 in (0, 1)
    stats = new_stats() if stats is None else stats
    kw = dict(qp=qp, gop=gop, first_index=first_index, stats=stats, search=search, subpel=subpel)
    if not intra4:
        return S.encode_planes(y, cb, cr, **kw)
    intra16 = R.encode_mb

    def idr_or_p(sy, sc, left, q, st):
        return encode_mb(sy, sc, left, q, stats, intra16) if st is stats["intra"] else intra16(sy, sc, left, q, st)

    with mock.patch.object(R, "encode_mb", idr_or_p):
        return S.encode_planes(y, cb, cr, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the decoder
# ------------------------------------------------------------------------------------------------------------------------------------
def pred4_clauses(p, mode):
    """8.3.1.2.1 - 8.3.1.2.9 as written: ``p`` maps (x, y) of the neighbouring samples that are available (after the substitution of
    8.3.1.2 for the top-right ones) to their values -> pred [4][4] (rows y, columns x).  A mode that reads a missing sample is refused."""
    pred = [[0] * 4 for _ in range(4)]
    if mode == 2:
        top, left = all((x, -1) in p for x in range(4)), all((-1, y) in p for y in range(4))
        st, sl = sum(p[(x, -1)] for x in range(4)) if top else 0, sum(p[(-1, y)] for y in range(4)) if left else 0
        v = (st + sl + 4) >> 3 if top and left else (sl + 2) >> 2 if left else (st + 2) >> 2 if top else 128
        return [[v] * 4 for _ in range(4)]
    for y in range(4):
        for x in range(4):
            if mode == 0:
                v = p[(x, -1)]
            elif mode == 1:
                v = p[(-1, y)]
            elif mode == 3:
                if x == 3 and y == 3:
                    v = (p[(6, -1)] + 3 * p[(7, -1)] + 2) >> 2
                else:
                    v = (p[(x + y, -1)] + 2 * p[(x + y + 1, -1)] + p[(x + y + 2, -1)] + 2) >> 2
            elif mode == 4:
                if x > y:
                    v = (p[(x - y - 2, -1)] + 2 * p[(x - y - 1, -1)] + p[(x - y, -1)] + 2) >> 2
                elif x < y:
                    v = (p[(-1, y - x - 2)] + 2 * p[(-1, y - x - 1)] + p[(-1, y - x)] + 2) >> 2
                else:
                    v = (p[(0, -1)] + 2 * p[(-1, -1)] + p[(-1, 0)] + 2) >> 2
            elif mode == 5:
                z, i = 2 * x - y, x - (y >> 1)
                if z in (0, 2, 4, 6):
                    v = (p[(i - 1, -1)] + p[(i, -1)] + 1) >> 1
                elif z in (1, 3, 5):
                    v = (p[(i - 2, -1)] + 2 * p[(i - 1, -1)] + p[(i, -1)] + 2) >> 2
                elif z == -1:
                    v = (p[(-1, 0)] + 2 * p[(-1, -1)] + p[(0, -1)] + 2) >> 2
                else:
                    v = (p[(-1, y - 1)] + 2 * p[(-1, y - 2)] + p[(-1, y - 3)] + 2) >> 2
            elif mode == 6:
                z, j = 2 * y - x, y - (x >> 1)
                if z in (0, 2, 4, 6):
                    v = (p[(-1, j - 1)] + p[(-1, j)] + 1) >> 1
                elif z in (1, 3, 5):
                    v = (p[(-1, j - 2)] + 2 * p[(-1, j - 1)] + p[(-1, j)] + 2) >> 2
                elif z == -1:
                    v = (p[(-1, 0)] + 2 * p[(-1, -1)] + p[(0, -1)] + 2) >> 2
                else:
                    v = (p[(x - 1, -1)] + 2 * p[(x - 2, -1)] + p[(x - 3, -1)] + 2) >> 2
            elif mode == 7:
                i = x + (y >> 1)
                if y in (0, 2):
                    v = (p[(i, -1)] + p[(i + 1, -1)] + 1) >> 1
                else:
                    v = (p[(i, -1)] + 2 * p[(i + 1, -1)] + p[(i + 2, -1)] + 2) >> 2
            elif mode == 8:
                z, j = x + 2 * y, y + (x >> 1)
                if z in (0, 2, 4):
                    v = (p[(-1, j)] + p[(-1, j + 1)] + 1) >> 1
                elif z in (1, 3):
                    v = (p[(-1, j)] + 2 * p[(-1, j + 1)] + p[(-1, j + 2)] + 2) >> 2
                elif z == 5:
                    v = (p[(-1, 2)] + 3 * p[(-1, 3)] + 2) >> 2
                else:
                    v = p[(-1, 3)]
            else:
                raise AssertionError("Intra4x4PredMode %r" % (mode,))
            pred[y][x] = v
    return pred


def _i4_state(pic):
    """Per 4x4 block of the picture: the slice it was decoded in (-1: not yet) and its Intra4x4PredMode (-1: not an Intra4x4 block)."""
    if not hasattr(pic, "blk_slice"):
        pic.blk_slice = np.full((4 * pic.mbh, 4 * pic.mbw), -1, dtype=np.int64)
        pic.i4_mode = np.full((4 * pic.mbh, 4 * pic.mbw), -1, dtype=np.int64)
        pic.n_i4 = 0
        pic.i4_modes = [0] * 9
    return pic.blk_slice, pic.i4_mode


def _neighbours(pic, gx, gy, slice_no):
    """The neighbouring samples of the 4x4 block at block coordinates (gx, gy) that are available (6.4.11.4 with 8.3.1.2): a sample is
    available when its 4x4 block lies in the picture and has been decoded in this slice."""
    blk = pic.blk_slice
    ok = lambda bx, by: 0 <= bx < 4 * pic.mbw and 0 <= by < 4 * pic.mbh and blk[by, bx] == slice_no
    x0, y0 = 4 * gx, 4 * gy
    p = {}
    if ok(gx, gy - 1):
        for x in range(4):
            p[(x, -1)] = int(pic.Y[y0 - 1, x0 + x])
        for x in range(4, 8):
            p[(x, -1)] = int(pic.Y[y0 - 1, x0 + x]) if ok(gx + 1, gy - 1) else p[(3, -1)]
    if ok(gx - 1, gy):
        for y in range(4):
            p[(-1, y)] = int(pic.Y[y0 + y, x0 - 1])
    if ok(gx - 1, gy - 1):
        p[(-1, -1)] = int(pic.Y[y0 - 1, x0 - 1])
    return p


def _decode_i4(rd, pic, mb, slice_no, qp, avail_a, avail_b):
    """An I_NxN macroblock (7.3.5, 7.3.5.1, 8.3.1); returns the new QP."""
    my, mx = divmod(mb, pic.mbw)
    blk, modes = _i4_state(pic)
    for b in range(16):                                                 # mb_pred(): the sixteen modes (8.3.1.1)
        bx, by = R.BLK_XY[b][0] // 4, R.BLK_XY[b][1] // 4
        gx, gy = 4 * mx + bx, 4 * my + by
        if not (bx > 0 or avail_a) or not (by > 0 or avail_b):         # dcPredModePredictedFlag
            predicted = 2
        else:
            ma, mb_ = int(modes[gy, gx - 1]), int(modes[gy - 1, gx])
            predicted = min(2 if ma < 0 else ma, 2 if mb_ < 0 else mb_)
        if rd.u(1):
            modes[gy, gx] = predicted
        else:
            rem = rd.u(3)
            modes[gy, gx] = rem if rem < predicted else rem + 1
    assert rd.ue() == 0, "only DC chroma prediction is decoded here"
    code = rd.ue()
    assert code < 48
    cbp = CBP_INTRA[code]
    if cbp:
        qp = (qp + rd.se() + 52) % 52
    res = []
    for b in range(16):
        bx, by = R.BLK_XY[b][0] // 4, R.BLK_XY[b][1] // 4
        if (cbp >> (b >> 2)) & 1:
            co, pic.nz_y[4 * my + by, 4 * mx + bx] = R._residual_block(rd, P._n_c(pic.nz_y, 4 * my + by, 4 * mx + bx, 4 * my, 4 * mx, avail_a, avail_b), 16)
            res.append(np.array(R._idct_rows_cols(P._scale16(co, qp))))
        else:
            pic.nz_y[4 * my + by, 4 * mx + bx] = 0
            res.append(0)
    for b in range(16):
        bx, by = R.BLK_XY[b][0] // 4, R.BLK_XY[b][1] // 4
        gx, gy = 4 * mx + bx, 4 * my + by
        pred = np.array(pred4_clauses(_neighbours(pic, gx, gy, slice_no), int(modes[gy, gx])))
        pic.Y[4 * gy:4 * gy + 4, 4 * gx:4 * gx + 4] = np.clip(pred + res[b], 0, 255)
        blk[gy, gx] = slice_no
        pic.i4_modes[int(modes[gy, gx])] += 1
    cres = P._chroma_residual(rd, pic, my, mx, cbp >> 4, R.QPC[qp], avail_a, avail_b) if cbp >> 4 else None
    if cres is None:
        pic.nz_c[:, 2 * my:2 * my + 2, 2 * mx:2 * mx + 2] = 0
    C, cy0, cx0 = pic.C, 8 * my, 8 * mx
    for cc in range(2):
        for b in range(4):
            by, bx = b >> 1, b & 1
            yy, xx = cy0 + 4 * by, cx0 + 4 * bx                         # 8.3.4 DC prediction of the chroma block at (4 bx, 4 by)
            top = int(C[cc, yy - 1, xx:xx + 4].sum()) if avail_b else None
            lft = int(C[cc, yy:yy + 4, cx0 - 1].sum()) if avail_a else None
            if (bx, by) in ((0, 0), (1, 1)):
                v = (top + lft + 4) >> 3 if (top is not None and lft is not None) else (lft + 2) >> 2 if lft is not None else \
                    (top + 2) >> 2 if top is not None else 128
            elif (bx, by) == (1, 0):
                v = (top + 2) >> 2 if top is not None else (lft + 2) >> 2 if lft is not None else 128
            else:
                v = (lft + 2) >> 2 if lft is not None else (top + 2) >> 2 if top is not None else 128
            C[cc, yy:yy + 4, xx:xx + 4] = np.clip(v + (cres[cc][b] if cres is not None else 0), 0, 255)
    pic.n_i4 += 1
    return qp


def _decode_picture(sample, mbw, mbh, ref_pic, pic_init_qp=26):
    """h264_p_ref._decode_picture with mb_type 0 of an I slice (and 5 of a P slice) decoded as I_NxN; every other macroblock goes through
    that module's functions."""
    pic = P._Picture(mbw, mbh)
    blk, modes = _i4_state(pic)
    headers, at, slice_no = [], 0, 0
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
        hd["deblock_idc"] = rd.ue()
        assert hd["deblock_idc"] == 1
        headers.append(hd)
        qp = pic_init_qp + hd["qp_delta"]
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
                    elif t == 0:
                        qp = _decode_i4(rd, pic, mb, slice_no, qp, avail_a, avail_b)
                        hd["n_i4"] = hd.get("n_i4", 0) + 1
                    else:
                        assert 1 <= t <= 24
                        qp = P._decode_intra16(rd, pic, mb, t, qp, avail_a, avail_b)
                        pic.n_intra += 1
                done(mb)
                mb += 1
                more = rd.more_rbsp_data()
        slice_no += 1
    assert all(s >= 0 for s in pic.slice_of), "a macroblock was never coded"
    decode_stream.pictures.append(pic)
    return pic, headers


def decode_stream(samples, width, height):
    """h264_p_ref.decode_stream's result plus ``n_i4`` (I_NxN macroblocks), ``i4_modes`` (histogram of their blocks' modes) and
    ``p_i4`` (I_NxN macroblocks inside P slices, which the rule never writes)."""
    decode_stream.pictures = []
    with mock.patch.object(P, "_decode_picture", _decode_picture), mock.patch.object(P, "_inter_pred", S.inter_pred):
        out = P.decode_stream(samples, width, height)
    pics = decode_stream.pictures
    out["n_i4"] = sum(p.n_i4 for p in pics)
    out["i4_modes"] = [sum(p.i4_modes[m] for p in pics) for m in range(9)]
    out["p_i4"] = sum(h.get("n_i4", 0) for hs in out["headers"] for h in hs if h["nal_unit_type"] != 5)
    return out


decode_stream.pictures = []


@functools.lru_cache(maxsize=None)
def reference(shape, kind, qp, setting=(1, 0, 0), intra4=1):
    """(planes, samples, (ry, rcb, rcr), stats) of one case, computed once for all the tests that read it."""
    n, h, w = shape
    gop, search, subpel = setting
    planes = make_planes(kind, n, h, w)
    stats = new_stats()
    samples, ry, rcb, rcr, _ = encode_planes(*planes, qp=qp, gop=gop, first_index=FIRST, stats=stats, search=search, subpel=subpel, intra4=intra4)
    return planes, samples, (ry, rcb, rcr), stats
