"""The H.264 GOP stream rule (DESIGN.md "H.264 P pictures", include/sdv_hip.h) restated in plain Python / numpy on top of h264_ref.py, and
a decoder for it written from the decoding clauses of ITU-T Rec. H.264.

(a) ``encode_planes``: IDR pictures by ``h264_ref.encode_mb``, P pictures macroblock by macroblock (mode decision, P_Skip, P_L0_16x16,
    Intra16x16 / I_PCM inside a P slice, mb_skip_run), with the reconstruction of every sample and the statistics the coverage check reads.
(b) ``decode_stream``: 7.3.3 slice headers of I and P slices, 7.3.4 slice data with mb_skip_run, P-slice mb_types 0, 5 .. 30 and skip,
    the inter column of me(v), 16-coefficient luma residual blocks, 8.4.1.1 / 8.4.1.3 motion vector prediction from neighbour
    availability plus mvd (a vector that is not whole-sample is refused), inter prediction as a copy with edge clamping, and the frame_num
    / idr_pic_id rules of 7.4.3 it can check.  Nothing here imports the package's encoder.
(c) ``make_planes``: the temporal frame kinds of the test suites.
"""
import functools

import numpy as np

import h264_ref as R

# Table 9-4, inter column, ChromaArrayType 1: codeNum -> coded_block_pattern
CBP_INTER = (0, 16, 1, 2, 4, 8, 32, 3, 5, 10, 12, 15, 47, 7, 11, 13, 14, 6, 9, 31, 35, 37, 42, 44, 33, 34, 36, 40, 39, 43, 45, 46, 17, 18, 20, 24,
             19, 21, 26, 28, 23, 27, 29, 30, 22, 25, 38, 41)
KINDS = ("still", "fade", "pan", "cut", "noise", "zeros_pcm")
EXTRA_KINDS = ("flash_pcm",)                    # planes that jump between 252 .. 255 and 0 .. 3: Intra16x16 in a P slice that needs level_prefix > 15
GOP_MAX = 256
# the case set of both suites: (n, H, W, gop) - one macroblock with no neighbour anywhere; left chains, two rows; crop plus edge padding;
# GOPs of 3, 3, 1; frame_num wrap; more waves than a trivial grid
SHAPES = ((4, 16, 16, 4), (5, 32, 48, 5), (3, 36, 50, 3), (7, 64, 64, 3), (18, 16, 16, 18), (6, 96, 128, 2))
QPS = (0, 16, 28, 51)
FIRST = 3


def slot_mbw(mbw):
    return mbw + 1 + mbw // 64


def p_rbsp_bound(mbw):
    """Bytes of a P slice's RBSP at most (sdv_hip.h "Capacity of the GOP path"): 68 bits of header, per macroblock an mb_skip_run of at most
    21 bits and a macroblock_layer() of at most 3200, a trailing run of at most 21, the stop bit and at most 7 alignment zeros."""
    return (68 + mbw * (21 + 3200) + 21 + 8 + 7) // 8


def slot_bytes(mbw):
    """The documented capacity of one slice of the GOP path: the intra slot of a picture ``slot_mbw(mbw)`` macroblocks wide."""
    return R.slot_bytes(slot_mbw(mbw))


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) frame kinds
# ------------------------------------------------------------------------------------------------------------------------------------
def make_frames(kind, n, h, w, seed=0):
    """uint8 RGB [n, h, w, 3] of one of the RGB kinds."""
    if kind == "still":
        return np.repeat(R.make_frames("glyphs", 1, h, w, seed), n, axis=0)
    if kind == "fade":
        a, b = R.make_frames("glyphs", 2, h, w, seed).astype(np.int64)
        return np.stack([(a * (2 * (n - 1) - 2 * k) + b * 2 * k + (n - 1)) // (2 * (n - 1)) if n > 1 else a for k in range(n)]).astype(np.uint8)
    if kind == "pan":
        g = R.make_frames("glyphs", 1, h, w, seed)[0]
        return np.stack([np.roll(g, k, axis=1) for k in range(n)])
    if kind == "cut":
        f = np.repeat(R.make_frames("glyphs", 1, h, w, seed), n, axis=0)
        f[n // 2:] = R.make_frames("noise", n - n // 2, h, w, seed)
        return f
    if kind == "noise":
        return R.make_frames("noise", n, h, w, seed)
    raise ValueError(kind)


def make_planes(kind, n, h, w, seed=0):
    if kind == "zeros_pcm":
        return R.make_planes("zeros_pcm", n, h, w, seed)
    if kind == "flash_pcm":
        y, cb, cr = R.make_planes("zeros_pcm", n, h, w, seed)
        y[0::2] = 255 - y[0::2]
        return y, cb, cr
    return R.rgb_to_planes(make_frames(kind, n, h, w, seed))


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    return dict(intra=R.new_stats(), modes=[], skip_runs=set(), only_run_slices=0, trailing_runs=0, inter_cbp_luma=set(), inter_cbp_chroma=set(),
                intra_after_inter=0, inter_after_intra=0, pcm_in_p=set(), inter_after_pcm=0, frame_nums=[], short_gop=False, n_pcm=0,
                p_mb_bits=[])


def p_slice_header(first_mb, frame_num, qp):
    return R.ue(first_mb) + R.ue(5) + R.ue(0) + format(frame_num & 15, "04b") + "000" + R.se(qp - 26) + R.ue(1)


def encode_p_mb(sy, sc, fy, fc, left, qp, stats):
    """One macroblock of a P slice: source ``sy`` [16, 16], ``sc`` [2, 8, 8], reference ``fy``, ``fc`` (the co-located reconstruction of
    the previous picture) -> (mode, bit string or None, recon Y, recon C, _Left).  mode: "skip" | "inter" | "intra" | "pcm"."""
    sy, sc, fy, fc = (a.astype(np.int64) for a in (sy, sc, fy, fc))
    pred_y = 128 if left is None else (int(left.ycol.sum()) + 8) >> 4
    sad_intra, sad_inter = int(np.abs(sy - pred_y).sum()), int(np.abs(sy - fy).sum())
    pcm_left = R._Left(sy[:, 15].copy(), sc[:, :, 7].copy(), np.full(4, 16), np.full((2, 2), 16))
    if sad_intra < sad_inter:
        probe = R.new_stats()
        bits, ry, rc, new_left, pcm = R.encode_mb(sy, sc, left, qp, probe)
        for key, v in probe.items():
            if isinstance(v, set):
                stats["intra"][key] |= v
        why = "level" if "level" in probe["pcm"] else "bits"
        if not pcm:
            z = len(bits) - len(bits.lstrip("0"))                                  # the I-slice mb_type ue(v) -> ue(5 + v)
            bits = R.ue(5 + int(bits[z:2 * z + 1], 2) - 1) + bits[2 * z + 1:]
            pcm = len(bits) > R.MAX_MB_BITS
        if pcm:
            stats["pcm_in_p"].add(why)
            return "pcm", None, sy, sc, pcm_left
        return "intra", bits, ry, rc, new_left
    qbits, k = 15 + qp // 6, qp // 6
    f = (1 << qbits) // 6
    mf, nv = np.array(R.MF[qp % 6])[R.POS_CLASS], np.array(R.NORM[qp % 6])[R.POS_CLASS]
    zz = list(R.ZIGZAG)
    lev_y = [R._quant(R.CF @ (sy - fy)[y:y + 4, x:x + 4] @ R.CF.T, mf, f, qbits).reshape(-1)[zz] for x, y in R.BLK_XY]
    qpc = R.QPC[qp]
    qbc, kc = 15 + qpc // 6, qpc // 6
    fcq = (1 << qbc) // 6
    mfc, nvc = np.array(R.MF[qpc % 6])[R.POS_CLASS], np.array(R.NORM[qpc % 6])[R.POS_CLASS]
    ac_c, dc_c = [[None] * 4, [None] * 4], []
    for c in range(2):
        d2 = np.zeros((2, 2), dtype=np.int64)
        for b in range(4):
            y, x = 4 * (b >> 1), 4 * (b & 1)
            w = R.CF @ (sc[c] - fc[c])[y:y + 4, x:x + 4] @ R.CF.T
            d2[b >> 1, b & 1] = w[0, 0]
            ac_c[c][b] = R._quant(w, mfc, fcq, qbc).reshape(-1)[zz][1:]
        dc_c.append(R._quant(R.H2 @ d2 @ R.H2, R.MF[qpc % 6][0], 2 * fcq, qbc + 1).reshape(-1))
    cbp_luma = sum(1 << i for i in range(4) if any(lev_y[4 * i + j].any() for j in range(4)))
    cbp_chroma = 2 if any(a.any() for cc in ac_c for a in cc) else 1 if any(d.any() for d in dc_c) else 0
    if cbp_luma == 0 and cbp_chroma == 0:
        return "skip", None, fy, fc, R._Left(fy[:, 15].copy(), fc[:, :, 7].copy(), np.zeros(4, dtype=np.int64), np.zeros((2, 2), dtype=np.int64))
    tc_y, tc_c = np.zeros((4, 4), dtype=np.int64), np.zeros((2, 2, 2), dtype=np.int64)
    why = None
    try:
        out = [R.ue(0), R.se(0), R.se(0), R.ue(CBP_INTER.index(cbp_luma + 16 * cbp_chroma)), R.se(0)]
        for b, (x, y) in enumerate(R.BLK_XY):
            if not (cbp_luma >> (b >> 2)) & 1:
                continue
            bx, by = x // 4, y // 4
            a = int(tc_y[by, bx - 1]) if bx else (None if left is None else int(left.tc_y[by]))
            t = int(tc_y[by - 1, bx]) if by else None
            bits, tc_y[by, bx] = R.code_block([int(v) for v in lev_y[b]], R._nc(a, t), stats["intra"])
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
        stats["pcm_in_p"].add(why)
        return "pcm", None, sy, sc, pcm_left
    stats["inter_cbp_luma"].add(cbp_luma)
    stats["inter_cbp_chroma"].add(cbp_chroma)
    ry = np.empty((16, 16), dtype=np.int64)
    for b, (x, y) in enumerate(R.BLK_XY):
        lv = np.zeros(16, dtype=np.int64)
        lv[zz] = lev_y[b]
        ry[y:y + 4, x:x + 4] = np.clip(fy[y:y + 4, x:x + 4] + R._inverse4x4((lv.reshape(4, 4) * nv) << k), 0, 255)
    rc = np.empty((2, 8, 8), dtype=np.int64)
    for c in range(2):
        dcc = ((R.H2 @ dc_c[c].reshape(2, 2) @ R.H2) * R.NORM[qpc % 6][0] << kc) >> 1
        for b in range(4):
            y, x = 4 * (b >> 1), 4 * (b & 1)
            lv = np.zeros(16, dtype=np.int64)
            lv[zz[1:]] = ac_c[c][b]
            d = (lv.reshape(4, 4) * nvc) << kc
            d[0, 0] = dcc[b >> 1, b & 1]
            rc[c, y:y + 4, x:x + 4] = np.clip(fc[c, y:y + 4, x:x + 4] + R._inverse4x4(d), 0, 255)
    return "inter", bits, ry, rc, R._Left(ry[:, 15].copy(), rc[:, :, 7].copy(), tc_y[:, 3].copy(), tc_c[:, :, 1].copy())


def encode_planes(y, cb, cr, qp=16, gop=1, first_index=0, stats=None):
    """Padded planes [n, 16 mbh, 16 mbw] / [n, 8 mbh, 8 mbw] -> (samples: list[bytes], recon Y, recon Cb, recon Cr).  Picture k is an IDR
    picture iff k % gop == 0."""
    assert 0 <= qp <= 51 and 1 <= gop <= GOP_MAX
    stats = new_stats() if stats is None else stats
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    ry, rcb, rcr = np.empty_like(y), np.empty_like(cb), np.empty_like(cr)
    samples = []
    if n % gop:
        stats["short_gop"] = True
    for k in range(n):
        is_p = k % gop != 0
        stats["frame_nums"].append(k % gop & 15)
        sample = bytearray()
        for r in range(mbh):
            bits = [p_slice_header(r * mbw, k % gop, qp) if is_p else R.slice_header(r * mbw, (first_index + k) & 1, qp)]
            left, run, prev = None, 0, None
            for m in range(mbw):
                ys, xs, yc, xc = slice(16 * r, 16 * r + 16), slice(16 * m, 16 * m + 16), slice(8 * r, 8 * r + 8), slice(8 * m, 8 * m + 8)
                sy, sc = y[k, ys, xs], np.stack([cb[k, yc, xc], cr[k, yc, xc]])
                if is_p:
                    mode, mb, py, pc, left = encode_p_mb(sy, sc, ry[k - 1, ys, xs], np.stack([rcb[k - 1, yc, xc], rcr[k - 1, yc, xc]]), left, qp, stats)
                else:
                    mb, py, pc, left, pcm = R.encode_mb(sy, sc, left, qp, stats["intra"])
                    mode = "pcm" if pcm else "intra"
                if is_p:
                    stats["modes"].append(mode)
                    if mode == "skip":
                        run += 1
                    else:
                        bits.append(R.ue(run))
                        stats["skip_runs"].add(run)
                        run = 0
                    if mode == "intra" and prev == "inter":
                        stats["intra_after_inter"] += 1
                    if mode == "inter" and prev == "intra":
                        stats["inter_after_intra"] += 1
                    if mode == "inter" and prev == "pcm":
                        stats["inter_after_pcm"] += 1
                if mode == "pcm":
                    bits.append(R.ue(30 if is_p else 25))
                    bits.append("0" * (-sum(map(len, bits)) % 8))
                    bits.append("".join(format(int(v), "08b") for v in np.concatenate([sy.reshape(-1), sc.reshape(-1)])))
                    stats["n_pcm"] += 1
                elif mode != "skip":
                    bits.append(mb)
                    if is_p:
                        stats["p_mb_bits"].append(len(mb))
                prev = mode
                ry[k, ys, xs] = py
                rcb[k, yc, xc], rcr[k, yc, xc] = pc[0], pc[1]
            if is_p and run:
                bits.append(R.ue(run))
                stats["skip_runs"].add(run)
                stats["trailing_runs"] += 1
                if run == mbw:
                    stats["only_run_slices"] += 1
            s = "".join(bits) + "1"
            s += "0" * (-len(s) % 8)
            rbsp = int(s, 2).to_bytes(len(s) // 8, "big")
            assert not is_p or len(rbsp) <= p_rbsp_bound(mbw)
            nal = bytes([0x41 if is_p else 0x65]) + R.escape(rbsp)
            assert 4 + len(nal) <= slot_bytes(mbw)
            sample += len(nal).to_bytes(4, "big") + nal
        samples.append(bytes(sample))
    return samples, ry, rcb, rcr


def sync_samples(n, gop):
    return [k for k in range(n) if k % gop == 0]


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the decoder
# ------------------------------------------------------------------------------------------------------------------------------------
class NotWholeSample(Exception):
    """A motion vector that would need sub-sample interpolation, which this decoder does not have."""


def _scale16(coeff16, q):
    """8.5.12.1 for a block with its own DC: scan positions 0 .. 15 -> d [4][4]."""
    d = [[0] * 4 for _ in range(4)]
    for k, c in enumerate(coeff16):
        i, j = divmod(R.ZIGZAG[k], 4)
        ls = R._level_scale(q, i, j)
        d[i][j] = (c * ls) << (q // 6 - 4) if q >= 24 else (c * ls + (1 << (3 - q // 6))) >> (4 - q // 6)
    return d


def _median(a, b, c):
    return a + b + c - min(a, b, c) - max(a, b, c)


class _Picture:
    def __init__(self, mbw, mbh):
        self.mbw, self.mbh = mbw, mbh
        self.Y = np.zeros((16 * mbh, 16 * mbw), dtype=np.int64)
        self.C = np.zeros((2, 8 * mbh, 8 * mbw), dtype=np.int64)
        self.slice_of = [-1] * (mbw * mbh)
        self.nz_y = np.zeros((4 * mbh, 4 * mbw), dtype=np.int64)
        self.nz_c = np.zeros((2, 2 * mbh, 2 * mbw), dtype=np.int64)
        self.mv = [(0, 0)] * (mbw * mbh)
        self.ref = [-1] * (mbw * mbh)                                  # refIdxL0, -1 = intra (or not yet decoded)
        self.n_pcm = self.n_skip = self.n_inter = self.n_intra = 0


def _neighbour(pic, mb, dx, dy, slice_no):
    """(available, refIdx, mv) of the macroblock at (dx, dy) from ``mb`` (6.4.8: in the picture, already decoded, same slice)."""
    my, mx = divmod(mb, pic.mbw)
    x, y = mx + dx, my + dy
    if not (0 <= x < pic.mbw and 0 <= y < pic.mbh):
        return False, -1, (0, 0)
    other = y * pic.mbw + x
    if other >= mb or pic.slice_of[other] != slice_no:
        return False, -1, (0, 0)
    return True, pic.ref[other], pic.mv[other]


def _mv_pred_16x16(pic, mb, slice_no):
    """8.4.1.3 for one 16x16 partition with refIdxL0 0: median prediction with its availability rules."""
    a, b, c, d = (_neighbour(pic, mb, dx, dy, slice_no) for dx, dy in ((-1, 0), (0, -1), (1, -1), (-1, -1)))
    if not c[0]:
        c = d
    if not b[0] and not c[0] and a[0]:
        b = c = a
    same = [n for n in (a, b, c) if n[1] == 0]
    if len(same) == 1:
        return same[0][2]
    return _median(a[2][0], b[2][0], c[2][0]), _median(a[2][1], b[2][1], c[2][1])


def _mv_skip(pic, mb, slice_no):
    """8.4.1.1: the inferred vector of a P_Skip macroblock."""
    a, b = _neighbour(pic, mb, -1, 0, slice_no), _neighbour(pic, mb, 0, -1, slice_no)
    if not a[0] or not b[0] or (a[1] == 0 and a[2] == (0, 0)) or (b[1] == 0 and b[2] == (0, 0)):
        return 0, 0
    return _mv_pred_16x16(pic, mb, slice_no)


def _inter_pred(ref, mv, x0, y0, size, shift):
    """8.4.2.2 for whole-sample vectors: a copy, reference coordinates clamped into the picture."""
    if mv[0] % (4 << shift) or mv[1] % (4 << shift):
        raise NotWholeSample(mv)
    h, w = ref.shape
    ys = np.clip(np.arange(y0, y0 + size) + mv[1] // (4 << shift), 0, h - 1)
    xs = np.clip(np.arange(x0, x0 + size) + mv[0] // (4 << shift), 0, w - 1)
    return ref[np.ix_(ys, xs)]


def _n_c(nz, by, bx, my4, mx4, avail_a, avail_b):
    a = int(nz[by, bx - 1]) if (bx > mx4 or avail_a) else None
    b = int(nz[by - 1, bx]) if (by > my4 or avail_b) else None
    return (a + b + 1) >> 1 if (a is not None and b is not None) else a if a is not None else b if b is not None else 0


def _chroma_residual(rd, pic, my, mx, cbp_chroma, qpc, avail_a, avail_b):
    """residual of both chroma components -> r [2][4] 4x4 arrays (8.5.11)."""
    dcs = [R._residual_block(rd, -1, 4)[0] if cbp_chroma else [0] * 4 for _ in range(2)]
    out = []
    for cc in range(2):
        fm = R.H2 @ np.array(dcs[cc], dtype=np.int64).reshape(2, 2) @ R.H2
        dcc = [[(int(fm[i, j]) * R._level_scale(qpc, 0, 0) << (qpc // 6)) >> 5 for j in range(2)] for i in range(2)]
        blocks = []
        for b in range(4):
            by, bx = b >> 1, b & 1
            ac = [0] * 15
            if cbp_chroma == 2:
                ac, pic.nz_c[cc, 2 * my + by, 2 * mx + bx] = R._residual_block(
                    rd, _n_c(pic.nz_c[cc], 2 * my + by, 2 * mx + bx, 2 * my, 2 * mx, avail_a, avail_b), 15)
            else:
                pic.nz_c[cc, 2 * my + by, 2 * mx + bx] = 0
            d = R._scale_ac(ac, qpc)
            d[0][0] = dcc[by][bx]
            blocks.append(np.array(R._idct_rows_cols(d)))
        out.append(blocks)
    return out


def _decode_intra16(rd, pic, mb, t, qp, avail_a, avail_b):
    """An Intra16x16 macroblock of I-slice mb_type ``t`` (1 .. 24); returns the new QP."""
    my, mx = divmod(mb, pic.mbw)
    y0, x0 = 16 * my, 16 * mx
    Y, C = pic.Y, pic.C
    pred_mode, cbp_chroma, cbp_luma = (t - 1) % 4, ((t - 1) // 4) % 3, 15 if t >= 13 else 0
    chroma_mode = rd.ue()
    qp = (qp + rd.se() + 52) % 52
    assert pred_mode == 2 and chroma_mode == 0, "only DC prediction is decoded here"
    if avail_a and avail_b:                                             # 8.3.3.3
        pred = (int(Y[y0 - 1, x0:x0 + 16].sum()) + int(Y[y0:y0 + 16, x0 - 1].sum()) + 16) >> 5
    elif avail_a:
        pred = (int(Y[y0:y0 + 16, x0 - 1].sum()) + 8) >> 4
    elif avail_b:
        pred = (int(Y[y0 - 1, x0:x0 + 16].sum()) + 8) >> 4
    else:
        pred = 128
    dc_coeff, _ = R._residual_block(rd, _n_c(pic.nz_y, 4 * my, 4 * mx, 4 * my, 4 * mx, avail_a, avail_b), 16)
    c = [[0] * 4 for _ in range(4)]
    for k, v in enumerate(dc_coeff):
        c[R.ZIGZAG[k] // 4][R.ZIGZAG[k] % 4] = v
    fm = R.H4 @ np.array(c, dtype=np.int64) @ R.H4                      # 8.5.10
    ls0 = R._level_scale(qp, 0, 0)
    dcy = [[int(fm[i, j]) * ls0 << (qp // 6 - 6) if qp >= 36 else (int(fm[i, j]) * ls0 + (1 << (5 - qp // 6))) >> (6 - qp // 6)
            for j in range(4)] for i in range(4)]
    for b in range(16):
        bx, by = R.BLK_XY[b][0] // 4, R.BLK_XY[b][1] // 4
        ac = [0] * 15
        if cbp_luma:
            ac, pic.nz_y[4 * my + by, 4 * mx + bx] = R._residual_block(rd, _n_c(pic.nz_y, 4 * my + by, 4 * mx + bx, 4 * my, 4 * mx, avail_a, avail_b), 15)
        else:
            pic.nz_y[4 * my + by, 4 * mx + bx] = 0
        d = R._scale_ac(ac, qp)
        d[0][0] = dcy[by][bx]
        Y[y0 + 4 * by:y0 + 4 * by + 4, x0 + 4 * bx:x0 + 4 * bx + 4] = np.clip(pred + np.array(R._idct_rows_cols(d)), 0, 255)
    cy0, cx0 = 8 * my, 8 * mx
    res = _chroma_residual(rd, pic, my, mx, cbp_chroma, R.QPC[qp], avail_a, avail_b)
    for cc in range(2):
        for b in range(4):
            by, bx = b >> 1, b & 1
            yy, xx = cy0 + 4 * by, cx0 + 4 * bx                         # 8.3.4 DC prediction of the chroma block at (4 bx, 4 by)
            top = int(C[cc, yy - 1, xx:xx + 4].sum()) if avail_b else None
            lft = int(C[cc, yy:yy + 4, cx0 - 1].sum()) if avail_a else None
            if (bx, by) in ((0, 0), (1, 1)):
                p = (top + lft + 4) >> 3 if (top is not None and lft is not None) else (lft + 2) >> 2 if lft is not None else \
                    (top + 2) >> 2 if top is not None else 128
            elif (bx, by) == (1, 0):
                p = (top + 2) >> 2 if top is not None else (lft + 2) >> 2 if lft is not None else 128
            else:
                p = (lft + 2) >> 2 if lft is not None else (top + 2) >> 2 if top is not None else 128
            C[cc, yy:yy + 4, xx:xx + 4] = np.clip(p + res[cc][b], 0, 255)
    return qp


def _decode_pcm(rd, pic, mb):
    my, mx = divmod(mb, pic.mbw)
    y0, x0 = 16 * my, 16 * mx
    while rd.pos % 8:
        assert rd.u(1) == 0
    pic.Y[y0:y0 + 16, x0:x0 + 16] = np.array([rd.u(8) for _ in range(256)]).reshape(16, 16)
    for c in range(2):
        pic.C[c, y0 // 2:y0 // 2 + 8, x0 // 2:x0 // 2 + 8] = np.array([rd.u(8) for _ in range(64)]).reshape(8, 8)
    pic.nz_y[4 * my:4 * my + 4, 4 * mx:4 * mx + 4] = 16
    pic.nz_c[:, 2 * my:2 * my + 2, 2 * mx:2 * mx + 2] = 16
    pic.n_pcm += 1


def _decode_inter(rd, pic, ref_pic, mb, mv, cbp, qp, avail_a, avail_b):
    """Prediction by ``mv`` from ``ref_pic`` plus the residual of coded_block_pattern ``cbp`` (0 for P_Skip); returns the new QP."""
    my, mx = divmod(mb, pic.mbw)
    y0, x0 = 16 * my, 16 * mx
    pic.mv[mb], pic.ref[mb] = mv, 0
    py = _inter_pred(ref_pic.Y, mv, x0, y0, 16, 0)
    pc = [_inter_pred(ref_pic.C[c], mv, x0 // 2, y0 // 2, 8, 1) for c in range(2)]    # chroma vectors are in 1/8 samples (8.4.1.4)
    if cbp:
        qp = (qp + rd.se() + 52) % 52
    for b in range(16):
        bx, by = R.BLK_XY[b][0] // 4, R.BLK_XY[b][1] // 4
        if (cbp >> (b >> 2)) & 1:
            co, pic.nz_y[4 * my + by, 4 * mx + bx] = R._residual_block(rd, _n_c(pic.nz_y, 4 * my + by, 4 * mx + bx, 4 * my, 4 * mx, avail_a, avail_b), 16)
            r = np.array(R._idct_rows_cols(_scale16(co, qp)))
        else:
            pic.nz_y[4 * my + by, 4 * mx + bx] = 0
            r = 0
        pic.Y[y0 + 4 * by:y0 + 4 * by + 4, x0 + 4 * bx:x0 + 4 * bx + 4] = np.clip(py[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] + r, 0, 255)
    if cbp >> 4:
        res = _chroma_residual(rd, pic, my, mx, cbp >> 4, R.QPC[qp], avail_a, avail_b)
    else:
        pic.nz_c[:, 2 * my:2 * my + 2, 2 * mx:2 * mx + 2] = 0
        res = [[0] * 4, [0] * 4]
    for cc in range(2):
        for b in range(4):
            by, bx = b >> 1, b & 1
            pic.C[cc, 8 * my + 4 * by:8 * my + 4 * by + 4, 8 * mx + 4 * bx:8 * mx + 4 * bx + 4] = \
                np.clip(pc[cc][4 * by:4 * by + 4, 4 * bx:4 * bx + 4] + res[cc][b], 0, 255)
    return qp


def _decode_picture(sample, mbw, mbh, ref_pic, pic_init_qp=26):
    """One mp4 sample -> (_Picture, list of slice header dicts)."""
    pic = _Picture(mbw, mbh)
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
        if is_p:                                                        # (pic_order_cnt_type 2: nothing; no redundant_pic_cnt)
            if rd.u(1):                                                 # num_ref_idx_active_override_flag
                assert rd.ue() == 0, "one active reference only"
            assert rd.u(1) == 0, "ref_pic_list_modification is not decoded here"
        if unit_type == 5:                                              # dec_ref_pic_marking()
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
        while more:                                                     # 7.3.4
            if is_p:
                run = rd.ue()
                hd.setdefault("skip_runs", []).append(run)
                for _ in range(run):
                    assert ref_pic is not None
                    pic.slice_of[mb] = slice_no
                    _decode_inter(rd, pic, ref_pic, mb, _mv_skip(pic, mb, slice_no), 0, qp, False, False)
                    pic.n_skip += 1
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
                    mvp = _mv_pred_16x16(pic, mb, slice_no)             # (ref_idx_l0 is absent: num_ref_idx_l0_active_minus1 is 0)
                    mv = (mvp[0] + rd.se(), mvp[1] + rd.se())
                    code = rd.ue()
                    assert code < 48
                    qp = _decode_inter(rd, pic, ref_pic, mb, mv, CBP_INTER[code], qp, avail_a, avail_b)
                    pic.n_inter += 1
                else:
                    t = mb_type - 5 if is_p else mb_type
                    if t == 25:
                        _decode_pcm(rd, pic, mb)
                    else:
                        assert 1 <= t <= 24, "only Intra16x16 and I_PCM of the intra types are decoded here"
                        qp = _decode_intra16(rd, pic, mb, t, qp, avail_a, avail_b)
                        pic.n_intra += 1
                mb += 1
                more = rd.more_rbsp_data()
        slice_no += 1
    assert all(s >= 0 for s in pic.slice_of), "a macroblock was never coded"
    return pic, headers


def decode_stream(samples, width, height):
    """The samples of one track in order -> dict(y [n, 16 mbh, 16 mbw], cb, cr: every decoded sample, the cropped-away border included;
    sync: positions of the IDR pictures; headers; n_pcm, n_skip, n_inter, n_intra)."""
    mbw, mbh = (width + 15) // 16, (height + 15) // 16
    ys, cbs, crs, sync, all_headers = [], [], [], [], []
    ref, prev_frame_num, prev_idr = None, None, None
    counts = dict(n_pcm=0, n_skip=0, n_inter=0, n_intra=0)
    for k, sample in enumerate(samples):
        pic, headers = _decode_picture(sample, mbw, mbh, ref)
        assert len({(h["nal_unit_type"], h["frame_num"], h["slice_type"] % 5, h.get("idr_pic_id")) for h in headers}) == 1, "one picture, one kind"
        h0 = headers[0]
        if h0["nal_unit_type"] == 5:                                    # 7.4.3
            assert h0["frame_num"] == 0
            if prev_idr is not None and prev_idr[0] == k - 1:
                assert h0["idr_pic_id"] != prev_idr[1], "two consecutive IDR pictures share idr_pic_id"
            prev_idr = (k, h0["idr_pic_id"])
            sync.append(k)
        else:
            assert prev_frame_num is not None, "a P picture with nothing before it"
            assert h0["frame_num"] == (prev_frame_num + 1) % 16, "frame_num must grow by one (mod 16) from reference picture to reference picture"
        prev_frame_num = h0["frame_num"]
        ref = pic
        ys.append(pic.Y.astype(np.uint8)), cbs.append(pic.C[0].astype(np.uint8)), crs.append(pic.C[1].astype(np.uint8))
        all_headers.append(headers)
        for key in counts:
            counts[key] += getattr(pic, key)
    return dict(y=np.stack(ys), cb=np.stack(cbs), cr=np.stack(crs), sync=sync, headers=all_headers, **counts)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, qp):
    """(planes, samples, (ry, rcb, rcr), stats) of one case of the case set, computed once for all the tests that read it."""
    n, h, w, gop = shape
    planes = make_planes(kind, n, h, w)
    stats = new_stats()
    samples, ry, rcb, rcr = encode_planes(*planes, qp=qp, gop=gop, first_index=FIRST, stats=stats)
    return planes, samples, (ry, rcb, rcr), stats
