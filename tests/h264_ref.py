"""The H.264 CAVLC intra stream rule (DESIGN.md "H.264 CAVLC intra encoder", include/sdv_hip.h) restated in plain Python / numpy, and a
decoder written separately from the decoding clauses of ITU-T Rec. H.264.

(a) ``encode_planes`` / ``encode_frames``: the encoder rule, macroblock by macroblock, with its own reconstruction.
(b) ``decode_sample``: 7.3.3 slice header, 7.3.5 / 7.3.5.3 macroblock and residual syntax, 9.2 CAVLC parsing, 8.3.3 / 8.3.4 intra
    prediction (DC), 8.5 inverse transforms, I_PCM.  Its VLC tables are the bit strings of Tables 9-5, 9-7, 9-8, 9-9 and 9-10, walked as a
    prefix tree; the encoder above looks its code words up in the same strings.  Nothing here imports the package's encoder.
(c) ``make_planes``: the frame kinds of the test suites.
"""
import numpy as np

# ------------------------------------------------------------------------------------------------------------------------------------
# Tables 9-5 (coeff_token; keys (TrailingOnes, TotalCoeff)), 9-7 / 9-8 / 9-9 (total_zeros), 9-10 (run_before) as bit strings
# ------------------------------------------------------------------------------------------------------------------------------------
COEFF_TOKEN = (  # 0 <= nC < 2 | 2 <= nC < 4 | 4 <= nC < 8 | 8 <= nC | nC == -1 (chroma DC)
    {(0, 0): "1", (0, 1): "000101", (1, 1): "01", (0, 2): "00000111", (1, 2): "000100", (2, 2): "001", (0, 3): "000000111", (1, 3): "00000110", (2, 3): "0000101", (3, 3): "00011", (0, 4): "0000000111", (1, 4): "000000110", (2, 4): "00000101", (3, 4): "000011", (0, 5): "00000000111", (1, 5): "0000000110", (2, 5): "000000101", (3, 5): "0000100", (0, 6): "0000000001111", (1, 6): "00000000110", (2, 6): "0000000101", (3, 6): "00000100", (0, 7): "0000000001011", (1, 7): "0000000001110", (2, 7): "00000000101", (3, 7): "000000100", (0, 8): "0000000001000", (1, 8): "0000000001010", (2, 8): "0000000001101", (3, 8): "0000000100", (0, 9): "00000000001111", (1, 9): "00000000001110", (2, 9): "0000000001001", (3, 9): "00000000100", (0, 10): "00000000001011", (1, 10): "00000000001010", (2, 10): "00000000001101", (3, 10): "0000000001100", (0, 11): "000000000001111", (1, 11): "000000000001110", (2, 11): "00000000001001", (3, 11): "00000000001100", (0, 12): "000000000001011", (1, 12): "000000000001010", (2, 12): "000000000001101", (3, 12): "00000000001000", (0, 13): "0000000000001111", (1, 13): "000000000000001", (2, 13): "000000000001001", (3, 13): "000000000001100", (0, 14): "0000000000001011", (1, 14): "0000000000001110", (2, 14): "0000000000001101", (3, 14): "000000000001000", (0, 15): "0000000000000111", (1, 15): "0000000000001010", (2, 15): "0000000000001001", (3, 15): "0000000000001100", (0, 16): "0000000000000100", (1, 16): "0000000000000110", (2, 16): "0000000000000101", (3, 16): "0000000000001000"},
    {(0, 0): "11", (0, 1): "001011", (1, 1): "10", (0, 2): "000111", (1, 2): "00111", (2, 2): "011", (0, 3): "0000111", (1, 3): "001010", (2, 3): "001001", (3, 3): "0101", (0, 4): "00000111", (1, 4): "000110", (2, 4): "000101", (3, 4): "0100", (0, 5): "00000100", (1, 5): "0000110", (2, 5): "0000101", (3, 5): "00110", (0, 6): "000000111", (1, 6): "00000110", (2, 6): "00000101", (3, 6): "001000", (0, 7): "00000001111", (1, 7): "000000110", (2, 7): "000000101", (3, 7): "000100", (0, 8): "00000001011", (1, 8): "00000001110", (2, 8): "00000001101", (3, 8): "0000100", (0, 9): "000000001111", (1, 9): "00000001010", (2, 9): "00000001001", (3, 9): "000000100", (0, 10): "000000001011", (1, 10): "000000001110", (2, 10): "000000001101", (3, 10): "00000001100", (0, 11): "000000001000", (1, 11): "000000001010", (2, 11): "000000001001", (3, 11): "00000001000", (0, 12): "0000000001111", (1, 12): "0000000001110", (2, 12): "0000000001101", (3, 12): "000000001100", (0, 13): "0000000001011", (1, 13): "0000000001010", (2, 13): "0000000001001", (3, 13): "0000000001100", (0, 14): "0000000000111", (1, 14): "00000000001011", (2, 14): "0000000000110", (3, 14): "0000000001000", (0, 15): "00000000001001", (1, 15): "00000000001000", (2, 15): "00000000001010", (3, 15): "0000000000001", (0, 16): "00000000000111", (1, 16): "00000000000110", (2, 16): "00000000000101", (3, 16): "00000000000100"},
    {(0, 0): "1111", (0, 1): "001111", (1, 1): "1110", (0, 2): "001011", (1, 2): "01111", (2, 2): "1101", (0, 3): "001000", (1, 3): "01100", (2, 3): "01110", (3, 3): "1100", (0, 4): "0001111", (1, 4): "01010", (2, 4): "01011", (3, 4): "1011", (0, 5): "0001011", (1, 5): "01000", (2, 5): "01001", (3, 5): "1010", (0, 6): "0001001", (1, 6): "001110", (2, 6): "001101", (3, 6): "1001", (0, 7): "0001000", (1, 7): "001010", (2, 7): "001001", (3, 7): "1000", (0, 8): "00001111", (1, 8): "0001110", (2, 8): "0001101", (3, 8): "01101", (0, 9): "00001011", (1, 9): "00001110", (2, 9): "0001010", (3, 9): "001100", (0, 10): "000001111", (1, 10): "00001010", (2, 10): "00001101", (3, 10): "0001100", (0, 11): "000001011", (1, 11): "000001110", (2, 11): "00001001", (3, 11): "00001100", (0, 12): "000001000", (1, 12): "000001010", (2, 12): "000001101", (3, 12): "00001000", (0, 13): "0000001101", (1, 13): "000000111", (2, 13): "000001001", (3, 13): "000001100", (0, 14): "0000001001", (1, 14): "0000001100", (2, 14): "0000001011", (3, 14): "0000001010", (0, 15): "0000000101", (1, 15): "0000001000", (2, 15): "0000000111", (3, 15): "0000000110", (0, 16): "0000000001", (1, 16): "0000000100", (2, 16): "0000000011", (3, 16): "0000000010"},
    {(0, 0): "000011", (0, 1): "000000", (1, 1): "000001", (0, 2): "000100", (1, 2): "000101", (2, 2): "000110", (0, 3): "001000", (1, 3): "001001", (2, 3): "001010", (3, 3): "001011", (0, 4): "001100", (1, 4): "001101", (2, 4): "001110", (3, 4): "001111", (0, 5): "010000", (1, 5): "010001", (2, 5): "010010", (3, 5): "010011", (0, 6): "010100", (1, 6): "010101", (2, 6): "010110", (3, 6): "010111", (0, 7): "011000", (1, 7): "011001", (2, 7): "011010", (3, 7): "011011", (0, 8): "011100", (1, 8): "011101", (2, 8): "011110", (3, 8): "011111", (0, 9): "100000", (1, 9): "100001", (2, 9): "100010", (3, 9): "100011", (0, 10): "100100", (1, 10): "100101", (2, 10): "100110", (3, 10): "100111", (0, 11): "101000", (1, 11): "101001", (2, 11): "101010", (3, 11): "101011", (0, 12): "101100", (1, 12): "101101", (2, 12): "101110", (3, 12): "101111", (0, 13): "110000", (1, 13): "110001", (2, 13): "110010", (3, 13): "110011", (0, 14): "110100", (1, 14): "110101", (2, 14): "110110", (3, 14): "110111", (0, 15): "111000", (1, 15): "111001", (2, 15): "111010", (3, 15): "111011", (0, 16): "111100", (1, 16): "111101", (2, 16): "111110", (3, 16): "111111"},
    {(0, 0): "01", (0, 1): "000111", (1, 1): "1", (0, 2): "000100", (1, 2): "000110", (2, 2): "001", (0, 3): "000011", (1, 3): "0000011", (2, 3): "0000010", (3, 3): "000101", (0, 4): "000010", (1, 4): "00000011", (2, 4): "00000010", (3, 4): "0000000"},
)
TOTAL_ZEROS = (  # [tzVlcIndex - 1][total_zeros], 4x4 blocks
    ("1", "011", "010", "0011", "0010", "00011", "00010", "000011", "000010", "0000011", "0000010", "00000011", "00000010", "000000011", "000000010", "000000001"),
    ("111", "110", "101", "100", "011", "0101", "0100", "0011", "0010", "00011", "00010", "000011", "000010", "000001", "000000"),
    ("0101", "111", "110", "101", "0100", "0011", "100", "011", "0010", "00011", "00010", "000001", "00001", "000000"),
    ("00011", "111", "0101", "0100", "110", "101", "100", "0011", "011", "0010", "00010", "00001", "00000"),
    ("0101", "0100", "0011", "111", "110", "101", "100", "011", "0010", "00001", "0001", "00000"),
    ("000001", "00001", "111", "110", "101", "100", "011", "010", "0001", "001", "000000"),
    ("000001", "00001", "101", "100", "011", "11", "010", "0001", "001", "000000"),
    ("000001", "0001", "00001", "011", "11", "10", "010", "001", "000000"),
    ("000001", "000000", "0001", "11", "10", "001", "01", "00001"),
    ("00001", "00000", "001", "11", "10", "01", "0001"),
    ("0000", "0001", "001", "010", "1", "011"),
    ("0000", "0001", "01", "1", "001"),
    ("000", "001", "1", "01"),
    ("00", "01", "1"),
    ("0", "1"),
)
TOTAL_ZEROS_CHROMA_DC = (("1", "01", "001", "000"), ("1", "01", "00"), ("1", "0"))
RUN_BEFORE = (  # [min(zerosLeft, 7) - 1][run_before]
    ("1", "0"),
    ("1", "01", "00"),
    ("11", "10", "01", "00"),
    ("11", "10", "01", "001", "000"),
    ("11", "10", "011", "010", "001", "000"),
    ("11", "000", "001", "011", "010", "101", "100"),
    ("111", "110", "101", "100", "011", "010", "001", "0001", "00001", "000001", "0000001", "00000001", "000000001", "0000000001", "00000000001"),
)

ZIGZAG = (0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15)               # raster index (row * 4 + column) of scan position k
BLK_XY = tuple((8 * ((i >> 2) & 1) + 4 * (i & 1), 8 * (i >> 3) + 4 * ((i >> 1) & 1)) for i in range(16))   # luma4x4BlkIdx -> (x, y), 6.4.3
CF = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], dtype=np.int64)
H4 = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], dtype=np.int64)
H2 = np.array([[1, 1], [1, -1]], dtype=np.int64)
MF = ((13107, 5243, 8066), (11916, 4660, 7490), (10082, 4194, 6554), (9362, 3647, 5825), (8192, 3355, 5243), (7282, 2893, 4559))
NORM = ((10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23))                 # normAdjust4x4, 8.5.9
POS_CLASS = np.array([[0 if (i % 2 == 0 and j % 2 == 0) else 1 if (i % 2 and j % 2) else 2 for j in range(4)] for i in range(4)])
QPC = tuple(range(30)) + (29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39)   # Table 8-15
MAX_MB_BITS = 3200                                                             # Annex A.3.1, Baseline
KINDS = ("flat", "ramp", "glyphs", "noise", "zeros_pcm")


def slot_bytes(mbw):
    """The documented capacity of one slice in the sample (sdv_hip.h): 4-byte length + NAL header + the RBSP bound (8 bytes of slice
    header and stop bit, 400 per macroblock) with an emulation-prevention byte behind every second byte."""
    rbsp = 400 * mbw + 8
    return 5 + rbsp + rbsp // 2


# ------------------------------------------------------------------------------------------------------------------------------------
# colour and planes
# ------------------------------------------------------------------------------------------------------------------------------------
def rgb_to_planes(frames):
    """uint8 RGB [n, H, W, 3] (H, W even) -> Y [n, 16 mbh, 16 mbw], Cb, Cr [n, 8 mbh, 8 mbw]: the integer BT.601 rule, edge-replicated."""
    f = np.asarray(frames).astype(np.int64)
    n, h, w, _ = f.shape
    assert h % 2 == 0 and w % 2 == 0
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16
    box = lambda c: c.reshape(n, h // 2, 2, w // 2, 2).sum(axis=(2, 4))
    cb = ((box(-38 * r - 74 * g + 112 * b) + 512) >> 10) + 128
    cr = ((box(112 * r - 94 * g - 18 * b) + 512) >> 10) + 128
    return pad_planes(y.astype(np.uint8), cb.astype(np.uint8), cr.astype(np.uint8))


def pad_planes(y, cb, cr):
    n, h, w = y.shape
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    y = np.pad(y, ((0, 0), (0, mbh * 16 - h), (0, mbw * 16 - w)), mode="edge")
    cb = np.pad(cb, ((0, 0), (0, mbh * 8 - h // 2), (0, mbw * 8 - w // 2)), mode="edge")
    cr = np.pad(cr, ((0, 0), (0, mbh * 8 - h // 2), (0, mbw * 8 - w // 2)), mode="edge")
    return y, cb, cr


def make_frames(kind, n, h, w, seed=0):
    """uint8 RGB [n, h, w, 3] of one of the RGB kinds."""
    rng = np.random.default_rng(seed + 17 * n + h + 3 * w)
    if kind == "flat":
        f = np.empty((n, h, w, 3), dtype=np.uint8)
        f[:] = np.array([90, 140, 200], dtype=np.uint8)
    elif kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        f = np.stack([np.stack([(3 * xx + k * 7) % 256, (2 * yy + xx) % 256, (xx * yy // 8 + 5 * k) % 256], axis=-1) for k in range(n)]).astype(np.uint8)
    elif kind == "glyphs":                                          # dark background, a few bright rectangles and single pixels
        f = np.full((n, h, w, 3), 8, dtype=np.uint8)
        for k in range(n):
            for _ in range(max(2, h * w // 400)):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                hh, ww = int(rng.integers(1, 7)), int(rng.integers(1, 9))
                f[k, y0:y0 + hh, x0:x0 + ww] = rng.integers(0, 256, 3, dtype=np.uint8) if rng.integers(0, 2) else 255
            f[k, :, w // 2:w // 2 + 16] = 250                        # a flat bright column of macroblocks next to the dark ones
    elif kind == "noise":
        f = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    else:
        raise ValueError(kind)
    return f


def make_planes(kind, n, h, w, seed=0):
    """Padded planes of every kind; ``zeros_pcm`` exists as planes only (sample values 0 .. 3, which no RGB input maps to)."""
    if kind == "zeros_pcm":
        rng = np.random.default_rng(seed + 5 * n + h + w)
        p = lambda s: np.where(rng.random(s) < 0.7, 0, rng.integers(0, 4, s)).astype(np.uint8)
        return pad_planes(p((n, h, w)), p((n, h // 2, w // 2)), p((n, h // 2, w // 2)))
    return rgb_to_planes(make_frames(kind, n, h, w, seed))


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
class Uncodable(Exception):
    pass


def ue(v):
    return format(v + 1, "b").zfill(2 * (v + 1).bit_length() - 1)


def se(v):
    return ue(2 * v - 1 if v > 0 else -2 * v)


def _quant(w, mf, f, qbits):
    a = (np.abs(w) * mf + f) >> qbits
    return np.where(w < 0, -a, a)


def _inverse4x4(d):
    """8.5.12.2: rows, then columns, then (x + 32) >> 6."""
    def one_d(v):
        e0, e1, e2, e3 = v[0] + v[2], v[0] - v[2], (v[1] >> 1) - v[3], v[1] + (v[3] >> 1)
        return np.array([e0 + e3, e1 + e2, e1 - e2, e0 - e3])
    f = np.stack([one_d(d[i]) for i in range(4)])
    g = np.stack([one_d(f[:, j]) for j in range(4)], axis=1)
    return (g + 32) >> 6


def _luma_dc_dequant(f, qp):
    v, k = NORM[qp % 6][0], qp // 6
    return (f * v) << (k - 2) if k >= 2 else (f * v + (1 << (1 - k))) >> (2 - k)      # = (f * 16 v << k) >> 6 with the rounding of 8.5.10


def level_code_bits(level_code, sl):
    """level_prefix / level_suffix of 9.2.2.1 for one levelCode at suffixLength ``sl``; Uncodable when level_prefix would pass 15."""
    if sl == 0:
        if level_code < 14:
            return level_code, "0" * level_code + "1"
        if level_code < 30:
            return 14, "0" * 14 + "1" + format(level_code - 14, "04b")
        rest = level_code - 30
    else:
        if level_code < (15 << sl):
            return level_code >> sl, "0" * (level_code >> sl) + "1" + format(level_code & ((1 << sl) - 1), "0%db" % sl)
        rest = level_code - (15 << sl)
    if rest >= 4096:
        raise Uncodable
    return 15, "0" * 15 + "1" + format(rest, "012b")


def code_block(levels, nC, stats=None):
    """residual_block_cavlc() of 7.3.5.3.2 for ``levels`` in scan order -> (bit string, TotalCoeff)."""
    maxc = len(levels)
    nz = [i for i, v in enumerate(levels) if v]
    total = len(nz)
    t1 = 0
    for i in reversed(nz):
        if abs(levels[i]) == 1 and t1 < 3:
            t1 += 1
        else:
            break
    table = 4 if nC < 0 else 0 if nC < 2 else 1 if nC < 4 else 2 if nC < 8 else 3
    out = [COEFF_TOKEN[table][(t1, total)]]
    if stats is not None:
        stats["nc_class"].add(table)
    if total == 0:
        return out[0], 0
    rev = nz[::-1]                                                   # highest frequency first
    for i in rev[:t1]:
        out.append("1" if levels[i] < 0 else "0")
    sl = 1 if total > 10 and t1 < 3 else 0
    for k, i in enumerate(rev[t1:]):
        v = levels[i]
        lc = 2 * v - 2 if v > 0 else -2 * v - 1
        if k == 0 and t1 < 3:
            lc -= 2
        prefix, bits = level_code_bits(lc, sl)
        if stats is not None:
            stats["suffix_length"].add(sl)
            stats["level_prefix"].add(prefix)
        out.append(bits)
        if sl == 0:
            sl = 1
        if abs(v) > (3 << (sl - 1)) and sl < 6:
            sl += 1
    if total < maxc:
        tz = nz[-1] + 1 - total
        out.append((TOTAL_ZEROS_CHROMA_DC if maxc == 4 else TOTAL_ZEROS)[total - 1][tz])
        left = tz
        for a, b in zip(rev[:-1], rev[1:]):
            if left <= 0:
                break
            run = a - b - 1
            out.append(RUN_BEFORE[min(left, 7) - 1][run])
            left -= run
    return "".join(out), total


def _nc(a, b):
    if a is not None and b is not None:
        return (a + b + 1) >> 1
    return a if a is not None else b if b is not None else 0


class _Left:
    """What a macroblock hands to its right neighbour: the reconstructed right columns and the AC TotalCoeff of its right blocks."""
    def __init__(self, ycol, ccol, tc_y, tc_c):
        self.ycol, self.ccol, self.tc_y, self.tc_c = ycol, ccol, tc_y, tc_c


def encode_mb(sy, sc, left, qp, stats):
    """One macroblock: source samples ``sy`` [16, 16], ``sc`` [2, 8, 8] -> (bit string, recon Y, recon C [2, 8, 8], _Left, is_pcm)."""
    sy, sc = sy.astype(np.int64), sc.astype(np.int64)
    qbits, f = 15 + qp // 6, (1 << (15 + qp // 6)) // 3
    mf, nv = np.array(MF[qp % 6])[POS_CLASS], np.array(NORM[qp % 6])[POS_CLASS]
    pred_y = 128 if left is None else (int(left.ycol.sum()) + 8) >> 4
    ac_y, dc = [None] * 16, np.zeros((4, 4), dtype=np.int64)
    for b, (x, y) in enumerate(BLK_XY):
        w = CF @ (sy[y:y + 4, x:x + 4] - pred_y) @ CF.T
        dc[y // 4, x // 4] = w[0, 0]
        ac_y[b] = _quant(w, mf, f, qbits).reshape(-1)[list(ZIGZAG)][1:]
    dc_lev = _quant((H4 @ dc @ H4 + 1) >> 1, MF[qp % 6][0], 2 * f, qbits + 1).reshape(-1)[list(ZIGZAG)]
    qpc = QPC[qp]
    qbc, fc = 15 + qpc // 6, (1 << (15 + qpc // 6)) // 3
    mfc, nvc = np.array(MF[qpc % 6])[POS_CLASS], np.array(NORM[qpc % 6])[POS_CLASS]
    pred_c = np.full((2, 8, 8), 128, dtype=np.int64)
    if left is not None:
        for c in range(2):
            pred_c[c, :4], pred_c[c, 4:] = (int(left.ccol[c, :4].sum()) + 2) >> 2, (int(left.ccol[c, 4:].sum()) + 2) >> 2
    ac_c, dc_c = [[None] * 4, [None] * 4], []
    for c in range(2):
        d2 = np.zeros((2, 2), dtype=np.int64)
        for b in range(4):
            y, x = 4 * (b >> 1), 4 * (b & 1)
            w = CF @ (sc[c, y:y + 4, x:x + 4] - pred_c[c, y:y + 4, x:x + 4]) @ CF.T
            d2[b >> 1, b & 1] = w[0, 0]
            ac_c[c][b] = _quant(w, mfc, fc, qbc).reshape(-1)[list(ZIGZAG)][1:]
        dc_c.append(_quant(H2 @ d2 @ H2, MF[qpc % 6][0], 2 * fc, qbc + 1).reshape(-1))
    cbp_luma = 15 if any(a.any() for a in ac_y) else 0
    cbp_chroma = 2 if any(a.any() for cc in ac_c for a in cc) else 1 if any(d.any() for d in dc_c) else 0
    # ---- bits
    tc_y, tc_c = np.zeros((4, 4), dtype=np.int64), np.zeros((2, 2, 2), dtype=np.int64)
    why = None
    try:
        out = [ue(1 + 2 + 4 * cbp_chroma + (12 if cbp_luma else 0)), ue(0), se(0)]
        la = None if left is None else int(left.tc_y[0])
        out.append(code_block([int(v) for v in dc_lev], _nc(la, None), stats)[0])
        if cbp_luma:
            for b, (x, y) in enumerate(BLK_XY):
                bx, by = x // 4, y // 4
                a = int(tc_y[by, bx - 1]) if bx else (None if left is None else int(left.tc_y[by]))
                t = int(tc_y[by - 1, bx]) if by else None
                bits, tc_y[by, bx] = code_block([int(v) for v in ac_y[b]], _nc(a, t), stats)
                out.append(bits)
        if cbp_chroma:
            for c in range(2):
                out.append(code_block([int(v) for v in dc_c[c]], -1, stats)[0])
        if cbp_chroma == 2:
            for c in range(2):
                for b in range(4):
                    by, bx = b >> 1, b & 1
                    a = int(tc_c[c, by, bx - 1]) if bx else (None if left is None else int(left.tc_c[c, by]))
                    t = int(tc_c[c, by - 1, bx]) if by else None
                    bits, tc_c[c, by, bx] = code_block([int(v) for v in ac_c[c][b]], _nc(a, t), stats)
                    out.append(bits)
        bits = "".join(out)
        if len(bits) > MAX_MB_BITS:
            why = "bits"
    except Uncodable:
        why = "level"
    if why is not None:
        stats["pcm"].add(why)
        return None, sy, sc, _Left(sy[:, 15].copy(), sc[:, :, 7].copy(), np.full(4, 16), np.full((2, 2), 16)), True
    stats["cbp_luma"].add(cbp_luma)
    stats["cbp_chroma"].add(cbp_chroma)
    if left is not None and int(left.tc_y[0]) == 16 and int(left.tc_c[0, 0]) == 16:
        stats["pcm_left"] = True
    # ---- reconstruction (8.5.2, 8.5.10, 8.5.11, 8.5.12)
    k = qp // 6
    c4 = np.zeros(16, dtype=np.int64)
    c4[list(ZIGZAG)] = dc_lev
    dcy = _luma_dc_dequant(H4 @ c4.reshape(4, 4) @ H4, qp)
    ry = np.empty((16, 16), dtype=np.int64)
    for b, (x, y) in enumerate(BLK_XY):
        lv = np.zeros(16, dtype=np.int64)
        lv[list(ZIGZAG)[1:]] = ac_y[b]
        d = (lv.reshape(4, 4) * nv) << k
        d[0, 0] = dcy[y // 4, x // 4]
        ry[y:y + 4, x:x + 4] = np.clip(pred_y + _inverse4x4(d), 0, 255)
    kc = qpc // 6
    rc = np.empty((2, 8, 8), dtype=np.int64)
    for c in range(2):
        dcc = ((H2 @ dc_c[c].reshape(2, 2) @ H2) * NORM[qpc % 6][0] << kc) >> 1
        for b in range(4):
            y, x = 4 * (b >> 1), 4 * (b & 1)
            lv = np.zeros(16, dtype=np.int64)
            lv[list(ZIGZAG)[1:]] = ac_c[c][b]
            d = (lv.reshape(4, 4) * nvc) << kc
            d[0, 0] = dcc[b >> 1, b & 1]
            rc[c, y:y + 4, x:x + 4] = np.clip(pred_c[c, y:y + 4, x:x + 4] + _inverse4x4(d), 0, 255)
    return bits, ry, rc, _Left(ry[:, 15].copy(), rc[:, :, 7].copy(), tc_y[:, 3].copy(), tc_c[:, :, 1].copy()), False


def new_stats():
    return dict(nc_class=set(), suffix_length=set(), level_prefix=set(), cbp_luma=set(), cbp_chroma=set(), pcm=set(), pcm_left=False,
                mb_bits=[], n_pcm=0)


def slice_header(first_mb, idr_pic_id, qp):
    return ue(first_mb) + ue(7) + ue(0) + "0000" + ue(idr_pic_id) + "00" + se(qp - 26) + ue(1)


_EPB_LIMIT = 3


def escape(rbsp):
    out, zeros = bytearray(), 0
    for b in rbsp:
        if zeros >= 2 and b <= _EPB_LIMIT:
            out.append(3)
            zeros = 0
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def encode_planes(y, cb, cr, qp=16, first_index=0, stats=None):
    """Padded planes [n, 16 mbh, 16 mbw] / [n, 8 mbh, 8 mbw] -> (samples: list[bytes], recon Y, recon Cb, recon Cr)."""
    assert 0 <= qp <= 51
    stats = new_stats() if stats is None else stats
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    ry, rcb, rcr = np.empty_like(y), np.empty_like(cb), np.empty_like(cr)
    samples = []
    for k in range(n):
        sample = bytearray()
        for r in range(mbh):
            bits, left = [slice_header(r * mbw, (first_index + k) & 1, qp)], None
            for m in range(mbw):
                sy = y[k, 16 * r:16 * r + 16, 16 * m:16 * m + 16]
                sc = np.stack([cb[k, 8 * r:8 * r + 8, 8 * m:8 * m + 8], cr[k, 8 * r:8 * r + 8, 8 * m:8 * m + 8]])
                mb, py, pc, left, pcm = encode_mb(sy, sc, left, qp, stats)
                if pcm:
                    bits.append(ue(25))
                    bits.append("0" * (-sum(map(len, bits)) % 8))
                    bits.append("".join(format(int(v), "08b") for v in np.concatenate([sy.reshape(-1), sc.reshape(-1)])))
                    stats["n_pcm"] += 1
                    stats["mb_bits"].append(len(bits[-1]) + len(bits[-2]) + 9)
                else:
                    bits.append(mb)
                    stats["mb_bits"].append(len(mb))
                ry[k, 16 * r:16 * r + 16, 16 * m:16 * m + 16] = py
                rcb[k, 8 * r:8 * r + 8, 8 * m:8 * m + 8], rcr[k, 8 * r:8 * r + 8, 8 * m:8 * m + 8] = pc[0], pc[1]
            s = "".join(bits) + "1"
            s += "0" * (-len(s) % 8)
            nal = bytes([0x65]) + escape(int(s, 2).to_bytes(len(s) // 8, "big"))
            assert 4 + len(nal) <= slot_bytes(mbw)
            sample += len(nal).to_bytes(4, "big") + nal
        samples.append(bytes(sample))
    return samples, ry, rcb, rcr


def encode_frames(frames, qp=16, first_index=0, stats=None):
    return encode_planes(*rgb_to_planes(frames), qp=qp, first_index=first_index, stats=stats)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the decoder
# ------------------------------------------------------------------------------------------------------------------------------------
def _trie(codes):
    root = [None, None]
    for sym, code in codes:
        node = root
        for ch in code[:-1]:
            i = int(ch)
            if node[i] is None:
                node[i] = [None, None]
            node = node[i]
            assert isinstance(node, list), "not prefix-free"
        assert node[int(code[-1])] is None, "not prefix-free"
        node[int(code[-1])] = (sym,)
    return root


_T_COEFF = tuple(_trie(t.items()) for t in COEFF_TOKEN)
_T_TZ = tuple(_trie(enumerate(t)) for t in TOTAL_ZEROS)
_T_TZC = tuple(_trie(enumerate(t)) for t in TOTAL_ZEROS_CHROMA_DC)
_T_RUN = tuple(_trie(enumerate(t)) for t in RUN_BEFORE)


class BitReader:
    def __init__(self, data):
        self.bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8)).tolist()
        self.pos = 0
        self.end = len(self.bits) - 1 - self.bits[::-1].index(1)      # the rbsp_stop_one_bit

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bits[self.pos]
            self.pos += 1
        return v

    def ue(self):
        z = 0
        while self.bits[self.pos] == 0:
            z += 1
            self.pos += 1
        return self.u(z + 1) - 1

    def se(self):
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)

    def vlc(self, trie):
        node = trie
        while True:
            node = node[self.bits[self.pos]]
            self.pos += 1
            assert node is not None, "no such code word"
            if isinstance(node, tuple):
                return node[0]

    def more_rbsp_data(self):
        return self.pos < self.end


def unescape(nal_payload):
    out, zeros = bytearray(), 0
    for b in nal_payload:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        assert not (zeros >= 2 and b < 3), "00 00 0x inside a NAL unit"
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def _residual_block(rd, nC, maxc):
    """9.2: -> (coefficient list in scan order, TotalCoeff)."""
    t1, total = rd.vlc(_T_COEFF[4 if nC < 0 else 0 if nC < 2 else 1 if nC < 4 else 2 if nC < 8 else 3])
    coeff = [0] * maxc
    if total == 0:
        return coeff, 0
    assert total <= maxc
    level = []
    suffix_length = 1 if total > 10 and t1 < 3 else 0
    for i in range(total):
        if i < t1:
            level.append(1 - 2 * rd.u(1))
            continue
        prefix = 0
        while rd.u(1) == 0:
            prefix += 1
        assert prefix <= 15, "level_prefix above 15 is not allowed in the Baseline profile"
        level_code = min(15, prefix) << suffix_length
        size = 4 if (prefix == 14 and suffix_length == 0) else prefix - 3 if prefix >= 15 else suffix_length
        if size:
            level_code += rd.u(size)
        if prefix >= 15 and suffix_length == 0:
            level_code += 15
        if i == t1 and t1 < 3:
            level_code += 2
        level.append((level_code + 2) >> 1 if level_code % 2 == 0 else (-level_code - 1) >> 1)
        if suffix_length == 0:
            suffix_length = 1
        if abs(level[-1]) > (3 << (suffix_length - 1)) and suffix_length < 6:
            suffix_length += 1
    zeros_left = 0
    if total < maxc:
        zeros_left = rd.vlc((_T_TZC if maxc == 4 else _T_TZ)[total - 1])
    run = []
    for i in range(total - 1):
        r = rd.vlc(_T_RUN[min(zeros_left, 7) - 1]) if zeros_left > 0 else 0
        run.append(r)
        zeros_left -= r
    run.append(zeros_left)
    pos = -1
    for i in range(total - 1, -1, -1):
        pos += run[i] + 1
        coeff[pos] = level[i]
    return coeff, total


def _idct_rows_cols(d):
    r = [[0] * 4 for _ in range(4)]
    for i in range(4):
        a, b, c, e = d[i]
        e0, e1, e2, e3 = a + c, a - c, (b >> 1) - e, b + (e >> 1)
        r[i] = [e0 + e3, e1 + e2, e1 - e2, e0 - e3]
    out = [[0] * 4 for _ in range(4)]
    for j in range(4):
        a, b, c, e = r[0][j], r[1][j], r[2][j], r[3][j]
        e0, e1, e2, e3 = a + c, a - c, (b >> 1) - e, b + (e >> 1)
        for i, v in enumerate((e0 + e3, e1 + e2, e1 - e2, e0 - e3)):
            out[i][j] = (v + 32) >> 6
    return out


def _level_scale(q, i, j):
    v = NORM[q % 6]
    return 16 * (v[0] if (i % 2 == 0 and j % 2 == 0) else v[1] if (i % 2 == 1 and j % 2 == 1) else v[2])


def _scale_ac(coeff15, q):
    """8.5.12.1 for a block whose DC comes from elsewhere: scan positions 1 .. 15 -> d [4][4] (d[0][0] left 0)."""
    d = [[0] * 4 for _ in range(4)]
    for k, c in enumerate(coeff15):
        i, j = divmod(ZIGZAG[k + 1], 4)
        ls = _level_scale(q, i, j)
        d[i][j] = (c * ls) << (q // 6 - 4) if q >= 24 else (c * ls + (1 << (3 - q // 6))) >> (4 - q // 6)
    return d


def decode_sample(sample, width, height, sps_pps_qp=26):
    """One mp4 sample (length-prefixed slice NAL units of one picture) -> dict(y, cb, cr cropped to the picture; headers: list of slice
    header fields; n_pcm)."""
    mbw, mbh = (width + 15) // 16, (height + 15) // 16
    Y = np.zeros((16 * mbh, 16 * mbw), dtype=np.int64)
    C = np.zeros((2, 8 * mbh, 8 * mbw), dtype=np.int64)
    slice_of = [-1] * (mbw * mbh)
    nz_y = np.zeros((4 * mbh, 4 * mbw), dtype=np.int64)
    nz_c = np.zeros((2, 2 * mbh, 2 * mbw), dtype=np.int64)
    headers, n_pcm, at, slice_no = [], 0, 0, 0
    while at < len(sample):
        size = int.from_bytes(sample[at:at + 4], "big")
        nal = sample[at + 4:at + 4 + size]
        at += 4 + size
        assert nal[0] == 0x65, "nal_ref_idc 3, nal_unit_type 5"
        assert nal[-1] != 0
        rd = BitReader(unescape(nal[1:]))
        hd = dict(first_mb=rd.ue(), slice_type=rd.ue(), pps_id=rd.ue(), frame_num=rd.u(4), idr_pic_id=rd.ue(), no_output=rd.u(1),
                  long_term=rd.u(1), qp_delta=rd.se(), deblock_idc=rd.ue(), nal_bytes=size)
        assert hd["deblock_idc"] == 1                                 # (idc != 1 would carry two offsets and need the loop filter)
        headers.append(hd)
        qp = sps_pps_qp + hd["qp_delta"]
        mb = hd["first_mb"]
        while True:
            my, mx = divmod(mb, mbw)
            slice_of[mb] = slice_no
            avail_a = mx > 0 and slice_of[mb - 1] == slice_no
            avail_b = my > 0 and slice_of[mb - mbw] == slice_no
            mb_type = rd.ue()
            y0, x0 = 16 * my, 16 * mx
            if mb_type == 25:
                while rd.pos % 8:
                    assert rd.u(1) == 0
                Y[y0:y0 + 16, x0:x0 + 16] = np.array([rd.u(8) for _ in range(256)]).reshape(16, 16)
                for c in range(2):
                    C[c, y0 // 2:y0 // 2 + 8, x0 // 2:x0 // 2 + 8] = np.array([rd.u(8) for _ in range(64)]).reshape(8, 8)
                nz_y[4 * my:4 * my + 4, 4 * mx:4 * mx + 4] = 16
                nz_c[:, 2 * my:2 * my + 2, 2 * mx:2 * mx + 2] = 16
                n_pcm += 1
            else:
                assert 1 <= mb_type <= 24, "only Intra16x16 and I_PCM are decoded here"
                pred_mode, cbp_chroma, cbp_luma = (mb_type - 1) % 4, ((mb_type - 1) // 4) % 3, 15 if mb_type >= 13 else 0
                chroma_mode = rd.ue()
                qp = (qp + rd.se() + 52) % 52
                assert pred_mode == 2 and chroma_mode == 0, "only DC prediction is decoded here"
                # 8.3.3.3 Intra_16x16_DC
                if avail_a and avail_b:
                    pred = (int(Y[y0 - 1, x0:x0 + 16].sum()) + int(Y[y0:y0 + 16, x0 - 1].sum()) + 16) >> 5
                elif avail_a:
                    pred = (int(Y[y0:y0 + 16, x0 - 1].sum()) + 8) >> 4
                elif avail_b:
                    pred = (int(Y[y0 - 1, x0:x0 + 16].sum()) + 8) >> 4
                else:
                    pred = 128

                def n_c(nz, by, bx, my4, mx4):
                    a = int(nz[by, bx - 1]) if (bx > mx4 or avail_a) else None
                    b = int(nz[by - 1, bx]) if (by > my4 or avail_b) else None
                    return (a + b + 1) >> 1 if (a is not None and b is not None) else a if a is not None else b if b is not None else 0

                dc_coeff, _ = _residual_block(rd, n_c(nz_y, 4 * my, 4 * mx, 4 * my, 4 * mx), 16)
                c = [[0] * 4 for _ in range(4)]
                for k, v in enumerate(dc_coeff):
                    c[ZIGZAG[k] // 4][ZIGZAG[k] % 4] = v
                fm = H4 @ np.array(c, dtype=np.int64) @ H4                                       # 8.5.10
                ls0 = _level_scale(qp, 0, 0)
                dcy = [[int(fm[i, j]) * ls0 << (qp // 6 - 6) if qp >= 36 else (int(fm[i, j]) * ls0 + (1 << (5 - qp // 6))) >> (6 - qp // 6)
                        for j in range(4)] for i in range(4)]
                for b in range(16):
                    bx, by = BLK_XY[b][0] // 4, BLK_XY[b][1] // 4
                    ac = [0] * 15
                    if cbp_luma:
                        ac, nz_y[4 * my + by, 4 * mx + bx] = _residual_block(rd, n_c(nz_y, 4 * my + by, 4 * mx + bx, 4 * my, 4 * mx), 15)
                    else:
                        nz_y[4 * my + by, 4 * mx + bx] = 0
                    d = _scale_ac(ac, qp)
                    d[0][0] = dcy[by][bx]
                    r = np.array(_idct_rows_cols(d))
                    Y[y0 + 4 * by:y0 + 4 * by + 4, x0 + 4 * bx:x0 + 4 * bx + 4] = np.clip(pred + r, 0, 255)
                qpc = QPC[qp]
                cy0, cx0 = 8 * my, 8 * mx
                dcs = []
                for cc in range(2):
                    dcs.append(_residual_block(rd, -1, 4)[0] if cbp_chroma else [0] * 4)
                for cc in range(2):
                    fm = H2 @ np.array(dcs[cc], dtype=np.int64).reshape(2, 2) @ H2                # 8.5.11
                    dcc = [[(int(fm[i, j]) * _level_scale(qpc, 0, 0) << (qpc // 6)) >> 5 for j in range(2)] for i in range(2)]
                    for b in range(4):
                        by, bx = b >> 1, b & 1
                        ac = [0] * 15
                        if cbp_chroma == 2:
                            ac, nz_c[cc, 2 * my + by, 2 * mx + bx] = _residual_block(rd, n_c(nz_c[cc], 2 * my + by, 2 * mx + bx, 2 * my, 2 * mx), 15)
                        else:
                            nz_c[cc, 2 * my + by, 2 * mx + bx] = 0
                        d = _scale_ac(ac, qpc)
                        d[0][0] = dcc[by][bx]
                        r = np.array(_idct_rows_cols(d))
                        # 8.3.4 DC prediction of the chroma 4x4 block at (xO, yO) = (4 bx, 4 by)
                        yy, xx = cy0 + 4 * by, cx0 + 4 * bx
                        top = int(C[cc, yy - 1, xx:xx + 4].sum()) if avail_b else None
                        lft = int(C[cc, yy:yy + 4, cx0 - 1].sum()) if avail_a else None
                        if (bx, by) in ((0, 0), (1, 1)):
                            order = (top, lft) if top is not None and lft is not None else None
                            p = (top + lft + 4) >> 3 if order else (lft + 2) >> 2 if lft is not None else (top + 2) >> 2 if top is not None else 128
                        elif (bx, by) == (1, 0):
                            p = (top + 2) >> 2 if top is not None else (lft + 2) >> 2 if lft is not None else 128
                        else:
                            p = (lft + 2) >> 2 if lft is not None else (top + 2) >> 2 if top is not None else 128
                        C[cc, yy:yy + 4, xx:xx + 4] = np.clip(p + r, 0, 255)
            mb += 1
            if not rd.more_rbsp_data():
                break
        slice_no += 1
    assert all(s >= 0 for s in slice_of), "a macroblock was never coded"
    return dict(y=Y[:height, :width].astype(np.uint8), cb=C[0, :height // 2, :width // 2].astype(np.uint8),
                cr=C[1, :height // 2, :width // 2].astype(np.uint8), headers=headers, n_pcm=n_pcm)


def mp4_samples(path):
    """(width, height, sample entry type, samples) of the video track of a file written by video.py."""
    data = open(path, "rb").read()

    def boxes(buf, lo, hi):
        while lo < hi:
            size, kind = int.from_bytes(buf[lo:lo + 4], "big"), buf[lo + 4:lo + 8]
            head = 8
            if size == 1:
                size, head = int.from_bytes(buf[lo + 8:lo + 16], "big"), 16
            yield kind, lo + head, lo + size
            lo += size

    def find(lo, hi, *path_):
        for kind, a, b in boxes(data, lo, hi):
            if kind == path_[0]:
                return (a, b) if len(path_) == 1 else find(a, b, *path_[1:])
        raise KeyError(path_)

    a, b = find(0, len(data), b"moov", b"trak", b"mdia", b"minf", b"stbl")
    sa, _ = find(a, b, b"stsd")
    entry = data[sa + 12:sa + 16]
    width, height = int.from_bytes(data[sa + 8 + 32:sa + 8 + 34], "big"), int.from_bytes(data[sa + 8 + 34:sa + 8 + 36], "big")
    za, _ = find(a, b, b"stsz")
    n = int.from_bytes(data[za + 8:za + 12], "big")
    sizes = [int.from_bytes(data[za + 12 + 4 * i:za + 16 + 4 * i], "big") for i in range(n)]
    ca, _ = find(a, b, b"stco")
    off = int.from_bytes(data[ca + 8:ca + 12], "big")
    samples = []
    for s in sizes:
        samples.append(data[off:off + s])
        off += s
    return width, height, entry, samples
