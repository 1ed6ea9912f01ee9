"""Reference restatement of the baseline JPEG stream of stable_diffusion_videos_amd/jpeg.py (helper, not a test).

Written from ITU-T T.81 (Annex A: FDCT / quantisation / zigzag, Annex F: Huffman coding of DC differences and AC run/size
pairs, Annex K: example tables, B.2: markers) and the JFIF 1.01 note, not from the kernels:

  * ``transform``  float64 numpy: edge replication to multiples of 16, JFIF full-range YCbCr, 2x2 chroma means, level shift,
                   orthonormal 8x8 DCT-II, division by the table entry, round half away from zero, zigzag.
  * ``pack``       a plain sequential Huffman packer: header + one restart interval per MCU row.

The decoder every file is held against is PIL (libjpeg); the code under test is never the reference.
"""
from __future__ import annotations

import io

import numpy as np

# ---- Annex K.1 / K.2 quantisation tables (natural, row-major order) ----------------------------------------------------------
K1_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
K2_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                      47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)

# ---- Annex K.3 - K.6 "typical" Huffman tables: BITS (codes per length 1..16) and HUFFVAL ------------------------------------------
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0,
    0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]
# header order: DC luma, AC luma, DC chroma, AC chroma  (Tc << 4 | Th, BITS, HUFFVAL)
HUFFMAN_SPECS = ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                 (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS))


def _zigzag_order():
    """ZZ[k] = natural (row * 8 + column) index of the k-th coefficient of the zigzag sequence (T.81 figure A.6)."""
    out = []
    for s in range(15):
        cells = [(i, s - i) for i in range(8) if 0 <= s - i < 8]          # (row, column) on the anti-diagonal row + column = s
        out += cells if s % 2 else cells[::-1]                              # even diagonals run bottom-left -> top-right
    return np.array([r * 8 + c for r, c in out])


ZZ = _zigzag_order()


def quant_tables(quality: int):
    """(luma, chroma) int arrays [64], natural order: Annex K scaled by the libjpeg rule."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be 1..100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (K1_LUMA, K2_CHROMA))


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def jfif_header(H: int, W: int, quality: int) -> bytes:
    """SOI, APP0, DQT x2, SOF0, DHT x4, DRI, SOS - everything in front of the entropy-coded data."""
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8"
    out += _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))                 # 1.01, aspect ratio 1:1, no thumbnail
    out += _segment(0xDB, bytes([0]) + bytes(int(v) for v in ql[ZZ]))
    out += _segment(0xDB, bytes([1]) + bytes(int(v) for v in qc[ZZ]))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") +
                    bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in HUFFMAN_SPECS:
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, ((W + 15) // 16).to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def _dct_matrix():
    x = np.arange(8)
    C = np.cos((2 * x[None, :] + 1) * x[:, None] * np.pi / 16) / 2
    C[0] /= np.sqrt(2.0)
    return C


def transform_real(frames_u8: np.ndarray, quality: int) -> np.ndarray:
    """float64 [n, mcu_rows, mcu_cols, 6, 64]: DCT coefficient / table entry BEFORE rounding, zigzag order."""
    f = np.asarray(frames_u8)
    assert f.dtype == np.uint8 and f.ndim == 4 and f.shape[3] == 3
    n, H, W, _ = f.shape
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    f = np.pad(f, ((0, 0), (0, Hp - H), (0, Wp - W), (0, 0)), mode="edge").astype(np.float64)
    R, G, B = f[..., 0], f[..., 1], f[..., 2]
    Y = 0.299 * R + 0.587 * G + 0.114 * B
    Cb = 128 - 0.168735892 * R - 0.331264108 * G + 0.5 * B
    Cr = 128 + 0.5 * R - 0.418687589 * G - 0.081312411 * B
    down = lambda p: p.reshape(n, Hp // 2, 2, Wp // 2, 2).mean(axis=(2, 4))
    ql, qc = quant_tables(quality)
    C = _dct_matrix()

    def blocks(p, q):                                  # [n, h, w] -> [n, h/8, w/8, 64] zigzag
        h, w = p.shape[1:]
        b = (p - 128.0).reshape(n, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4)
        d = np.einsum("ui,nrcij,vj->nrcuv", C, b, C)
        return (d / q.reshape(8, 8).astype(np.float64)).reshape(n, h // 8, w // 8, 64)[..., ZZ]

    y, cb, cr = blocks(Y, ql), blocks(down(Cb), qc), blocks(down(Cr), qc)
    out = np.empty((n, Hp // 16, Wp // 16, 6, 64), dtype=np.float64)
    out[:, :, :, 0], out[:, :, :, 1] = y[:, 0::2, 0::2], y[:, 0::2, 1::2]
    out[:, :, :, 2], out[:, :, :, 3] = y[:, 1::2, 0::2], y[:, 1::2, 1::2]
    out[:, :, :, 4], out[:, :, :, 5] = cb, cr
    return out


def round_half_away(x: np.ndarray) -> np.ndarray:
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int16)


def transform(frames_u8: np.ndarray, quality: int) -> np.ndarray:
    """int16 [n, mcu_rows, mcu_cols, 6, 64] quantised coefficients, zigzag order, MCU block order Y00 Y01 Y10 Y11 Cb Cr."""
    return round_half_away(transform_real(frames_u8, quality))


def _huffman_codes(bits, vals):
    """symbol -> (code, length): T.81 Annex C (codes of one length are consecutive, next length = (code + 1) << 1)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


class _BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value: int, length: int):
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self) -> bytes:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)       # pad with 1-bits
        return bytes(self.out)


def _category_bits(v: int):
    a = abs(v)
    size = a.bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def pack(coef: np.ndarray, H: int, W: int, quality: int):
    """list[bytes]: one complete file per frame of int16 ``coef`` [n, mcu_rows, mcu_cols, 6, 64]."""
    dc = [_huffman_codes(DC_LUMA_BITS, DC_VALS), _huffman_codes(DC_CHROMA_BITS, DC_VALS)]
    ac = [_huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), _huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    header = jfif_header(H, W, quality)
    coef = np.asarray(coef)
    n, rows, cols = coef.shape[:3]
    assert (rows, cols) == ((H + 15) // 16, (W + 15) // 16) and coef.shape[3:] == (6, 64)
    files = []
    for f in range(n):
        body = bytearray(header)
        for r in range(rows):
            bw = _BitWriter()
            pred = [0, 0, 0]
            for m in range(cols):
                for k in range(6):
                    comp = max(k - 3, 0)
                    t = 0 if comp == 0 else 1
                    blk = [int(v) for v in coef[f, r, m, k]]
                    size, extra = _category_bits(blk[0] - pred[comp])
                    pred[comp] = blk[0]
                    bw.put(*dc[t][size])
                    bw.put(extra, size)
                    run = 0
                    for v in blk[1:]:
                        if v == 0:
                            run += 1
                            continue
                        while run > 15:
                            bw.put(*ac[t][0xF0])
                            run -= 16
                        size, extra = _category_bits(v)
                        bw.put(*ac[t][(run << 4) | size])
                        bw.put(extra, size)
                        run = 0
                    if run:
                        bw.put(*ac[t][0x00])
            body += bw.flush()
            if r < rows - 1:
                body += bytes([0xFF, 0xD0 + (r & 7)])
        body += b"\xff\xd9"
        files.append(bytes(body))
    return files


def encode(frames_u8: np.ndarray, quality: int):
    n, H, W, _ = frames_u8.shape
    return pack(transform(frames_u8, quality), H, W, quality)


# ---- shared by the CPU and the GPU tests -----------------------------------------------------------------------------------------
def decode(data: bytes) -> np.ndarray:
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.format == "JPEG" and im.mode == "RGB"
    return np.asarray(im)


def pil_encode(frame_u8: np.ndarray, quality: int) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame_u8).save(buf, format="JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def make_frames(kind: str, n: int, H: int, W: int, seed: int = 3) -> np.ndarray:
    """The test contents: seeded, uint8 [n, H, W, 3].  (Seed 3: every GPU case stays under MAX_EXCUSED_SHARE by the restatement alone -
    test_jpeg_cpu.py checks it; with seed 0 the 16 x 16 smooth image at quality 95 has 9 of its 384 coefficients in the window.)"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    if kind == "smooth":                                # smooth pattern + Gaussian noise + one saturated rectangle
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        out = np.empty((n, H, W, 3))
        for k in range(n):
            for c in range(3):
                out[k, :, :, c] = 128 + 90 * np.sin(x / (5.0 + 2 * c) + k) * np.cos(y / (7.0 - c) + 0.3 * c)
        out += rng.normal(0, 6, out.shape)
        out[:, H // 4:H // 2, W // 4:W // 2 + 1] = (255, 0, 255)
        return np.clip(np.round(out), 0, 255).astype(np.uint8)
    if kind == "grey":
        return np.full((n, H, W, 3), 128, dtype=np.uint8)
    if kind == "white":
        return np.full((n, H, W, 3), 255, dtype=np.uint8)
    if kind == "black":
        return np.zeros((n, H, W, 3), dtype=np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:H, 0:W]
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[None, :, :, None], 3, axis=3).repeat(n, axis=0)
    if kind == "noise":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    raise ValueError(kind)


# Half-integer window of test (a): where the float64 value / q lies within DELTA of k + 0.5 the fp32 kernel may round the other way.
# 16 fp32 FMAs per output on partial sums of at most 1024 (1024 * 16 * 2^-24 = 1e-3) + the colour conversion's rounding amplified by
# the DCT gain of 8 (4e-4), with a margin; the share of coefficients excused this way is capped per case.
DELTA = 5e-3
MAX_EXCUSED_SHARE = 0.02

# Measured on the CPU by tests/test_jpeg_cpu.py::test_restatement_against_pil (which asserts them): how far this stream format,
# evaluated in float64, falls short of PIL's own save(quality=q, subsampling=2) on the same image - PSNR against the source in dB
# (libjpeg's integer colour conversion, DCT and chroma filter differ from the float arithmetic, in either direction) and file size
# (restart markers and byte padding per MCU row; tiny files are mostly header).  Obtained by running that test's loop with a print
# in place of the assertion, over every content at every GPU-test shape and quality 1 / 75 / 95 / 100: the largest PSNR gap was
# 0.18 dB (smooth, 72 x 24, quality 1; 0.03 dB at quality 75 / 95), the largest size ratio 1.108.  Rounded up:
PSNR_MARGIN_DB = 0.2
SIZE_RATIO_MAX = 1.12
TIE_FLIP_DB = 0.2          # on top, for the GPU: coefficients inside the DELTA window that the fp32 kernel rounds the other way

SHAPES = ((1, 16, 16), (2, 40, 56), (1, 72, 24), (1, 32, 208), (1, 160, 16))
KINDS = ("smooth", "grey", "white", "black", "checker", "noise")


def gpu_qualities(kind: str, shape) -> tuple:
    """Qualities the GPU suite runs a content at: 75 and 95 everywhere, 100 for uniform noise on every shape (longest codes, most
    0xFF stuffing, the payload outgrows the encoder's first buffer) and for the smooth image on one, 1 on one shape."""
    q = [75, 95]
    if kind == "noise" or (kind == "smooth" and tuple(shape) == (2, 40, 56)):
        q.append(100)
    if kind == "smooth" and tuple(shape) == (1, 72, 24):
        q.append(1)
    return tuple(q)
