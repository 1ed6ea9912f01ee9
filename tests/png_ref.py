"""Restatement of the PNG encoder's stream (stable_diffusion_videos_amd/png.py, csrc/sdv_png.hip) in numpy and Python integers: the
row filters with libpng's choice, heap Huffman for the optimal cost, a sequential bit writer that produces a whole file from given
code lengths, a chunk parser that checks every CRC.  No tolerance anywhere: the codec is lossless."""
import heapq
import io
import struct
import zlib

import numpy as np
from PIL import Image

# (n, H, W), stripe_rows (None = the encoder's default): the cases of tests/test_png_gpu.py
CASES = (((1, 1, 1), None),        # the smallest frame
         ((2, 5, 7), 2),           # a batch, a ragged last stripe, odd row bytes
         ((1, 33, 19), 16),        # three stripes, the last one a single row
         ((1, 3, 400), 1),         # a row longer than one workgroup pass; the row-0 prior
         ((1, 70, 24), 1),         # more than 64 stripes in a frame: the scan beyond one wave
         ((3, 40, 56), None))      # a plain batch
KINDS = ("zeros", "const255", "noise", "smooth")
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)     # RFC 1951 3.2.7


def default_stripe_rows(H, W):
    return max(1, min(H, 32768 // (1 + 3 * W)))


def make_frames(kind, n, H, W, seed=5):
    """The test contents: seeded, uint8 [n, H, W, 3]."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    if kind == "zeros":
        return np.zeros((n, H, W, 3), dtype=np.uint8)
    if kind == "const255":
        return np.full((n, H, W, 3), 255, dtype=np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    if kind == "smooth":                                # smooth pattern + a little noise + one saturated rectangle
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        out = np.empty((n, H, W, 3))
        for k in range(n):
            for c in range(3):
                out[k, :, :, c] = 128 + 90 * np.sin(x / (5.0 + 2 * c) + k) * np.cos(y / (7.0 - c) + 0.3 * c)
        out += rng.normal(0, 2, out.shape)
        out[:, H // 4:H // 2, W // 4:W // 2 + 1] = (255, 0, 255)
        return np.clip(np.round(out), 0, 255).astype(np.uint8)
    raise ValueError(kind)


# ---- filters ---------------------------------------------------------------------------------------------------------------------
def _candidates(cur, up):
    """The five filtered versions of one row: int64 [5, 3W] (bpp = 3; cur / up as int64 [3W])."""
    a = np.concatenate([np.zeros(3, dtype=np.int64), cur[:-3]])
    c = np.concatenate([np.zeros(3, dtype=np.int64), up[:-3]])
    p = a + up - c
    pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
    return np.stack([cur, cur - a, cur - up, cur - (a + up) // 2, cur - paeth]) & 0xFF


def filter_rows(frames):
    """uint8 [n, H, W, 3] -> uint8 [n, H, 1 + 3W]: per row the type with the smallest sum of (v < 128 ? v : 256 - v), ties to the
    lowest type; row 0 sees a row of zeros above."""
    n, H, W, _ = frames.shape
    out = np.empty((n, H, 1 + 3 * W), dtype=np.uint8)
    for k in range(n):
        up = np.zeros(3 * W, dtype=np.int64)
        for y in range(H):
            cur = frames[k, y].reshape(-1).astype(np.int64)
            cand = _candidates(cur, up)
            cost = np.where(cand < 128, cand, 256 - cand).sum(axis=1)
            t = int(np.argmin(cost))                    # (argmin returns the first minimum)
            out[k, y, 0] = t
            out[k, y, 1:] = cand[t]
            up = cur
    return out


def adler_partials(filtered):
    """int32 [n, H, 2]: per row (sum d_j, sum (R - j) d_j) mod 65521 - what the filter kernel hands to the packer."""
    n, H, R = filtered.shape
    d = filtered.astype(np.int64)
    w = R - np.arange(R, dtype=np.int64)
    return np.stack([d.sum(axis=2) % 65521, (d * w).sum(axis=2) % 65521], axis=2).astype(np.int32)


# ---- Huffman ---------------------------------------------------------------------------------------------------------------------
def stripe_histograms(filtered_frame, stripe_rows):
    """int64 [stripes, 257] of one frame's filtered rows [H, R]; end-of-block counts 1."""
    H = filtered_frame.shape[0]
    hists = []
    for r0 in range(0, H, stripe_rows):
        h = np.bincount(filtered_frame[r0:r0 + stripe_rows].reshape(-1), minlength=257).astype(np.int64)
        h[256] = 1
        hists.append(h)
    return np.stack(hists)


def heap_lengths(hist, shallow=False):
    """Code lengths of one unrestricted Huffman code of the histogram: int list [len(hist)].  Heap; among equal weights a merged node
    goes before a leaf (then the older node, the smaller symbol).  Every tie-break gives the same cost; this one gives the DEEP trees -
    on Fibonacci counts with one more 1, where every merge is a tie, the single chain - so `optimal_depth(h) <= 15` is the cautious
    premise.  ``shallow=True``: a leaf goes before a node, which gives the flattest of the equally cheap trees."""
    heap = [(int(c), 0 if shallow else 1, i, (i,)) for i, c in enumerate(hist) if c > 0]
    lengths = [0] * len(hist)
    if len(heap) == 1:
        lengths[heap[0][2]] = 1
        return lengths
    heapq.heapify(heap)
    tick = 0
    while len(heap) > 1:
        c1, _, _, s1 = heapq.heappop(heap)
        c2, _, _, s2 = heapq.heappop(heap)
        for s in s1 + s2:
            lengths[s] += 1
        heapq.heappush(heap, (c1 + c2, 1 if shallow else 0, tick, s1 + s2))
        tick += 1
    return lengths


def optimal_cost(hist):
    return sum(int(c) * l for c, l in zip(hist, heap_lengths(hist)))


def optimal_depth(hist, shallow=False):
    """The depth of the heap's code (see heap_lengths for which of the equally cheap codes that is)."""
    return max(heap_lengths(hist, shallow))


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f


def fibonacci_buffer():
    """The length-limiting case: uint8 [1, 1, 4181], a type byte 0 and behind it 4180 bytes of the 17 values 0 .. 16 with the Fibonacci
    counts 1597, 987, ..., 2, 1, 1, shuffled (seeded).  With the type byte and end-of-block the counts are 1, 1, 1, 2, 3, ..., 987,
    1598: a Huffman code of them can be a single chain, 17 deep - but every merge on the way is a tie, and the flattest of the equally
    cheap trees is 10 deep.  Whether an encoder has to limit lengths here depends on how it breaks ties.
    4181 is no 1 + 3W, so the 4181 bytes go to the packer as [1, 113, 37] (W = 12) with stripe_rows = 113: one stripe, the same bytes
    in the same order; the packer never looks at rows."""
    fib = _fib(17)
    assert sum(fib) == 4180 and fib[-1] == 1597
    body = np.repeat(np.arange(17, dtype=np.uint8), fib[::-1])
    np.random.default_rng(11).shuffle(body)
    return np.concatenate([np.zeros(1, dtype=np.uint8), body]).reshape(1, 113, 37)


def forced_deep_buffer():
    """uint8 [1, 1, 6763]: the 17 values 0 .. 16 with the counts F18 = 2584, ..., F3 = 2, F2 = 1 over all 6763 bytes (the type byte 0
    is one of the 2584), shuffled (seeded).  End-of-block is the F1 = 1: the counts are exactly Fibonacci, each larger than the sum of
    all up to the one-but-last before it, so no merge is a tie and EVERY Huffman code of them is the 17-deep chain: no encoder gets
    past this one without limiting lengths."""
    fib = _fib(18)[1:]
    assert sum(fib) == 6763 and (6763 - 1) % 3 == 0
    body = np.repeat(np.arange(17, dtype=np.uint8), fib[::-1])[1:]                # (one of the zeros is the type byte)
    np.random.default_rng(12).shuffle(body)
    return np.concatenate([np.zeros(1, dtype=np.uint8), body]).reshape(1, 1, 6763)


def check_lengths(lengths, hist, optimal):
    """Valid: 0 exactly for unused symbols, at most 15, Kraft sum exactly 1; and, where asked, the optimal cost."""
    lengths = [int(l) for l in lengths]
    assert len(lengths) == 257 == len(hist)
    for s in range(257):
        assert (lengths[s] == 0) == (hist[s] == 0), (s, lengths[s], int(hist[s]))
        assert 0 <= lengths[s] <= 15, (s, lengths[s])
    assert sum(1 << (15 - l) for l in lengths if l) == 1 << 15
    if optimal:
        assert sum(int(c) * l for c, l in zip(hist, lengths)) == optimal_cost(hist)


# ---- the sequential packer -------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):                        # plain integer field
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, nbits):                    # Huffman code: most significant bit first
        self.put(int(format(code, f"0{nbits}b")[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def canonical_codes(lengths):
    """RFC 1951 3.2.2."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def png_header(H, W):
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))


def deflate_stripes(filtered_frame, lengths, stripe_rows):
    """The zlib stream of one frame: 78 01 | per stripe a dynamic block (no matches, plain 4-bit table) + an empty stored block | 03 00 |
    Adler-32.  filtered_frame uint8 [H, R]; lengths [stripes, 257]."""
    H = filtered_frame.shape[0]
    out = bytearray(b"\x78\x01")
    for s, r0 in enumerate(range(0, H, stripe_rows)):
        ls = [int(l) for l in lengths[s]]
        codes = canonical_codes(ls)
        w = BitWriter()
        w.put(0, 1)                                     # BFINAL
        w.put(2, 2)                                     # BTYPE = 10: dynamic Huffman
        w.put(0, 5)                                     # HLIT: 257 literal / length codes
        w.put(0, 5)                                     # HDIST: 1 distance code
        w.put(15, 4)                                    # HCLEN: all 19 code-length code lengths
        for sym in CL_ORDER:
            w.put(0 if sym >= 16 else 4, 3)
        for l in ls + [0]:                              # 257 lengths + the one distance length, each the 4-bit code of its value
            w.put_code(l, 4)
        for v in filtered_frame[r0:r0 + stripe_rows].reshape(-1).tolist():
            w.put_code(codes[v], ls[v])
        w.put_code(codes[256], ls[256])
        w.put(0, 3)                                     # BFINAL 0, BTYPE 00: stored, empty
        w.align()
        out += w.out + b"\x00\x00\xff\xff"
    out += b"\x03\x00"
    return bytes(out) + struct.pack(">I", zlib.adler32(filtered_frame.tobytes()))


def pack(filtered, lengths, H, W, stripe_rows):
    """list[bytes]: the whole files from filtered rows uint8 [n, H, 1 + 3W] and code lengths [n, stripes, 257]."""
    assert filtered.shape[1:] == (H, 1 + 3 * W)
    return [png_header(H, W) + chunk(b"IDAT", deflate_stripes(filtered[k], lengths[k], stripe_rows)) + chunk(b"IEND", b"")
            for k in range(filtered.shape[0])]


def encode(frames, stripe_rows=None):
    """The whole restatement: filter, heap Huffman per stripe, pack."""
    n, H, W, _ = frames.shape
    sr = stripe_rows or default_stripe_rows(H, W)
    filtered = filter_rows(frames)
    lengths = [[heap_lengths(h) for h in stripe_histograms(filtered[k], sr)] for k in range(n)]
    return pack(filtered, lengths, H, W, sr), filtered


# ---- decoders --------------------------------------------------------------------------------------------------------------------
def chunks(data):
    """[(tag, payload)] of a PNG file; asserts the signature, every CRC, and that nothing follows IEND."""
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(data):
        (length,), tag = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        payload = data[pos + 8:pos + 8 + length]
        assert len(payload) == length
        assert struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])[0] == zlib.crc32(tag + payload), tag
        out.append((tag, payload))
        pos += 12 + length
    assert pos == len(data) and out[-1][0] == b"IEND"
    return out


def idat(data):
    """The zlib stream of a file with the layout signature | IHDR | one IDAT | IEND (every CRC checked)."""
    cs = chunks(data)
    assert [t for t, _ in cs] == [b"IHDR", b"IDAT", b"IEND"]
    return cs[1][1]


def decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == "RGB"
    return np.asarray(im)
