"""Restatement of the PNG encoder's matching mode (png.PngEncoder(matches=True), csrc/sdv_png.hip "Matches") in plain Python on top
of tests/png_ref.py: the tokeniser (nine candidates per position, the price rule, greedy parse), the token histograms, a sequential
packer that produces a whole file from given tokens and code lengths, and a bitwise CRC-32.  No tolerance anywhere."""
import struct
import zlib

import numpy as np

import png_ref as R

MAX_DIST = 32768
MAX_LEN = 258
GROUP = 64                                              # the hash sees only positions of earlier 64-position groups
# RFC 1951 3.2.5: (base, extra bits) of the length symbols 257 .. 285 and the distance symbols 0 .. 29
LEN_TABLE = ((3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2), (27, 2),
             (31, 2), (35, 3), (43, 3), (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5), (227, 5), (258, 0))
DIST_TABLE = ((1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (7, 1), (9, 2), (13, 2), (17, 3), (25, 3), (33, 4), (49, 4), (65, 5), (97, 5), (129, 6),
              (193, 6), (257, 7), (385, 7), (513, 8), (769, 8), (1025, 9), (1537, 9), (2049, 10), (3073, 10), (4097, 11), (6145, 11),
              (8193, 12), (12289, 12), (16385, 13), (24577, 13))
KINDS = R.KINDS + ("plateaus", "glyphs")


def make_frames(kind, n, H, W, seed=5):
    """png_ref's contents and two more: ``plateaus`` (a smooth pattern quantised to multiples of 8) and ``glyphs`` (a flat frame with
    a rectangle and a grid of thin lines)."""
    if kind in R.KINDS:
        return R.make_frames(kind, n, H, W, seed)
    rng = np.random.default_rng(seed + 1000 * H + W + 7)
    if kind == "plateaus":
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        out = np.empty((n, H, W, 3))
        for k in range(n):
            for c in range(3):
                out[k, :, :, c] = 128 + 100 * np.sin(x / (9.0 + 3 * c) + 0.7 * k) * np.cos(y / (11.0 - 2 * c) + 0.3 * c)
        return (np.clip(np.round(out), 0, 255).astype(np.uint8) // 8 * 8).astype(np.uint8)
    if kind == "glyphs":
        out = np.empty((n, H, W, 3), dtype=np.uint8)
        out[:] = (236, 238, 240)
        for k in range(n):
            out[k, ::7, :] = (20, 30, 40 + k)
            out[k, :, ::9] = (200, 10, 10)
            y0, x0 = int(rng.integers(0, max(1, H // 2))), int(rng.integers(0, max(1, W // 2)))
            out[k, y0:y0 + max(1, H // 3), x0:x0 + max(1, W // 3)] = (0, 90, 180)
        return out
    raise ValueError(kind)


def periodic_rows(period, H=56, Rb=1201, seed=21):
    """Hand-made filtered buffer uint8 [1, H, Rb]: ``period`` seeded noise rows, repeated.  No three consecutive bytes occur twice
    within the period (cyclically), so every repeat of three or more bytes lies a multiple of period * Rb back: 33 628 for period 28
    (beyond deflate's 32 768), 32 427 for period 27.  The packer never looks at rows, so the type bytes are noise too."""
    n = period * Rb
    assert n + 2 < 1 << 20
    for attempt in range(8):
        draw = np.random.default_rng(seed + attempt).integers(0, 256, 2 * n + 64, dtype=np.uint8).tolist()
        seq, seen, at = [], set(), 0
        while len(seq) < n and at < len(draw):
            b = draw[at]
            at += 1
            if len(seq) >= 2:
                key = (seq[-2], seq[-1], b)
                if key in seen:
                    continue
                seen.add(key)
            seq.append(b)
        cyc = seq + seq[:2]
        if len(seq) == n and len({tuple(cyc[i:i + 3]) for i in range(n)}) == n:
            base = np.array(seq, dtype=np.uint8).reshape(period, Rb)
            return base[np.arange(H) % period][None].copy()
    raise AssertionError("no sequence without a repeated trigram")


def len_symbol(length):
    """(symbol 257 .. 285, extra bits, extra value)"""
    for k in range(len(LEN_TABLE) - 1, -1, -1):
        if length >= LEN_TABLE[k][0]:
            return 257 + k, LEN_TABLE[k][1], length - LEN_TABLE[k][0]
    raise ValueError(length)


def dist_symbol(d):
    for k in range(len(DIST_TABLE) - 1, -1, -1):
        if d >= DIST_TABLE[k][0]:
            return k, DIST_TABLE[k][1], d - DIST_TABLE[k][0]
    raise ValueError(d)


def hashes(s):
    """h(p) for every p with p + 3 <= len(s): int64 array."""
    v = s.astype(np.uint64)
    if len(v) < 3:
        return np.zeros(0, dtype=np.int64)
    key = v[:-2] | (v[1:-1] << np.uint64(8)) | (v[2:] << np.uint64(16))
    return (((key * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(20)).astype(np.int64)


def tokenize(s, l0, Rb):
    """One stripe: bytes ``s`` (uint8 array), literal prices ``l0`` [257], row bytes ``Rb`` -> list of tokens, a literal as its byte,
    a match as (length, distance)."""
    data = s.tobytes()
    L = len(data)
    price = [int(p) for p in l0]
    h = hashes(s).tolist()
    head = {}
    inserted = 0                                        # positions < inserted are in the head table (whole groups only)
    fixed = (1, 2, 3, 4, 6, Rb - 3, Rb, Rb + 3)
    tokens, i = [], 0
    while i < L:
        taken = None
        if i + 3 <= L:
            limit = GROUP * (i // GROUP)
            while inserted < limit:
                if inserted + 3 <= L:
                    head[h[inserted]] = inserted        # ascending: the largest position stays
                inserted += 1
            cands = list(fixed)
            j = head.get(h[i])
            if j is not None:
                cands.append(i - j)
            cap = min(MAX_LEN, L - i)
            best, bd = 0, 0
            for d in cands:
                if not (1 <= d <= i and d <= MAX_DIST):
                    continue
                n = 0
                while n < cap and data[i + n] == data[i - d + n]:
                    n += 1
                if n > best or (n == best and d < bd):
                    best, bd = n, d
            if best >= 3 and sum(price[b] for b in data[i:i + best]) > 12 + len_symbol(best)[1] + dist_symbol(bd)[1]:
                taken = (best, bd)
        if taken:
            tokens.append(taken)
            i += taken[0]
        else:
            tokens.append(data[i])
            i += 1
    return tokens


def check_tokens(tokens, s):
    """Every token legal, and the tokens reproduce the stripe."""
    data = s.tobytes()
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            assert 3 <= n <= MAX_LEN and 1 <= d <= min(len(out), MAX_DIST), (t, len(out))
            for _ in range(n):
                out.append(out[-d])
        else:
            assert 0 <= t <= 255
            out.append(t)
        at = len(out) - (t[0] if isinstance(t, tuple) else 1)
        assert data[at:len(out)] == bytes(out[at:]), (t, at)
    assert bytes(out) == data


def histograms(tokens):
    """(literal / length histogram [286] with end-of-block 1, distance histogram [30])"""
    ll, dd = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            ll[len_symbol(t[0])[0]] += 1
            dd[dist_symbol(t[1])[0]] += 1
        else:
            ll[t] += 1
    return ll, dd


def code_lengths(tokens):
    """Heap Huffman of both histograms; a single used distance symbol gets length 1."""
    ll, dd = histograms(tokens)
    return R.heap_lengths(ll), R.heap_lengths(dd)


def deflate_stripe(s, tokens, l0, ll, dl):
    """One stripe's bytes: the dynamic block + the empty stored block.  No match among the tokens: today's Huffman-only block
    (HLIT 0, HDIST 0) with the literal prices as the code; else HLIT 29, HDIST 29, 286 + 30 plain 4-bit lengths, tokens."""
    w = R.BitWriter()
    w.put(0, 1)
    w.put(2, 2)
    matched = any(isinstance(t, tuple) for t in tokens)
    if not matched:
        ll, dl = [int(l) for l in l0], [0]
        w.put(0, 5)
        w.put(0, 5)
    else:
        ll, dl = [int(l) for l in ll], [int(l) for l in dl]
        assert len(ll) == 286 and len(dl) == 30
        w.put(29, 5)
        w.put(29, 5)
    w.put(15, 4)
    for sym in R.CL_ORDER:
        w.put(0 if sym >= 16 else 4, 3)
    for l in ll + dl:
        w.put_code(l, 4)
    lc, dc = R.canonical_codes(ll), R.canonical_codes(dl)
    for t in tokens:
        if isinstance(t, tuple):
            sym, eb, ev = len_symbol(t[0])
            w.put_code(lc[sym], ll[sym])
            w.put(ev, eb)
            sym, eb, ev = dist_symbol(t[1])
            w.put_code(dc[sym], dl[sym])
            w.put(ev, eb)
        else:
            w.put_code(lc[t], ll[t])
    w.put_code(lc[256], ll[256])
    w.put(0, 3)
    w.align()
    return bytes(w.out) + b"\x00\x00\xff\xff"


def crc32_bitwise(data, crc=0):
    """zlib's CRC-32: reflected, polynomial 0xEDB88320, register preset to and finally inverted with 0xFFFFFFFF."""
    crc ^= 0xFFFFFFFF
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (0xEDB88320 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", crc32_bitwise(tag + data))


def pack(filtered, tokens, l0, ll, dl, H, W, stripe_rows):
    """list[bytes]: whole files from filtered rows uint8 [n, H, R], tokens[k][s] (lists), literal prices [n, stripes, 257] and the
    final code lengths [n, stripes, 286] / [n, stripes, 30]; every CRC by the bitwise routine."""
    files = []
    for k in range(filtered.shape[0]):
        z = bytearray(b"\x78\x01")
        for s, r0 in enumerate(range(0, H, stripe_rows)):
            z += deflate_stripe(filtered[k, r0:r0 + stripe_rows].reshape(-1), tokens[k][s], l0[k][s], ll[k][s], dl[k][s])
        z += b"\x03\x00" + struct.pack(">I", zlib.adler32(filtered[k].tobytes()))
        files.append(R.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", bytes(z)) + chunk(b"IEND", b""))
    return files


def tokenize_frames(filtered, l0, stripe_rows):
    """tokens[k][s] for filtered rows [n, H, R] and literal prices [n, stripes, 257]."""
    n, H, Rb = filtered.shape
    return [[tokenize(filtered[k, r0:r0 + stripe_rows].reshape(-1), l0[k][s], Rb) for s, r0 in enumerate(range(0, H, stripe_rows))]
            for k in range(n)]


def encode(frames, stripe_rows=None):
    """The whole restatement: (files with matches, Huffman-only files, filtered rows, tokens)."""
    n, H, W, _ = frames.shape
    sr = stripe_rows or R.default_stripe_rows(H, W)
    filtered = R.filter_rows(frames)
    l0 = [[R.heap_lengths(h) for h in R.stripe_histograms(filtered[k], sr)] for k in range(n)]
    tokens = tokenize_frames(filtered, l0, sr)
    lens = [[code_lengths(t) for t in tokens[k]] for k in range(n)]
    ll = [[c[0] for c in lens[k]] for k in range(n)]
    dl = [[c[1] for c in lens[k]] for k in range(n)]
    return pack(filtered, tokens, l0, ll, dl, H, W, sr), R.pack(filtered, l0, H, W, sr), filtered, tokens


def unpack_tokens(words, count):
    """The kernel's uint32 tokens (len << 16 | dist, or the byte) -> the lists used here."""
    return [(int(t) >> 16, int(t) & 0xFFFF) if int(t) >> 16 else int(t) for t in words[:count]]
