"""The sub-sample motion rule of the H.264 GOP stream (include/sdv_hip_h264_sub.h, DESIGN.md "H.264 sub-sample motion") restated in plain
Python / numpy on top of h264_me_ref.py, h264_p_ref.py and h264_ref.py, none of which is edited.  Nothing here imports the package's encoder.

(a) ``inter_pred``: 8.4.2.2.1 (6-tap luma, quarter samples) and 8.4.2.2.2 (bilinear chroma, eighth samples) with the standard's coordinate
    clamp.  ``decode_stream`` installs it into h264_p_ref's decoder for the duration of a decode, which makes that decoder one for the new
    streams.
(b) ``search_planes``: the three-stage search on source luma.
(c) ``encode_planes(..., search, subpel, mv=None)``: the GOP stream with one quarter-sample vector per macroblock - searched or injected
    (an injected vector the rule does not admit is coded as (0, 0)) - with the reconstruction and the statistics the coverage check reads.
(d) ``make_planes``: the kinds of h264_me_ref plus ``glide<s>``, an analytic band-limited texture that moves by exactly s quarter samples
    a picture (it is evaluated at x - k s / 4: no resampling is involved).
"""
import functools
from unittest import mock

import numpy as np

import h264_me_ref as M
import h264_p_ref as P
import h264_ref as R

SUBPELS = (1, 2, 4)
KINDS = ("still", "pan1", "glide1", "glide2", "glide6", "cut", "noise", "zeros_pcm")
SHAPES = tuple(s for s in P.SHAPES if s[:3] in ((4, 16, 16), (5, 32, 48), (3, 36, 50), (6, 96, 128)))
QPS = (0, 16, 28, 51)
SEARCHES = (2, 8)
FIRST = P.FIRST
LAMBDA = M.LAMBDA


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) prediction
# ------------------------------------------------------------------------------------------------------------------------------------
def _tap6(a, axis):
    """E - 5F + 20G + 20H - 5I + J along ``axis``: element i of the result lies between elements i + 2 and i + 3 of ``a``."""
    n = a.shape[axis] - 5
    s = [np.take(a, range(i, i + n), axis=axis) for i in range(6)]
    return s[0] - 5 * s[1] + 20 * s[2] + 20 * s[3] - 5 * s[4] + s[5]


def _luma_pred(ref, mv, x0, y0, size):
    ix, xf, iy, yf = mv[0] >> 2, mv[0] & 3, mv[1] >> 2, mv[1] & 3
    h, w = ref.shape
    ys = np.clip(np.arange(y0 + iy - 2, y0 + iy + size + 3), 0, h - 1)
    xs = np.clip(np.arange(x0 + ix - 2, x0 + ix + size + 3), 0, w - 1)
    win = ref[np.ix_(ys, xs)].astype(np.int64)                                      # G of sample (x, y) at win[y + 2, x + 2]
    clip1 = lambda v: np.clip(v, 0, 255)
    whole = lambda dy, dx: win[2 + dy:2 + dy + size, 2 + dx:2 + dx + size]
    b1, h1 = _tap6(win, 1), _tap6(win, 0)                                           # [size + 5, size], [size, size + 5]
    b_at = lambda dy: clip1((b1[2 + dy:2 + dy + size] + 16) >> 5)                   # the b-type sample dy rows below
    h_at = lambda dx: clip1((h1[:, 2 + dx:2 + dx + size] + 16) >> 5)                # the h-type sample dx columns to the right
    j = lambda: clip1((_tap6(b1, 0) + 512) >> 10)
    avg = lambda p, q: (p + q + 1) >> 1
    G, H, M_ = whole(0, 0), whole(0, 1), whole(1, 0)
    table = {
        (0, 0): lambda: G, (1, 0): lambda: avg(G, b_at(0)), (2, 0): lambda: b_at(0), (3, 0): lambda: avg(H, b_at(0)),
        (0, 1): lambda: avg(G, h_at(0)), (1, 1): lambda: avg(b_at(0), h_at(0)), (2, 1): lambda: avg(b_at(0), j()), (3, 1): lambda: avg(b_at(0), h_at(1)),
        (0, 2): lambda: h_at(0), (1, 2): lambda: avg(h_at(0), j()), (2, 2): j, (3, 2): lambda: avg(j(), h_at(1)),
        (0, 3): lambda: avg(M_, h_at(0)), (1, 3): lambda: avg(h_at(0), b_at(1)), (2, 3): lambda: avg(j(), b_at(1)), (3, 3): lambda: avg(h_at(1), b_at(1)),
    }
    return table[(xf, yf)]()


def _chroma_pred(ref, mv, x0, y0, size):
    ix, xf, iy, yf = mv[0] >> 3, mv[0] & 7, mv[1] >> 3, mv[1] & 7
    h, w = ref.shape
    ys = np.clip(np.arange(y0 + iy, y0 + iy + size + 1), 0, h - 1)
    xs = np.clip(np.arange(x0 + ix, x0 + ix + size + 1), 0, w - 1)
    win = ref[np.ix_(ys, xs)].astype(np.int64)
    a, b, c, d = win[:-1, :-1], win[:-1, 1:], win[1:, :-1], win[1:, 1:]
    return ((8 - xf) * (8 - yf) * a + xf * (8 - yf) * b + (8 - xf) * yf * c + xf * yf * d + 32) >> 6


def inter_pred(ref, mv, x0, y0, size, shift):
    """h264_p_ref._inter_pred's signature: ``shift`` 0 = luma (``mv`` in quarter samples), 1 = chroma (the same numbers are eighth samples)."""
    mv = (int(mv[0]), int(mv[1]))
    return _chroma_pred(ref, mv, x0, y0, size) if shift else _luma_pred(ref, mv, x0, y0, size)


def decode_stream(samples, width, height):
    with mock.patch.object(P, "_inter_pred", inter_pred):
        return P.decode_stream(samples, width, height)


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) frame kinds
# ------------------------------------------------------------------------------------------------------------------------------------
def glide_frames(s, n, h, w):
    """RGB frames of a sum of low-frequency sinusoids (periods >= 7 samples) evaluated at x - k s / 4 in picture k."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = np.empty((n, h, w, 3), dtype=np.uint8)
    for k in range(n):
        x = xx - k * s / 4.0
        v = 128 + 38 * np.sin(2 * np.pi * x / 11 + 0.3) + 30 * np.sin(2 * np.pi * (x / 7.3 + yy / 19)) + 24 * np.sin(2 * np.pi * yy / 9 + 1.0) \
            + 20 * np.sin(2 * np.pi * (x / 23 - yy / 13))
        c = 128 + 50 * np.sin(2 * np.pi * (x / 29 + yy / 37) + 0.7)
        frames[k] = np.clip(np.rint(np.stack([v, 0.5 * v + 0.5 * c, c], axis=-1)), 0, 255).astype(np.uint8)
    return frames


def make_frames(kind, n, h, w, seed=0):
    if kind.startswith("glide"):
        return glide_frames(int(kind[5:]), n, h, w)
    return M.make_frames(kind, n, h, w, seed)


def make_planes(kind, n, h, w, seed=0):
    if kind.startswith("glide"):
        return R.rgb_to_planes(make_frames(kind, n, h, w, seed))
    return M.make_planes(kind, n, h, w, seed)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the search
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vector_bits(c):
    """B(c): the length in bits of se(c), c in quarter samples."""
    return len(R.se(c))


def admitted(vx, vy, search, subpel, mx, my, mbw, mbh):
    """``vx``, ``vy`` in quarter samples; ``subpel`` 1, 2 or 4."""
    step = 4 // subpel
    if vx % step or vy % step or abs(vx) > 4 * search or abs(vy) > 4 * search:
        return False
    x0, x1, y0, y1 = vx >> 2, -((-vx) >> 2), vy >> 2, -((-vy) >> 2)                # floor and ceiling of v / 4
    return 0 <= 16 * mx + x0 and 16 * mx + x1 + 16 <= 16 * mbw and 0 <= 16 * my + y0 and 16 * my + y1 + 16 <= 16 * mbh


def candidates(search, subpel, mx, my, mbw, mbh):
    step = 4 // subpel
    rng = range(-4 * search, 4 * search + 1, step)
    return [(vx, vy) for vy in rng for vx in rng if admitted(vx, vy, search, subpel, mx, my, mbw, mbh)]


def _key(s, lam, vx, vy):
    return (s + lam * (vector_bits(vx) + vector_bits(vy)), abs(vx) + abs(vy), vy, vx, s)


def search_planes(y, qp, gop, search, subpel):
    """Source luma [n, 16 mbh, 16 mbw] -> (mv int16 [n, mbh, mbw, 2] in QUARTER samples, sad int32 [n, mbh, mbw]): picture k against source
    picture k - 1, zeros for the IDR pictures.  Stage 1: the minimum of (cost, |vx| + |vy|, vy, vx) over all admitted whole-sample vectors;
    stage 2 (subpel >= 2): over the winner and its admitted neighbours at +- 2 quarter samples; stage 3 (subpel 4): at +- 1."""
    assert subpel in SUBPELS
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    mv, sad = np.zeros((n, mbh, mbw, 2), dtype=np.int16), np.zeros((n, mbh, mbw), dtype=np.int32)
    lam = LAMBDA[qp]
    for k in range(n):
        if k % gop == 0:
            continue
        cur = y[k].astype(np.int64)
        prev = y[k - 1].astype(np.int64)
        ref = np.zeros((hh + 2 * search, ww + 2 * search), dtype=np.int64)          # (a candidate that reads the zeros is never admitted)
        ref[search:search + hh, search:search + ww] = prev
        best = [[None] * mbw for _ in range(mbh)]
        for vy in range(-search, search + 1):
            for vx in range(-search, search + 1):
                moved = ref[search + vy:search + vy + hh, search + vx:search + vx + ww]
                sads = np.abs(cur - moved).reshape(mbh, 16, mbw, 16).sum(axis=(1, 3))
                for my in range(mbh):
                    for mx in range(mbw):
                        if admitted(4 * vx, 4 * vy, search, 1, mx, my, mbw, mbh):
                            key = _key(int(sads[my, mx]), lam, 4 * vx, 4 * vy)
                            if best[my][mx] is None or key < best[my][mx]:
                                best[my][mx] = key
        for my in range(mbh):
            for mx in range(mbw):
                win = best[my][mx]
                block = cur[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
                for step in (2, 1):
                    if step * subpel < 4:
                        continue
                    cx, cy = win[3], win[2]
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            vx, vy = cx + step * dx, cy + step * dy
                            if (dx, dy) == (0, 0) or not admitted(vx, vy, search, subpel, mx, my, mbw, mbh):
                                continue
                            s = int(np.abs(block - _luma_pred(prev, (vx, vy), 16 * mx, 16 * my, 16)).sum())
                            win = min(win, _key(s, lam, vx, vy))
                mv[k, my, mx], sad[k, my, mx] = (win[3], win[2]), win[4]
    return mv, sad


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    st = M.new_stats()
    st.update(fractions=set(), tap_edges=set())
    return st


def encode_p_mb(sy, sc, fy, fc, left, mvp, v, qp, stats):
    """h264_me_ref.encode_p_mb with ``v`` and ``mvp`` in quarter samples (mvd = v - mvp) and ``fy`` / ``fc`` the interpolated prediction."""
    probe = P.new_stats()
    mode, bits, ry, rc, new_left = P.encode_p_mb(sy, sc, fy, fc, left, qp, probe)
    for key in ("inter_cbp_luma", "inter_cbp_chroma", "pcm_in_p"):
        stats[key] |= probe[key]
    for key, val in probe["intra"].items():
        if isinstance(val, set):
            stats["intra"][key] |= val
    if mode in ("intra", "pcm"):
        return mode, bits, ry, rc, new_left, (0, 0)
    mvd = (v[0] - mvp[0], v[1] - mvp[1])
    if mode == "skip":
        if v == (0, 0):
            return mode, bits, ry, rc, new_left, (0, 0)
        bits = R.ue(0) + R.se(mvd[0]) + R.se(mvd[1]) + R.ue(0)                     # P_L0_16x16, coded_block_pattern codeNum 0, no mb_qp_delta
        stats["nonzero_cbp0"] += 1
    else:
        assert bits[:3] == "111"                                                   # mb_type ue(0), mvd_l0 se(0) se(0)
        bits = R.ue(0) + R.se(mvd[0]) + R.se(mvd[1]) + bits[3:]
        if len(bits) > R.MAX_MB_BITS:                                              # the counting pass includes the mvd bits
            stats["pcm_in_p"].add("bits")
            stats["pcm_by_mvd"] += 1
            sy, sc = sy.astype(np.int64), sc.astype(np.int64)
            return "pcm", None, sy, sc, R._Left(sy[:, 15].copy(), sc[:, :, 7].copy(), np.full(4, 16), np.full((2, 2), 16)), (0, 0)
    stats["mvd_x"].add(mvd[0]), stats["mvd_y"].add(mvd[1]), stats["vectors"].add(v)
    stats["counted"].append(len(bits))
    return "inter", bits, ry, rc, new_left, v


def _note_taps(stats, v, m, r, mbw, mbh):
    """Which picture edges the filter taps of ``v`` at macroblock (m, r) are clamped at."""
    ix, iy = v[0] >> 2, v[1] >> 2
    if v[0] & 3:
        if 16 * m + ix - 2 < 0:
            stats["tap_edges"].add("left")
        if 16 * m + ix + 18 > 16 * mbw - 1:
            stats["tap_edges"].add("right")
    if v[1] & 3:
        if 16 * r + iy - 2 < 0:
            stats["tap_edges"].add("top")
        if 16 * r + iy + 18 > 16 * mbh - 1:
            stats["tap_edges"].add("bottom")


def encode_planes(y, cb, cr, qp=16, gop=1, first_index=0, stats=None, search=0, subpel=0, mv=None):
    """Padded planes -> (samples, recon Y, recon Cb, recon Cr, mv used [n, mbh, mbw, 2] in QUARTER samples).  ``subpel`` 0 (or ``search`` 0
    or ``gop`` 1) is h264_me_ref.encode_planes, its vectors times 4.  ``mv`` None: the searched vectors; else injected ones in quarter
    samples, each coded as (0, 0) where the rule does not admit it."""
    assert subpel in (0,) + SUBPELS
    stats = new_stats() if stats is None else stats
    if subpel == 0 or search == 0 or gop == 1:
        assert mv is None
        samples, ry, rcb, rcr, used = M.encode_planes(y, cb, cr, qp=qp, gop=gop, first_index=first_index, stats=stats, search=search)
        return samples, ry, rcb, rcr, (4 * used).astype(np.int16)
    assert 0 <= qp <= 51 and 1 <= gop <= P.GOP_MAX and 2 <= search <= M.SEARCH_MAX and search % 2 == 0
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    if mv is None:
        mv = search_planes(y, qp, gop, search, subpel)[0]
    used = np.zeros((n, mbh, mbw, 2), dtype=np.int16)
    ry, rcb, rcr = np.empty_like(y), np.empty_like(cb), np.empty_like(cr)
    samples = []
    for k in range(n):
        is_p = k % gop != 0
        stats["frame_nums"].append(k % gop & 15)
        sample = bytearray()
        for r in range(mbh):
            bits = [P.p_slice_header(r * mbw, k % gop, qp) if is_p else R.slice_header(r * mbw, (first_index + k) & 1, qp)]
            left, run, prev, mvp = None, 0, None, (0, 0)
            for m in range(mbw):
                ys, xs, yc, xc = slice(16 * r, 16 * r + 16), slice(16 * m, 16 * m + 16), slice(8 * r, 8 * r + 8), slice(8 * m, 8 * m + 8)
                sy, sc = y[k, ys, xs], np.stack([cb[k, yc, xc], cr[k, yc, xc]])
                if is_p:
                    v = (int(mv[k, r, m, 0]), int(mv[k, r, m, 1]))
                    if not admitted(v[0], v[1], search, subpel, m, r, mbw, mbh):
                        v = (0, 0)
                        stats["invalid_as_zero"] += 1
                    used[k, r, m] = v
                    fy = inter_pred(ry[k - 1], v, 16 * m, 16 * r, 16, 0).astype(np.uint8)
                    fc = np.stack([inter_pred(p[k - 1], v, 8 * m, 8 * r, 8, 1) for p in (rcb, rcr)]).astype(np.uint8)
                    before = mvp
                    mode, mb, py, pc, left, mvp = encode_p_mb(sy, sc, fy, fc, left, mvp, v, qp, stats)
                    stats["modes"].append(mode)
                    if mode == "inter":
                        stats["fractions"].add((v[0] & 3, v[1] & 3))
                        _note_taps(stats, v, m, r, mbw, mbh)
                    if mode == "skip":
                        run += 1
                        if before != (0, 0):
                            stats["skip_after_nonzero"] += 1
                            if before[0] & 3 or before[1] & 3:
                                stats["skip_after_fraction"] = stats.get("skip_after_fraction", 0) + 1
                    else:
                        bits.append(R.ue(run))
                        stats["skip_runs"].add(run)
                        run = 0
                    if mode == "inter" and v != (0, 0) and prev in ("intra", "pcm", "skip"):
                        stats["nonzero_after"].add(prev)
                else:
                    mb, py, pc, left, pcm = R.encode_mb(sy, sc, left, qp, stats["intra"])
                    mode = "pcm" if pcm else "intra"
                if mode == "pcm":
                    bits.append(R.ue(30 if is_p else 25))
                    bits.append("0" * (-sum(map(len, bits)) % 8))
                    bits.append("".join(format(int(s), "08b") for s in np.concatenate([sy.reshape(-1), sc.reshape(-1)])))
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
            s = "".join(bits) + "1"
            s += "0" * (-len(s) % 8)
            rbsp = int(s, 2).to_bytes(len(s) // 8, "big")
            assert not is_p or len(rbsp) <= P.p_rbsp_bound(mbw)
            nal = bytes([0x41 if is_p else 0x65]) + R.escape(rbsp)
            assert 4 + len(nal) <= P.slot_bytes(mbw)
            sample += len(nal).to_bytes(4, "big") + nal
        samples.append(bytes(sample))
    return samples, ry, rcb, rcr, used


INVALID = ((1, 0), (0, -3), (2, 6), (4, 2), (32767, 4), (4, -32768), (64, 64), (-64, 0), (0, 65), (3, 3))


def inject(kind, n, mbh, mbw, search, subpel, seed=0):
    """Vectors that are not searched, int16 [n, mbh, mbw, 2] in quarter samples.  ``fractions`` walks through all 16 fractional positions
    (on the quarter grid) with small whole parts of both signs; ``extreme`` alternates -4 search and +4 search along a row (|mvd| = 8
    search); ``random`` draws admitted vectors of the grid; ``edges`` puts fractional vectors with zero whole part on every macroblock, so
    that the border macroblocks' taps clamp; ``invalid`` holds off-grid (for subpel 1 and 2), out-of-range and not-admitted vectors."""
    rng = np.random.default_rng(seed)
    step = 4 // subpel
    mv = np.zeros((n, mbh, mbw, 2), dtype=np.int16)
    for k in range(n):
        for r in range(mbh):
            for m in range(mbw):
                i = k + 3 * r + 5 * m
                if kind == "fractions":
                    v = (4 * ((i // 16) % 3 - 1) + i % 4, 4 * ((i // 48) % 3 - 1) + (i // 4) % 4)
                    if not admitted(v[0], v[1], search, subpel, m, r, mbw, mbh):
                        v = (v[0] % 4 - (4 if m else 0), v[1] % 4 - (4 if r else 0))    # the same fractions, pointing inward
                elif kind == "extreme":
                    s = -4 * search if m % 2 else 4 * search
                    v = (s if admitted(s, 0, search, subpel, m, r, mbw, mbh) else 0, s if admitted(0, s, search, subpel, m, r, mbw, mbh) else 0)
                elif kind == "random":                                             # one in four (0, 0)
                    c = candidates(search, subpel, m, r, mbw, mbh)
                    v = c[int(rng.integers(len(c)))] if rng.integers(4) else (0, 0)
                elif kind == "edges":
                    fx, fy = (step * (1 + i % 3)) % 4, (step * (1 + (i // 3) % 3)) % 4
                    v = (fx - (4 if m == mbw - 1 and fx else 0), fy - (4 if r == mbh - 1 and fy else 0))
                elif kind == "invalid":
                    v = INVALID[i % len(INVALID)]
                else:
                    raise ValueError(kind)
                mv[k, r, m] = v
    return mv


def plant(n, h, w, mv, search, subpel, seed=0):
    """h264_me_ref.plant with quarter-sample vectors: macroblock (r, m) of picture k is the PREDICTION of that macroblock from picture k - 1
    by ``mv[k, r, m]`` ((0, 0) where the rule does not admit it), luma and chroma - except the ``fresh`` ones, which are new noise."""
    y0, cb0, cr0 = R.rgb_to_planes(R.make_frames("noise", 1, h, w, seed))
    mbh, mbw = y0.shape[1] // 16, y0.shape[2] // 16
    noise = R.rgb_to_planes(R.make_frames("noise", n, 16 * mbh, 16 * mbw, seed + 1))
    planes = [np.repeat(p, n, axis=0) for p in (y0, cb0, cr0)]
    for k in range(1, n):
        for r in range(mbh):
            for m in range(mbw):
                v = (int(mv[k, r, m, 0]), int(mv[k, r, m, 1]))
                if not admitted(v[0], v[1], search, subpel, m, r, mbw, mbh):
                    v = (0, 0)
                for p, q, size, shift in zip(planes, noise, (16, 8, 8), (0, 1, 1)):
                    ya, xa = size * r, size * m
                    if M.fresh(k, r, m):
                        p[k, ya:ya + size, xa:xa + size] = q[k, ya:ya + size, xa:xa + size]
                    else:
                        p[k, ya:ya + size, xa:xa + size] = inter_pred(p[k - 1], v, xa, ya, size, shift)
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, qp, search, subpel, injected=None):
    """(planes, samples, (ry, rcb, rcr), stats, mv used) of one case, computed once for all the tests that read it.  ``injected``: a kind of
    ``inject`` - the vectors are those, the planes ``plant``ed with them (``kind`` is then only a name)."""
    n, h, w, gop = shape
    mbh, mbw = (h + 15) // 16, (w + 15) // 16
    stats = new_stats()
    mv = None if injected is None else inject(injected, n, mbh, mbw, search, subpel)
    planes = make_planes(kind, n, h, w) if injected is None else plant(n, h, w, mv, search, subpel)
    samples, ry, rcb, rcr, used = encode_planes(*planes, qp=qp, gop=gop, first_index=FIRST, stats=stats, search=search, subpel=subpel, mv=mv)
    return planes, samples, (ry, rcb, rcr), stats, used


@functools.lru_cache(maxsize=None)
def searched(shape, kind, qp, search, subpel):
    """(mv, sad) of ``search_planes`` on the source luma of one case."""
    n, h, w, gop = shape
    return search_planes(make_planes(kind, n, h, w)[0], qp, gop, search, subpel)
