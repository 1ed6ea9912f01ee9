"""The motion search rule of the H.264 GOP stream (include/sdv_hip_ext.h, DESIGN.md "H.264 motion search") restated in plain Python / numpy on
top of h264_p_ref.py and h264_ref.py.  Nothing here imports the package's encoder; ``h264_p_ref.decode_stream`` is the independent decoder.

(a) ``search_planes``: the exhaustive search on source luma, its cost and its total order.
(b) ``encode_planes(..., search, mv=None)``: the GOP stream with one vector per macroblock - the searched ones, or injected ones (an
    injected vector the rule does not admit is coded as (0, 0)) - with the reconstruction of every sample and the statistics the coverage
    check reads.
(c) ``make_planes``: the temporal kinds of h264_p_ref plus pan2 / drift / pan1.
"""
import functools

import numpy as np

import h264_p_ref as P
import h264_ref as R

SEARCH_MAX = 16
KINDS = ("still", "fade", "pan2", "drift", "pan1", "cut", "noise", "zeros_pcm")
SHAPES = tuple(s for s in P.SHAPES if s[:3] in ((4, 16, 16), (5, 32, 48), (3, 36, 50), (7, 64, 64), (6, 96, 128)))
QPS = (0, 16, 28, 51)
SEARCHES = (2, 8, 16)
FIRST = P.FIRST
LAMBDA = tuple(max(1, round(2 ** ((qp - 12) / 6))) for qp in range(52))


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) frame kinds
# ------------------------------------------------------------------------------------------------------------------------------------
def make_frames(kind, n, h, w, seed=0):
    if kind in ("pan2", "drift", "pan1"):
        g = R.make_frames("glyphs", 1, h, w, seed)[0]
        dx, dy = dict(pan2=(2, 0), drift=(2, -2), pan1=(1, 0))[kind]
        return np.stack([np.roll(g, (dy * k, dx * k), axis=(0, 1)) for k in range(n)])
    return P.make_frames(kind, n, h, w, seed)


def make_planes(kind, n, h, w, seed=0):
    if kind == "zeros_pcm":
        return P.make_planes(kind, n, h, w, seed)
    return R.rgb_to_planes(make_frames(kind, n, h, w, seed))


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) the search
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vector_bits(c):
    """B(c): the length in bits of se(4 c)."""
    return len(R.se(4 * c))


def admitted(vx, vy, search, mx, my, mbw, mbh):
    if vx % 2 or vy % 2 or abs(vx) > search or abs(vy) > search:
        return False
    return 0 <= 16 * mx + vx and 16 * mx + vx + 16 <= 16 * mbw and 0 <= 16 * my + vy and 16 * my + vy + 16 <= 16 * mbh


def candidates(search, mx, my, mbw, mbh):
    return [(vx, vy) for vy in range(-search, search + 1, 2) for vx in range(-search, search + 1, 2) if admitted(vx, vy, search, mx, my, mbw, mbh)]


def search_planes(y, qp, gop, search):
    """Source luma [n, 16 mbh, 16 mbw] -> (mv int16 [n, mbh, mbw, 2] in luma samples, sad int32 [n, mbh, mbw]): picture k against picture
    k - 1, zeros for the IDR pictures.  Minimum of (cost, |vx| + |vy|, vy, vx) over the admitted candidates."""
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    mv, sad = np.zeros((n, mbh, mbw, 2), dtype=np.int16), np.zeros((n, mbh, mbw), dtype=np.int32)
    lam = LAMBDA[qp]
    for k in range(n):
        if k % gop == 0:
            continue
        cur = y[k].astype(np.int64)
        ref = np.zeros((hh + 2 * search, ww + 2 * search), dtype=np.int64)
        ref[search:search + hh, search:search + ww] = y[k - 1]
        best = [[None] * mbw for _ in range(mbh)]
        for vy in range(-search, search + 1, 2):
            for vx in range(-search, search + 1, 2):
                moved = ref[search + vy:search + vy + hh, search + vx:search + vx + ww]
                sads = np.abs(cur - moved).reshape(mbh, 16, mbw, 16).sum(axis=(1, 3))
                for my in range(mbh):
                    for mx in range(mbw):
                        if not admitted(vx, vy, search, mx, my, mbw, mbh):
                            continue
                        s = int(sads[my, mx])
                        key = (s + lam * (vector_bits(vx) + vector_bits(vy)), abs(vx) + abs(vy), vy, vx, s)
                        if best[my][mx] is None or key < best[my][mx]:
                            best[my][mx] = key
        for my in range(mbh):
            for mx in range(mbw):
                _, _, vy, vx, s = best[my][mx]
                mv[k, my, mx], sad[k, my, mx] = (vx, vy), s
    return mv, sad


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the encoder rule
# ------------------------------------------------------------------------------------------------------------------------------------
def new_stats():
    st = P.new_stats()
    st.update(mvd_x=set(), mvd_y=set(), vectors=set(), nonzero_cbp0=0, nonzero_after=set(), skip_after_nonzero=0, invalid_as_zero=0, counted=[],
              pcm_by_mvd=0)
    return st


def encode_p_mb(sy, sc, fy, fc, left, mvp, v, qp, stats):
    """h264_p_ref.encode_p_mb with the displaced reference ``fy`` / ``fc`` of vector ``v`` and the predictor ``mvp`` (both luma samples)
    -> (mode, bits, recon Y, recon C, _Left, the vector the right neighbour predicts from)."""
    probe = P.new_stats()
    mode, bits, ry, rc, new_left = P.encode_p_mb(sy, sc, fy, fc, left, qp, probe)
    for key in ("inter_cbp_luma", "inter_cbp_chroma", "pcm_in_p"):
        stats[key] |= probe[key]
    for key, val in probe["intra"].items():
        if isinstance(val, set):
            stats["intra"][key] |= val
    if mode in ("intra", "pcm"):
        return mode, bits, ry, rc, new_left, (0, 0)
    mvd = (4 * (v[0] - mvp[0]), 4 * (v[1] - mvp[1]))
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


def encode_planes(y, cb, cr, qp=16, gop=1, first_index=0, stats=None, search=0, mv=None):
    """Padded planes -> (samples, recon Y, recon Cb, recon Cr, mv used [n, mbh, mbw, 2]).  ``mv`` None: the searched vectors; else injected
    ones, [n, mbh, mbw, 2] (vx, vy) in luma samples, each coded as (0, 0) where the rule does not admit it."""
    assert 0 <= qp <= 51 and 1 <= gop <= P.GOP_MAX and 0 <= search <= SEARCH_MAX and search % 2 == 0
    stats = new_stats() if stats is None else stats
    n, hh, ww = y.shape
    mbh, mbw = hh // 16, ww // 16
    if mv is None:
        mv = search_planes(y, qp, gop, search)[0] if search else np.zeros((n, mbh, mbw, 2), dtype=np.int16)
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
                    if not admitted(v[0], v[1], search, m, r, mbw, mbh):
                        v = (0, 0)
                        stats["invalid_as_zero"] += 1
                    used[k, r, m] = v
                    y0, x0 = 16 * r + v[1], 16 * m + v[0]
                    fy = ry[k - 1, y0:y0 + 16, x0:x0 + 16]
                    fc = np.stack([p[k - 1, y0 // 2:y0 // 2 + 8, x0 // 2:x0 // 2 + 8] for p in (rcb, rcr)])
                    assert fy.shape == (16, 16) and fc.shape == (2, 8, 8)
                    before = mvp
                    mode, mb, py, pc, left, mvp = encode_p_mb(sy, sc, fy, fc, left, mvp, v, qp, stats)
                    stats["modes"].append(mode)
                    if mode == "skip":
                        run += 1
                        if before != (0, 0):
                            stats["skip_after_nonzero"] += 1
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


def inject(kind, n, mbh, mbw, search, seed=0):
    """Vectors that are not searched, [n, mbh, mbw, 2]: ``extreme`` alternates (-search, -search) and (+search, +search) along a row
    (|mvd| = 8 search in both signs, clipped at the edges to (0, 0) by being inadmissible there); ``random`` draws admitted vectors;
    ``invalid`` holds odd, too long and picture-leaving vectors."""
    rng = np.random.default_rng(seed)
    mv = np.zeros((n, mbh, mbw, 2), dtype=np.int16)
    for k in range(n):
        for r in range(mbh):
            for m in range(mbw):
                if kind == "extreme":
                    s = -search if m % 2 else search
                    v = (s if admitted(s, 0, search, m, r, mbw, mbh) else 0, s if admitted(0, s, search, m, r, mbw, mbh) else 0)
                elif kind == "random":                                             # one in four (0, 0)
                    c = candidates(search, m, r, mbw, mbh)
                    v = c[int(rng.integers(len(c)))] if rng.integers(4) else (0, 0)
                elif kind == "invalid":
                    v = ((1, 0), (0, -3), (search + 2, 0), (-16, -16), (2, 32767), (-32768, 2), (16, 16))[(k + r + m) % 7]
                else:
                    raise ValueError(kind)
                mv[k, r, m] = v
    return mv


def fresh(k, r, m):
    """The macroblocks of ``plant`` that are new noise (intra or I_PCM in a P picture) instead of a displaced copy."""
    return (k + 2 * r + m) % 4 == 3


def plant(n, h, w, mv, search, seed=0):
    """Planes in which macroblock (r, m) of picture k is the block of picture k - 1 displaced by ``mv[k, r, m]`` ((0, 0) where the rule does
    not admit it), luma and chroma, so that inter prediction with exactly these vectors leaves next to no residual - except the ``fresh``
    macroblocks, which are new noise.  Picture 0 is noise."""
    y0, cb0, cr0 = R.rgb_to_planes(R.make_frames("noise", 1, h, w, seed))
    mbh, mbw = y0.shape[1] // 16, y0.shape[2] // 16
    noise = R.rgb_to_planes(R.make_frames("noise", n, 16 * mbh, 16 * mbw, seed + 1))
    planes = [np.repeat(p, n, axis=0) for p in (y0, cb0, cr0)]
    for k in range(1, n):
        for r in range(mbh):
            for m in range(mbw):
                v = (int(mv[k, r, m, 0]), int(mv[k, r, m, 1]))
                if not admitted(v[0], v[1], search, m, r, mbw, mbh):
                    v = (0, 0)
                for p, q, size, d in zip(planes, noise, (16, 8, 8), (1, 2, 2)):
                    ya, xa = size * r, size * m
                    src = q[k] if fresh(k, r, m) else p[k - 1]
                    yb, xb = (ya, xa) if fresh(k, r, m) else (ya + v[1] // d, xa + v[0] // d)
                    p[k, ya:ya + size, xa:xa + size] = src[yb:yb + size, xb:xb + size]
    return tuple(planes)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, qp, search, injected=None):
    """(planes, samples, (ry, rcb, rcr), stats, mv used) of one case, computed once for all the tests that read it.  ``injected``: a kind of
    ``inject`` - the vectors are those, the planes ``plant``ed with them (``kind`` is then only a name)."""
    n, h, w, gop = shape
    mbh, mbw = (h + 15) // 16, (w + 15) // 16
    stats = new_stats()
    mv = None if injected is None else inject(injected, n, mbh, mbw, search)
    planes = make_planes(kind, n, h, w) if injected is None else plant(n, h, w, mv, search)
    samples, ry, rcb, rcr, used = encode_planes(*planes, qp=qp, gop=gop, first_index=FIRST, stats=stats, search=search, mv=mv)
    return planes, samples, (ry, rcb, rcr), stats, used
