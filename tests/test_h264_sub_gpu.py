"""Sub-sample motion vectors on the GPU (sdv_h264_motion_search_sub and sdv_h264_encode_gop_step_sub behind
h264_cavlc.H264Encoder(gop=..., search=..., subpel=...)) against tests/h264_sub_ref.py: vectors, SADs, samples and reconstruction planes
equal the restatement's exactly, and the GPU's bytes decode in h264_p_ref.py's decoder (with the restatement's interpolator installed) to
the same pictures.  All integer: every comparison is exact.  Small shapes only."""
import functools

import numpy as np
import pytest
import torch

import h264_me_ref as M
import h264_p_ref as P
import h264_ref as R
import h264_sub_ref as S

pytestmark = pytest.mark.gpu

SMALL = tuple(s for s in S.SHAPES if s[:3] in ((4, 16, 16), (5, 32, 48), (3, 36, 50)))
CASES = [(s, k, r, p) for s in SMALL for k in S.KINDS for r in S.SEARCHES for p in S.SUBPELS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-gop{s[3]}-{k}-search{r}-subpel{p}" for s, k, r, p in CASES]
INJECTED = [((5, 32, 48, 5), 28, 2, 4, "fractions"), ((3, 36, 50, 3), 16, 8, 4, "fractions"), ((7, 64, 64, 3), 0, 16, 4, "extreme"),
            ((3, 36, 50, 3), 16, 2, 1, "extreme"), ((5, 32, 48, 5), 28, 8, 2, "random"), ((3, 36, 50, 3), 28, 8, 4, "edges"),
            ((5, 32, 48, 5), 16, 2, 2, "edges"), ((4, 16, 16, 4), 16, 16, 4, "fractions"), ((5, 32, 48, 5), 51, 16, 1, "invalid"),
            ((3, 36, 50, 3), 16, 8, 2, "invalid"), ((4, 16, 16, 4), 16, 16, 4, "invalid")]


@functools.lru_cache(maxsize=None)
def _encoder(qp, gop, search, subpel):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=subpel)


def _gpu(shape, kind, qp, search, subpel, first_index=S.FIRST, sl=slice(None)):
    """(samples, recon planes as numpy) of pictures ``sl`` of the case, coded in one call."""
    n, h, w, gop = shape
    enc = _encoder(qp, gop, search, subpel)
    if kind == "zeros_pcm":
        samples, recon = enc.encode_planes(*(torch.from_numpy(p[sl]).cuda() for p in S.make_planes(kind, n, h, w)), first_index=first_index,
                                           return_recon=True)
    else:
        samples, recon = enc.encode(torch.from_numpy(S.make_frames(kind, n, h, w)[sl]).cuda(), first_index=first_index, return_recon=True)
    return samples, tuple(r.cpu().numpy() for r in recon)


def _steps(hip, planes, qp, gop, search, subpel, first_index, mv, recon, scratch):
    n = planes[0].shape[0]
    for k in range(min(gop, n)):
        hip.h264_encode_gop_step_sub(*planes, qp, gop, k, search, subpel, first_index, mv, *recon, scratch)


def _gpu_with_vectors(hip, planes, qp, gop, search, subpel, mv, first_index=S.FIRST):
    """The launches of H264Encoder._rows_and_pack with given vectors in place of the searched ones."""
    n, mbh, mbw = planes[0].shape[0], planes[0].shape[1] // 16, planes[0].shape[2] // 16
    dev = [torch.from_numpy(p).cuda() for p in planes]
    recon = [torch.empty_like(p) for p in dev]
    scratch = torch.empty((hip.h264_gop_scratch_bytes(n, mbh, mbw),), dtype=torch.uint8, device="cuda")
    out = torch.empty((hip.h264_gop_out_bytes(n, mbh, mbw),), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    _steps(hip, dev, qp, gop, search, subpel, first_index, torch.from_numpy(mv).cuda(), recon, scratch)
    hip.h264_pack(scratch, n, mbh, hip.h264_gop_slot_mbw(mbw), out, offsets)
    offs, data = offsets.cpu().tolist(), out.cpu().numpy()
    return [data[offs[k]:offs[k + 1]].tobytes() for k in range(n)], tuple(r.cpu().numpy() for r in recon)


def _same(got, recon, want, want_recon):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, len(a), len(b))
        assert a == b, (k, next(i for i in range(len(a)) if a[i] != b[i]))
    for a, b in zip(recon, want_recon):
        assert a.shape == b.shape and np.array_equal(a, b)


def _search(hip, y, qp, gop, search, subpel):
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    mv = torch.full((n, mbh, mbw, 2), 99, dtype=torch.int16, device="cuda")
    sad = torch.full((n, mbh, mbw), -1, dtype=torch.int32, device="cuda")
    hip.h264_motion_search_sub(torch.from_numpy(y).cuda(), qp, gop, search, subpel, mv, sad)
    return mv.cpu().numpy(), sad.cpu().numpy()


@pytest.mark.parametrize("subpel", S.SUBPELS)
@pytest.mark.parametrize("search", (2, 8, 16))
def test_search_kernel_alone_equals_the_numpy_search(hip, search, subpel):
    """Vectors and SADs: flat input where every candidate ties, a striped picture where many shifts tie, one macroblock, pictures whose
    every macroblock is an edge macroblock (their fractional candidates read clamped taps), whole- and fractional-sample motion, planted
    quarter-sample vectors, noise; qp moves lambda."""
    flat = np.full((3, 48, 64), 77, dtype=np.uint8)
    stripes = flat.copy()
    stripes[:, ::2] = 200
    planted = lambda n, h, w, kind: S.plant(n, h, w, S.inject(kind, n, (h + 15) // 16, (w + 15) // 16, search, 4), search, 4)[0]
    inputs = [(flat, 16, 3), (stripes, 16, 3), (S.make_planes("noise", 4, 16, 16)[0], 16, 4), (S.make_planes("glide1", 4, 16, 16)[0], 16, 4),
              (S.make_planes("noise", 5, 32, 48)[0], 0, 2), (S.make_planes("pan1", 3, 36, 50)[0], 28, 3), (S.make_planes("glide1", 3, 36, 50)[0], 16, 3),
              (S.make_planes("glide2", 5, 32, 48)[0], 51, 5), (S.make_planes("glide6", 3, 36, 50)[0], 16, 3), (planted(5, 32, 48, "random"), 16, 5),
              (planted(3, 36, 50, "fractions"), 40, 3), (planted(5, 32, 48, "extreme"), 16, 5)]
    for y, qp, gop in inputs:
        want_mv, want_sad = S.search_planes(y, qp, gop, search, subpel)
        mv, sad = _search(hip, y, qp, gop, search, subpel)
        assert np.array_equal(mv, want_mv), (y.shape, qp, gop, np.argwhere(mv != want_mv)[:4])
        assert np.array_equal(sad, want_sad), (y.shape, qp, gop)
    mv, _ = _search(hip, flat, 16, 3, search, subpel)
    assert not mv.any()
    mv, sad = _search(hip, stripes, 0, 1, search, subpel)                           # gop 1: every picture an IDR picture
    assert not mv.any() and not sad.any()


@pytest.mark.parametrize("shape,kind,search,subpel", CASES, ids=IDS)
def test_samples_and_reconstruction_equal_the_restatement_and_decode(hip, shape, kind, search, subpel):
    n, h, w, gop = shape
    for qp in S.QPS:
        got, recon = _gpu(shape, kind, qp, search, subpel)
        _, want, want_recon, _, _ = S.reference(shape, kind, qp, search, subpel)
        assert len(got) == n
        _same(got, recon, want, want_recon)
        d = S.decode_stream(got, w, h)                                              # the GPU's own bytes
        assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon))
        assert d["sync"] == _encoder(qp, gop, search, subpel).last_sync == list(range(0, n, gop))


@pytest.mark.parametrize("shape,qp,search,subpel,kind", INJECTED,
                         ids=[f"{s[0]}x{s[1]}x{s[2]}-gop{s[3]}-qp{q}-search{r}-subpel{p}-{k}" for s, q, r, p, k in INJECTED])
def test_injected_vectors_equal_the_restatement_and_decode(hip, shape, qp, search, subpel, kind):
    """Given vectors on planes planted with them: all 16 fractions, both signs and the largest |mvd|, nonzero vectors without a residual,
    after intra, I_PCM and skip, taps clamped at every edge, the one-macroblock picture - and off-grid, out-of-range and not-admitted
    vectors, which the kernel codes as (0, 0)."""
    n, h, w, gop = shape
    planes, want, want_recon, _, used = S.reference(shape, "planted", qp, search, subpel, kind)
    mv = S.inject(kind, n, used.shape[1], used.shape[2], search, subpel)
    got, recon = _gpu_with_vectors(hip, planes, qp, gop, search, subpel, mv)
    _same(got, recon, want, want_recon)
    d = S.decode_stream(got, w, h)
    assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon))


def test_two_runs_give_the_same_bytes(hip):
    for kind, qp, search, subpel in (("noise", 16, 8, 4), ("glide1", 0, 16, 4), ("pan1", 28, 2, 1), ("glide2", 16, 8, 2)):
        a, b = _gpu((5, 32, 48, 5), kind, qp, search, subpel), _gpu((5, 32, 48, 5), kind, qp, search, subpel)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_a_gop_codes_the_same_alone_and_inside_a_longer_call(hip):
    shape = (7, 64, 64, 3)
    for kind, qp, search, subpel in (("glide1", 16, 8, 4), ("cut", 0, 16, 2), ("pan1", 28, 2, 1)):
        whole, recon = _gpu(shape, kind, qp, search, subpel)
        for lo, hi in ((0, 3), (3, 6), (6, 7), (3, 7)):
            part, part_recon = _gpu(shape, kind, qp, search, subpel, first_index=S.FIRST + lo, sl=slice(lo, hi))
            assert part == whole[lo:hi] and all(np.array_equal(a, b[lo:hi]) for a, b in zip(part_recon, recon))


def test_buffers_at_exactly_the_documented_capacity(hip, monkeypatch):
    """Canary-guarded mv, sad, scratch, output and reconstruction buffers at exactly their sizes, on planted planes with fractional
    vectors whose taps clamp at every edge and on hostile samples that make every macroblock I_PCM: the guards stay intact and the samples
    are right; one byte less of scratch is refused before any launch."""
    guard, qp, gop, search, subpel = 64, 0, 2, 16, 4
    n, mbh, mbw = 4, 2, 3
    rng = np.random.default_rng(5)
    hostile = lambda *sh: np.where(rng.random(sh) < 0.5, rng.integers(0, 4, sh), 252 + rng.integers(0, 4, sh)).astype(np.uint8)
    for planes in (S.plant(n, 32, 48, S.inject("edges", n, mbh, mbw, search, subpel), search, subpel),
                   S.plant(n, 32, 48, S.inject("extreme", n, mbh, mbw, search, subpel), search, subpel),
                   (hostile(4, 32, 48), hostile(4, 16, 24), hostile(4, 16, 24))):
        want, *want_recon, used = S.encode_planes(*planes, qp=qp, gop=gop, first_index=S.FIRST, search=search, subpel=subpel)
        y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
        need_s, need_o = hip.h264_gop_scratch_bytes(n, mbh, mbw), hip.h264_gop_out_bytes(n, mbh, mbw)
        canary = lambda size: torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        big_s, big_o, big_mv, big_sad = canary(need_s), canary(need_o), canary(used.size * 2), canary(n * mbh * mbw * 4)
        big_r = [canary(p.size) for p in planes]
        recon = [b[guard:guard + p.size].view(p.shape) for b, p in zip(big_r, planes)]
        mv = big_mv[guard:guard + used.size * 2].view(torch.int16).view(n, mbh, mbw, 2)
        sad = big_sad[guard:guard + n * mbh * mbw * 4].view(torch.int32).view(n, mbh, mbw)
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
        launches = []
        monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind, info, fn: (launches.append(kind), fn()))
        with pytest.raises(hip.SdvHipError, match="scratch holds"):
            hip.h264_encode_gop_step_sub(y, cb, cr, qp, gop, 0, search, subpel, S.FIRST, mv, *recon, big_s[guard:guard + need_s - 1])
        assert launches == []
        hip.h264_motion_search_sub(y, qp, gop, search, subpel, mv, sad)
        _steps(hip, (y, cb, cr), qp, gop, search, subpel, S.FIRST, mv, recon, big_s[guard:guard + need_s])
        hip.h264_pack(big_s[guard:guard + need_s], n, mbh, hip.h264_gop_slot_mbw(mbw), big_o[guard:guard + need_o], offsets)
        torch.cuda.synchronize()
        assert launches == ["h264_motion_search_sub", "h264_encode_gop_step_sub", "h264_encode_gop_step_sub", "h264_pack"]
        monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
        for big, need in [(big_s, need_s), (big_o, need_o), (big_mv, used.size * 2), (big_sad, n * mbh * mbw * 4)] + [(b, p.size) for b, p in zip(big_r, planes)]:
            host = big.cpu().numpy()
            assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
        assert np.array_equal(mv.cpu().numpy(), used)
        offs = offsets.cpu().tolist()
        out = big_o.cpu().numpy()[guard:]
        assert [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == want
        assert (out[offs[n]:need_o] == 0xA5).all()
        assert all(np.array_equal(r.cpu().numpy(), w) for r, w in zip(recon, want_recon))


def test_subpel_0_and_subpel_omitted_give_the_parents_bytes(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    for shape, kind, qp, search in (((5, 32, 48, 5), "pan2", 16, 8), ((3, 36, 50, 3), "pan1", 28, 2), ((5, 32, 48, 5), "glide1", 0, 16)):
        n, h, w, gop = shape
        frames = torch.from_numpy(S.make_frames(kind, n, h, w)).cuda()
        want = M.reference(shape, kind, qp, search)[1] if kind != "glide1" else M.encode_planes(*S.make_planes(kind, n, h, w), qp=qp, gop=gop,
                                                                                                 first_index=S.FIRST, search=search)[0]
        omitted = H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search).encode(frames, first_index=S.FIRST)
        zero = H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=0).encode(frames, first_index=S.FIRST)
        assert omitted == zero == want
        # accepted without effect where there is no search or no P picture
        assert H264Encoder(qp, torch.device("cuda", 0), gop=gop, subpel=4).encode(frames, first_index=S.FIRST) == \
            H264Encoder(qp, torch.device("cuda", 0), gop=gop).encode(frames, first_index=S.FIRST)
        assert H264Encoder(qp, torch.device("cuda", 0), search=search, subpel=4).encode(frames, first_index=S.FIRST) == \
            H264Encoder(qp, torch.device("cuda", 0)).encode(frames, first_index=S.FIRST)


def _check_file(path, frames, qp, gop, search, subpel):
    """The mp4's samples are the restatement's and decode to the restatement's reconstruction."""
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want, ry, rcb, rcr, _ = S.encode_planes(*R.rgb_to_planes(frames), qp=qp, gop=gop, first_index=0, search=search, subpel=subpel)
    assert samples == want
    d = S.decode_stream(samples, w, h)
    assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr)
    return ry, rcb, rcr


def test_make_video_pyav_gives_the_same_file_whatever_the_upload_batch(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = S.make_frames("glide1", 10, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)
    kw = dict(fps=5, codec="h264-cavlc", h264_gop=4, h264_search=8)
    a = video.make_video_pyav(t, output_filepath=tmp_path / "a.mp4", h264_subpel=4, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8, subpel 4)" and video.LAST_CODEC["subpel"] == 4 and video.LAST_CODEC["search"] == 8
    _check_file(a, frames, 16, 4, 8, 4)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 36 * 50 * 3)                     # one frame's worth: rounded up to one GOP per batch
    b = video.make_video_pyav(torch.from_numpy(frames), output_filepath=tmp_path / "b.mp4", h264_subpel=4, **kw)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 9 * 36 * 50 * 3)                 # nine frames' worth: rounded down to two GOPs
    c = video.make_video_pyav(t, output_filepath=tmp_path / "c.mp4", h264_subpel=4, **kw)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    d = video.make_video_pyav(t, output_filepath=tmp_path / "d.mp4", **kw)
    e = video.make_video_pyav(t, output_filepath=tmp_path / "e.mp4", h264_subpel=0, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8)" and "subpel" not in video.LAST_CODEC
    assert open(d, "rb").read() == open(e, "rb").read() != open(a, "rb").read()
    f = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "f.mp4", codec="h264-cavlc", h264_gop=4, h264_subpel=4)   # no search: no effect
    g = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "g.mp4", codec="h264-cavlc", h264_gop=4)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4)" and open(f, "rb").read() == open(g, "rb").read()
    f = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "h.mp4", codec="h264-cavlc", h264_search=8, h264_subpel=4)  # gop 1: no effect
    g = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "i.mp4", codec="h264-cavlc")
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra)" and open(f, "rb").read() == open(g, "rb").read()


def test_walk_refines_on_request_and_writes_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    for var in ("SDV_VIDEO_CODEC", "SDV_H264_QP", "SDV_H264_GOP", "SDV_H264_SEARCH", "SDV_H264_SUBPEL"):
        monkeypatch.delenv(var, raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=6, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.h264_subpel == 0
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    pipe.h264_subpel = 4                                                             # without the codec, P pictures and a search it changes nothing
    pipe.walk(name="q", **kw)
    assert (tmp_path / "q" / "q.mp4").read_bytes() == default
    pipe.video_codec, pipe.h264_gop, pipe.h264_search = "h264-cavlc", 4, 8
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8, subpel 4)"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (6, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 16, 4, 8, 4)
    monkeypatch.setenv("SDV_H264_SUBPEL", "2")                                       # the variable wins
    pipe.walk(name="e", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8, subpel 2)"
    _check_file(tmp_path / "e" / "e.mp4", frames, 16, 4, 8, 2)


def test_third_party_decoder_agrees(hip, tmp_path, monkeypatch):
    """Where pyav exists: the mp4 with quarter-sample vectors decodes there to exactly the restatement's reconstruction."""
    av = pytest.importorskip("av", reason="pyav is not installed: the stream has met no third-party decoder here")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    for kind in ("glide1", "pan1", "cut"):
        frames = S.make_frames(kind, 7, 64, 64)
        path = video.make_video_pyav(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / f"{kind}.mp4",
                                     codec="h264-cavlc", h264_gop=3, h264_search=8, h264_subpel=4)
        ry, rcb, rcr = _check_file(path, frames, 16, 3, 8, 4)
        with av.open(str(path)) as container:
            decoded = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
        assert len(decoded) == 7
        for k, f in enumerate(decoded):
            assert np.array_equal(f[:64], ry[k]) and np.array_equal(f[64:80].reshape(32, 32), rcb[k]) and np.array_equal(f[80:].reshape(32, 32), rcr[k])
