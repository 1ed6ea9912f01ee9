"""Motion-compensated P pictures on the GPU (sdv_h264_motion_search and sdv_h264_encode_gop_step behind
h264_cavlc.H264Encoder(gop=..., search=...)) against tests/h264_me_ref.py: vectors, SADs, samples and reconstruction planes equal the
restatement's exactly, and the GPU's bytes decode in the separately written decoder of tests/h264_p_ref.py to the same pictures.  All
integer: every comparison is exact.  Shapes (n, H, W, gop), kinds, qp and search ranges: h264_me_ref.SHAPES / KINDS / QPS / SEARCHES.  Only
vectors the rule admits are handed to the GPU here; the others are the host program's (test_h264_me_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

import h264_me_ref as M
import h264_p_ref as P
import h264_ref as R

pytestmark = pytest.mark.gpu

CASES = [(s, k, q, r) for s in M.SHAPES for k in M.KINDS for q in M.QPS for r in M.SEARCHES]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-gop{s[3]}-{k}-qp{q}-search{r}" for s, k, q, r in CASES]
INJECTED = [((7, 64, 64, 3), 16, 8, "random"), ((7, 64, 64, 3), 0, 16, "extreme"), ((5, 32, 48, 5), 28, 2, "random"),
            ((6, 96, 128, 2), 28, 16, "random"), ((3, 36, 50, 3), 16, 2, "extreme")]


@functools.lru_cache(maxsize=None)
def _encoder(qp, gop, search):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search)


def _gpu(shape, kind, qp, search, first_index=M.FIRST, sl=slice(None)):
    """(samples, recon planes as numpy) of pictures ``sl`` of the case, coded in one call."""
    n, h, w, gop = shape
    enc = _encoder(qp, gop, search)
    if kind == "zeros_pcm":
        samples, recon = enc.encode_planes(*(torch.from_numpy(p[sl]).cuda() for p in M.make_planes(kind, n, h, w)), first_index=first_index,
                                           return_recon=True)
    else:
        samples, recon = enc.encode(torch.from_numpy(M.make_frames(kind, n, h, w)[sl]).cuda(), first_index=first_index, return_recon=True)
    return samples, tuple(r.cpu().numpy() for r in recon)


def _steps(hip, planes, qp, gop, search, first_index, mv, recon, scratch):
    n = planes[0].shape[0]
    for k in range(min(gop, n)):
        hip.h264_encode_gop_step(*planes, qp, gop, k, search, first_index, mv, *recon, scratch)


def _gpu_with_vectors(hip, planes, qp, gop, search, mv, first_index=M.FIRST):
    """The launches of H264Encoder._rows_and_pack with given vectors in place of the searched ones."""
    n, mbh, mbw = planes[0].shape[0], planes[0].shape[1] // 16, planes[0].shape[2] // 16
    dev = [torch.from_numpy(p).cuda() for p in planes]
    recon = [torch.empty_like(p) for p in dev]
    scratch = torch.empty((hip.h264_gop_scratch_bytes(n, mbh, mbw),), dtype=torch.uint8, device="cuda")
    out = torch.empty((hip.h264_gop_out_bytes(n, mbh, mbw),), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    _steps(hip, dev, qp, gop, search, first_index, torch.from_numpy(mv).cuda(), recon, scratch)
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


def _search(hip, y, qp, gop, search):
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    mv = torch.full((n, mbh, mbw, 2), 99, dtype=torch.int16, device="cuda")
    sad = torch.full((n, mbh, mbw), -1, dtype=torch.int32, device="cuda")
    hip.h264_motion_search(torch.from_numpy(y).cuda(), qp, gop, search, mv, sad)
    return mv.cpu().numpy(), sad.cpu().numpy()


@pytest.mark.parametrize("search", (2, 8, 16))
def test_search_kernel_alone_equals_the_numpy_search(hip, search):
    """Vectors and SADs: flat input where every candidate ties, a period-2 picture where every even shift ties, one macroblock, pictures
    whose every macroblock is an edge macroblock, shifted and planted content, noise; qp moves lambda."""
    flat = np.full((3, 48, 64), 77, dtype=np.uint8)
    stripes = flat.copy()
    stripes[:, ::2] = 200
    inputs = [(flat, 16, 3), (stripes, 16, 3), (M.make_planes("noise", 3, 16, 16)[0], 16, 3), (M.make_planes("noise", 4, 32, 32)[0], 0, 2),
              (M.make_planes("pan2", 4, 96, 128)[0], 16, 4), (M.make_planes("drift", 4, 96, 128)[0], 51, 3), (M.make_planes("pan1", 3, 36, 50)[0], 28, 3),
              (M.plant(5, 64, 64, M.inject("random", 5, 4, 4, search), search)[0], 16, 5),
              (M.plant(3, 64, 64, M.inject("extreme", 3, 4, 4, search), search)[0], 40, 3)]
    for y, qp, gop in inputs:
        want_mv, want_sad = M.search_planes(y, qp, gop, search)
        mv, sad = _search(hip, y, qp, gop, search)
        assert np.array_equal(mv, want_mv), (y.shape, qp, gop, np.argwhere(mv != want_mv)[:4])
        assert np.array_equal(sad, want_sad), (y.shape, qp, gop)
    mv, _ = _search(hip, flat, 16, 3, search)
    assert not mv.any()
    mv, sad = _search(hip, stripes, 0, 1, search)                                   # gop 1: every picture an IDR picture
    assert not mv.any() and not sad.any()


@pytest.mark.parametrize("shape,kind,qp,search", CASES, ids=IDS)
def test_samples_and_reconstruction_equal_the_restatement_and_decode(hip, shape, kind, qp, search):
    n, h, w, gop = shape
    got, recon = _gpu(shape, kind, qp, search)
    _, want, want_recon, _, _ = M.reference(shape, kind, qp, search)
    assert len(got) == n
    _same(got, recon, want, want_recon)
    d = P.decode_stream(got, w, h)                                                  # the GPU's own bytes
    assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon))
    assert d["sync"] == _encoder(qp, gop, search).last_sync == list(range(0, n, gop))


@pytest.mark.parametrize("shape,qp,search,kind", INJECTED, ids=[f"{s[0]}x{s[1]}x{s[2]}-gop{s[3]}-qp{q}-search{r}-{k}" for s, q, r, k in INJECTED])
def test_injected_vectors_equal_the_restatement_and_decode(hip, shape, qp, search, kind):
    """Given vectors (all admitted) on planes planted with them: both signs and the largest |mvd|, nonzero vectors without a residual,
    after intra, I_PCM and skip, at every edge of the picture."""
    n, h, w, gop = shape
    planes, want, want_recon, _, used = M.reference(shape, "planted", qp, search, kind)
    mv = M.inject(kind, n, used.shape[1], used.shape[2], search)
    on_p = mv.copy()
    on_p[::gop] = 0                                                                 # (IDR pictures carry no vector)
    assert np.array_equal(on_p, used)                                               # nothing here that the rule does not admit
    got, recon = _gpu_with_vectors(hip, planes, qp, gop, search, mv)
    _same(got, recon, want, want_recon)
    d = P.decode_stream(got, w, h)
    assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon))
    searched, searched_recon = _encoder(qp, gop, search).encode_planes(*(torch.from_numpy(p).cuda() for p in planes), first_index=M.FIRST,
                                                                       return_recon=True)
    ref = M.encode_planes(*planes, qp=qp, gop=gop, first_index=M.FIRST, search=search)
    _same(searched, tuple(r.cpu().numpy() for r in searched_recon), ref[0], ref[1:4])


def test_two_runs_give_the_same_bytes(hip):
    for kind, qp, search in (("noise", 16, 8), ("drift", 0, 16), ("pan1", 28, 2)):
        a, b = _gpu((7, 64, 64, 3), kind, qp, search), _gpu((7, 64, 64, 3), kind, qp, search)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_a_gop_codes_the_same_alone_and_inside_a_longer_call(hip):
    shape = (7, 64, 64, 3)
    for kind, qp, search in (("drift", 16, 8), ("cut", 0, 16), ("pan2", 28, 2)):
        whole, recon = _gpu(shape, kind, qp, search)
        for lo, hi in ((0, 3), (3, 6), (6, 7), (3, 7)):
            part, part_recon = _gpu(shape, kind, qp, search, first_index=M.FIRST + lo, sl=slice(lo, hi))
            assert part == whole[lo:hi] and all(np.array_equal(a, b[lo:hi]) for a, b in zip(part_recon, recon))


def test_buffers_at_exactly_the_documented_capacity(hip, monkeypatch):
    """Canary-guarded mv, sad, scratch, output and reconstruction buffers at exactly their sizes, on planted planes with the longest
    vectors at every edge and on hostile samples that make every macroblock I_PCM: the guards stay intact and the samples are right; one
    byte less of scratch is refused before any launch."""
    guard, qp, gop, search = 64, 0, 2, 16
    n, mbh, mbw = 4, 2, 3
    rng = np.random.default_rng(5)
    hostile = lambda *sh: np.where(rng.random(sh) < 0.5, rng.integers(0, 4, sh), 252 + rng.integers(0, 4, sh)).astype(np.uint8)
    for planes in (M.plant(n, 32, 48, M.inject("extreme", n, mbh, mbw, search), search), (hostile(4, 32, 48), hostile(4, 16, 24), hostile(4, 16, 24))):
        want, *want_recon, used = M.encode_planes(*planes, qp=qp, gop=gop, first_index=M.FIRST, search=search)
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
            hip.h264_encode_gop_step(y, cb, cr, qp, gop, 0, search, M.FIRST, mv, *recon, big_s[guard:guard + need_s - 1])
        assert launches == []
        hip.h264_motion_search(y, qp, gop, search, mv, sad)
        _steps(hip, (y, cb, cr), qp, gop, search, M.FIRST, mv, recon, big_s[guard:guard + need_s])
        hip.h264_pack(big_s[guard:guard + need_s], n, mbh, hip.h264_gop_slot_mbw(mbw), big_o[guard:guard + need_o], offsets)
        torch.cuda.synchronize()
        assert launches == ["h264_motion_search", "h264_encode_gop_step", "h264_encode_gop_step", "h264_pack"]
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


def _check_file(path, frames, qp, gop, search):
    """The mp4's samples are the restatement's and decode to the restatement's reconstruction."""
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want, ry, rcb, rcr, _ = M.encode_planes(*R.rgb_to_planes(frames), qp=qp, gop=gop, first_index=0, search=search)
    assert samples == want
    d = P.decode_stream(samples, w, h)
    assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr)
    return ry, rcb, rcr


def test_make_video_pyav_gives_the_same_file_whatever_the_upload_batch(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = M.make_frames("drift", 10, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)
    a = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=4, h264_search=8)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8)" and video.LAST_CODEC["search"] == 8
    _check_file(a, frames, 16, 4, 8)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 36 * 50 * 3)                     # one frame's worth: rounded up to one GOP per batch
    b = video.make_video_pyav(torch.from_numpy(frames), fps=5, output_filepath=tmp_path / "b.mp4", codec="h264-cavlc", h264_gop=4, h264_search=8)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 9 * 36 * 50 * 3)                 # nine frames' worth: rounded down to two GOPs
    c = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "c.mp4", codec="h264-cavlc", h264_gop=4, h264_search=8)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    d = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "d.mp4", codec="h264-cavlc", h264_gop=4)
    e = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "e.mp4", codec="h264-cavlc", h264_gop=4, h264_search=0)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4)" and open(d, "rb").read() == open(e, "rb").read() != open(a, "rb").read()
    f = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "f.mp4", codec="h264-cavlc", h264_search=8)       # gop 1: no effect
    g = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "g.mp4", codec="h264-cavlc")
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra)" and open(f, "rb").read() == open(g, "rb").read()


def test_walk_searches_on_request_and_writes_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    for var in ("SDV_VIDEO_CODEC", "SDV_H264_QP", "SDV_H264_GOP", "SDV_H264_SEARCH"):
        monkeypatch.delenv(var, raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=6, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.h264_search == 0
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    pipe.h264_search = 8                                                             # without the codec, and without P pictures, it changes nothing
    pipe.walk(name="q", **kw)
    assert (tmp_path / "q" / "q.mp4").read_bytes() == default
    pipe.video_codec = "h264-cavlc"
    pipe.walk(name="i", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra)"
    pipe.h264_search = 0
    pipe.walk(name="j", **kw)
    assert (tmp_path / "i" / "i.mp4").read_bytes() == (tmp_path / "j" / "j.mp4").read_bytes()
    pipe.h264_gop, pipe.h264_search = 4, 8
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8)"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (6, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 16, 4, 8)
    monkeypatch.setenv("SDV_H264_SEARCH", "2")                                       # the variable wins
    pipe.walk(name="e", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 2)"
    _check_file(tmp_path / "e" / "e.mp4", frames, 16, 4, 2)


def test_third_party_decoder_agrees(hip, tmp_path, monkeypatch):
    """Where pyav exists: the mp4 with motion-compensated P pictures decodes there to exactly the restatement's reconstruction."""
    av = pytest.importorskip("av", reason="pyav is not installed: the stream has met no third-party decoder here")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    for kind in ("drift", "pan1", "cut"):
        frames = M.make_frames(kind, 7, 64, 64)
        path = video.make_video_pyav(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / f"{kind}.mp4",
                                     codec="h264-cavlc", h264_gop=3, h264_search=8)
        ry, rcb, rcr = _check_file(path, frames, 16, 3, 8)
        with av.open(str(path)) as container:
            decoded = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
        assert len(decoded) == 7
        for k, f in enumerate(decoded):
            assert np.array_equal(f[:64], ry[k]) and np.array_equal(f[64:80].reshape(32, 32), rcb[k]) and np.array_equal(f[80:].reshape(32, 32), rcr[k])
