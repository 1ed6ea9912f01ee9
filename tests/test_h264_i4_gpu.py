"""Intra4x4 IDR pictures on the GPU (sdv_h264_encode_idr4 behind h264_cavlc.H264Encoder(intra4=1)) against tests/h264_i4_ref.py: samples
and reconstruction planes equal the restatement's exactly, and the GPU's bytes decode in that module's decoder to the same pictures.  All
integer: every comparison is exact.  Small shapes only."""
import functools

import numpy as np
import pytest
import torch

import h264_i4_ref as I
import h264_ref as R

pytestmark = pytest.mark.gpu

CASES = [(s, k, g) for s in I.SHAPES for k in I.KINDS for g in I.SETTINGS] + [((2, 96, 128), k, (1, 0, 0)) for k in I.EXTRA_KINDS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}-gop{g[0]}-search{g[1]}-subpel{g[2]}" for s, k, g in CASES]


@functools.lru_cache(maxsize=None)
def _encoder(qp, gop, search, subpel, intra4=1):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=subpel, intra4=intra4)


def _gpu(shape, kind, qp, setting, first_index=I.FIRST, sl=slice(None)):
    """(samples, recon planes as numpy) of pictures ``sl`` of the case, coded in one call."""
    n, h, w = shape
    enc = _encoder(qp, *setting)
    if kind.endswith("_pcm"):
        samples, recon = enc.encode_planes(*(torch.from_numpy(p[sl]).cuda() for p in I.make_planes(kind, n, h, w)), first_index=first_index,
                                           return_recon=True)
    else:
        samples, recon = enc.encode(torch.from_numpy(I.make_frames(kind, n, h, w)[sl]).cuda(), first_index=first_index, return_recon=True)
    return samples, tuple(r.cpu().numpy() for r in recon)


def _same(got, recon, want, want_recon):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, len(a), len(b))
        assert a == b, (k, next(i for i in range(len(a)) if a[i] != b[i]))
    for a, b in zip(recon, want_recon):
        assert a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("shape,kind,setting", CASES, ids=IDS)
def test_samples_and_reconstruction_equal_the_restatement_and_decode(hip, shape, kind, setting):
    n, h, w = shape
    for qp in I.QPS:
        got, recon = _gpu(shape, kind, qp, setting)
        _, want, want_recon, _ = I.reference(shape, kind, qp, setting)
        assert len(got) == n
        _same(got, recon, want, want_recon)
        d = I.decode_stream(got, w, h)                                              # the GPU's own bytes
        assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon))
        assert d["sync"] == _encoder(qp, *setting).last_sync == list(range(0, n, setting[0])) and d["p_i4"] == 0


def test_two_runs_give_the_same_bytes(hip):
    for kind, qp, setting in (("noise", 16, (1, 0, 0)), ("glyphs", 0, (3, 8, 4)), ("grat5", 28, (3, 0, 0)), ("zeros_pcm", 51, (1, 0, 0))):
        a, b = _gpu((3, 36, 50), kind, qp, setting), _gpu((3, 36, 50), kind, qp, setting)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_a_batch_of_idr_pictures_against_each_coded_alone(hip):
    shape = (3, 36, 50)
    for kind, qp in (("glyphs", 16), ("noise", 0), ("grat7", 28)):
        whole, recon = _gpu(shape, kind, qp, (1, 0, 0))
        for k in range(shape[0]):
            part, part_recon = _gpu(shape, kind, qp, (1, 0, 0), first_index=I.FIRST + k, sl=slice(k, k + 1))
            assert part == whole[k:k + 1] and all(np.array_equal(a, b[k:k + 1]) for a, b in zip(part_recon, recon))


def test_buffers_at_exactly_the_documented_capacity(hip, monkeypatch):
    """Canary-guarded scratch, output and reconstruction buffers at exactly their sizes on hostile samples that make every macroblock
    I_PCM (from the I_NxN candidate or the Intra16x16 one): the guards stay intact and the samples are right; one byte less of scratch is
    refused before any launch."""
    guard, qp = 64, 0
    n, mbh, mbw = 3, 2, 3
    rng = np.random.default_rng(5)
    hostile = lambda *sh: np.where(rng.random(sh) < 0.5, rng.integers(0, 4, sh), 252 + rng.integers(0, 4, sh)).astype(np.uint8)
    planes = (hostile(n, 32, 48), hostile(n, 16, 24), hostile(n, 16, 24))
    for gop in (1, 2):
        stats = I.new_stats()
        want, *want_recon, _ = I.encode_planes(*planes, qp=qp, gop=gop, first_index=I.FIRST, stats=stats, intra4=1)
        idr = len(range(0, n, gop))
        assert stats["n_pcm"] >= idr * mbh * mbw and stats["i4"]["pcm_from_i4"] > 0
        y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
        need_s, need_o = hip.h264_gop_scratch_bytes(n, mbh, mbw), hip.h264_gop_out_bytes(n, mbh, mbw)
        canary = lambda size: torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        big_s, big_o = canary(need_s), canary(need_o)
        big_r = [canary(p.size) for p in planes]
        recon = [b[guard:guard + p.size].view(p.shape) for b, p in zip(big_r, planes)]
        mv = torch.zeros((n, mbh, mbw, 2), dtype=torch.int16, device="cuda")
        offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
        launches = []
        monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind, info, fn: (launches.append(kind), fn()))
        with pytest.raises(hip.SdvHipError, match="scratch holds"):
            hip.h264_encode_idr4(y, cb, cr, qp, gop, I.FIRST, *recon, big_s[guard:guard + need_s - 1])
        assert launches == []
        hip.h264_encode_idr4(y, cb, cr, qp, gop, I.FIRST, *recon, big_s[guard:guard + need_s])
        for k in range(1, min(gop, n)):
            hip.h264_encode_gop_step(y, cb, cr, qp, gop, k, 2, I.FIRST, mv, *recon, big_s[guard:guard + need_s])
        hip.h264_pack(big_s[guard:guard + need_s], n, mbh, hip.h264_gop_slot_mbw(mbw), big_o[guard:guard + need_o], offsets)
        torch.cuda.synchronize()
        assert launches == ["h264_encode_idr4"] + ["h264_encode_gop_step"] * (min(gop, n) - 1) + ["h264_pack"]
        monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
        for big, need in [(big_s, need_s), (big_o, need_o)] + [(b, p.size) for b, p in zip(big_r, planes)]:
            host = big.cpu().numpy()
            assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
        offs = offsets.cpu().tolist()
        out = big_o.cpu().numpy()[guard:]
        assert [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == want
        assert (out[offs[n]:need_o] == 0xA5).all()
        assert all(np.array_equal(r.cpu().numpy(), w) for r, w in zip(recon, want_recon))


def test_intra4_0_and_intra4_omitted_give_the_parents_bytes(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    for shape, kind, qp, (gop, search, subpel) in (((3, 36, 50), "glyphs", 16, (1, 0, 0)), ((3, 32, 48), "grat4", 28, (3, 8, 4)),
                                                   ((3, 36, 50), "noise", 0, (3, 0, 0))):
        n, h, w = shape
        frames = torch.from_numpy(I.make_frames(kind, n, h, w)).cuda()
        want = I.reference(shape, kind, qp, (gop, search, subpel), 0)[1]
        omitted = H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=subpel).encode(frames, first_index=I.FIRST)
        zero = H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=subpel, intra4=0).encode(frames, first_index=I.FIRST)
        assert omitted == zero == want


def _check_file(path, frames, qp, gop, search, subpel, expect_i4=True):
    """The mp4's samples are the restatement's and decode to the restatement's reconstruction."""
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want, ry, rcb, rcr, _ = I.encode_planes(*R.rgb_to_planes(frames), qp=qp, gop=gop, first_index=0, search=search, subpel=subpel, intra4=1)
    assert samples == want
    d = I.decode_stream(samples, w, h)
    assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr) and (d["n_i4"] > 0 or not expect_i4)
    return ry, rcb, rcr


def test_make_video_pyav_gives_the_same_file_whatever_the_upload_batch(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = I.make_frames("glyphs", 10, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)
    kw = dict(fps=5, codec="h264-cavlc", h264_gop=4, h264_search=8)
    a = video.make_video_pyav(t, output_filepath=tmp_path / "a.mp4", h264_intra4=1, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8) + intra4" and video.LAST_CODEC["intra4"] == 1
    _check_file(a, frames, 16, 4, 8, 0)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 36 * 50 * 3)                     # one frame's worth: rounded up to one GOP per batch
    b = video.make_video_pyav(torch.from_numpy(frames), output_filepath=tmp_path / "b.mp4", h264_intra4=1, **kw)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 9 * 36 * 50 * 3)                 # nine frames' worth: rounded down to two GOPs
    c = video.make_video_pyav(t, output_filepath=tmp_path / "c.mp4", h264_intra4=1, **kw)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    d = video.make_video_pyav(t, output_filepath=tmp_path / "d.mp4", **kw)
    e = video.make_video_pyav(t, output_filepath=tmp_path / "e.mp4", h264_intra4=0, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8)" and "intra4" not in video.LAST_CODEC
    assert open(d, "rb").read() == open(e, "rb").read() != open(a, "rb").read()
    f = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "f.mp4", codec="h264-cavlc", h264_intra4=1)      # all intra
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra) + intra4"
    _check_file(f, frames, 16, 1, 0, 0)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 3 * 36 * 50 * 3)
    g = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "g.mp4", codec="h264-cavlc", h264_intra4=1)
    assert open(f, "rb").read() == open(g, "rb").read()


def test_walk_uses_intra4_on_request_and_writes_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    for var in ("SDV_VIDEO_CODEC", "SDV_H264_QP", "SDV_H264_GOP", "SDV_H264_SEARCH", "SDV_H264_SUBPEL", "SDV_H264_INTRA4"):
        monkeypatch.delenv(var, raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=6, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.h264_intra4 == 0
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    pipe.h264_intra4 = 1                                                             # without the codec it changes nothing
    pipe.walk(name="q", **kw)
    assert (tmp_path / "q" / "q.mp4").read_bytes() == default
    pipe.video_codec, pipe.h264_gop = "h264-cavlc", 4
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4) + intra4"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (6, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 16, 4, 0, 0, expect_i4=False)
    monkeypatch.setenv("SDV_H264_INTRA4", "0")                                       # the variable wins
    pipe.walk(name="e", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4)" and "intra4" not in video.LAST_CODEC
    width, height, entry, samples = R.mp4_samples(tmp_path / "e" / "e.mp4")
    assert samples == I.encode_planes(*R.rgb_to_planes(frames), qp=16, gop=4, first_index=0)[0]


def test_third_party_decoder_agrees(hip, tmp_path, monkeypatch):
    """Where pyav exists: the mp4 with I_NxN macroblocks decodes there to exactly the restatement's reconstruction."""
    av = pytest.importorskip("av", reason="pyav is not installed: the stream has met no third-party decoder here")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    for kind in ("glyphs", "grat5", "noise"):
        frames = I.make_frames(kind, 7, 64, 64)
        path = video.make_video_pyav(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / f"{kind}.mp4",
                                     codec="h264-cavlc", h264_gop=3, h264_search=8, h264_subpel=4, h264_intra4=1)
        ry, rcb, rcr = _check_file(path, frames, 16, 3, 8, 4)
        with av.open(str(path)) as container:
            decoded = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
        assert len(decoded) == 7
        for k, f in enumerate(decoded):
            assert np.array_equal(f[:64], ry[k]) and np.array_equal(f[64:80].reshape(32, 32), rcb[k]) and np.array_equal(f[80:].reshape(32, 32), rcr[k])
