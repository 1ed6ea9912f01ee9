"""The in-loop deblocking filter on the GPU (sdv_h264_deblock and the _lf entry points behind h264_cavlc.H264Encoder(deblock=1)) against
tests/h264_lf_ref.py: samples and FILTERED reconstruction planes equal the restatement's exactly, and the GPU's bytes decode in that
module's decoder - whose filter is written separately and reads only what it parsed - to the same pictures.  All integer: every comparison
is exact.  Small shapes only."""
import functools

import numpy as np
import pytest
import torch

import h264_i4_ref as I
import h264_lf_ref as L
import h264_ref as R

pytestmark = pytest.mark.gpu
CASES, IDS, _info, _planes = L.CASES, L.IDS, L.random_info, L.random_planes


@functools.lru_cache(maxsize=None)
def _encoder(qp, gop, search, subpel, intra4, deblock=1):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=subpel, intra4=intra4, deblock=deblock)


def _gpu(shape, kind, qp, setting, first_index=L.FIRST, sl=slice(None)):
    """(samples, recon planes as numpy) of pictures ``sl`` of the case, coded in one call from the case's planes."""
    n, h, w = shape
    planes = L.make_planes(kind, n, h, w)
    samples, recon = _encoder(qp, *setting).encode_planes(*(torch.from_numpy(p[sl]).cuda() for p in planes), first_index=first_index, return_recon=True)
    return samples, tuple(r.cpu().numpy() for r in recon)


def _same(got, recon, want, want_recon):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, len(a), len(b))
        assert a == b, (k, next(i for i in range(len(a)) if a[i] != b[i]))
    for a, b in zip(recon, want_recon):
        assert a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("shape,kind,setting", CASES, ids=IDS)
def test_samples_and_filtered_reconstruction_equal_the_restatement_and_decode(hip, shape, kind, setting):
    n, h, w = shape
    for qp in L.QPS:
        got, recon = _gpu(shape, kind, qp, setting)
        _, want, want_recon, _, _ = L.reference(shape, kind, qp, setting)
        assert len(got) == n
        _same(got, recon, want, want_recon)
        d = L.decode_stream(got, w, h)                                              # the GPU's own bytes
        assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon))
        assert d["sync"] == _encoder(qp, *setting).last_sync == list(range(0, n, setting[0]))


def _deblock_alone(hip, planes, info, qp, subpel, waves, n=1, gop=1, k=0):
    """sdv_h264_deblock on ``n`` copies of one picture's planes (position ``k`` of GOPs of ``gop``) -> the planes of every picture."""
    words = torch.from_numpy(np.repeat(L.mbinfo_words([info]), n, axis=0)).cuda()
    mv = (info["mv"] if subpel else info["mv"] // 4).copy()
    mv[~info["mv"].any(axis=-1)] = 6                                                # stale vectors under bit 18 and in intra macroblocks: never read
    mv = torch.from_numpy(np.repeat(mv[None].astype(np.int16), n, axis=0)).cuda()
    dev = [torch.from_numpy(np.repeat(p[None].astype(np.uint8), n, axis=0)).cuda() for p in planes]
    hip.h264_deblock(*dev, qp, gop, k, subpel, words, mv, waves)
    torch.cuda.synchronize()
    return [p.cpu().numpy() for p in dev]


def test_the_filter_alone_does_not_depend_on_the_number_of_waves(hip):
    """Synthetic planes, side information (every bS, I_PCM sides at indexA >= 16, bit 18 against stale vectors) and vectors against the
    restatement on the 3 x 5 and 6 x 8 macroblock grids - their diagonals x + 2 y hold up to 3 and 4 macroblocks, more than one and two
    waves - and on a one-row, a one-column and a one-macroblock picture; whole-sample and quarter-sample vectors."""
    rng = np.random.default_rng(11)
    for mbh, mbw, qp, subpel, lo, hi in ((3, 5, 36, 0, 100, 130), (6, 8, 40, 4, 0, 256), (6, 8, 28, 0, 90, 120), (1, 5, 51, 4, 60, 200), (5, 1, 33, 0, 100, 112),
                                         (1, 1, 40, 0, 0, 256), (3, 5, 15, 4, 100, 104)):
        info = _info(rng, mbh, mbw)
        if not subpel:
            info["mv"] = info["mv"] // 4 * 4 * 2                                    # even whole samples
        planes = _planes(rng, mbh, mbw, lo, hi)
        want = [p.astype(np.int64).copy() for p in planes]
        L.filter_diagonals(*want, qp, info)
        assert qp < 16 or hi - lo > 40 or any(not np.array_equal(a, b) for a, b in zip(want, planes))   # (smooth planes: the filter has work)
        outs = [_deblock_alone(hip, planes, info, qp, subpel, waves) for waves in (1, 2, 0, 16)]
        for got in outs:
            assert all(np.array_equal(g[0], w_) for g, w_ in zip(got, want)), (mbh, mbw, qp)
    # positions: three GOPs of two pictures, position 1 filtered, position 0 left alone
    info, planes = _info(rng, 3, 5), _planes(rng, 3, 5, 100, 130)
    want = [p.astype(np.int64).copy() for p in planes]
    L.filter_diagonals(*want, 36, info)
    got = _deblock_alone(hip, planes, info, 36, 4, 0, n=5, gop=2, k=1)
    for g, w_, p in zip(got, want, planes):
        assert all(np.array_equal(g[f], w_) for f in (1, 3)) and all(np.array_equal(g[f], p) for f in (0, 2, 4))


def test_two_runs_give_the_same_bytes(hip):
    for kind, qp, setting in (("noise", 28, (1, 0, 0, 0)), ("glyphs", 40, (3, 8, 4, 1)), ("pan2", 28, (3, 8, 0, 0)), ("zeros_pcm", 51, (1, 0, 0, 1))):
        runs = [_gpu((3, 36, 50), kind, qp, setting) for _ in range(3)]
        assert all(r[0] == runs[0][0] and all(np.array_equal(x, y) for x, y in zip(r[1], runs[0][1])) for r in runs[1:])


def test_a_batch_of_gops_against_each_gop_coded_alone(hip):
    shape = (6, 36, 50)
    for kind, qp, setting in (("fade", 28, (3, 8, 4, 1)), ("glyphs", 40, (2, 0, 0, 0)), ("noise", 28, (1, 0, 0, 1))):
        gop = setting[0]
        whole, recon = _gpu(shape, kind, qp, setting)
        for g in range(0, shape[0], gop):
            part, part_recon = _gpu(shape, kind, qp, setting, first_index=L.FIRST + g, sl=slice(g, g + gop))
            assert part == whole[g:g + gop] and all(np.array_equal(a, b[g:g + gop]) for a, b in zip(part_recon, recon))


def test_buffers_at_exactly_their_size(hip, monkeypatch):
    """Canary-guarded reconstruction planes, side information and scratch at exactly their sizes through the _lf entry points and the
    filter: the guards stay intact, samples and filtered planes are the restatement's; a side information tensor of another size is
    refused before any launch."""
    guard, qp, gop = 64, 28, 3
    shape, kind, setting = (3, 36, 50), "glyphs", (3, 8, 4, 1)
    planes, want, want_recon, _, infos = L.reference(shape, kind, qp, setting)
    n, mbh, mbw = 3, 3, 4
    y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
    need_s, need_o = hip.h264_gop_scratch_bytes(n, mbh, mbw), hip.h264_gop_out_bytes(n, mbh, mbw)
    canary = lambda size: torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    big_s, big_o, big_i = canary(need_s), canary(need_o), canary(4 * n * mbh * mbw)
    big_r = [canary(p.size) for p in planes]
    recon = [b[guard:guard + p.size].view(p.shape) for b, p in zip(big_r, planes)]
    words = big_i[guard:guard + 4 * n * mbh * mbw].view(torch.int32).view(n, mbh, mbw)
    scratch = big_s[guard:guard + need_s]
    mv = torch.zeros((n, mbh, mbw, 2), dtype=torch.int16, device="cuda")
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
    small = torch.zeros((n, mbh, mbw - 1), dtype=torch.int32, device="cuda")
    with pytest.raises(hip.SdvHipError, match="mbinfo must be"):
        hip.h264_encode_idr4_lf(y, cb, cr, qp, gop, L.FIRST, *recon, scratch, small)
    with pytest.raises(hip.SdvHipError, match="mbinfo must be"):
        hip.h264_deblock(*recon, qp, gop, 0, 4, small, mv)
    with pytest.raises(hip.SdvHipError, match="waves must be"):
        hip.h264_deblock(*recon, qp, gop, 0, 4, words, mv, 17)
    assert launches == []
    hip.h264_motion_search_sub(y, qp, gop, 8, 4, mv)
    hip.h264_encode_idr4_lf(y, cb, cr, qp, gop, L.FIRST, *recon, scratch, words)
    hip.h264_deblock(*recon, qp, gop, 0, 4, words, mv)
    for k in (1, 2):
        hip.h264_encode_gop_step_sub_lf(y, cb, cr, qp, gop, k, 8, 4, L.FIRST, mv, *recon, scratch, words)
        hip.h264_deblock(*recon, qp, gop, k, 4, words, mv, 1 + k)
    hip.h264_pack(scratch, n, mbh, hip.h264_gop_slot_mbw(mbw), big_o[guard:guard + need_o], offsets)
    torch.cuda.synchronize()
    assert launches == ["h264_motion_search_sub", "h264_encode_idr4_lf", "h264_deblock", "h264_encode_gop_step_sub_lf", "h264_deblock",
                        "h264_encode_gop_step_sub_lf", "h264_deblock", "h264_pack"]
    monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
    for big, need in [(big_s, need_s), (big_o, need_o), (big_i, 4 * n * mbh * mbw)] + [(b, p.size) for b, p in zip(big_r, planes)]:
        host = big.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    offs = offsets.cpu().tolist()
    out = big_o.cpu().numpy()[guard:]
    assert [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == want
    assert all(np.array_equal(r.cpu().numpy(), w_) for r, w_ in zip(recon, want_recon))
    assert np.array_equal(words.cpu().numpy(), L.mbinfo_words(infos))


def test_deblock_0_and_deblock_omitted_give_the_parents_bytes_and_launches(hip, monkeypatch):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    dev = torch.device("cuda", 0)
    for shape, kind, qp, (gop, search, subpel, intra4) in (((3, 36, 50), "glyphs", 16, (1, 0, 0, 0)), ((3, 32, 48), "grat4", 28, (3, 8, 4, 1)),
                                                           ((3, 36, 50), "noise", 28, (3, 0, 0, 0))):
        n, h, w = shape
        frames = torch.from_numpy(I.make_frames(kind, n, h, w)).cuda()
        want = I.reference(shape, kind, qp, (gop, search, subpel), intra4)[1]
        traces = []
        for kw in ({}, dict(deblock=0)):
            launches = []
            monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
            got = H264Encoder(qp, dev, gop=gop, search=search, subpel=subpel, intra4=intra4, **kw).encode(frames, first_index=I.FIRST)
            monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
            assert got == want
            traces.append(launches)
        assert traces[0] == traces[1] and not any("_lf" in k or "deblock" in k for k in traces[0])
    launches = []                                                                   # and with it: one filter launch after every position but the last
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
    H264Encoder(28, dev, gop=3, deblock=1).encode(frames, first_index=0)
    monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
    assert launches == ["h264_planes", "h264_encode_gop_step_lf", "h264_deblock", "h264_encode_gop_step_lf", "h264_deblock", "h264_encode_gop_step_lf",
                        "h264_pack"]


def _check_file(path, frames, qp, gop, search, subpel, intra4):
    """The mp4's samples are the restatement's and decode to the restatement's filtered reconstruction."""
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want, ry, rcb, rcr, _, _ = L.encode_planes(*R.rgb_to_planes(frames), qp=qp, gop=gop, first_index=0, search=search, subpel=subpel, intra4=intra4)
    assert samples == want
    d = L.decode_stream(samples, w, h)
    assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr)
    return ry, rcb, rcr


def test_make_video_pyav_gives_the_same_file_whatever_the_upload_batch(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = I.make_frames("glyphs", 10, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)
    kw = dict(fps=5, codec="h264-cavlc", h264_qp=28, h264_gop=4, h264_search=8)
    a = video.make_video_pyav(t, output_filepath=tmp_path / "a.mp4", h264_deblock=1, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8) + deblock" and video.LAST_CODEC["deblock"] == 1
    _check_file(a, frames, 28, 4, 8, 0, 0)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 36 * 50 * 3)                     # one frame's worth: rounded up to one GOP per batch
    b = video.make_video_pyav(torch.from_numpy(frames), output_filepath=tmp_path / "b.mp4", h264_deblock=1, **kw)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 9 * 36 * 50 * 3)                 # nine frames' worth: rounded down to two GOPs
    c = video.make_video_pyav(t, output_filepath=tmp_path / "c.mp4", h264_deblock=1, **kw)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    d = video.make_video_pyav(t, output_filepath=tmp_path / "d.mp4", **kw)
    e = video.make_video_pyav(t, output_filepath=tmp_path / "e.mp4", h264_deblock=0, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8)" and "deblock" not in video.LAST_CODEC
    assert open(d, "rb").read() == open(e, "rb").read() != open(a, "rb").read()
    f = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "f.mp4", codec="h264-cavlc", h264_qp=28, h264_intra4=1, h264_deblock=1)   # all intra
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra) + intra4 + deblock"
    _check_file(f, frames, 28, 1, 0, 0, 1)


def test_walk_filters_on_request_and_writes_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    for var in ("SDV_VIDEO_CODEC", "SDV_H264_QP", "SDV_H264_GOP", "SDV_H264_SEARCH", "SDV_H264_SUBPEL", "SDV_H264_INTRA4", "SDV_H264_DEBLOCK"):
        monkeypatch.delenv(var, raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=6, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.h264_deblock == 0
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    pipe.h264_deblock = 1                                                            # without the codec it changes nothing
    pipe.walk(name="q", **kw)
    assert (tmp_path / "q" / "q.mp4").read_bytes() == default
    pipe.video_codec, pipe.h264_gop, pipe.h264_qp = "h264-cavlc", 4, 30
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4) + deblock"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (6, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 30, 4, 0, 0, 0)
    monkeypatch.setenv("SDV_H264_DEBLOCK", "0")                                      # the variable wins
    pipe.walk(name="e", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4)" and "deblock" not in video.LAST_CODEC
    width, height, entry, samples = R.mp4_samples(tmp_path / "e" / "e.mp4")
    assert samples == I.encode_planes(*R.rgb_to_planes(frames), qp=30, gop=4, first_index=0)[0]


def test_third_party_decoder_agrees(hip, tmp_path, monkeypatch):
    """Where pyav exists: the mp4 with the loop filter on decodes there to exactly the restatement's filtered reconstruction."""
    av = pytest.importorskip("av", reason="pyav is not installed: the stream has met no third-party decoder here")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    for kind in ("glyphs", "grat5", "noise"):
        frames = I.make_frames(kind, 7, 64, 64)
        path = video.make_video_pyav(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / f"{kind}.mp4",
                                     codec="h264-cavlc", h264_qp=28, h264_gop=3, h264_search=8, h264_subpel=4, h264_intra4=1, h264_deblock=1)
        ry, rcb, rcr = _check_file(path, frames, 28, 3, 8, 4, 1)
        with av.open(str(path)) as container:
            decoded = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
        assert len(decoded) == 7
        for k, f in enumerate(decoded):
            assert np.array_equal(f[:64], ry[k]) and np.array_equal(f[64:80].reshape(32, 32), rcb[k]) and np.array_equal(f[80:].reshape(32, 32), rcr[k])
