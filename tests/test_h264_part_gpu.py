"""Macroblock partitions on the GPU (the four entry points of include/sdv_hip_h264_part.h behind h264_cavlc.H264Encoder(part=1)) against
tests/h264_part_ref.py: samples, reconstruction planes, vectors, SADs and side information equal the restatement's exactly, and the GPU's
own bytes decode in that module's decoder - its own sub_mb_pred reader, general neighbour derivation and per-partition prediction - to the
GPU's reconstruction.  All integer: every comparison is exact.  Small shapes only."""
import functools

import numpy as np
import pytest
import torch

import h264_i4_ref as I
import h264_lf_ref as L
import h264_part_ref as Q
import h264_ref as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _encoder(qp, gop, search, subpel, intra4, deblock, part=1):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part)


def _same(got, recon, want, want_recon):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, len(a), len(b))
        assert a == b, (k, next(i for i in range(len(a)) if a[i] != b[i]))
    for a, b in zip(recon, want_recon):
        assert a.shape == b.shape and np.array_equal(a, b)


def _steps(hip, planes, mv, qp, gop, search, subpel, intra4, deblock, first_index=Q.FIRST, waves=0):
    """The route of H264Encoder(part=1) with given vectors instead of searched ones -> (samples, recon, words or None)."""
    y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    recon = [torch.empty_like(t) for t in (y, cb, cr)]
    scratch = torch.empty((hip.h264_gop_scratch_bytes(n, mbh, mbw),), dtype=torch.uint8, device="cuda")
    out = torch.empty((hip.h264_gop_out_bytes(n, mbh, mbw),), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    words = torch.zeros((n, mbh, mbw), dtype=torch.int32, device="cuda") if deblock else None
    mvt = torch.from_numpy(np.ascontiguousarray(mv)).cuda()
    for k in range(min(gop, n)):
        if k == 0 and intra4 and deblock:
            hip.h264_encode_idr4_lf(y, cb, cr, qp, gop, first_index, *recon, scratch, words)
        elif k == 0 and intra4:
            hip.h264_encode_idr4(y, cb, cr, qp, gop, first_index, *recon, scratch)
        elif deblock:
            hip.h264_encode_gop_step_part_lf(y, cb, cr, qp, gop, k, search, subpel, first_index, mvt, *recon, scratch, words)
        else:
            hip.h264_encode_gop_step_part(y, cb, cr, qp, gop, k, search, subpel, first_index, mvt, *recon, scratch)
        if deblock:
            hip.h264_deblock_part(*recon, qp, gop, k, words, mvt, waves)
    hip.h264_pack(scratch, n, mbh, hip.h264_gop_slot_mbw(mbw), out, offsets)
    torch.cuda.synchronize()
    offs, host = offsets.cpu().tolist(), out.cpu().numpy()
    return [host[offs[k]:offs[k + 1]].tobytes() for k in range(n)], tuple(r.cpu().numpy() for r in recon), None if words is None else words.cpu().numpy()


@pytest.mark.parametrize("qp", Q.QPS)
@pytest.mark.parametrize("shape,kind,injected", Q.CASES, ids=Q.IDS)
def test_samples_and_reconstruction_equal_the_restatement_and_decode(hip, shape, kind, injected, qp):
    """Every CPU round-trip case.  Searched kinds go through H264Encoder (the search launch included); injected kinds - off-grid,
    out-of-range and not admitted vectors in one partition among them - through the step entry points with those vectors."""
    n, h, w = shape
    for subpel in Q.SUBPELS:
        for intra4, deblock in Q.FILTERS:
            planes, want, want_recon, used, infos, _ = Q.reference(shape, kind, qp, subpel, (intra4, deblock), injected=injected)
            if injected is None:
                enc = _encoder(qp, n, Q.SEARCH, subpel, intra4, deblock)
                got, recon = enc.encode_planes(*(torch.from_numpy(p).cuda() for p in planes), first_index=Q.FIRST, return_recon=True)
                recon = tuple(r.cpu().numpy() for r in recon)
                assert enc.last_sync == [0]
            else:
                mv = Q.inject(injected, n, (h + 15) // 16, (w + 15) // 16, Q.SEARCH, subpel)
                got, recon, words = _steps(hip, planes, mv, qp, n, Q.SEARCH, subpel, intra4, deblock)
                if deblock:
                    assert np.array_equal(words, Q.mbinfo_words(infos)), (qp, subpel)
            _same(got, recon, want, want_recon)
            d = Q.decode_stream(got, w, h)                                      # the GPU's own bytes
            assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon)), (qp, subpel, intra4, deblock)


@pytest.mark.parametrize("shape", Q.SHAPES, ids=["x".join(map(str, s)) for s in Q.SHAPES])
def test_the_search_alone_equals_the_restatement(hip, shape):
    """Vectors and the five SADs of every macroblock, the edge macroblocks of every shape among them, at every subpel; search 2 and 16 on
    the kinds that move, 8 everywhere."""
    n, h, w = shape
    for kind, qp, searches in (("split8", 28, (2, 8, 16)), ("noise", 40, (8,)), ("still", 16, (8,)), ("pan2", 28, (8,))):
        y = torch.from_numpy(Q.make_planes(kind, n, h, w)[0]).cuda()
        for search in searches:
            for subpel in Q.SUBPELS:
                mv = torch.full((n, y.shape[1] // 16, y.shape[2] // 16, 4, 2), 77, dtype=torch.int16, device="cuda")
                sad = torch.full(tuple(mv.shape[:3]) + (5,), -1, dtype=torch.int32, device="cuda")
                hip.h264_motion_search_part(y, qp, n, search, subpel, mv, sad)
                want_mv, want_sad, _ = Q.searched(shape, kind, qp, search, subpel)
                assert np.array_equal(mv.cpu().numpy(), want_mv), (kind, search, subpel)
                assert np.array_equal(sad.cpu().numpy(), want_sad), (kind, search, subpel)
                mv2 = torch.zeros_like(mv)
                hip.h264_motion_search_part(y, qp, n, search, subpel, mv2)          # sad is optional
                assert torch.equal(mv, mv2)


def _random_part_info(rng, mbh, mbw):
    """h264_lf_ref.random_info with four vectors a macroblock: some macroblocks with four equal vectors, some with one zero partition."""
    info = L.random_info(rng, mbh, mbw)
    mv = rng.integers(-6, 7, (mbh, mbw, 4, 2))
    same = rng.random((mbh, mbw)) < 0.3
    mv[same] = mv[same][:, :1]
    mv[rng.random((mbh, mbw, 4)) < 0.3] = 0
    mv[info["intra"]] = 0
    info["mv"] = mv.astype(np.int64)
    info["mv4"] = np.repeat(np.repeat(mv.reshape(mbh, mbw, 2, 2, 2).transpose(0, 2, 1, 3, 4).reshape(2 * mbh, 2 * mbw, 2), 2, axis=0), 2, axis=1)
    return info


def test_the_filter_alone_with_stale_vectors_and_any_number_of_waves(hip):
    rng = np.random.default_rng(5)
    for mbh, mbw, qp, lo, hi in ((3, 5, 36, 100, 130), (6, 8, 40, 0, 256), (1, 5, 51, 60, 200), (5, 1, 33, 100, 112), (1, 1, 40, 0, 256), (3, 4, 15, 100, 104)):
        info = _random_part_info(rng, mbh, mbw)
        planes = L.random_planes(rng, mbh, mbw, lo, hi)
        want = [p.astype(np.int64).copy() for p in planes]
        Q.filter_picture(*want, qp, info)
        words = torch.from_numpy(Q.mbinfo_words([info])).cuda()
        stale = info["mv"].copy()
        stale[~info["mv"].any(axis=-1)] = 6                                         # under bits 18 .. 22 and in intra macroblocks: never read
        mv = torch.from_numpy(stale[None].astype(np.int16)).cuda()
        for waves in (1, 2, 16, 0):
            dev = [torch.from_numpy(p[None].astype(np.uint8)).cuda() for p in planes]
            hip.h264_deblock_part(*dev, qp, 1, 0, words, mv, waves)
            assert all(np.array_equal(d.cpu().numpy()[0], w_) for d, w_ in zip(dev, want)), (mbh, mbw, qp, waves)


def test_a_batch_of_gops_against_each_gop_coded_alone(hip):
    n, h, w, gop = 6, 36, 50, 3
    planes = Q.make_planes("split8", n, h, w)
    for qp, subpel, intra4, deblock in ((28, 4, 1, 1), (16, 0, 0, 0)):
        enc = _encoder(qp, gop, Q.SEARCH, subpel, intra4, deblock)
        whole, recon = enc.encode_planes(*(torch.from_numpy(p).cuda() for p in planes), first_index=Q.FIRST, return_recon=True)
        recon = [r.cpu().numpy() for r in recon]
        assert enc.last_sync == [0, 3]
        for g in range(0, n, gop):
            part, part_recon = enc.encode_planes(*(torch.from_numpy(p[g:g + gop]).cuda() for p in planes), first_index=Q.FIRST + g, return_recon=True)
            assert part == whole[g:g + gop] and all(np.array_equal(a.cpu().numpy(), b[g:g + gop]) for a, b in zip(part_recon, recon))
        want = Q.encode_planes(*planes, qp=qp, gop=gop, first_index=Q.FIRST, search=Q.SEARCH, subpel=subpel, intra4=intra4, deblock=deblock)
        _same(whole, recon, want[0], want[1:4])


def test_buffers_at_exactly_their_size(hip, monkeypatch):
    """Canary-guarded planes, vectors, words, scratch and out at exactly their sizes through the four entry points; one element less is
    refused before any launch."""
    guard, qp, gop, subpel = 64, 28, 3, 4
    shape = (3, 36, 50)
    planes, want, want_recon, used, infos, _ = Q.reference(shape, "split8", qp, subpel, (0, 1))
    n, mbh, mbw = 3, 3, 4
    y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
    need_s, need_o = hip.h264_gop_scratch_bytes(n, mbh, mbw), hip.h264_gop_out_bytes(n, mbh, mbw)
    canary = lambda size: torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    nmb = n * mbh * mbw
    big_s, big_o, big_i, big_v, big_d = canary(need_s), canary(need_o), canary(4 * nmb), canary(16 * nmb), canary(20 * nmb)
    big_r = [canary(p.size) for p in planes]
    recon = [b[guard:guard + p.size].view(p.shape) for b, p in zip(big_r, planes)]
    words = big_i[guard:guard + 4 * nmb].view(torch.int32).view(n, mbh, mbw)
    mv = big_v[guard:guard + 16 * nmb].view(torch.int16).view(n, mbh, mbw, 4, 2)
    sad = big_d[guard:guard + 20 * nmb].view(torch.int32).view(n, mbh, mbw, 5)
    scratch = big_s[guard:guard + need_s]
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
    short_mv = torch.zeros((n, mbh, mbw, 4, 1), dtype=torch.int16, device="cuda")
    for call in (lambda: hip.h264_motion_search_part(y, qp, gop, 8, subpel, short_mv),
                 lambda: hip.h264_motion_search_part(y, qp, gop, 8, subpel, mv, sad[..., :4].contiguous()),
                 lambda: hip.h264_motion_search_part(y, qp, gop, 7, subpel, mv), lambda: hip.h264_motion_search_part(y, qp, gop, 8, 3, mv),
                 lambda: hip.h264_encode_gop_step_part(y, cb, cr, qp, gop, 0, 8, subpel, 0, short_mv, *recon, scratch),
                 lambda: hip.h264_encode_gop_step_part(y, cb, cr, qp, gop, 0, 8, subpel, 0, mv, *recon, scratch[:-1]),
                 lambda: hip.h264_encode_gop_step_part_lf(y, cb, cr, qp, gop, 0, 8, subpel, 0, mv, *recon, scratch, words[:, :, :-1].contiguous()),
                 lambda: hip.h264_encode_gop_step_part(y, cb, cr, qp, gop, 0, 8, subpel, 0, mv, recon[0][:, :-16].contiguous(), recon[1], recon[2], scratch),
                 lambda: hip.h264_deblock_part(*recon, qp, gop, 0, words, short_mv), lambda: hip.h264_deblock_part(*recon, qp, gop, 0, words[:-1], mv)):
        with pytest.raises(hip.SdvHipError):
            call()
    assert launches == []
    hip.h264_motion_search_part(y, qp, gop, 8, subpel, mv, sad)
    for k in range(3):
        hip.h264_encode_gop_step_part_lf(y, cb, cr, qp, gop, k, 8, subpel, Q.FIRST, mv, *recon, scratch, words)
        hip.h264_deblock_part(*recon, qp, gop, k, words, mv, 1 + k)
    hip.h264_pack(scratch, n, mbh, hip.h264_gop_slot_mbw(mbw), big_o[guard:guard + need_o], offsets)
    torch.cuda.synchronize()
    assert launches == ["h264_motion_search_part"] + ["h264_encode_gop_step_part_lf", "h264_deblock_part"] * 3 + ["h264_pack"]
    monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
    for big, need in [(big_s, need_s), (big_o, need_o), (big_i, 4 * nmb), (big_v, 16 * nmb), (big_d, 20 * nmb)] + [(b, p.size) for b, p in zip(big_r, planes)]:
        host = big.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    offs = offsets.cpu().tolist()
    out = big_o.cpu().numpy()[guard:]
    assert [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == want
    assert all(np.array_equal(r.cpu().numpy(), w_) for r, w_ in zip(recon, want_recon))
    assert np.array_equal(words.cpu().numpy(), Q.mbinfo_words(infos))
    want_mv, want_sad, _ = Q.searched(shape, "split8", qp, 8, subpel)
    assert np.array_equal(mv.cpu().numpy(), want_mv) and np.array_equal(sad.cpu().numpy(), want_sad)


def test_part_0_and_part_omitted_give_the_parents_bytes_and_launches(hip, monkeypatch):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    dev = torch.device("cuda", 0)
    n, h, w = 3, 36, 50
    frames = torch.from_numpy(I.make_frames("glyphs", n, h, w)).cuda()
    for qp, (gop, search, subpel, intra4, deblock) in ((16, (1, 0, 0, 0, 0)), (28, (3, 8, 4, 1, 1)), (28, (3, 8, 0, 0, 0)), (28, (3, 0, 0, 0, 1)), (28, (1, 8, 4, 0, 0))):
        want = L.reference((n, h, w), "glyphs", qp, (gop, search, subpel, intra4), deblock=deblock)[1]
        traces = []
        for kw in ({}, dict(part=0)) + ((dict(part=1),) if gop == 1 or search == 0 else ()):   # part 1 without P pictures or a search: today's route
            launches = []
            monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
            got = H264Encoder(qp, dev, gop=gop, search=search, subpel=subpel, intra4=intra4, deblock=deblock, **kw).encode(frames, first_index=L.FIRST)
            monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
            assert got == want
            traces.append(launches)
        assert all(t == traces[0] for t in traces) and not any("part" in k for k in traces[0])
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
    H264Encoder(28, dev, gop=3, search=8, deblock=1, part=1).encode(frames, first_index=0)
    monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
    assert launches == ["h264_planes", "h264_motion_search_part", "h264_encode_gop_step_part_lf", "h264_deblock_part", "h264_encode_gop_step_part_lf",
                        "h264_deblock_part", "h264_encode_gop_step_part_lf", "h264_pack"]


def _check_file(path, frames, qp, gop, search, subpel, intra4, deblock, part=1):
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want = Q.encode_planes(*R.rgb_to_planes(frames), qp=qp, gop=gop, first_index=0, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part)
    assert samples == want[0]
    d = Q.decode_stream(samples, w, h)
    assert np.array_equal(d["y"], want[1]) and np.array_equal(d["cb"], want[2]) and np.array_equal(d["cr"], want[3])
    return d


def test_make_video_pyav_gives_the_same_file_whatever_the_upload_batch(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = Q.split_frames(8, 10, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)
    kw = dict(fps=5, codec="h264-cavlc", h264_qp=28, h264_gop=4, h264_search=8, h264_subpel=4, h264_deblock=1)
    a = video.make_video_pyav(t, output_filepath=tmp_path / "a.mp4", h264_part=1, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8, subpel 4) + deblock + part" and video.LAST_CODEC["part"] == 1
    assert _check_file(a, frames, 28, 4, 8, 4, 0, 1)["part"]["p8x8"] > 0
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 36 * 50 * 3)                     # one frame's worth: rounded up to one GOP per batch
    b = video.make_video_pyav(torch.from_numpy(frames), output_filepath=tmp_path / "b.mp4", h264_part=1, **kw)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 9 * 36 * 50 * 3)                 # nine frames' worth: rounded down to two GOPs
    c = video.make_video_pyav(t, output_filepath=tmp_path / "c.mp4", h264_part=1, **kw)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    d = video.make_video_pyav(t, output_filepath=tmp_path / "d.mp4", **kw)
    e = video.make_video_pyav(t, output_filepath=tmp_path / "e.mp4", h264_part=0, **kw)
    assert "part" not in video.LAST_CODEC and open(d, "rb").read() == open(e, "rb").read() != open(a, "rb").read()
    f = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "f.mp4", codec="h264-cavlc", h264_qp=28, h264_gop=4, h264_part=1)   # no search: no effect
    g = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "g.mp4", codec="h264-cavlc", h264_qp=28, h264_gop=4)
    assert "part" not in video.LAST_CODEC and open(f, "rb").read() == open(g, "rb").read()


def test_walk_partitions_on_request_and_writes_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    for var in ("SDV_VIDEO_CODEC", "SDV_H264_QP", "SDV_H264_GOP", "SDV_H264_SEARCH", "SDV_H264_SUBPEL", "SDV_H264_INTRA4", "SDV_H264_DEBLOCK", "SDV_H264_PART"):
        monkeypatch.delenv(var, raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=6, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.h264_part == 0
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    pipe.h264_part = 1                                                               # without the codec it changes nothing
    pipe.walk(name="q", **kw)
    assert (tmp_path / "q" / "q.mp4").read_bytes() == default
    pipe.video_codec, pipe.h264_gop, pipe.h264_qp, pipe.h264_search = "h264-cavlc", 4, 30, 8
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8) + part"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (6, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 30, 4, 8, 0, 0, 0)
    monkeypatch.setenv("SDV_H264_PART", "0")                                         # the variable wins
    pipe.walk(name="e", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4, search 8)" and "part" not in video.LAST_CODEC
    _check_file(tmp_path / "e" / "e.mp4", frames, 30, 4, 8, 0, 0, 0, part=0)


def test_third_party_decoder_agrees(hip, tmp_path, monkeypatch):
    """Where pyav exists: the mp4 with P_8x8 macroblocks decodes there to exactly the restatement's reconstruction."""
    av = pytest.importorskip("av", reason="pyav is not installed: the stream has met no third-party decoder here")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = Q.split_frames(6, 7, 64, 64)
    path = video.make_video_pyav(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", codec="h264-cavlc",
                                 h264_qp=28, h264_gop=3, h264_search=8, h264_subpel=4, h264_intra4=1, h264_deblock=1, h264_part=1)
    d = _check_file(path, frames, 28, 3, 8, 4, 1, 1)
    with av.open(str(path)) as container:
        decoded = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
    assert len(decoded) == 7
    for k, f in enumerate(decoded):
        assert np.array_equal(f[:64], d["y"][k]) and np.array_equal(f[64:80].reshape(32, 32), d["cb"][k]) and np.array_equal(f[80:].reshape(32, 32), d["cr"][k])
