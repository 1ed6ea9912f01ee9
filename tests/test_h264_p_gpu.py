"""The H.264 GOP path on the GPU (sdv_h264_encode_gops behind h264_cavlc.H264Encoder(gop=...)) against tests/h264_p_ref.py: samples and
reconstruction planes equal the restatement's byte for byte, and the GPU's bytes decode in its separately written decoder to the same
pictures.  All integer: every comparison is exact.  Shapes (n, H, W, gop) and kinds: h264_p_ref.SHAPES, the six temporal kinds plus
``flash_pcm``, qp 0 / 16 / 28 / 51."""
import functools

import numpy as np
import pytest
import torch

import h264_p_ref as P
import h264_ref as R

pytestmark = pytest.mark.gpu

KINDS = P.KINDS + P.EXTRA_KINDS
CASES = [(s, k, q) for s in P.SHAPES for k in KINDS for q in P.QPS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-gop{s[3]}-{k}-qp{q}" for s, k, q in CASES]
PLANE_KINDS = ("zeros_pcm", "flash_pcm")                                          # exist as planes only


@functools.lru_cache(maxsize=None)
def _encoder(qp, gop):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0), gop=gop)


def _gpu(shape, kind, qp, first_index=P.FIRST, gop=None, sl=slice(None)):
    """(samples, recon planes as numpy) of pictures ``sl`` of the case, coded in one call."""
    n, h, w, g = shape
    enc = _encoder(qp, g if gop is None else gop)
    if kind in PLANE_KINDS:
        samples, recon = enc.encode_planes(*(torch.from_numpy(p[sl]).cuda() for p in P.make_planes(kind, n, h, w)), first_index=first_index,
                                           return_recon=True)
    else:
        samples, recon = enc.encode(torch.from_numpy(P.make_frames(kind, n, h, w)[sl]).cuda(), first_index=first_index, return_recon=True)
    return samples, tuple(r.cpu().numpy() for r in recon)


@pytest.mark.parametrize("shape,kind,qp", CASES, ids=IDS)
def test_samples_and_reconstruction_equal_the_restatement_and_decode(hip, shape, kind, qp):
    n, h, w, gop = shape
    got, recon = _gpu(shape, kind, qp)
    _, want, want_recon, _ = P.reference(shape, kind, qp)
    assert len(got) == len(want) == n
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, len(a), len(b))
        assert a == b, (k, next(i for i in range(len(a)) if a[i] != b[i]))
    for a, b in zip(recon, want_recon):
        assert a.shape == b.shape and np.array_equal(a, b)
    d = P.decode_stream(got, w, h)                                                  # the GPU's own bytes
    assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon))
    assert d["sync"] == _encoder(qp, gop).last_sync == list(range(0, n, gop))


def test_gop_1_through_the_new_surface_is_todays_encoder(hip):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder, encoder_for
    for kind, qp in (("pan", 16), ("noise", 0), ("cut", 28)):
        frames = torch.from_numpy(P.make_frames(kind, 5, 36, 50)).cuda()
        want = H264Encoder(qp, torch.device("cuda", 0)).encode(frames, first_index=P.FIRST)
        enc = H264Encoder(qp, torch.device("cuda", 0), gop=1)
        assert enc.encode(frames, first_index=P.FIRST) == want and enc.last_sync == [0, 1, 2, 3, 4]
        assert encoder_for(qp, torch.device("cuda", 0), gop=1).encode(frames, first_index=P.FIRST) == want
        assert want == R.encode_frames(frames.cpu().numpy(), qp=qp, first_index=P.FIRST)[0]
        with pytest.raises(hip.SdvHipError, match="return_recon"):
            enc.encode(frames, return_recon=True)


def test_two_runs_give_the_same_bytes(hip):
    for kind, qp in (("noise", 16), ("fade", 0), ("pan", 28)):
        a, b = _gpu((7, 64, 64, 3), kind, qp), _gpu((7, 64, 64, 3), kind, qp)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_a_gop_codes_the_same_alone_and_inside_a_longer_call(hip):
    """Every call starts a new GOP and no reference crosses one: a call split at a multiple of gop, with first_index moved along (the
    parity of idr_pic_id), gives the same samples."""
    shape = (7, 64, 64, 3)
    for kind, qp in (("fade", 16), ("cut", 0), ("pan", 28)):
        whole, recon = _gpu(shape, kind, qp)
        for lo, hi in ((0, 3), (3, 6), (6, 7), (3, 7)):
            part, part_recon = _gpu(shape, kind, qp, first_index=P.FIRST + lo, sl=slice(lo, hi))
            assert part == whole[lo:hi] and all(np.array_equal(a, b[lo:hi]) for a, b in zip(part_recon, recon))
        assert _gpu(shape, kind, qp, first_index=P.FIRST, sl=slice(3, 6))[0] != whole[3:6]      # (the other parity is another stream)


def test_buffers_at_exactly_the_documented_capacity_and_one_byte_less(hip, monkeypatch):
    """Canary-guarded scratch, output and reconstruction planes at exactly the documented sizes, on the input that fills the slots most
    (every macroblock I_PCM, in IDR and P slices, hostile sample values): the guards stay intact and the samples are right; one byte
    less of scratch or output is refused before any launch."""
    shape, guard, qp, gop = (4, 32, 48), 64, 0, 2
    n, mbh, mbw = 4, 2, 3
    rng = np.random.default_rng(5)                                                  # every sample 0 .. 3 or 252 .. 255, independently
    hostile = lambda *sh: np.where(rng.random(sh) < 0.5, rng.integers(0, 4, sh), 252 + rng.integers(0, 4, sh)).astype(np.uint8)
    planes = (hostile(4, 32, 48), hostile(4, 16, 24), hostile(4, 16, 24))
    stats = P.new_stats()
    want, *want_recon = P.encode_planes(*planes, qp=qp, gop=gop, first_index=P.FIRST, stats=stats)
    assert stats["n_pcm"] == n * mbh * mbw
    y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
    need_s, need_o = hip.h264_gop_scratch_bytes(n, mbh, mbw), hip.h264_gop_out_bytes(n, mbh, mbw)
    assert need_o == n * mbh * P.slot_bytes(mbw)
    canary = lambda size: torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    big_s, big_o = canary(need_s), canary(need_o)
    big_r = [canary(p.size) for p in planes]
    recon = [b[guard:guard + p.size].view(p.shape) for b, p in zip(big_r, planes)]
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind, info, fn: (launches.append(kind), fn()))
    with pytest.raises(hip.SdvHipError, match="scratch holds"):
        hip.h264_encode_gops(y, cb, cr, qp, gop, P.FIRST, *recon, big_s[guard:guard + need_s - 1])
    with pytest.raises(hip.SdvHipError, match="capacity bound"):
        hip.h264_pack(big_s[guard:guard + need_s], n, mbh, hip.h264_gop_slot_mbw(mbw), big_o[guard:guard + need_o - 1], offsets)
    lib = hip.load()
    assert lib.sdv_h264_encode_gops(y.data_ptr(), cb.data_ptr(), cr.data_ptr(), n, mbh, mbw, qp, gop, P.FIRST, *(r.data_ptr() for r in recon),
                                    big_s.data_ptr() + guard, need_s - 1, None) == -1
    assert b"scratch buffer too small" in lib.sdv_last_error()
    assert launches == []
    hip.h264_encode_gops(y, cb, cr, qp, gop, P.FIRST, *recon, big_s[guard:guard + need_s])
    hip.h264_pack(big_s[guard:guard + need_s], n, mbh, hip.h264_gop_slot_mbw(mbw), big_o[guard:guard + need_o], offsets)
    torch.cuda.synchronize()
    assert launches == ["h264_encode_gops", "h264_pack"]
    for big, need in [(big_s, need_s), (big_o, need_o)] + [(b, p.size) for b, p in zip(big_r, planes)]:
        host = big.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    offs = offsets.cpu().tolist()
    out = big_o.cpu().numpy()[guard:]
    assert [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == want
    assert (out[offs[n]:need_o] == 0xA5).all()                                   # nothing written behind the last sample either
    assert all(np.array_equal(r.cpu().numpy(), w) for r, w in zip(recon, want_recon))


def _stss(path):
    data = open(path, "rb").read()
    ftyp = int.from_bytes(data[:4], "big")
    moov = ftyp + int.from_bytes(data[ftyp + 8:ftyp + 16], "big")
    at = data.find(b"stss", moov)
    if at < 0:
        return None
    count = int.from_bytes(data[at + 8:at + 12], "big")
    return [int.from_bytes(data[at + 12 + 4 * i:at + 16 + 4 * i], "big") - 1 for i in range(count)]


def _check_file(path, frames, qp, gop):
    """The mp4's samples are the restatement's, its stss box names the IDR pictures, and it decodes to the restatement's reconstruction."""
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want, ry, rcb, rcr = P.encode_planes(*R.rgb_to_planes(frames), qp=qp, gop=gop, first_index=0)
    assert samples == want
    assert _stss(path) == (list(range(0, n, gop)) if gop < n else None)
    d = P.decode_stream(samples, w, h)
    assert np.array_equal(d["y"], ry) and np.array_equal(d["cb"], rcb) and np.array_equal(d["cr"], rcr)
    return ry, rcb, rcr


def test_make_video_pyav_gives_the_same_file_whatever_the_upload_batch(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = P.make_frames("fade", 10, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)                          # (T, C, H, W) like the reference
    a = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "a.mp4", codec="h264-cavlc", h264_gop=3)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 3)"
    _check_file(a, frames, 16, 3)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 36 * 50 * 3)                     # one frame's worth: rounded up to one GOP per batch
    b = video.make_video_pyav(torch.from_numpy(frames), fps=5, output_filepath=tmp_path / "b.mp4", codec="h264-cavlc", h264_gop=3)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 7 * 36 * 50 * 3)                 # seven frames' worth: rounded down to two GOPs
    c = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "c.mp4", codec="h264-cavlc", h264_gop=3)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    d = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "d.mp4", codec="h264-cavlc", h264_gop=1)
    e = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "e.mp4", codec="h264-cavlc")
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra)" and open(d, "rb").read() == open(e, "rb").read() and _stss(e) is None


def test_walk_writes_p_pictures_on_request_and_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    for var in ("SDV_VIDEO_CODEC", "SDV_H264_QP", "SDV_H264_GOP"):
        monkeypatch.delenv(var, raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=6, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.video_codec is None and pipe.h264_gop == 1
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    again = video.make_video_pyav(tmp_path / "p", fps=3, output_filepath=tmp_path / "again.mp4", glob_pattern="**/*.png")
    assert open(again, "rb").read() == default and _stss(again) is None               # the default call, untouched by the new keywords
    pipe.h264_gop = 4                                                                 # without the codec it changes nothing
    pipe.walk(name="q", **kw)
    assert (tmp_path / "q" / "q.mp4").read_bytes() == default
    pipe.video_codec = "h264-cavlc"
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 4)"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (6, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 16, 4)
    monkeypatch.setenv("SDV_H264_GOP", "2")                                           # the variable wins
    pipe.walk(name="e", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 2)"
    _check_file(tmp_path / "e" / "e.mp4", frames, 16, 2)


def test_third_party_decoder_agrees(hip, tmp_path, monkeypatch):
    """Where pyav exists: the mp4 with P pictures decodes there to exactly the restatement's reconstruction."""
    av = pytest.importorskip("av", reason="pyav is not installed: the stream has met no third-party decoder here")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    for kind in ("fade", "pan", "cut"):
        frames = P.make_frames(kind, 7, 64, 64)
        path = video.make_video_pyav(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / f"{kind}.mp4",
                                     codec="h264-cavlc", h264_gop=3)
        ry, rcb, rcr = _check_file(path, frames, 16, 3)
        with av.open(str(path)) as container:
            decoded = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
        assert len(decoded) == 7
        for k, f in enumerate(decoded):
            assert np.array_equal(f[:64], ry[k]) and np.array_equal(f[64:80].reshape(32, 32), rcb[k]) and np.array_equal(f[80:].reshape(32, 32), rcr[k])
