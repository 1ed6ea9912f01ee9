"""The H.264 CAVLC intra encoder on the GPU (csrc/sdv_h264.hip behind h264_cavlc.H264Encoder) against tests/h264_ref.py: the samples
equal the restatement's byte for byte, and decode in its separately written decoder.  All integer: every comparison is exact.  Shapes:
one macroblock (no neighbour at all); left chains, two rows, two frames; crop plus edge pad; a plain batch; more rows than a trivial
grid.  Each crossed with the frame kinds and qp 0 / 10 / 16 / 28 / 51."""
import functools

import numpy as np
import pytest
import torch

import h264_ref as R

pytestmark = pytest.mark.gpu

SHAPES = ((1, 16, 16), (2, 32, 48), (1, 36, 50), (3, 64, 64), (1, 96, 128))
QPS = (0, 10, 16, 28, 51)
CASES = [(s, k, q) for s in SHAPES for k in R.KINDS for q in QPS]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}-qp{q}" for s, k, q in CASES]
FIRST = 3


@functools.lru_cache(maxsize=None)
def _encoder(qp):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0))


def _gpu_samples(shape, kind, qp, first_index=FIRST):
    if kind == "zeros_pcm":                                                     # planes only: no RGB input maps to sample values 0 .. 3
        return _encoder(qp).encode_planes(*(torch.from_numpy(p).cuda() for p in R.make_planes(kind, *shape)), first_index=first_index)
    return _encoder(qp).encode(torch.from_numpy(R.make_frames(kind, *shape)).cuda(), first_index=first_index)


@functools.lru_cache(maxsize=None)
def _reference(shape, kind, qp):
    return R.encode_planes(*R.make_planes(kind, *shape), qp=qp, first_index=FIRST)


@pytest.mark.parametrize("shape,kind,qp", CASES, ids=IDS)
def test_samples_equal_the_restatement_byte_for_byte(hip, shape, kind, qp):
    got = _gpu_samples(shape, kind, qp)
    want = _reference(shape, kind, qp)[0]
    assert len(got) == len(want) == shape[0]
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, len(a), len(b))
        assert a == b, (k, next(i for i in range(len(a)) if a[i] != b[i]))


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in SHAPES])
def test_planes_kernel_equals_the_integer_rule(hip, shape):
    for kind in ("flat", "ramp", "glyphs", "noise"):
        frames = R.make_frames(kind, *shape)
        y, cb, cr = hip.h264_planes(torch.from_numpy(frames).cuda())
        for got, want in zip((y, cb, cr), R.rgb_to_planes(frames)):
            assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), kind


def test_two_runs_give_the_same_bytes(hip):
    for kind, qp in (("noise", 10), ("glyphs", 0), ("ramp", 28)):
        assert _gpu_samples((3, 64, 64), kind, qp) == _gpu_samples((3, 64, 64), kind, qp)


def test_a_frame_codes_the_same_alone_and_inside_a_batch(hip):
    """idr_pic_id is the only thing a picture takes from its place in the batch: first_index holds it fixed."""
    for kind, qp in (("noise", 16), ("glyphs", 10)):
        frames = torch.from_numpy(R.make_frames(kind, 3, 64, 64)).cuda()
        batch = _encoder(qp).encode(frames, first_index=FIRST)
        for k in range(3):
            assert _encoder(qp).encode(frames[k:k + 1], first_index=FIRST + k) == [batch[k]]
        assert _encoder(qp).encode(frames[1:2], first_index=FIRST) != [batch[1]]          # (the other parity is another stream)


def test_buffers_at_exactly_the_documented_capacity_and_one_byte_less(hip, monkeypatch):
    """Canary-guarded scratch and output at exactly h264_scratch_bytes / h264_out_bytes, on the input that fills the slots most (every
    macroblock I_PCM, hostile sample values): the guards stay intact and the samples are right; one byte less of either is refused
    before any launch."""
    shape, guard = (2, 32, 48), 64
    n, mbh, mbw = 2, 2, 3
    y, cb, cr = (torch.from_numpy(p).cuda() for p in R.make_planes("zeros_pcm", *shape))
    need_s, need_o = hip.h264_scratch_bytes(n, mbh, mbw), hip.h264_out_bytes(n, mbh, mbw)
    assert need_o == n * mbh * R.slot_bytes(mbw)
    big_s = torch.full((guard + need_s + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    big_o = torch.full((guard + need_o + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind, info, fn: (launches.append(kind), fn()))
    with pytest.raises(hip.SdvHipError, match="scratch holds"):
        hip.h264_encode_rows(y, cb, cr, 0, FIRST, big_s[guard:guard + need_s - 1])
    with pytest.raises(hip.SdvHipError, match="capacity bound"):
        hip.h264_pack(big_s[guard:guard + need_s], n, mbh, mbw, big_o[guard:guard + need_o - 1], offsets)
    lib = hip.load()
    assert lib.sdv_h264_pack(big_s.data_ptr() + guard, need_s, n, mbh, mbw, big_o.data_ptr() + guard, need_o - 1, offsets.data_ptr(), None) == -1
    assert b"output capacity" in lib.sdv_last_error()
    assert launches == []
    hip.h264_encode_rows(y, cb, cr, 0, FIRST, big_s[guard:guard + need_s])
    hip.h264_pack(big_s[guard:guard + need_s], n, mbh, mbw, big_o[guard:guard + need_o], offsets)
    torch.cuda.synchronize()
    assert launches == ["h264_encode_rows", "h264_pack"]
    for big, need in ((big_s, need_s), (big_o, need_o)):
        host = big.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    offs = offsets.cpu().tolist()
    out = big_o.cpu().numpy()[guard:]
    want = _reference(shape, "zeros_pcm", 0)[0]
    assert [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == want
    assert (out[offs[n]:need_o] == 0xA5).all()                                   # nothing written behind the last sample either


def _check_file(path, frames, qp):
    """The mp4's samples are the restatement's and decode to its reconstruction."""
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want, ry, rcb, rcr = R.encode_frames(frames, qp=qp, first_index=0)
    assert samples == want
    for k, s in enumerate(samples):
        d = R.decode_sample(s, w, h)
        assert np.array_equal(d["y"], ry[k, :h, :w]) and np.array_equal(d["cb"], rcb[k, :h // 2, :w // 2])
        assert np.array_equal(d["cr"], rcr[k, :h // 2, :w // 2])


def test_make_video_pyav_writes_an_avc1_file_of_cavlc_samples(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = R.make_frames("ramp", 3, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)                          # (T, C, H, W) like the reference
    out = video.make_video_pyav(t, fps=5, output_filepath=tmp_path / "g.mp4", codec="h264-cavlc")
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra)" and video.LAST_CODEC["why"] == "codec argument"
    _check_file(out, frames, 16)
    monkeypatch.setenv("SDV_VIDEO_CODEC", "h264-cavlc")                              # the variable, a CPU tensor (uploaded), another qp
    out = video.make_video_pyav(torch.from_numpy(frames), fps=5, output_filepath=tmp_path / "c.mp4", h264_qp=28)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra)" and video.LAST_CODEC["why"] == "SDV_VIDEO_CODEC"
    _check_file(out, frames, 28)


def test_walk_writes_the_cavlc_track_on_request_and_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    monkeypatch.delenv("SDV_H264_QP", raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=3, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.video_codec is None
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    again = video.make_video_pyav(tmp_path / "p", fps=3, output_filepath=tmp_path / "again.mp4", glob_pattern="**/*.png")
    assert open(again, "rb").read() == default                                        # the default call, untouched by the new keywords
    pipe.video_codec = "h264-cavlc"
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC intra)"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (3, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 16)
