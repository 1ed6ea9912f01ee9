"""Several slices per macroblock row on the GPU (the four entry points of include/sdv_hip_h264_seg.h behind
h264_cavlc.H264Encoder(row_slices=S)) against tests/h264_seg_ref.py: samples, reconstruction planes and side information equal the
restatement's exactly, and the GPU's own bytes decode in that module's decoder - neighbour availability from slice membership - to the GPU's
reconstruction.  All integer: every comparison is exact.  Small shapes only."""
import functools

import numpy as np
import pytest
import torch

import h264_i4_ref as I
import h264_lf_ref as L
import h264_part_ref as PT
import h264_ref as R
import h264_seg_ref as G

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _encoder(qp, gop, search, subpel, intra4, deblock, part, row_slices):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    return H264Encoder(qp, torch.device("cuda", 0), gop=gop, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part, row_slices=row_slices)


def _same(got, recon, want, want_recon):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), (k, len(a), len(b))
        assert a == b, (k, next(i for i in range(len(a)) if a[i] != b[i]))
    for a, b in zip(recon, want_recon):
        assert a.shape == b.shape and np.array_equal(a, b)


def _steps(hip, planes, mv, qp, gop, search, subpel, intra4, deblock, segs, first_index=G.FIRST, seg=True):
    """The route of H264Encoder(row_slices=S) with given vectors -> (samples, recon, words or None).  ``seg`` False: the same positions
    through the entry points without ``segs`` (sdv_hip_h264_part.h / sdv_hip_h264_i4.h / sdv_hip_h264_lf.h), for the comparison at segs 1."""
    y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
    n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
    recon = [torch.empty_like(t) for t in (y, cb, cr)]
    scratch = torch.empty((hip.h264_seg_scratch_bytes(n, mbh, mbw, segs),), dtype=torch.uint8, device="cuda")
    out = torch.empty((hip.h264_seg_out_bytes(n, mbh, mbw, segs),), dtype=torch.uint8, device="cuda")
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    words = torch.zeros((n, mbh, mbw), dtype=torch.int32, device="cuda") if deblock else None
    mvt = torch.from_numpy(np.ascontiguousarray(mv)).cuda()
    tail = (segs,) if seg else ()
    step, step_lf = (hip.h264_encode_gop_step_seg, hip.h264_encode_gop_step_seg_lf) if seg else (hip.h264_encode_gop_step_part, hip.h264_encode_gop_step_part_lf)
    idr, idr_lf = (hip.h264_encode_idr4_seg, hip.h264_encode_idr4_seg_lf) if seg else (hip.h264_encode_idr4, hip.h264_encode_idr4_lf)
    for k in range(min(gop, n)):
        if k == 0 and intra4 and deblock:
            idr_lf(y, cb, cr, qp, gop, first_index, *recon, scratch, words, *tail)
        elif k == 0 and intra4:
            idr(y, cb, cr, qp, gop, first_index, *recon, scratch, *tail)
        elif deblock:
            step_lf(y, cb, cr, qp, gop, k, search, subpel, first_index, mvt, *recon, scratch, words, *tail)
        else:
            step(y, cb, cr, qp, gop, k, search, subpel, first_index, mvt, *recon, scratch, *tail)
        if deblock:
            hip.h264_deblock_part(*recon, qp, gop, k, words, mvt)
    hip.h264_pack(scratch, n, mbh * segs, hip.h264_seg_slot_mbw(mbw, segs), out, offsets)
    torch.cuda.synchronize()
    offs, host = offsets.cpu().tolist(), out.cpu().numpy()
    return [host[offs[k]:offs[k + 1]].tobytes() for k in range(n)], tuple(r.cpu().numpy() for r in recon), None if words is None else words.cpu().numpy()


@pytest.mark.parametrize("shape,kind,setting,qp,row_slices,injected", G.CASES, ids=G.IDS)
def test_samples_reconstruction_and_mbinfo_equal_the_restatement_and_decode(hip, shape, kind, setting, qp, row_slices, injected):
    """Every CPU round-trip case.  Searched kinds go through H264Encoder (the search launch and the expansion to four vectors included);
    injected kinds - off-grid, out-of-range and not admitted vectors among them - through the seg entry points with those vectors."""
    n, h, w = shape
    _, gop, search, subpel, intra4, deblock, part = setting
    planes, want, want_recon, used, infos, segs, _ = G.reference(shape, kind, qp, setting, row_slices, injected)
    if injected is None:
        enc = _encoder(qp, gop, search, subpel, intra4, deblock, part, row_slices)
        got, recon = enc.encode_planes(*(torch.from_numpy(p).cuda() for p in planes), first_index=G.FIRST, return_recon=True)
        recon = tuple(r.cpu().numpy() for r in recon)
        assert enc.last_sync == list(range(0, n, gop))
        ws = next(w_ for key, w_ in enc._ws.items() if key[:3] == (n, planes[0].shape[1] // 16, planes[0].shape[2] // 16))
        assert ws.get("segs", 1) == segs
        words = ws["mbinfo"].cpu().numpy() if deblock and segs > 1 else None
    else:
        mv = G.injected_case(shape, injected, search, subpel)[1]
        got, recon, words = _steps(hip, planes, mv, qp, gop, search, subpel, intra4, deblock, segs)
    _same(got, recon, want, want_recon)
    if words is not None:
        assert np.array_equal(words, PT.mbinfo_words(infos)), (qp, setting)
    d = G.decode_stream(got, w, h)                                              # the GPU's own bytes
    assert all(np.array_equal(d[key], r) for key, r in zip(("y", "cb", "cr"), recon)), (qp, setting)
    assert d["seg"]["slices"] == n * (planes[0].shape[1] // 16) * segs


def test_segs_1_gives_the_part_and_idr4_entry_points_bytes_and_planes(hip):
    for shape, kind, setting, qp, injected in (((4, 32, 48), "planted", G.SETTINGS[4], 28, "mixed"), ((5, 40, 72), "split8", G.SETTINGS[2], 16, None),
                                               ((3, 48, 128), "noise", G.SETTINGS[5], 0, None), ((3, 16, 16), "pan2", G.SETTINGS[3], 51, None),
                                               ((4, 32, 48), "planted", G.SETTINGS[4], 0, "invalid")):
        _, gop, search, subpel, intra4, deblock, part = setting
        planes, _, _, used, _, _, _ = G.reference(shape, kind, qp, setting, 1, injected)
        mv = used if injected is None else G.injected_case(shape, injected, search, subpel)[1]
        a = _steps(hip, planes, mv, qp, gop, search or 2, subpel if search else 0, intra4, deblock, 1, seg=True)
        b = _steps(hip, planes, mv, qp, gop, search or 2, subpel if search else 0, intra4, deblock, 1, seg=False)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])), (shape, kind, setting)
        assert (a[2] is None and b[2] is None) or np.array_equal(a[2], b[2])


def test_row_slices_1_and_omitted_give_the_parents_launches_and_bytes(hip, monkeypatch):
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    dev = torch.device("cuda", 0)
    n, h, w = 3, 36, 50
    frames = torch.from_numpy(I.make_frames("glyphs", n, h, w)).cuda()
    parent = {(1, 0, 0, 0, 0, 0): ["h264_planes", "h264_encode_rows", "h264_pack"],
              (3, 0, 0, 0, 0, 0): ["h264_planes", "h264_encode_gops", "h264_pack"],
              (3, 8, 0, 0, 0, 0): ["h264_planes", "h264_motion_search"] + ["h264_encode_gop_step"] * 3 + ["h264_pack"],
              (3, 8, 4, 1, 1, 1): ["h264_planes", "h264_motion_search_part", "h264_encode_idr4_lf", "h264_deblock_part", "h264_encode_gop_step_part_lf",
                                   "h264_deblock_part", "h264_encode_gop_step_part_lf", "h264_pack"]}
    for (gop, search, subpel, intra4, deblock, part), trace in parent.items():
        want = PT.encode_planes(*R.rgb_to_planes(frames.cpu().numpy()), qp=28, gop=gop, first_index=L.FIRST, search=search, subpel=subpel, intra4=intra4,
                                deblock=deblock, part=part)[0]
        for kw in ({}, dict(row_slices=1)):
            launches = []
            monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
            got = H264Encoder(28, dev, gop=gop, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part, **kw).encode(frames, first_index=L.FIRST)
            monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
            assert got == want and launches == trace and not any("seg" in k for k in launches), (gop, search, kw, launches)
    one = torch.from_numpy(I.make_frames("glyphs", 2, 64, 16)).cuda()                # one macroblock wide: segs 1 whatever S
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
    a = H264Encoder(28, dev, row_slices=8).encode(one)
    monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
    assert launches == parent[(1, 0, 0, 0, 0, 0)] and a == H264Encoder(28, dev).encode(one)
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
    H264Encoder(28, dev, gop=3, search=8, deblock=1, row_slices=2).encode(frames, first_index=0)
    H264Encoder(28, dev, gop=1, intra4=1, row_slices=2).encode(frames, first_index=0)
    monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
    assert launches == ["h264_planes", "h264_motion_search", "h264_encode_gop_step_seg_lf", "h264_deblock_part", "h264_encode_gop_step_seg_lf",
                        "h264_deblock_part", "h264_encode_gop_step_seg_lf", "h264_pack", "h264_planes", "h264_encode_idr4_seg", "h264_pack"]


def test_determinism_and_a_gop_alone_against_the_same_gop_in_a_longer_call(hip):
    n, h, w, gop = 6, 40, 72, 3
    planes = PT.make_planes("split8", n, h, w)
    for qp, search, subpel, intra4, deblock, part, s in ((28, 8, 4, 1, 1, 1, 2), (16, 8, 0, 0, 0, 0, 4), (28, 0, 0, 0, 1, 0, 3)):
        enc = _encoder(qp, gop, search, subpel, intra4, deblock, part, s)
        dev = [torch.from_numpy(p).cuda() for p in planes]
        whole, recon = enc.encode_planes(*dev, first_index=G.FIRST, return_recon=True)
        recon = [r.cpu().numpy() for r in recon]
        again, recon2 = enc.encode_planes(*dev, first_index=G.FIRST, return_recon=True)
        assert again == whole and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(recon2, recon))
        assert enc.last_sync == [0, 3]
        for g in range(0, n, gop):
            part_, part_recon = enc.encode_planes(*(torch.from_numpy(p[g:g + gop]).cuda() for p in planes), first_index=G.FIRST + g, return_recon=True)
            assert part_ == whole[g:g + gop] and all(np.array_equal(a.cpu().numpy(), b[g:g + gop]) for a, b in zip(part_recon, recon))
        want = G.encode_planes(*planes, qp=qp, gop=gop, first_index=G.FIRST, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part, row_slices=s)
        _same(whole, recon, want[0], want[1:4])


def test_buffers_at_exactly_their_size_on_an_all_pcm_input(hip, monkeypatch):
    """Canary-guarded scratch, out, reconstruction, mv and mbinfo at exactly their sizes on an input (noise at qp 0) whose every macroblock is I_PCM (the
    longest slices there are); one byte less of scratch is refused before any launch."""
    guard, qp, gop = 64, 0, 3
    shape, setting, s = (3, 48, 128), ("pcm", 3, 8, 4, 1, 1, 1), 3
    planes, want, want_recon, used, infos, segs, _ = G.reference(shape, "noise", qp, setting, s)
    n, mbh, mbw = 3, 3, 8
    assert segs == 3 and all(info["pcm"].all() for info in infos)
    y, cb, cr = (torch.from_numpy(p).cuda() for p in planes)
    need_s, need_o = hip.h264_seg_scratch_bytes(n, mbh, mbw, segs), hip.h264_seg_out_bytes(n, mbh, mbw, segs)
    canary = lambda size: torch.full((guard + size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    nmb = n * mbh * mbw
    big_s, big_o, big_i, big_v = canary(need_s), canary(need_o), canary(4 * nmb), canary(16 * nmb)
    big_r = [canary(p.size) for p in planes]
    recon = [b[guard:guard + p.size].view(p.shape) for b, p in zip(big_r, planes)]
    words = big_i[guard:guard + 4 * nmb].view(torch.int32).view(n, mbh, mbw)
    mv = big_v[guard:guard + 16 * nmb].view(torch.int16).view(n, mbh, mbw, 4, 2)
    scratch = big_s[guard:guard + need_s]
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda")
    launches = []
    monkeypatch.setattr(hip, "LAUNCH_HOOK", lambda kind_, info, fn: (launches.append(kind_), fn()))
    hip.h264_motion_search_part(y, qp, gop, 8, 4, mv)
    torch.cuda.synchronize()
    launches.clear()
    for call in (lambda: hip.h264_encode_gop_step_seg(y, cb, cr, qp, gop, 1, 8, 4, 0, mv, *recon, scratch[:-1], segs),
                 lambda: hip.h264_encode_gop_step_seg_lf(y, cb, cr, qp, gop, 1, 8, 4, 0, mv, *recon, scratch[:-1], words, segs),
                 lambda: hip.h264_encode_idr4_seg(y, cb, cr, qp, gop, 0, *recon, scratch[:-1], segs),
                 lambda: hip.h264_encode_idr4_seg_lf(y, cb, cr, qp, gop, 0, *recon, scratch[:-1], words, segs),
                 lambda: hip.h264_encode_idr4_seg(y, cb, cr, qp, gop, 0, *recon, scratch, 9),
                 lambda: hip.h264_encode_gop_step_seg(y, cb, cr, qp, gop, 1, 8, 4, 0, mv, *recon, scratch, 0),
                 lambda: hip.h264_encode_gop_step_seg_lf(y, cb, cr, qp, gop, 1, 8, 4, 0, mv, *recon, scratch, words[:, :, :-1].contiguous(), segs),
                 lambda: hip.h264_pack(scratch[:-1], n, mbh * segs, hip.h264_seg_slot_mbw(mbw, segs), big_o[guard:guard + need_o], offsets)):
        with pytest.raises(hip.SdvHipError):
            call()
    assert launches == []
    lib = hip.load()                                                               # and the library itself, below the binding's own check
    args = [t.data_ptr() for t in (y, cb, cr)] + [n, mbh, mbw, qp, gop, 0] + [t.data_ptr() for t in recon] + [scratch.data_ptr(), need_s - 1]
    assert lib.sdv_h264_encode_idr4_seg(*args, segs, None) == -1 and b"scratch buffer too small" in lib.sdv_last_error()
    hip.h264_encode_idr4_seg_lf(y, cb, cr, qp, gop, G.FIRST, *recon, scratch, words, segs)
    hip.h264_deblock_part(*recon, qp, gop, 0, words, mv)
    for k in (1, 2):
        hip.h264_encode_gop_step_seg_lf(y, cb, cr, qp, gop, k, 8, 4, G.FIRST, mv, *recon, scratch, words, segs)
        hip.h264_deblock_part(*recon, qp, gop, k, words, mv)
    hip.h264_pack(scratch, n, mbh * segs, hip.h264_seg_slot_mbw(mbw, segs), big_o[guard:guard + need_o], offsets)
    torch.cuda.synchronize()
    assert launches == ["h264_encode_idr4_seg_lf", "h264_deblock_part"] + ["h264_encode_gop_step_seg_lf", "h264_deblock_part"] * 2 + ["h264_pack"]
    monkeypatch.setattr(hip, "LAUNCH_HOOK", None)
    for big, need in [(big_s, need_s), (big_o, need_o), (big_i, 4 * nmb), (big_v, 16 * nmb)] + [(b, p.size) for b, p in zip(big_r, planes)]:
        host = big.cpu().numpy()
        assert (host[:guard] == 0xA5).all() and (host[guard + need:] == 0xA5).all()
    offs = offsets.cpu().tolist()
    out = big_o.cpu().numpy()[guard:]
    assert [out[offs[k]:offs[k + 1]].tobytes() for k in range(n)] == want
    assert all(np.array_equal(r.cpu().numpy(), w_) for r, w_ in zip(recon, want_recon))
    assert np.array_equal(words.cpu().numpy(), PT.mbinfo_words(infos))
    # the same input without the filter and without Intra4x4: the k = 0 step codes the IDR pictures
    got, rec, _ = _steps(hip, planes, mv.cpu().numpy(), qp, gop, 8, 4, 0, 0, segs)
    ref = G.encode_planes(*planes, qp=qp, gop=gop, first_index=G.FIRST, search=8, subpel=4, part=1, row_slices=s, mv=mv.cpu().numpy())
    _same(got, rec, ref[0], ref[1:4])


def _check_file(path, frames, qp, gop, row_slices, search=0, subpel=0, intra4=0, deblock=0, part=0):
    n, h, w, _ = frames.shape
    width, height, entry, samples = R.mp4_samples(path)
    assert (width, height, entry) == (w, h, b"avc1") and len(samples) == n
    want = G.encode_planes(*R.rgb_to_planes(frames), qp=qp, gop=gop, first_index=0, search=search, subpel=subpel, intra4=intra4, deblock=deblock, part=part,
                           row_slices=row_slices)
    assert samples == want[0]
    d = G.decode_stream(samples, w, h)
    assert np.array_equal(d["y"], want[1]) and np.array_equal(d["cb"], want[2]) and np.array_equal(d["cr"], want[3])
    assert d["seg"]["slices"] == n * ((h + 15) // 16) * want[6]
    return d


def test_make_video_pyav_decodes_to_the_restatement_whatever_the_upload_batch(hip, tmp_path, monkeypatch):
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = PT.split_frames(8, 10, 36, 50)
    t = torch.from_numpy(frames).cuda().permute(0, 3, 1, 2)
    kw = dict(fps=5, codec="h264-cavlc", h264_qp=28, h264_gop=3)
    a = video.make_video_pyav(t, output_filepath=tmp_path / "a.mp4", h264_row_slices=2, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 3) + 2 row slices" and video.LAST_CODEC["row_slices"] == 2
    _check_file(a, frames, 28, 3, 2)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 36 * 50 * 3)                     # one frame's worth: rounded up to one GOP per batch
    b = video.make_video_pyav(torch.from_numpy(frames), output_filepath=tmp_path / "b.mp4", h264_row_slices=2, **kw)
    monkeypatch.setattr(video, "H264_BATCH_BYTES", 7 * 36 * 50 * 3)                 # seven frames' worth: rounded down to two GOPs
    c = video.make_video_pyav(t, output_filepath=tmp_path / "c.mp4", h264_row_slices=2, **kw)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    d = video.make_video_pyav(t, output_filepath=tmp_path / "d.mp4", **kw)
    e = video.make_video_pyav(t, output_filepath=tmp_path / "e.mp4", h264_row_slices=1, **kw)
    assert "row_slices" not in video.LAST_CODEC and open(d, "rb").read() == open(e, "rb").read() != open(a, "rb").read()
    f = video.make_video_pyav(t, output_filepath=tmp_path / "f.mp4", h264_row_slices=4, h264_search=8, h264_subpel=4, h264_intra4=1, h264_deblock=1, h264_part=1, **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 3, search 8, subpel 4) + intra4 + deblock + part + 4 row slices"
    assert _check_file(f, frames, 28, 3, 4, 8, 4, 1, 1, 1)["seg"]["boundary_edges"] > 0


def test_walk_cuts_rows_on_request_and_writes_the_same_bytes_by_default(hip, dev, tmp_path, monkeypatch):
    from PIL import Image
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline, video
    for var in ("SDV_VIDEO_CODEC", "SDV_H264_QP", "SDV_H264_GOP", "SDV_H264_SEARCH", "SDV_H264_SUBPEL", "SDV_H264_INTRA4", "SDV_H264_DEBLOCK", "SDV_H264_PART",
                "SDV_H264_ROW_SLICES"):
        monkeypatch.delenv(var, raising=False)
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    kw = dict(prompts=["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=6, batch_size=2, output_dir=str(tmp_path), fps=3,
              num_inference_steps=2, height=64, width=64)
    assert pipe.h264_row_slices == 1
    pipe.walk(name="p", **kw)
    assert video.LAST_CODEC["video"] == "h264 (I_PCM)"
    default = (tmp_path / "p" / "p.mp4").read_bytes()
    pipe.h264_row_slices = 2                                                         # without the codec it changes nothing
    pipe.walk(name="q", **kw)
    assert (tmp_path / "q" / "q.mp4").read_bytes() == default
    pipe.video_codec, pipe.h264_gop, pipe.h264_qp = "h264-cavlc", 3, 30
    pipe.walk(name="g", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 3) + 2 row slices"
    files = sorted((tmp_path / "g").glob("**/*.png"))
    frames = np.stack([np.asarray(Image.open(f).convert("RGB")) for f in files])
    assert frames.shape == (6, 64, 64, 3)
    _check_file(tmp_path / "g" / "g.mp4", frames, 30, 3, 2)
    monkeypatch.setenv("SDV_H264_ROW_SLICES", "1")                                   # the variable wins
    pipe.walk(name="e", **kw)
    assert video.LAST_CODEC["video"] == "h264 (CAVLC, gop 3)" and "row_slices" not in video.LAST_CODEC
    _check_file(tmp_path / "e" / "e.mp4", frames, 30, 3, 1)


def test_third_party_decoder_agrees(hip, tmp_path, monkeypatch):
    """Where pyav exists: the mp4 with several slices a row decodes there to exactly the restatement's reconstruction."""
    av = pytest.importorskip("av", reason="pyav is not installed: the stream has met no third-party decoder here")
    from stable_diffusion_videos_amd import video
    monkeypatch.delenv("SDV_VIDEO_CODEC", raising=False)
    frames = PT.split_frames(6, 7, 64, 64)
    path = video.make_video_pyav(torch.from_numpy(frames).cuda().permute(0, 3, 1, 2), fps=5, output_filepath=tmp_path / "s.mp4", codec="h264-cavlc",
                                 h264_qp=28, h264_gop=3, h264_search=8, h264_subpel=4, h264_intra4=1, h264_deblock=1, h264_part=1, h264_row_slices=3)
    d = _check_file(path, frames, 28, 3, 3, 8, 4, 1, 1, 1)
    with av.open(str(path)) as container:
        decoded = [f.to_ndarray(format="yuv420p") for f in container.decode(video=0)]
    assert len(decoded) == 7
    for k, f in enumerate(decoded):
        assert np.array_equal(f[:64], d["y"][k]) and np.array_equal(f[64:80].reshape(32, 32), d["cb"][k]) and np.array_equal(f[80:].reshape(32, 32), d["cr"][k])
