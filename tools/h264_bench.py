"""GPU H.264 CAVLC intra encoder (h264_cavlc.H264Encoder) against the two video tracks it can stand in for, on the same box.

    python tools/h264_bench.py [--out FILE] [--reps 5] [--gop N [--search R[,R...] [--subpel S[,S...]]]]
    python tools/h264_bench.py [--out FILE] [--reps 5] --gop N[,N...] --search R[,R...] --intra4 0,1
    python tools/h264_bench.py [--out FILE] [--reps 5] --gop N --search R[,R...] --qp Q[,Q...] --deblock 0,1
    python tools/h264_bench.py [--out FILE] [--reps 5] --gop N --search R --subpel S[,S...] --deblock D[,D...] --qp Q[,Q...] --part 0,1
    python tools/h264_bench.py [--out FILE] [--reps 5] --gop N --search R[,R...] --subpel S[,S...] --deblock D[,D...] --part P[,P...] --qp Q[,Q...] --row-slices 1,2,4,8

Cases: 128 frames of 512 x 512 and 8 frames of 2048 x 2048, each with two contents: what the tiny pipeline decodes (seeded synthetic
weights; the 2048 x 2048 frames are its 512 x 512 frames through the x4 upsampler, as ``walk(upsample=True)`` makes them) and uniform
noise (the worst case).  Per case:
  * frames/s of encode() at qp 16 on frames already in HBM - HIP events and the host clock around the call, copies back included
    (encode() ends in a synchronise) - and of its three entry points alone;
  * frames/s of the host ``I_PCM`` writer (h264.idr_picture, one thread, as video.write_h264_mp4 runs it) after the raw copy it needs,
    and of the Motion-JPEG branch on the GPU (jpeg encoder, quality 95);
  * bytes per frame at qp 10 / 16 / 22 against I_PCM and Motion-JPEG q95;
  * at 512 x 512, Y-PSNR of the reconstruction at qp 10 / 16 / 22: the first frame's sample decoded by the decoder of
    tests/h264_ref.py against the integer-rule Y' of the source.
With ``--gop N`` (N > 1) the tool measures the GOP path instead (P pictures, h264_cavlc.H264Encoder(gop=N)): per frame set one row for
gop 1 - the all-intra code, the comparison - and one for gop N, side by side: encode() ms and frames/s with warm workspaces, bytes per
frame, and Y-PSNR of the reconstruction of all frames (the planes sdv_h264_encode_gops leaves in HBM; at gop 1 that entry point writes
the intra stream's bytes).  Frame sets: the tiny pipeline's frames, and the temporal kinds ``fade`` (lerp between two glyph frames) and
``pan`` (a glyph frame shifted by k pixels in picture k) of tests/h264_p_ref.py, at 128 x 512 x 512 and 8 x 2048 x 2048.
With ``--gop N --search R[,R...]`` (each R even, 0 .. 16) the tool measures motion search on top of the GOP path
(h264_cavlc.H264Encoder(gop=N, search=R)): per frame set one row per R, in the order given - R = 0 is the GOP path without search, the
comparison of the same run: encode() ms and frames/s, bytes per frame, Y-PSNR of the reconstruction of all frames, and for R > 0 the
search kernel alone and its share of encode().  Frame sets as with ``--gop`` plus ``pan2``, the glyph frame shifted by 2 k pixels in
picture k (``pan`` moves one sample a picture, which no even vector matches).
With ``--gop N --search R --subpel S[,S...]`` (one R > 0; each S one of 0, 1, 2, 4) the tool measures the vector grid on top of the search
(h264_cavlc.H264Encoder(gop=N, search=R, subpel=S)): per frame set one row per S, in the order given - S = 0 is the even whole-sample
search, the comparison of the same run: the columns above, the search kernel alone (sdv_h264_motion_search for S = 0,
sdv_h264_motion_search_sub otherwise) and the share of vectors with a fractional component.  Frame sets as with ``--search`` plus
``glide``, the analytic texture of tests/h264_sub_ref.py that moves by a quarter sample a picture.
With ``--intra4 I[,I...]`` (each I 0 or 1; ``--gop`` and ``--search`` may then be lists, a search > 0 is measured only at a gop > 1) the
tool measures Intra4x4 prediction in the IDR pictures (h264_cavlc.H264Encoder(gop=N, search=R, intra4=I)): per frame set one row per
(N, R, I) - I = 0 is the comparison of the same run: encode() ms and frames/s, bytes per frame, Y-PSNR of the reconstruction of all
frames, the sdv_h264_encode_idr4 launch alone, and for I = 1 (512 x 512 sets, at the first N) the share of I_NxN macroblocks and the mode
histogram of picture 0, read from its bytes by tests/h264_i4_ref.py's decoder.  Frame sets: the tiny pipeline's frames (128 x 512 x 512,
and 8 x 2048 x 2048 through the x4 upsampler) and 48 x 512 x 512 frames of every kind of tests/h264_i4_ref.py.
With ``--deblock D[,D...]`` (each D 0 or 1; one ``--gop``, ``--search`` a list, ``--qp Q[,Q...]`` the quantisers, default 16) the tool
measures the in-loop deblocking filter (h264_cavlc.H264Encoder(qp=Q, gop=N, search=R, deblock=D)): per frame set one row per (Q, R, D) -
D = 0 is the comparison of the same run: encode() ms and frames/s, bytes per frame, Y-PSNR of the returned reconstruction of all frames
against the source, and for D = 1 one sdv_h264_deblock launch alone (position 0: one picture of every GOP) and the filter launches' share
of encode().  Frame sets: the tiny pipeline's frames (128 x 512 x 512, and 8 x 2048 x 2048 through the x4 upsampler) and 48 x 512 x 512
frames of the synthetic kinds ``fade``, ``pan2``, ``glyphs``, ``vramp`` and ``noise``.
With ``--part P[,P...]`` (each P 0 or 1; one ``--gop`` N > 1, one ``--search`` R > 0, ``--subpel S[,S...]``, ``--deblock D[,D...]`` and
``--qp Q[,Q...]`` lists, defaults 0, 0 and 16) the tool measures macroblock partitions (h264_cavlc.H264Encoder(..., part=P)): per frame set
one row per (Q, S, D, P) - bytes per frame, encode() ms (HIP events, the copy back included), Y-PSNR of the reconstruction, the search
launch alone, and for P = 1 the share of the P pictures' macroblocks for which the search wrote four vectors that are not all equal (the
P_8x8 candidates; the mode decision may still code one of them intra).  Two more synthetic kinds have motion that differs inside a
macroblock: ``split`` (the upper 8 rows of every macroblock row glide right by 2 samples a picture, the lower 8 left) and ``zoom`` (the
same texture magnified by 0.4 % a picture about the centre).  The P = 0 rows of a run are the comparison.

With ``--row-slices S[,S...]`` (each S 1 .. 16; one ``--gop`` N, and ``--search``, ``--subpel``, ``--deblock``, ``--part`` and ``--qp`` lists,
defaults 0, 0, 0, 0 and 16) the tool measures several slices per macroblock row (h264_cavlc.H264Encoder(..., row_slices=S)) on the tiny
pipeline's frames (128 x 512 x 512, and 8 x 2048 x 2048 through the x4 upsampler): one row per (Q, R, S', D, P, S) - combinations in
which a setting has no effect (subpel or part without a search) are left out - with encode() ms (HIP events, the copy back included;
median and the spread of the repetitions), frames/s, bytes per frame, Y-PSNR of the reconstruction and the number of chains
(GOPs x macroblock rows x slices a row) of a per-position launch.  The S values alternate in the innermost loop.  The S = 1 rows are the
comparison: they run the code of the other settings alone.

There is no fallback: without a GPU this tool fails.
"""
from __future__ import annotations

import argparse
import json
import platform
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

QPS = (10, 16, 22)


def pipeline_frames(pipe, n: int, batch: int = 16) -> torch.Tensor:
    """n frames of 512 x 512 from the tiny pipeline, uint8 NHWC in GPU memory."""
    T = np.linspace(0.0, 1.0, n)
    out = []
    for _, embeds, noise in pipe.generate_inputs("a cat", "a dog", 42, 1337, (1, 4, 64, 64), T, batch):
        out.append(pipe(latents=noise, text_embeddings=embeds, height=512, width=512, num_inference_steps=4, output_type="u8_cuda")["images"].clone())
    return torch.cat(out)


def timed(fn, reps: int):
    """(median HIP-event ms, median host-clock ms) of fn() after two warm-up calls."""
    fn(), fn()
    gpu_ms, wall_ms = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        gpu_ms.append(e0.elapsed_time(e1))
    return float(np.median(gpu_ms)), float(np.median(wall_ms))


def measure(name: str, dev_frames: torch.Tensor, reps: int) -> dict:
    import h264_ref as R
    from stable_diffusion_videos_amd import h264, hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    from stable_diffusion_videos_amd.jpeg import encoder_for as jpeg_encoder_for
    n, H, W, _ = dev_frames.shape
    mbh, mbw = hip.h264_mb_grid(H, W)
    case = dict(content=name, n=n, H=H, W=W)
    enc = H264Encoder(16, dev_frames.device)
    ev, wall = timed(lambda: enc.encode(dev_frames), reps)
    case.update(cavlc_encode_ms_events=round(ev, 3), cavlc_encode_ms_host_clock=round(wall, 3), cavlc_frames_per_sec=round(n / wall * 1e3, 1),
                cavlc_bytes_to_host_per_frame=int(enc.last_bytes_to_host // n))
    ws = next(iter(enc._ws.values()))
    stages = (("planes", lambda: hip.h264_planes(dev_frames, ws["y"], ws["cb"], ws["cr"])),
              ("rows", lambda: hip.h264_encode_rows(ws["y"], ws["cb"], ws["cr"], 16, 0, ws["scratch"])),
              ("pack", lambda: hip.h264_pack(ws["scratch"], n, mbh, mbw, ws["out"], ws["offsets"])))
    for stage, fn in stages:
        case[f"cavlc_{stage}_kernel_ms"] = round(timed(fn, reps)[0], 3)
    jenc = jpeg_encoder_for(95, dev_frames.device)
    ev, wall = timed(lambda: jenc.encode(dev_frames), reps)
    jpegs = jenc.encode(dev_frames)
    case.update(mjpeg_q95_encode_ms_host_clock=round(wall, 3), mjpeg_q95_frames_per_sec=round(n / wall * 1e3, 1),
                mjpeg_q95_bytes_per_frame=int(sum(len(j) for j in jpegs) // n))
    pinned = torch.empty(dev_frames.shape, dtype=torch.uint8, pin_memory=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pinned.copy_(dev_frames, non_blocking=True)
    torch.cuda.synchronize()
    copy_ms = (time.perf_counter() - t0) * 1e3
    host = pinned.numpy()
    k = min(n, 8)
    pcm_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        sizes = [4 + len(h264.idr_picture(host[i], i)) for i in range(k)]
        pcm_ms.append((time.perf_counter() - t0) * 1e3 / k)
    per_frame = min(pcm_ms) + copy_ms / n
    case.update(pcm_host_ms_per_frame_incl_copy=round(per_frame, 3), pcm_host_frames_per_sec=round(1e3 / per_frame, 1), pcm_bytes_per_frame=int(sizes[0]),
                raw_copy_ms=round(copy_ms, 3))
    case["cavlc_vs_pcm_host_speed"] = round(case["cavlc_frames_per_sec"] / case["pcm_host_frames_per_sec"], 2)
    case["cavlc_vs_mjpeg_gpu_speed"] = round(case["cavlc_frames_per_sec"] / case["mjpeg_q95_frames_per_sec"], 2)
    for qp in QPS:
        samples = H264Encoder(qp, dev_frames.device).encode(dev_frames)
        size = int(sum(len(s) for s in samples) // n)
        case[f"cavlc_qp{qp}_bytes_per_frame"] = size
        case[f"cavlc_qp{qp}_vs_pcm_bytes"] = round(size / case["pcm_bytes_per_frame"], 4)
        case[f"cavlc_qp{qp}_vs_mjpeg_q95_bytes"] = round(size / case["mjpeg_q95_bytes_per_frame"], 3)
        if H * W <= 512 * 512:
            d = R.decode_sample(samples[0], W, H)
            y = R.rgb_to_planes(host[:1])[0][0, :H, :W].astype(np.float64)
            mse = float(np.mean((d["y"].astype(np.float64) - y) ** 2))
            case[f"cavlc_qp{qp}_y_psnr_db"] = round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None
            case[f"cavlc_qp{qp}_pcm_macroblocks_frame0"] = int(d["n_pcm"])
    print(json.dumps(case), flush=True)
    return case


def temporal_frames(kind: str, n: int, size: int, dev) -> torch.Tensor:
    """``fade`` / ``pan`` of tests/h264_p_ref.py at n x size x size, built in GPU memory from its glyph frames."""
    import h264_ref as R
    if kind == "glide":
        import h264_sub_ref as S
        return torch.from_numpy(S.glide_frames(1, n, size, size)).to(dev).contiguous()
    g = torch.from_numpy(R.make_frames("glyphs", 2, size, size)).to(dev)
    if kind in ("pan", "pan2"):
        return torch.stack([torch.roll(g[0], k * (2 if kind == "pan2" else 1), dims=1) for k in range(n)]).contiguous()
    a, b = g[0].to(torch.int64), g[1].to(torch.int64)
    return torch.stack([((a * (2 * (n - 1) - 2 * k) + b * 2 * k + (n - 1)) // (2 * (n - 1))).to(torch.uint8) for k in range(n)]).contiguous()


def measure_gop(name: str, dev_frames: torch.Tensor, gop: int, reps: int) -> list:
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    n, H, W, _ = dev_frames.shape
    mbh, mbw = hip.h264_mb_grid(H, W)
    y, cb, cr = hip.h264_planes(dev_frames)
    rows = []
    for g in (1, gop):
        enc = H264Encoder(16, dev_frames.device, gop=g)
        ev, wall = timed(lambda: enc.encode(dev_frames), reps)
        samples = enc.encode(dev_frames)
        recon = [torch.empty_like(p) for p in (y, cb, cr)]
        scratch = torch.empty((hip.h264_gop_scratch_bytes(n, mbh, mbw),), dtype=torch.uint8, device=dev_frames.device)
        hip.h264_encode_gops(y, cb, cr, 16, g, 0, *recon, scratch)
        mse = float(((recon[0][:, :H, :W].to(torch.float64) - y[:, :H, :W].to(torch.float64)) ** 2).mean())
        row = dict(content=name, n=n, H=H, W=W, qp=16, gop=g, chains=-(-n // g) * mbh, encode_ms_events=round(ev, 3), encode_ms_host_clock=round(wall, 3),
                   frames_per_sec=round(n / wall * 1e3, 1), bytes_per_frame=int(sum(len(s) for s in samples) // n),
                   y_psnr_db=round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del enc, recon, scratch
        torch.cuda.empty_cache()
    return rows


def measure_search(name: str, dev_frames: torch.Tensor, gop: int, searches, reps: int) -> list:
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    n, H, W, _ = dev_frames.shape
    y = hip.h264_planes(dev_frames)[0]
    rows = []
    for search in searches:
        enc = H264Encoder(16, dev_frames.device, gop=gop, search=search)
        ev, wall = timed(lambda: enc.encode(dev_frames), reps)
        samples, recon = enc.encode(dev_frames, return_recon=True)
        mse = float(((recon[0][:, :H, :W].to(torch.float64) - y[:, :H, :W].to(torch.float64)) ** 2).mean())
        row = dict(content=name, n=n, H=H, W=W, qp=16, gop=gop, search=search, launches=3 + (1 + min(gop, n) if search else 1),
                   encode_ms_events=round(ev, 3), encode_ms_host_clock=round(wall, 3), frames_per_sec=round(n / wall * 1e3, 1),
                   bytes_per_frame=int(sum(len(s) for s in samples) // n), y_psnr_db=round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None)
        if search:
            mv = torch.empty((n, y.shape[1] // 16, y.shape[2] // 16, 2), dtype=torch.int16, device=dev_frames.device)
            ms = timed(lambda: hip.h264_motion_search(y, 16, gop, search, mv), reps)[0]
            row.update(search_kernel_ms=round(ms, 3), search_share_of_encode=round(ms / ev, 3),
                       nonzero_vectors=round(float((mv != 0).any(dim=-1).float().mean()), 4))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del enc, recon
        torch.cuda.empty_cache()
    return rows


def measure_subpel(name: str, dev_frames: torch.Tensor, gop: int, search: int, subpels, reps: int) -> list:
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    n, H, W, _ = dev_frames.shape
    y = hip.h264_planes(dev_frames)[0]
    rows = []
    for subpel in subpels:
        enc = H264Encoder(16, dev_frames.device, gop=gop, search=search, subpel=subpel)
        ev, wall = timed(lambda: enc.encode(dev_frames), reps)
        samples, recon = enc.encode(dev_frames, return_recon=True)
        mse = float(((recon[0][:, :H, :W].to(torch.float64) - y[:, :H, :W].to(torch.float64)) ** 2).mean())
        mv = torch.empty((n, y.shape[1] // 16, y.shape[2] // 16, 2), dtype=torch.int16, device=dev_frames.device)
        if subpel:
            ms = timed(lambda: hip.h264_motion_search_sub(y, 16, gop, search, subpel, mv), reps)[0]
        else:
            ms = timed(lambda: hip.h264_motion_search(y, 16, gop, search, mv), reps)[0]
        row = dict(content=name, n=n, H=H, W=W, qp=16, gop=gop, search=search, subpel=subpel, launches=4 + min(gop, n),
                   encode_ms_events=round(ev, 3), encode_ms_host_clock=round(wall, 3), frames_per_sec=round(n / wall * 1e3, 1),
                   bytes_per_frame=int(sum(len(s) for s in samples) // n), y_psnr_db=round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None,
                   search_kernel_ms=round(ms, 3), search_share_of_encode=round(ms / ev, 3),
                   nonzero_vectors=round(float((mv != 0).any(dim=-1).float().mean()), 4),
                   fractional_vectors=round(float((mv % 4 != 0).any(dim=-1).float().mean()), 4) if subpel else 0.0)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del enc, recon
        torch.cuda.empty_cache()
    return rows


def measure_intra4(name: str, frames, gops, searches, intra4s, reps: int) -> list:
    """``frames``: uint8 NHWC frames in GPU memory, or padded planes (y, cb, cr) for the kinds that exist as planes only."""
    import h264_i4_ref as I4
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    planes = isinstance(frames, tuple)
    y, cb, cr = frames if planes else hip.h264_planes(frames)
    n, H, W = y.shape if planes else frames.shape[:3]
    mbh, mbw = y.shape[1] // 16, y.shape[2] // 16
    rows = []
    for gop in gops:
        for search in searches:
            if search and gop == 1:
                continue
            for intra4 in intra4s:
                enc = H264Encoder(16, y.device, gop=gop, search=search, intra4=intra4)
                run = (lambda **kw: enc.encode_planes(y, cb, cr, **kw)) if planes else (lambda **kw: enc.encode(frames, **kw))
                ev, wall = timed(run, reps)
                if intra4 or gop > 1:
                    samples, recon = run(return_recon=True)
                    mse = float(((recon[0][:, :H, :W].to(torch.float64) - y[:, :H, :W].to(torch.float64)) ** 2).mean())
                    psnr = round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None
                else:                                                               # the all-intra rows kernel keeps no reconstruction
                    samples, psnr = run(), None
                row = dict(content=name, n=n, H=H, W=W, qp=16, gop=gop, search=search, intra4=intra4, encode_ms_events=round(ev, 3),
                           encode_ms_host_clock=round(wall, 3), frames_per_sec=round(n / wall * 1e3, 1),
                           bytes_per_frame=int(sum(len(s) for s in samples) // n), y_psnr_db=psnr)
                if intra4:
                    recon = [torch.empty_like(p) for p in (y, cb, cr)]
                    scratch = torch.empty((hip.h264_gop_scratch_bytes(n, mbh, mbw),), dtype=torch.uint8, device=y.device)
                    ms = timed(lambda: hip.h264_encode_idr4(y, cb, cr, 16, gop, 0, *recon, scratch), reps)[0]
                    row.update(idr4_kernel_ms=round(ms, 3), idr4_share_of_encode=round(ms / ev, 3))
                    del recon, scratch
                    if H * W <= 512 * 512 and gop == gops[0] and not search:
                        d = I4.decode_stream(samples[:1], W, H)
                        row.update(i_nxn_share_picture0=round(d["n_i4"] / (mbh * mbw), 4), pcm_share_picture0=round(d["n_pcm"] / (mbh * mbw), 4),
                                   mode_histogram_picture0=d["i4_modes"])
                print(json.dumps(row), flush=True)
                rows.append(row)
                del enc
                torch.cuda.empty_cache()
    return rows


def measure_deblock(name: str, frames: torch.Tensor, gop: int, searches, qps, deblocks, reps: int) -> list:
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    n, H, W, _ = frames.shape
    y = hip.h264_planes(frames)[0]
    rows = []
    for qp in qps:
        for search in searches:
            for deblock in deblocks:
                enc = H264Encoder(qp, frames.device, gop=gop, search=search, deblock=deblock)
                ev, wall = timed(lambda: enc.encode(frames), reps)
                samples, recon = enc.encode(frames, return_recon=True)
                mse = float(((recon[0][:, :H, :W].to(torch.float64) - y[:, :H, :W].to(torch.float64)) ** 2).mean())
                row = dict(content=name, n=n, H=H, W=W, qp=qp, gop=gop, search=search, deblock=deblock, encode_ms_events=round(ev, 3),
                           encode_ms_host_clock=round(wall, 3), frames_per_sec=round(n / wall * 1e3, 1),
                           bytes_per_frame=int(sum(len(s) for s in samples) // n), y_psnr_db=round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None)
                if deblock:
                    ws = next(iter(enc._ws.values()))
                    ms = timed(lambda: hip.h264_deblock(*recon, qp, gop, 0, 0, ws["mbinfo"], ws["mv"]), reps)[0]
                    launches = min(gop, n) - 1                                      # encode() leaves out the last position's filter
                    row.update(deblock_kernel_ms=round(ms, 3), deblock_launches=launches, deblock_share_of_encode=round(ms * launches / ev, 3))
                print(json.dumps(row), flush=True)
                rows.append(row)
                del enc, recon
                torch.cuda.empty_cache()
    return rows


def zoom_frames(n: int, size: int) -> np.ndarray:
    """tests/h264_sub_ref.py's analytic texture magnified by 0.4 % a picture about the centre: every 8x8 block moves a little differently."""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    c = (size - 1) / 2.0
    frames = np.empty((n, size, size, 3), dtype=np.uint8)
    for k in range(n):
        x, y = c + (xx - c) / (1.0 + 0.004 * k), c + (yy - c) / (1.0 + 0.004 * k)
        v = 128 + 38 * np.sin(2 * np.pi * x / 11 + 0.3) + 30 * np.sin(2 * np.pi * (x / 7.3 + y / 19)) + 24 * np.sin(2 * np.pi * y / 9 + 1.0) \
            + 20 * np.sin(2 * np.pi * (x / 23 - y / 13))
        ch = 128 + 50 * np.sin(2 * np.pi * (x / 29 + y / 37) + 0.7)
        frames[k] = np.clip(np.rint(np.stack([v, 0.5 * v + 0.5 * ch, ch], axis=-1)), 0, 255).astype(np.uint8)
    return frames


def measure_part(name: str, frames: torch.Tensor, gop: int, search: int, subpels, deblocks, qps, parts, reps: int) -> list:
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    n, H, W, _ = frames.shape
    y = hip.h264_planes(frames)[0]
    p_pictures = n - len(range(0, n, gop))
    rows = []
    for qp in qps:
        for subpel in subpels:
            for deblock in deblocks:
                for part in parts:
                    enc = H264Encoder(qp, frames.device, gop=gop, search=search, subpel=subpel, deblock=deblock, part=part)
                    ev, wall = timed(lambda: enc.encode(frames), reps)
                    samples, recon = enc.encode(frames, return_recon=True)
                    mse = float(((recon[0][:, :H, :W].to(torch.float64) - y[:, :H, :W].to(torch.float64)) ** 2).mean())
                    row = dict(content=name, n=n, H=H, W=W, qp=qp, gop=gop, search=search, subpel=subpel, deblock=deblock, part=part,
                               encode_ms_events=round(ev, 3), encode_ms_host_clock=round(wall, 3), frames_per_sec=round(n / wall * 1e3, 1),
                               bytes_per_frame=int(sum(len(s) for s in samples) // n),
                               y_psnr_db=round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None)
                    ws = next(iter(enc._ws.values()))
                    mv = ws["mv"]
                    if part:
                        split = (mv != mv[:, :, :, :1]).any(dim=-1).any(dim=-1)
                        row["p8x8_share_of_p_macroblocks"] = round(float(split.sum()) / max(1, p_pictures * mv.shape[1] * mv.shape[2]), 4)
                        ms = timed(lambda: hip.h264_motion_search_part(ws["y"], qp, gop, search, subpel, mv), reps)[0]
                    elif subpel:
                        ms = timed(lambda: hip.h264_motion_search_sub(ws["y"], qp, gop, search, subpel, mv), reps)[0]
                    else:
                        ms = timed(lambda: hip.h264_motion_search(ws["y"], qp, gop, search, mv), reps)[0]
                    row.update(search_kernel_ms=round(ms, 3), search_share_of_encode=round(ms / ev, 3))
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                    del enc, recon, ws, mv
                    torch.cuda.empty_cache()
    return rows


def main_part(args):
    import h264_i4_ref as I4
    import h264_me_ref as ME
    import h264_part_ref as PT
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    dev = torch.device("cuda", 0)
    result = dict(tool=f"tools/h264_bench.py --gop {args.gop} --search {args.search} --subpel {args.subpel} --deblock {args.deblock} --qp {args.qp} "
                       f"--part {args.part}", gpu=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(), reps=args.reps, rows=[])
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    small = pipeline_frames(pipe, 128)
    up = RealESRGANModel.from_pretrained("nateraw/real-esrgan")
    up.to(dev)
    big = torch.cat([up.upsample_u8(small[k:k + 2]) for k in range(0, 8, 2)])
    del pipe, up
    sets = [("tiny pipeline", lambda: small.contiguous()), ("tiny pipeline x4 upsampler", lambda: big.contiguous())]
    for kind in ("fade", "pan2"):
        sets.append((kind, lambda kind=kind: torch.from_numpy(ME.make_frames(kind, 48, 512, 512)).to(dev).contiguous()))
    for kind in ("glyphs", "noise"):
        sets.append((kind, lambda kind=kind: torch.from_numpy(I4.make_frames(kind, 48, 512, 512)).to(dev).contiguous()))
    sets.append(("split", lambda: torch.from_numpy(PT.split_frames(8, 48, 512, 512)).to(dev).contiguous()))
    sets.append(("zoom", lambda: torch.from_numpy(zoom_frames(48, 512)).to(dev).contiguous()))
    for name, make in sets:
        result["rows"] += measure_part(name, make(), args.gops[0], args.searches[0], args.subpels, args.deblocks, args.qps, args.parts, args.reps)
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


def timed_spread(fn, reps: int):
    """``timed`` that keeps the repetitions: (median, minimum, maximum HIP-event ms, median host-clock ms) of fn() after two warm-up calls."""
    fn(), fn()
    gpu_ms, wall_ms = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        gpu_ms.append(e0.elapsed_time(e1))
    return float(np.median(gpu_ms)), float(min(gpu_ms)), float(max(gpu_ms)), float(np.median(wall_ms))


def measure_seg(name: str, frames: torch.Tensor, gop: int, searches, subpels, deblocks, parts, qps, row_slices, reps: int) -> list:
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.h264_cavlc import H264Encoder
    n, H, W, _ = frames.shape
    mbh, mbw = hip.h264_mb_grid(H, W)
    y = hip.h264_planes(frames)[0]
    rows = []
    for qp in qps:
        for search in searches:
            for subpel in subpels:
                for deblock in deblocks:
                    for part in parts:
                        if (subpel or part) and not (search and gop > 1):                   # no effect: the row would repeat another
                            continue
                        for s in row_slices:
                            enc = H264Encoder(qp, frames.device, gop=gop, search=search, subpel=subpel, deblock=deblock, part=part, row_slices=s)
                            ev, lo, hi, wall = timed_spread(lambda: enc.encode(frames), reps)
                            samples, recon = enc.encode(frames, return_recon=True)
                            mse = float(((recon[0][:, :H, :W].to(torch.float64) - y[:, :H, :W].to(torch.float64)) ** 2).mean())
                            segs = hip.h264_row_segments(mbh, mbw, s)
                            row = dict(content=name, n=n, H=H, W=W, qp=qp, gop=gop, search=search, subpel=subpel, deblock=deblock, part=part, row_slices=s,
                                       segs=segs, chains=-(-n // gop) * mbh * segs, encode_ms_events=round(ev, 3), encode_ms_events_min=round(lo, 3),
                                       encode_ms_events_max=round(hi, 3), encode_ms_host_clock=round(wall, 3), frames_per_sec=round(n / wall * 1e3, 1),
                                       bytes_per_frame=int(sum(len(b) for b in samples) // n),
                                       y_psnr_db=round(10.0 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None)
                            print(json.dumps(row), flush=True)
                            rows.append(row)
                            del enc, recon, samples
                            torch.cuda.empty_cache()
    return rows


def main_seg(args):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    dev = torch.device("cuda", 0)
    result = dict(tool=f"tools/h264_bench.py --gop {args.gop} --search {args.search} --subpel {args.subpel} --deblock {args.deblock} --part {args.part} "
                       f"--qp {args.qp} --row-slices {args.row_slices}", gpu=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(),
                  reps=args.reps, rows=[])
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    small = pipeline_frames(pipe, 128)
    up = RealESRGANModel.from_pretrained("nateraw/real-esrgan")
    up.to(dev)
    big = torch.cat([up.upsample_u8(small[k:k + 2]) for k in range(0, 8, 2)])
    del pipe, up
    torch.cuda.empty_cache()
    for name, frames in (("tiny pipeline x4 upsampler", big.contiguous()), ("tiny pipeline", small.contiguous())):
        result["rows"] += measure_seg(name, frames, args.gops[0], args.searches, args.subpels, args.deblocks, args.parts, args.qps, args.slices, args.reps)
        if args.out:                                                                        # (kept as it grows: a long run leaves what it measured)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(result) + "\n")
    line = json.dumps(result)
    if args.out:
        Path(args.out).write_text(line + "\n")
    print(line)


def main_deblock(args):
    import h264_i4_ref as I4
    import h264_me_ref as ME
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    dev = torch.device("cuda", 0)
    result = dict(tool=f"tools/h264_bench.py --gop {args.gop} --search {args.search} --qp {args.qp} --deblock {args.deblock}",
                  gpu=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(), reps=args.reps, rows=[])
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    small = pipeline_frames(pipe, 128)
    up = RealESRGANModel.from_pretrained("nateraw/real-esrgan")
    up.to(dev)
    big = torch.cat([up.upsample_u8(small[k:k + 2]) for k in range(0, 8, 2)])
    del pipe, up
    sets = [("tiny pipeline", lambda: small.contiguous()), ("tiny pipeline x4 upsampler", lambda: big.contiguous())]
    for kind in ("fade", "pan2"):
        sets.append((kind, lambda kind=kind: torch.from_numpy(ME.make_frames(kind, 48, 512, 512)).to(dev).contiguous()))
    for kind in ("glyphs", "vramp", "noise"):
        sets.append((kind, lambda kind=kind: torch.from_numpy(I4.make_frames(kind, 48, 512, 512)).to(dev).contiguous()))
    for name, make in sets:
        result["rows"] += measure_deblock(name, make(), args.gops[0], args.searches, args.qps, args.deblocks, args.reps)
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


def main_intra4(args):
    import h264_i4_ref as I4
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    dev = torch.device("cuda", 0)
    result = dict(tool=f"tools/h264_bench.py --gop {args.gop} --search {args.search} --intra4 {args.intra4}", gpu=torch.cuda.get_device_name(0),
                  host=platform.processor() or platform.machine(), reps=args.reps, qp=16, rows=[])
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    small = pipeline_frames(pipe, 128)
    up = RealESRGANModel.from_pretrained("nateraw/real-esrgan")
    up.to(dev)
    big = torch.cat([up.upsample_u8(small[k:k + 2]) for k in range(0, 8, 2)])
    del pipe, up
    sets = [("tiny pipeline", lambda: small.contiguous()), ("tiny pipeline x4 upsampler", lambda: big.contiguous())]
    for kind in I4.KINDS:
        if kind.endswith("_pcm"):
            sets.append((kind, lambda kind=kind: tuple(torch.from_numpy(p).to(dev) for p in I4.make_planes(kind, 48, 512, 512))))
        else:
            sets.append((kind, lambda kind=kind: torch.from_numpy(I4.make_frames(kind, 48, 512, 512)).to(dev).contiguous()))
    for name, make in sets:
        result["rows"] += measure_intra4(name, make(), args.gops, args.searches, args.intra4s, args.reps)
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


def main_gop(args):
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    dev = torch.device("cuda", 0)
    result = dict(tool=f"tools/h264_bench.py --gop {args.gop}", gpu=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(),
                  reps=args.reps, qp=16, rows=[])
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    small = pipeline_frames(pipe, 128)
    up = RealESRGANModel.from_pretrained("nateraw/real-esrgan")
    up.to(dev)
    big = torch.cat([up.upsample_u8(small[k:k + 2]) for k in range(0, 8, 2)])
    del pipe, up
    sets = [("tiny pipeline", lambda: small), ("fade", lambda: temporal_frames("fade", 128, 512, dev)),
            ("pan", lambda: temporal_frames("pan", 128, 512, dev)), ("tiny pipeline x4 upsampler", lambda: big),
            ("fade", lambda: temporal_frames("fade", 8, 2048, dev)), ("pan", lambda: temporal_frames("pan", 8, 2048, dev))]
    if args.search is not None:
        result["tool"] += f" --search {args.search}"
        sets.insert(3, ("pan2", lambda: temporal_frames("pan2", 128, 512, dev)))
        sets.append(("pan2", lambda: temporal_frames("pan2", 8, 2048, dev)))
    if args.subpel is not None:
        result["tool"] += f" --subpel {args.subpel}"
        sets.insert(4, ("glide", lambda: temporal_frames("glide", 128, 512, dev)))
        sets.append(("glide", lambda: temporal_frames("glide", 8, 2048, dev)))
    for name, make in sets:
        if args.subpel is not None:
            result["rows"] += measure_subpel(name, make().contiguous(), args.gop, args.searches[0], args.subpels, args.reps)
        elif args.search is not None:
            result["rows"] += measure_search(name, make().contiguous(), args.gop, args.searches, args.reps)
        else:
            result["rows"] += measure_gop(name, make().contiguous(), args.gop, args.reps)
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gop", default="1", help="N > 1: measure the GOP path, rows for gop 1 and gop N side by side (with --intra4: N[,N...])")
    ap.add_argument("--search", default=None, help="with --gop N: R[,R...] (even, 0 .. 16): one row per motion search range, 0 = none")
    ap.add_argument("--subpel", default=None, help="with --gop N --search R (one R > 0): S[,S...] (0, 1, 2, 4): one row per vector grid, 0 = even samples")
    ap.add_argument("--intra4", default=None, help="I[,I...] (0, 1): one row per (gop, search, I); --gop and --search are then lists, 0 = Intra16x16 only")
    ap.add_argument("--deblock", default=None, help="D[,D...] (0, 1): one row per (qp, search, D) at one --gop N; 0 = the loop filter off")
    ap.add_argument("--qp", default=None, help="with --deblock: Q[,Q...] (0 .. 51), default 16")
    ap.add_argument("--part", default=None, help="P[,P...] (0, 1): one row per (qp, subpel, deblock, P) at one --gop N > 1 and one --search R > 0")
    ap.add_argument("--row-slices", default=None, help="S[,S...] (1 .. 16): one row per (qp, search, subpel, deblock, part, S) at one --gop N")
    args = ap.parse_args()
    if args.row_slices is not None:
        args.gops = [int(v) for v in args.gop.split(",")]
        args.search, args.subpel, args.deblock = args.search or "0", args.subpel or "0", args.deblock or "0"
        args.part, args.qp = args.part or "0", args.qp or "16"
        args.searches, args.subpels = [int(v) for v in args.search.split(",")], [int(v) for v in args.subpel.split(",")]
        args.deblocks, args.parts = [int(v) for v in args.deblock.split(",")], [int(v) for v in args.part.split(",")]
        args.qps, args.slices = [int(v) for v in args.qp.split(",")], [int(v) for v in args.row_slices.split(",")]
        if args.intra4 is not None or len(args.gops) != 1 or not 2 <= args.gops[0] <= 256 or any(v % 2 or not 0 <= v <= 16 for v in args.searches) \
                or any(v not in (0, 1, 2, 4) for v in args.subpels) or any(v not in (0, 1) for v in args.deblocks + args.parts) \
                or any(not 0 <= v <= 51 for v in args.qps) or any(not 1 <= v <= 16 for v in args.slices):
            raise SystemExit("--row-slices takes 1 .. 16, with one --gop N (2 .. 256), --search R[,R...] (even, 0 .. 16), --subpel S[,S...] (0, 1, 2, 4), "
                             "--deblock D[,D...] (0, 1), --part P[,P...] (0, 1) and --qp Q[,Q...] (0 .. 51), without --intra4")
        if not torch.cuda.is_available():
            raise SystemExit("h264_bench needs the GPU (no fallback)")
        return main_seg(args)
    if args.part is not None:
        args.gops = [int(v) for v in args.gop.split(",")]
        args.searches = [int(v) for v in (args.search or "0").split(",")]
        args.subpel, args.deblock, args.qp = args.subpel or "0", args.deblock or "0", args.qp or "16"
        args.subpels, args.deblocks = [int(v) for v in args.subpel.split(",")], [int(v) for v in args.deblock.split(",")]
        args.qps, args.parts = [int(v) for v in args.qp.split(",")], [int(v) for v in args.part.split(",")]
        if args.intra4 is not None or len(args.gops) != 1 or not 2 <= args.gops[0] <= 256 or len(args.searches) != 1 or args.searches[0] % 2 \
                or not 2 <= args.searches[0] <= 16 or any(v not in (0, 1, 2, 4) for v in args.subpels) or any(v not in (0, 1) for v in args.deblocks + args.parts) \
                or any(not 0 <= v <= 51 for v in args.qps):
            raise SystemExit("--part takes 0 and 1, with one --gop N (2 .. 256), one --search R (even, 2 .. 16), --subpel S[,S...] (0, 1, 2, 4), "
                             "--deblock D[,D...] (0, 1) and --qp Q[,Q...] (0 .. 51), without --intra4")
        if not torch.cuda.is_available():
            raise SystemExit("h264_bench needs the GPU (no fallback)")
        return main_part(args)
    if args.qp is not None and args.deblock is None:
        raise SystemExit("--qp goes with --deblock (the other measurements are taken at qp 16)")
    if args.deblock is not None:
        args.gops = [int(v) for v in args.gop.split(",")]
        args.searches = [int(v) for v in (args.search or "0").split(",")]
        args.search, args.qp = args.search or "0", args.qp or "16"
        args.qps = [int(v) for v in args.qp.split(",")]
        args.deblocks = [int(v) for v in args.deblock.split(",")]
        if args.subpel is not None or args.intra4 is not None or len(args.gops) != 1 or not 1 <= args.gops[0] <= 256 \
                or any(v % 2 or not 0 <= v <= 16 for v in args.searches) or any(not 0 <= v <= 51 for v in args.qps) or any(v not in (0, 1) for v in args.deblocks):
            raise SystemExit("--deblock takes 0 and 1, with one --gop N (1 .. 256), --search R[,R...] (even, 0 .. 16) and --qp Q[,Q...] (0 .. 51), "
                             "without --subpel and --intra4")
        if not torch.cuda.is_available():
            raise SystemExit("h264_bench needs the GPU (no fallback)")
        return main_deblock(args)
    if args.intra4 is not None:
        args.gops = [int(v) for v in args.gop.split(",")]
        args.searches = [int(v) for v in (args.search or "0").split(",")]
        args.search = args.search or "0"
        args.intra4s = [int(v) for v in args.intra4.split(",")]
        if args.subpel is not None or any(not 1 <= v <= 256 for v in args.gops) or any(v % 2 or not 0 <= v <= 16 for v in args.searches) \
                or any(v not in (0, 1) for v in args.intra4s):
            raise SystemExit("--intra4 takes 0 and 1, with --gop N[,N...] (1 .. 256) and --search R[,R...] (even, 0 .. 16), without --subpel")
        if not torch.cuda.is_available():
            raise SystemExit("h264_bench needs the GPU (no fallback)")
        return main_intra4(args)
    args.gop = int(args.gop)
    if args.search is not None:
        if args.gop == 1:
            raise SystemExit("--search needs --gop N > 1 (there are no P pictures at gop 1)")
        args.searches = [int(v) for v in args.search.split(",")]
        if any(v % 2 or not 0 <= v <= 16 for v in args.searches):
            raise SystemExit("--search takes even values 0 .. 16")
    if args.subpel is not None:
        if args.search is None or len(args.searches) != 1 or args.searches[0] == 0:
            raise SystemExit("--subpel needs --gop N > 1 and --search R with one R > 0")
        args.subpels = [int(v) for v in args.subpel.split(",")]
        if any(v not in (0, 1, 2, 4) for v in args.subpels):
            raise SystemExit("--subpel takes the values 0, 1, 2, 4")
    if not torch.cuda.is_available():
        raise SystemExit("h264_bench needs the GPU (no fallback)")
    if args.gop != 1:
        if not 2 <= args.gop <= 256:
            raise SystemExit("--gop must be 2 .. 256 (1 = the intra measurement)")
        return main_gop(args)
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    dev = torch.device("cuda", 0)
    result = dict(tool="tools/h264_bench.py", gpu=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(), reps=args.reps,
                  qp_timed=16, cases=[])
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    small = pipeline_frames(pipe, 128)
    up = RealESRGANModel.from_pretrained("nateraw/real-esrgan")
    up.to(dev)
    big = torch.cat([up.upsample_u8(small[k:k + 2]) for k in range(0, 8, 2)])
    gen = torch.Generator(device="cpu").manual_seed(0)
    for name, frames in (("tiny pipeline", small), ("uniform noise", torch.randint(0, 256, (128, 512, 512, 3), dtype=torch.uint8, generator=gen).to(dev)),
                         ("tiny pipeline x4 upsampler", big),
                         ("uniform noise", torch.randint(0, 256, (8, 2048, 2048, 3), dtype=torch.uint8, generator=gen).to(dev))):
        result["cases"].append(measure(name, frames.contiguous(), args.reps))
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
