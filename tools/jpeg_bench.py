"""GPU JPEG encoder (jpeg.JpegEncoder) against the host-side PIL encode it replaces, on the same box.

    python tools/jpeg_bench.py [--out FILE] [--reps 5]

Cases: 128 frames of 512 x 512 and 16 frames of 2048 x 2048 (an upsampled walk), quality 75 and 95.  The frames are a seeded smooth
pattern with Gaussian noise (photo-like spectra; no model needed).  GPU time: HIP events around encode() of frames already in HBM,
the copies back to pinned memory included (encode() ends in a synchronise), plus the host clock around the same call (which adds
the slicing into bytes objects).  PIL: Image.fromarray(frame).save(buffer, "JPEG", quality, subsampling 4:2:0) on FrameWriter's
thread count - what the parent path does after copying the raw frames to the host; that copy is timed separately.
There is no fallback: without a GPU this tool fails.
"""
from __future__ import annotations

import argparse
import io
import json
import platform
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def make_frames(n: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W, 3), dtype=np.float32)
    for k in range(n):
        for c in range(3):
            out[k, :, :, c] = 128 + 70 * np.sin(x / (23.0 + 5 * c) + 0.2 * k) * np.cos(y / (31.0 - 4 * c) + 0.3 * c) \
                + 30 * np.sin((x + y) / (3.0 + c))
        out[k] += rng.normal(0, 4, (H, W, 3))
    return np.clip(np.round(out), 0, 255).astype(np.uint8)


def pil_encode(frame: np.ndarray, quality: int) -> int:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="JPEG", quality=quality, subsampling=2)
    return len(buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs the GPU (no fallback)")
    from stable_diffusion_videos_amd.jpeg import JpegEncoder
    from stable_diffusion_videos_amd.utils import FrameWriter
    dev = torch.device("cuda", 0)
    writer = FrameWriter()
    threads = writer.workers
    writer.close()
    result = dict(tool="tools/jpeg_bench.py", gpu=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(),
                  pil_threads=threads, reps=args.reps, cases=[])
    for n, H, W in ((128, 512, 512), (16, 2048, 2048)):
        frames = make_frames(n, H, W)
        dev_frames = torch.from_numpy(frames).to(dev)
        pinned = torch.empty(frames.shape, dtype=torch.uint8, pin_memory=True)
        for quality in (75, 95):
            enc = JpegEncoder(quality, dev)
            files = enc.encode(dev_frames)                                       # warm-up: workspaces, code objects (and a retry, if any)
            files = enc.encode(dev_frames)
            gpu_ms, wall_ms = [], []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                files = enc.encode(dev_frames)
                e1.record()
                e1.synchronize()
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                gpu_ms.append(e0.elapsed_time(e1))
            copy_ms = []
            for _ in range(args.reps):                                           # the raw copy the PIL path needs first
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pinned.copy_(dev_frames, non_blocking=True)
                torch.cuda.synchronize()
                copy_ms.append((time.perf_counter() - t0) * 1e3)
            host = pinned.numpy()
            pil_ms, pil_bytes = [], 0
            with ThreadPoolExecutor(max_workers=threads) as pool:
                list(pool.map(lambda f: pil_encode(f, quality), host[:min(n, threads)]))
                for _ in range(max(2, args.reps // 2)):
                    t0 = time.perf_counter()
                    sizes = list(pool.map(lambda f: pil_encode(f, quality), host))
                    pil_ms.append((time.perf_counter() - t0) * 1e3)
                    pil_bytes = sum(sizes)
            from PIL import Image
            back = np.asarray(Image.open(io.BytesIO(files[0])))
            mse = float(((back.astype(np.float64) - frames[0]) ** 2).mean())
            case = dict(n=n, H=H, W=W, quality=quality,
                        gpu_encode_ms_events=round(float(np.median(gpu_ms)), 3), gpu_encode_ms_host_clock=round(float(np.median(wall_ms)), 3),
                        gpu_ms_per_frame=round(float(np.median(gpu_ms)) / n, 4),
                        pil_encode_ms=round(float(np.median(pil_ms)), 3), raw_copy_ms=round(float(np.median(copy_ms)), 3),
                        pil_ms_per_frame=round((float(np.median(pil_ms)) + float(np.median(copy_ms))) / n, 4),
                        bytes_to_host_per_frame_gpu=int(enc.last_bytes_to_host // n), bytes_to_host_per_frame_pil=H * W * 3,
                        file_bytes_per_frame_gpu=int(sum(len(f) for f in files) // n), file_bytes_per_frame_pil=int(pil_bytes // n),
                        psnr_first_frame_db=round(10 * np.log10(255.0 ** 2 / max(mse, 1e-12)), 2), retries=enc.retries)
            case["speedup_vs_pil_incl_copy"] = round(case["pil_ms_per_frame"] / case["gpu_ms_per_frame"], 2)
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
