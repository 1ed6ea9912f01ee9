"""GPU PNG encoder (png.PngEncoder) against the host-side PIL encode it can replace, on the same box.

    python tools/png_bench.py [--out FILE] [--reps 5] [--no-walk] [--matches]

Cases: 128 frames of 512 x 512 and 8 frames of 2048 x 2048, each with two contents: what the tiny pipeline decodes (seeded synthetic
weights; the 2048 x 2048 frames are its 512 x 512 frames through the x4 upsampler, as ``walk(upsample=True)`` makes them) and uniform
noise (the worst case: nothing to gain, every file a little larger than raw).  GPU time: HIP events around encode() of frames already
in HBM, the copies back to pinned memory and the host CRC-32 included (encode() ends in a synchronise), plus the host clock around
the same call.  PIL: Image.fromarray(frame).save(buffer, "PNG") on FrameWriter's thread count - what the default path does after
copying the raw frames to the host; per-core time is that of one thread.  Then a 60-frame walk() of the tiny pipeline at 512 x 512 with
SDV_PNG=hip and without.  There is no fallback: without a GPU this tool fails.

--matches: the same table with, per case, the four encoder modes (Huffman-only / matches x host CRC / GPU CRC) side by side: kernel
launches per encode(), encode() time (HIP events and host clock), the deflate stage alone, file bytes per frame against PIL's; the
walk is then run a third time with SDV_PNG_MATCHES=1.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import platform
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def pil_encode(frame: np.ndarray) -> int:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format="PNG")
    return len(buf.getvalue())


def pipeline_frames(pipe, n: int, batch: int = 16) -> torch.Tensor:
    """n frames of 512 x 512 from the tiny pipeline, uint8 NHWC in GPU memory."""
    T = np.linspace(0.0, 1.0, n)
    out = []
    for _, embeds, noise in pipe.generate_inputs("a cat", "a dog", 42, 1337, (1, 4, 64, 64), T, batch):
        out.append(pipe(latents=noise, text_embeddings=embeds, height=512, width=512, num_inference_steps=4, output_type="u8_cuda")["images"].clone())
    return torch.cat(out)


def measure(name: str, dev_frames: torch.Tensor, threads: int, reps: int) -> dict:
    from PIL import Image
    from stable_diffusion_videos_amd.png import PngEncoder
    n, H, W, _ = dev_frames.shape
    enc = PngEncoder(dev_frames.device)
    files = enc.encode(dev_frames)                                               # warm-up: workspaces, code objects (and a retry, if any)
    files = enc.encode(dev_frames)
    gpu_ms, wall_ms = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        files = enc.encode(dev_frames)
        e1.record()
        e1.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        gpu_ms.append(e0.elapsed_time(e1))
    kernel_ms = []
    ws = next(iter(enc._ws.values()))
    from stable_diffusion_videos_amd import hip
    for _ in range(reps):                                                        # the launches alone: no copy, no CRC
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        e[0].record()
        hip.png_filter(dev_frames, ws["filtered"], ws["adler"])
        e[1].record()
        hip.png_deflate_pack(ws["filtered"], ws["adler"], ws["stripe_rows"], ws["header"], ws["scratch"], ws["out"], ws["meta"][:n + 1], ws["meta"][n + 1:])
        e[2].record()
        e[2].synchronize()
        kernel_ms.append((e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])))
    pinned = torch.empty(dev_frames.shape, dtype=torch.uint8, pin_memory=True)
    copy_ms = []
    for _ in range(reps):                                                        # the raw copy the PIL path needs first
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pinned.copy_(dev_frames, non_blocking=True)
        torch.cuda.synchronize()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    host = pinned.numpy()
    t0 = time.perf_counter()
    one = [pil_encode(f) for f in host[:min(n, 4)]]
    pil_core_ms = (time.perf_counter() - t0) * 1e3 / len(one)
    pil_ms = []
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for _ in range(2):
            t0 = time.perf_counter()
            sizes = list(pool.map(pil_encode, host))
            pil_ms.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[0]))), host[0]), "the GPU's file does not decode to the frame"
    med = lambda v: float(np.median(v))
    case = dict(content=name, n=n, H=H, W=W, stripe_rows=ws["stripe_rows"],
                gpu_encode_ms_events=round(med(gpu_ms), 3), gpu_encode_ms_host_clock=round(med(wall_ms), 3),
                gpu_ms_per_frame=round(med(gpu_ms) / n, 4),
                filter_kernel_ms=round(med([k[0] for k in kernel_ms]), 3), deflate_kernels_ms=round(med([k[1] for k in kernel_ms]), 3),
                pil_ms_per_frame_per_core=round(pil_core_ms, 3), pil_pool_ms=round(min(pil_ms), 3), raw_copy_ms=round(med(copy_ms), 3),
                pil_pool_ms_per_frame_incl_copy=round((min(pil_ms) + med(copy_ms)) / n, 4),
                bytes_to_host_per_frame_gpu=int(enc.last_bytes_to_host // n), bytes_to_host_per_frame_pil=H * W * 3,
                file_bytes_per_frame_gpu=int(sum(len(f) for f in files) // n), file_bytes_per_frame_pil=int(sum(sizes) // n),
                retries=enc.retries)
    case["gpu_vs_pil_pool_incl_copy"] = round(case["pil_pool_ms_per_frame_incl_copy"] / case["gpu_ms_per_frame"], 2)
    print(json.dumps(case), flush=True)
    return case


def measure_modes(dev_frames: torch.Tensor, reps: int, pil_bytes: int) -> list:
    """encode() in the four modes of PngEncoder on the same frames."""
    from stable_diffusion_videos_amd import hip
    from stable_diffusion_videos_amd.png import PngEncoder
    n = dev_frames.shape[0]
    rows = []
    for matches in (False, True):
        for gpu_crc in (False, True):
            enc = PngEncoder(dev_frames.device, matches=matches, gpu_crc=gpu_crc)
            enc.encode(dev_frames)                                               # warm-up (and the retry, if any)
            files = enc.encode(dev_frames)
            gpu_ms, wall_ms, pack_ms = [], [], []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                files = enc.encode(dev_frames)
                e1.record()
                e1.synchronize()
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                gpu_ms.append(e0.elapsed_time(e1))
            ws = next(iter(enc._ws.values()))
            for _ in range(reps):                                                # deflate (+ CRC) launches alone
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                enc._pack(ws, n, False)
                e1.record()
                e1.synchronize()
                pack_ms.append(e0.elapsed_time(e1))
            med = lambda v: float(np.median(v))
            size = int(sum(len(f) for f in files) // n)
            rows.append(dict(matches=matches, gpu_crc=gpu_crc, kernel_launches=1 + (6 if matches else 3) + (2 if gpu_crc else 0),
                             encode_ms_events=round(med(gpu_ms), 3), encode_ms_host_clock=round(med(wall_ms), 3),
                             encode_ms_per_frame=round(med(wall_ms) / n, 4), deflate_crc_kernels_ms=round(med(pack_ms), 3),
                             file_bytes_per_frame=size, file_bytes_vs_pil=round(size / pil_bytes, 3), retries=enc.retries,
                             token_scratch_bytes=int(ws["lz_scratch"].numel()) if matches else 0))
            del enc, ws
            torch.cuda.empty_cache()
    return rows


def walk_rate(pipe, png: str, frames: int = 60, matches: bool = False) -> dict:
    os.environ["SDV_PNG"] = png
    if matches:
        os.environ["SDV_PNG_MATCHES"] = "1"
    rates = []
    try:
        for rep in range(2):                                                     # the first walk pays graph capture and workspaces
            with tempfile.TemporaryDirectory() as tmp:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.walk(["a cat", "a dog"], seeds=[1, 2], num_interpolation_steps=frames, output_dir=tmp, name="w", batch_size=20,
                          num_inference_steps=4, height=512, width=512, make_video=False, image_file_ext=".png")
                rates.append(frames / (time.perf_counter() - t0))
                size = sum(f.stat().st_size for f in Path(tmp).rglob("*.png")) // frames
    finally:
        del os.environ["SDV_PNG"]
        os.environ.pop("SDV_PNG_MATCHES", None)
    case = dict(walk_frames=frames, SDV_PNG=png, SDV_PNG_MATCHES=int(matches), frames_per_sec=round(rates[-1], 2), first_walk_frames_per_sec=round(rates[0], 2),
                file_bytes_per_frame=int(size))
    print(json.dumps(case), flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-walk", action="store_true")
    ap.add_argument("--matches", action="store_true", help="also measure the matching mode and the GPU-side CRC-32")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_bench needs the GPU (no fallback)")
    from stable_diffusion_videos_amd import StableDiffusionWalkPipeline
    from stable_diffusion_videos_amd.upsampling import RealESRGANModel
    from stable_diffusion_videos_amd.utils import FrameWriter
    dev = torch.device("cuda", 0)
    writer = FrameWriter()
    threads = writer.workers
    writer.close()
    result = dict(tool="tools/png_bench.py", gpu=torch.cuda.get_device_name(0), host=platform.processor() or platform.machine(),
                  pil_threads=threads, reps=args.reps, cases=[], walks=[])
    pipe = StableDiffusionWalkPipeline.from_pretrained("tiny").to(dev)
    small = pipeline_frames(pipe, 128)
    up = RealESRGANModel.from_pretrained("nateraw/real-esrgan")
    up.to(dev)
    big = torch.cat([up.upsample_u8(small[k:k + 2]) for k in range(0, 8, 2)])
    gen = torch.Generator(device="cpu").manual_seed(0)
    for name, frames in (("tiny pipeline", small), ("uniform noise", torch.randint(0, 256, (128, 512, 512, 3), dtype=torch.uint8, generator=gen).to(dev)),
                         ("tiny pipeline x4 upsampler", big),
                         ("uniform noise", torch.randint(0, 256, (8, 2048, 2048, 3), dtype=torch.uint8, generator=gen).to(dev))):
        case = measure(name, frames.contiguous(), threads, args.reps)
        if args.matches:
            case["modes"] = measure_modes(frames.contiguous(), args.reps, case["file_bytes_per_frame_pil"])
            print(json.dumps(case["modes"]), flush=True)
        result["cases"].append(case)
    del small, big, up
    if not args.no_walk:
        for png in ("pil", "hip"):
            result["walks"].append(walk_rate(pipe, png))
        if args.matches:
            result["walks"].append(walk_rate(pipe, "hip", matches=True))
    line = json.dumps(result)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
