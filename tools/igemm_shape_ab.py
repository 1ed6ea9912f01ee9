#!/usr/bin/env python
"""Time the 256 x 320 igemm tile (tile 6, plain store epilogue, random operands) on three UNet shapes with ONE library build - the
arm of an A/B over MFMA shapes / K loops: run it once per build (SDV_HIP_LIB=... selects the other one), alternating, in the same
session; never compare against numbers of another session or device (DESIGN.md "What the hardware said").
usage: igemm_shape_ab.py [label] [reps] [launches per rep, conv]      `--pmc`: a few launches per shape only, for a rocprofv3 --pmc pass"""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from stable_diffusion_videos_amd import hip  # noqa: E402

SHAPES = (("conv 320->320 @64x64", True, 256, 64, 320, 320),        # M 1 048 576, N 320, K 2880
          ("conv 1280->1280 @16x16", True, 256, 16, 1280, 1280),    # M 65 536, N 1280, K 11 520
          ("dense 262144x640x640", False, 64, 64, 640, 640))


def main():
    pmc = "--pmc" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--pmc"]
    label = args[0] if args else "lib"
    reps = int(args[1]) if len(args) > 1 else 5
    per_rep = int(args[2]) if len(args) > 2 else 100
    dev = torch.device("cuda")
    hip.load()
    g = torch.Generator(device=dev).manual_seed(1)
    for name, conv, nimg, H, cin, cout in SHAPES:
        M, K = nimg * H * H, (9 * cin if conv else cin)
        x = (torch.randn((M, cin), device=dev, generator=g) * 0.5).to(torch.bfloat16)
        w = (torch.randn((cout, K), device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
        out = torch.empty((M, cout), dtype=torch.bfloat16, device=dev)
        fn = (lambda: hip.conv3x3(x, w, None, nimg=nimg, H=H, W=H, out=out, tile=6)) if conv else (lambda: hip.linear(x, w, None, out=out, tile=6))
        flops = 2.0 * M * K * cout
        n = per_rep if conv else 4 * per_rep
        if pmc:
            for _ in range(12):
                fn()
            torch.cuda.synchronize()
            continue
        for _ in range(n):                      # the clock the chip holds under this load, not the one it starts with
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                fn()
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e) / n)
        med = sorted(ms)[len(ms) // 2]
        print(f"{label:8s} {name:24s} us/launch " + " ".join(f"{1e3 * t:8.2f}" for t in ms) +
              f" | median {1e3 * med:8.2f} spread {100 * (max(ms) - min(ms)) / med:5.2f} % {flops / med / 1e9:7.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    main()
