#!/usr/bin/env python
"""Generator of tests/golden/launch_trace.json: the launch trace (tests/launch_trace.py) of every transformer-block case and every
whole-UNet case, on the meta device - no GPU, no shared library.

    python tests/golden/make_golden_launch_trace.py        # rewrites tests/golden/launch_trace.json (deterministic)

Regenerate it only with a change that is MEANT to alter which kernels run or what they are handed, and read the diff of the file:
every changed hash is a launch whose arguments changed.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent.parent), str(HERE.parent)]

import launch_trace as lt  # noqa: E402
from stable_diffusion_videos_amd import hip  # noqa: E402


def build():
    hip.load = lambda *a, **k: None              # the meta device needs no library
    out = {}
    for name in lt.block_case_names():
        saved = []

        def setattr_(obj, attr, value):
            saved.append((obj, attr, getattr(obj, attr)))
            setattr(obj, attr, value)
        try:
            out["block/" + name] = lt.digest(lt.trace_block_case(name, setattr_))
        finally:
            for obj, attr, value in saved:
                setattr(obj, attr, value)
    for arch, sizes in lt.ENGINES.items():
        engine = lt.build_engine(arch, "meta")
        for size in sizes:
            out["unet/" + lt.engine_case_name(arch, size)] = lt.digest(lt.trace_engine(engine, *size))
    return out


if __name__ == "__main__":
    fx = build()
    with open(lt.GOLDEN_FILE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in fx.items()) + "\n}\n")
    print(f"wrote {lt.GOLDEN_FILE} ({lt.GOLDEN_FILE.stat().st_size >> 10} KiB, {len(fx)} cases, "
          f"{sum(len(v['ops']) for v in fx.values())} ops)")
