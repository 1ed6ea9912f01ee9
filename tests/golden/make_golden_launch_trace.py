#!/usr/bin/env python
"""Generator of tests/golden/launch_trace.json: the launch trace (tests/launch_trace.py) of every transformer-block case and every
whole-UNet and VAE-decode case, on the meta device - no GPU, no shared library - and of the whole CLIP text / vision calls, which
only a GPU can run.

    python tests/golden/make_golden_launch_trace.py        # rewrites the meta cases (deterministic), keeps the clip_call/* entries
    python tests/golden/make_golden_launch_trace.py cuda   # records the clip_call/* entries on that device as well

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


def build_meta():
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
    arch, size = lt.TILED
    out["unet/" + lt.engine_case_name(arch, size) + "_tiled"] = lt.digest(lt.trace_engine(lt.build_engine(arch, "meta", tiled=True), *size))
    for arch, sizes in lt.FP8_ENGINES.items():
        engine = lt.build_engine(arch, "meta", fp8=True)
        for size in sizes:
            out["unet_fp8/" + lt.engine_case_name(arch, size)] = lt.digest(lt.trace_engine(engine, *size))
    arch, size = lt.FP8_CALIBRATING
    out["unet_fp8/" + lt.engine_case_name(arch, size) + "_calibrating"] = lt.digest(lt.trace_engine_calibrating(arch, size))
    for arch in lt.VAE_CONFIGS:
        for name, (nimg, side, want_float, per_chunk, tiled) in lt.VAE_CASES.items():
            out[f"vae/{arch}_{name}"] = lt.digest(lt.trace_vae(lt.build_vae(arch, "meta", tiled=tiled), nimg, side, want_float, per_chunk))
    return out


if __name__ == "__main__":
    with lt.on_meta():
        fx = build_meta()
    if len(sys.argv) > 1:
        fx.update(("clip_call/" + name, lt.digest(lt.trace_clip_call(name, sys.argv[1]))) for name in lt.CLIP_CALLS)
    else:
        fx.update((k, v) for k, v in json.loads(lt.GOLDEN_FILE.read_text()).items() if k.startswith("clip_call/"))
    with open(lt.GOLDEN_FILE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in fx.items()) + "\n}\n")
    print(f"wrote {lt.GOLDEN_FILE} ({lt.GOLDEN_FILE.stat().st_size >> 10} KiB, {len(fx)} cases, "
          f"{sum(len(v['ops']) for v in fx.values())} ops)")
