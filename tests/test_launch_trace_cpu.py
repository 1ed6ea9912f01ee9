"""Which kernel the UNet's transformer block picks at which size, and what it hands it: the launch traces of tests/launch_trace.py
on the meta device against tests/golden/launch_trace.json (regenerate: tests/golden/make_golden_launch_trace.py).  The block cases
sit on both sides of every threshold of the panel-or-igemm policy (hip.PANEL_MIN_ROWS_*, hip.FORCE_TILE, the A/B knobs); the
whole-engine cases add the CFG-shared prefix and the cache-blocked forward, in bf16 and with the fp8 ResBlock convs, the VAE decode
with its chunked mid-block attention, and the CLIP text and vision calls."""
import json

import pytest

import launch_trace as lt


@pytest.fixture(scope="module")
def golden():
    return json.loads(lt.GOLDEN_FILE.read_text())


@pytest.fixture(scope="module")
def meta_engines():
    """Built once per module, on first use; ``hip.load`` is patched out only while one is built."""
    built = {}

    def get(arch, **kw):
        key = (arch, tuple(sorted(kw)))
        if key not in built:
            with lt.on_meta():
                built[key] = lt.build_engine(arch, "meta", **kw)
        return built[key]
    return get


def test_golden_holds_exactly_these_cases(golden):
    names = ["block/" + n for n in lt.block_case_names()]
    names += ["unet/" + lt.engine_case_name(a, s) for a, sizes in lt.ENGINES.items() for s in sizes]
    names += ["unet/" + lt.engine_case_name(*lt.TILED) + "_tiled"]
    names += ["unet_fp8/" + lt.engine_case_name(a, s) for a, sizes in lt.FP8_ENGINES.items() for s in sizes]
    names += ["unet_fp8/" + lt.engine_case_name(*lt.FP8_CALIBRATING) + "_calibrating"]
    names += [f"vae/{a}_{n}" for a in lt.VAE_CONFIGS for n in lt.VAE_CASES]
    names += ["clip_call/" + n for n in lt.CLIP_CALLS]
    assert sorted(golden) == sorted(names)


@pytest.mark.parametrize("name", lt.block_case_names())
def test_block_launch_trace(golden, monkeypatch, name):
    diff = lt.first_difference(lt.trace_block_case(name, monkeypatch.setattr), golden["block/" + name])
    assert diff is None, diff


@pytest.mark.parametrize("arch,size", [(a, s) for a, sizes in lt.ENGINES.items() for s in sizes],
                         ids=[lt.engine_case_name(a, s) for a, sizes in lt.ENGINES.items() for s in sizes])
def test_unet_launch_trace(golden, meta_engines, arch, size):
    diff = lt.first_difference(lt.trace_engine(meta_engines(arch), *size), golden["unet/" + lt.engine_case_name(arch, size)])
    assert diff is None, diff


def test_tiled_unet_launch_trace(golden, meta_engines):
    arch, size = lt.TILED
    want = golden["unet/" + lt.engine_case_name(arch, size) + "_tiled"]
    diff = lt.first_difference(lt.trace_engine(meta_engines(arch, tiled=True), *size), want)
    assert diff is None, diff


@pytest.mark.parametrize("arch,size", [(a, s) for a, sizes in lt.FP8_ENGINES.items() for s in sizes],
                         ids=[lt.engine_case_name(a, s) for a, sizes in lt.FP8_ENGINES.items() for s in sizes])
def test_fp8_unet_launch_trace(golden, meta_engines, arch, size):
    want = golden["unet_fp8/" + lt.engine_case_name(arch, size)]
    diff = lt.first_difference(lt.trace_engine(meta_engines(arch, fp8=True), *size), want)
    assert diff is None, diff


def test_fp8_calibrating_unet_launch_trace(golden):
    """While the scales are calibrated every norm of a ResBlock runs twice: in bf16 for the scale, then in e4m3 with it."""
    arch, size = lt.FP8_CALIBRATING
    with lt.on_meta():
        trace = lt.trace_engine_calibrating(arch, size)
    diff = lt.first_difference(trace, golden["unet_fp8/" + lt.engine_case_name(arch, size) + "_calibrating"])
    assert diff is None, diff
    fixed = golden["unet_fp8/" + lt.engine_case_name(arch, size)]["ops"]
    nres = 4 * 2 + 2 + 4 * 3                   # ResBlocks of the 4-level topology: down, mid, up
    assert [n for n, _ in trace].count("k_groupnorm") == fixed.count("k_groupnorm") + 2 * nres


@pytest.mark.parametrize("arch", list(lt.VAE_CONFIGS))
@pytest.mark.parametrize("case", list(lt.VAE_CASES))
def test_vae_launch_trace(golden, arch, case):
    nimg, side, want_float, per_chunk, tiled = lt.VAE_CASES[case]
    with lt.on_meta():
        engine = lt.build_vae(arch, "meta", tiled=tiled)
    diff = lt.first_difference(lt.trace_vae(engine, nimg, side, want_float, per_chunk), golden[f"vae/{arch}_{case}"])
    assert diff is None, diff


@pytest.mark.parametrize("name", list(lt.CLIP_CALLS))
def test_clip_launches_on_meta_are_those_of_the_recorded_call(golden, name):
    """The ``clip_call/*`` entries were recorded on the device, where the engines' host-side checks add ``aten`` ops; every launch
    and its arguments must be the recorded ones."""
    with lt.on_meta():
        got = lt.sdv_ops(lt.digest(lt.trace_clip_on_meta(name)))
    want = lt.sdv_ops(golden["clip_call/" + name])
    assert len(want) >= 14
    diff = next((f"launch {i}: expected {w}, got {g}" for i, (g, w) in enumerate(zip(got, want)) if g != w), None)
    assert diff is None and len(got) == len(want), diff or f"{len(got)} launches, expected {len(want)}"
