"""Which kernel the UNet's transformer block picks at which size, and what it hands it: the launch traces of tests/launch_trace.py
on the meta device against tests/golden/launch_trace.json (regenerate: tests/golden/make_golden_launch_trace.py).  The block cases
sit on both sides of every threshold of the panel-or-igemm policy (hip.PANEL_MIN_ROWS_*, hip.FORCE_TILE, the A/B knobs); the
whole-engine cases add the CFG-shared prefix and the cache-blocked forward."""
import json

import pytest

import launch_trace as lt
from stable_diffusion_videos_amd import hip


@pytest.fixture(scope="module")
def golden():
    return json.loads(lt.GOLDEN_FILE.read_text())


@pytest.fixture(scope="module")
def meta_engines():
    """Built once per module, on first use; ``hip.load`` is patched out only while one is built."""
    built = {}

    def get(arch):
        if arch not in built:
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(hip, "load", lambda *a, **k: None)
                built[arch] = lt.build_engine(arch, "meta")
        return built[arch]
    return get


def test_golden_holds_exactly_these_cases(golden):
    names = ["block/" + n for n in lt.block_case_names()]
    names += ["unet/" + lt.engine_case_name(a, s) for a, sizes in lt.ENGINES.items() for s in sizes]
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
