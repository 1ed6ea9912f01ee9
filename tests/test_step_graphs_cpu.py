"""The denoise-step graph cache (stable_diffusion_videos_amd/step_graphs.py) without a GPU and without libsdv_hip.so: real
``StepKey`` / ``DenoiseStep`` / ``StepGraphCache`` objects on CPU tensors, with the module's two seams filled by fakes - a step
whose ``body`` only counts, and a ``cuda`` namespace whose graphs, streams and pool handles only record."""
import contextlib
import gc
import weakref
from types import SimpleNamespace

import pytest
import torch

from stable_diffusion_videos_amd.step_graphs import DenoiseStep, StepGraphCache, StepKey

UNET = SimpleNamespace(cfg=SimpleNamespace(in_channels=4))
DDIM_ROWS = torch.zeros((3, 3))
SCHED = ("DDIMScheduler", (2.0, 1.0, 0.0), 0.0, "cfg")


def key(B=1, cfg=True, **kw):
    fields = dict(schedule=SCHED, nimg=2 * B if cfg else B, h=8, w=8, cfg=cfg, guidance=7.5, stochastic=False, ctx_len=77,
                  cfg_shared_prefix=True, tiled=False)
    fields.update(kw)
    return StepKey(**fields)


class FakeCuda:
    """What ``StepGraphCache._capture`` uses of ``torch.cuda``."""

    def __init__(self):
        self.pools, self.begun, self.log = [], [], []
        self.capturing = False
        self.end_raises = None
        self.main = FakeStream(self, "main")

    def graph_pool_handle(self):
        self.pools.append(object())
        return self.pools[-1]

    def CUDAGraph(self):
        return FakeGraph(self)

    def Stream(self, device=None):
        return FakeStream(self, "side")

    def current_stream(self):
        return self.main

    @contextlib.contextmanager
    def stream(self, s):
        yield


class FakeStream:
    def __init__(self, cuda, name):
        self.cuda, self.name = cuda, name

    def wait_stream(self, other):
        self.cuda.log.append(f"{self.name} waits for {other.name}")


class FakeGraph:
    def __init__(self, cuda):
        self.cuda, self.replays = cuda, 0

    def capture_begin(self, pool, capture_error_mode):
        assert not gc.isenabled() and capture_error_mode == "global"
        self.cuda.begun.append(pool)
        self.cuda.capturing = True

    def capture_end(self):
        self.cuda.capturing = False
        if self.cuda.end_raises is not None:
            raise self.cuda.end_raises

    def replay(self):
        self.replays += 1


class FakeStep(DenoiseStep):
    """The real buffers (on the CPU) and flags; the body counts its eager and its captured executions."""

    def __init__(self, cuda, B=1, cfg=True, raises=None):
        super().__init__(UNET, B, 8, 8, cfg, cfg, 7.5, DDIM_ROWS)
        self.cuda, self.raises, self.eager, self.captured = cuda, raises, 0, 0

    def body(self):
        if self.cuda.capturing:
            self.captured += 1
            if self.raises is not None:
                raise self.raises
        else:
            self.eager += 1


@pytest.fixture
def cache():
    released = []
    c = StepGraphCache(release=released.append, cuda=FakeCuda())
    c.released = released
    return c


def put(cache, k, capture=False, **kw):
    return cache.step(k, lambda: FakeStep(cache.cuda, **kw), capture=capture)


def test_step_buffers():
    s = DenoiseStep(UNET, 3, 8, 16, True, True, 7.5, DDIM_ROWS)
    assert s.nimg == 6 and s.latents.shape == (3, 8, 16, 4) and s.x2.shape == (6 * 8 * 16, 4) and s.x2.dtype == torch.bfloat16
    assert s.step.dtype == torch.int32 and s.hist is None and s.xsave is None and s.noise is None and s.graph is None
    m = DenoiseStep(UNET, 3, 8, 16, False, False, 1.0, torch.zeros((3, 16)))
    assert m.nimg == 3 and m.hist.shape == (4, 3, 8, 16, 4) and m.xsave.shape == (3, 8, 16, 4)


def test_lru_order_and_release(cache):
    cache.bound = 2
    a, b, c, d = key(1), key(2), key(3), key(4)
    sa = put(cache, a)
    put(cache, b)
    put(cache, c)
    assert len(cache) == 2 and list(cache._steps) == [b, c] and cache.released == [a.nimg]
    assert put(cache, a) is not sa and list(cache._steps) == [c, a]           # (a was really gone)
    cache.released.clear()
    sc = cache._steps[c]
    assert put(cache, c) is sc and list(cache._steps) == [a, c]               # a hit moves to the end ...
    put(cache, d)
    assert list(cache._steps) == [c, d] and cache.released == [a.nimg]        # ... so the insert evicts a, not c


def test_release_only_for_sizes_left_without_a_step(cache):
    cache.bound = 2
    put(cache, key(2))
    put(cache, key(2, guidance=3.0))
    put(cache, key(3))                                      # evicts key(2); guidance 3.0 still runs at 4 samples
    assert cache.released == []
    put(cache, key(5))                                      # evicts the other 4-sample step
    assert cache.released == [4]


def test_never_releases_the_size_about_to_run(cache):
    cache.bound = 1
    put(cache, key(2))
    put(cache, key(2, guidance=3.0))                        # same batch size: prepare_context has already filled its buffers
    assert cache.released == [] and len(cache) == 1
    cache.evict(key(2, guidance=3.0), running=4)
    assert cache.released == []
    put(cache, key(2))
    cache.evict(key(2), running=6)
    assert cache.released == [4]


def test_drop_schedule(cache):
    other = ("DDIMScheduler", (1.0, 0.0), 0.0, "cfg")
    put(cache, key(1))
    put(cache, key(2))
    put(cache, key(2, schedule=other))
    put(cache, key(3, schedule=other))
    cache.drop_schedule(other)
    assert list(cache._steps) == [key(1), key(2)] and cache.released == [6]  # 4 samples still has a step
    cache.drop_schedule(("never", (), 0.0, ""))
    assert len(cache) == 2 and cache.released == [6]


def test_clear_releases_every_size_once(cache):
    for k in (key(1), key(2), key(2, guidance=3.0)):
        put(cache, k)
    cache.clear()
    assert len(cache) == 0 and sorted(cache.released) == [2, 4]


def test_pipeline_surface_on_the_cache():
    """``_drop_graphs``, ``max_cached_graphs``, ``last_graph_build`` and ``_schedule``'s bound of 8 go through the one cache."""
    from stable_diffusion_videos_amd import DDIMScheduler, StableDiffusionWalkPipeline
    released = []
    unet = SimpleNamespace(release=released.append, prepare_timesteps=lambda ts: None, res=[])
    pipe = StableDiffusionWalkPipeline(vae=SimpleNamespace(config=SimpleNamespace(block_out_channels=(32, 64))), text_encoder=None,
                                       tokenizer=None, unet=unet, scheduler=DDIMScheduler())
    cache = pipe._graphs
    cache.cuda = FakeCuda()
    assert pipe.max_cached_graphs == cache.bound == 4 and pipe.last_graph_build == {}
    pipe.max_cached_graphs = 2
    for B in (1, 2, 3):
        put(cache, key(B))
    assert len(pipe._graphs) == 2 and released == [2]
    pipe._drop_graphs()
    assert len(pipe._graphs) == 0 and sorted(released) == [2, 4, 6]
    # the ninth schedule pushes out the first: its steps go, and the batch sizes only they ran at are released
    pipe.max_cached_graphs = 4
    del released[:]
    keys = [pipe._schedule(n, 0.0)[0] for n in range(1, 9)]
    put(cache, key(1, schedule=keys[0]))
    put(cache, key(2, schedule=keys[0]))
    put(cache, key(2, schedule=keys[1]))
    assert pipe._schedule(3, 0.0)[0] == keys[2] and len(cache) == 3
    pipe._schedule(9, 0.0)
    assert list(cache._steps) == [key(2, schedule=keys[1])] and released == [2] and len(pipe._sched_cache) == 8


def test_capture_after_the_first_eager_step_then_replay(cache):
    s = put(cache, key(1), capture=True)
    assert s.capture_pending and s.graph is None
    cache.run(s)
    assert (s.eager, s.captured) == (1, 1) and s.graph is not None and not s.capture_pending
    assert cache.cuda.log == ["side waits for main", "main waits for side"] and gc.isenabled()
    assert set(cache.last_build) == {"capture_s"}
    cache.run(s)
    cache.run(s)
    assert (s.eager, s.captured, s.graph.replays) == (1, 1, 2) and len(cache.cuda.begun) == 1


def test_graphs_off_never_captures_and_on_again_captures(cache):
    s = put(cache, key(1), capture=False)
    for _ in range(3):
        cache.run(s)
    assert (s.eager, s.captured) == (3, 0) and s.graph is None and cache.cuda.begun == []
    assert put(cache, key(1), capture=False) is s and not s.capture_pending
    assert put(cache, key(1), capture=True) is s and s.capture_pending
    cache.run(s)
    cache.run(s)
    assert (s.eager, s.captured, s.graph.replays) == (4, 1, 1)
    assert put(cache, key(1), capture=False) is s and s.graph is not None     # (a captured step keeps replaying)


def test_failed_capture_keeps_the_first_error_and_is_not_retried(cache):
    first, second = RuntimeError("launch failed during capture"), RuntimeError("capture_end on a broken capture")
    cache.cuda.end_raises = second
    s = put(cache, key(1), capture=True, raises=first)
    with pytest.raises(RuntimeError) as info:
        cache.run(s)
    assert info.value is first
    assert s.capture_failed and not s.capture_pending and s.graph is None and gc.isenabled()
    assert cache.cuda.log[-1] == "main waits for side"
    assert put(cache, key(1), capture=True) is s and not s.capture_pending
    cache.run(s)
    cache.run(s)
    assert (s.eager, s.captured) == (3, 1) and s.graph is None
    # capture_end alone failing is reported too
    t = put(cache, key(2), capture=True)
    with pytest.raises(RuntimeError) as info:
        cache.run(t)
    assert info.value is second and t.capture_failed


def test_pool_handle_lives_as_long_as_one_graph_does(cache):
    a, b = put(cache, key(1), capture=True), put(cache, key(2), capture=True)
    cache.run(a)
    cache.run(b)
    cuda = cache.cuda
    assert len(cuda.pools) == 1 and cuda.begun == [cuda.pools[0]] * 2
    cache.evict(key(1))
    cache.run(put(cache, key(3), capture=True))             # b still holds a graph in the pool
    assert len(cuda.pools) == 1 and cuda.begun[-1] is cuda.pools[0]
    cache.clear()
    cache.run(put(cache, key(1), capture=True))
    assert len(cuda.pools) == 2 and cuda.begun[-1] is cuda.pools[1]
    # an entry that runs eagerly does not keep the pool alive
    cache.clear()
    put(cache, key(2), capture=False)
    cache.run(put(cache, key(1), capture=True))
    assert len(cuda.pools) == 3 and cuda.begun[-1] is cuda.pools[2]


def test_ragged_lookup(cache):
    put(cache, key(4))
    assert cache.padded_batch(key(3), 3) == 4
    assert cache.padded_batch(key(2), 2) is None            # a pad of 2 is more than a quarter of 4
    assert cache.padded_batch(key(4), 4) is None and cache.padded_batch(key(5), 5) is None
    put(cache, key(8))
    assert cache.padded_batch(key(3), 3) == 4               # the smallest that fits
    assert cache.padded_batch(key(6), 6) == 8 and cache.padded_batch(key(7), 7) == 8
    put(cache, key(3))
    assert cache.padded_batch(key(3), 3) is None            # an exact step is cached
    assert list(cache._steps) == [key(4), key(8), key(3)]   # (asking moves nothing)


def test_ragged_lookup_without_cfg(cache):
    put(cache, key(4, cfg=False))
    assert cache.padded_batch(key(3, cfg=False), 3) == 4 and cache.padded_batch(key(3), 3) is None


@pytest.mark.parametrize("field, other", [
    ("h", 16), ("w", 16), ("cfg", False), ("guidance", 3.0), ("stochastic", True), ("ctx_len", 154),
    ("cfg_shared_prefix", False), ("tiled", True), ("schedule", ("DDIMScheduler", (1.0, 0.0), 0.0, "cfg"))])
def test_ragged_lookup_needs_every_other_field_equal(cache, field, other):
    assert field in StepKey._fields
    put(cache, key(4)._replace(**{field: other}))
    assert cache.padded_batch(key(3), 3) is None
    put(cache, key(4))
    assert cache.padded_batch(key(3), 3) == 4


def test_evicted_step_is_freed_by_reference_count_alone(cache):
    was_on = gc.isenabled()
    gc.disable()
    try:
        s = put(cache, key(1), capture=True)
        cache.run(s)
        cache.run(s)
        ref, graph = weakref.ref(s), weakref.ref(s.graph)
        del s
        assert ref() is not None
        cache.evict(key(1))
        assert ref() is None and graph() is None
    finally:
        if was_on:
            gc.enable()
