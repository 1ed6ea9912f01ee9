"""The denoise step as the pipeline runs it: static buffers + ONE hipGraph of (UNet forward + CFG / scheduler update + step++),
and the cache that decides which captured step a call replays, when a step is captured and when a step - and the per-batch-size
cross-attention buffers it points into - is freed.

    StepKey         everything a captured step bakes in, by name
    DenoiseStep     the static buffers, the eager body, the graph (None while the step runs eagerly) and the two capture flags
    StepGraphCache  LRU order + bound, the shared private pool, capture, the ragged-batch lookup and the ONE eviction routine

Of the package it uses ``hip`` (the step body's three launches; the library is only loaded on first use, not at import) and
``parallel.world()``.  Two seams for the CPU tests (tests/test_step_graphs_cpu.py): a step's ``body`` and the ``cuda`` namespace
the capture goes through.
"""
from __future__ import annotations

import gc
import time
from typing import Callable, Dict, NamedTuple, Optional

import torch

from . import hip, parallel

F32 = torch.float32
BF16 = torch.bfloat16


class StepKey(NamedTuple):
    """Everything a captured step bakes in: the pointers of the schedule's coefficient / time-embedding tables and of the
    (nimg, ctx_len) cross-attention K / V^T buffers, the shared-prefix structure, padding mode, guidance scale."""
    schedule: tuple
    nimg: int
    h: int
    w: int
    cfg: bool
    guidance: float
    stochastic: bool
    ctx_len: int
    cfg_shared_prefix: bool
    tiled: bool


class DenoiseStep:
    """Static buffers of ONE denoise step at ``B`` frames and its eager body.  Holds the engine, not the pipeline or the cache:
    nothing points back at a step, so dropping the last reference frees the buffers (and the graph) at once."""

    def __init__(self, unet, B: int, h: int, w: int, cfg: bool, cfg_shared: bool, guidance: float, coefs, noise=None):
        dev, C = coefs.device, unet.cfg.in_channels
        self.unet, self.h, self.w, self.cfg, self.cfg_shared, self.guidance = unet, h, w, cfg, cfg_shared, guidance
        self.nimg = 2 * B if cfg else B
        self.coefs, self.noise = coefs, noise                  # noise: [evaluation, B, h, w, C] of a stochastic scheduler / eta > 0
        self.latents = torch.zeros((B, h, w, C), dtype=F32, device=dev)
        self.x2 = torch.zeros((self.nimg * h * w, C), dtype=BF16, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hist = self.xsave = None
        if coefs.shape[1] == 16:                               # sdv_cfg_multistep_step rows (every scheduler but DDIM)
            self.hist = torch.zeros((4, B, h, w, C), dtype=F32, device=dev)       # ring of earlier model outputs
            self.xsave = torch.zeros((B, h, w, C), dtype=F32, device=dev)         # PLMS: the sample of the first evaluation
        self.graph = None
        self.capture_pending = self.capture_failed = False

    def body(self):
        eps = self.unet.forward(self.x2, self.nimg, self.h, self.w, self.step, cfg_shared=self.cfg_shared)
        n = self.latents.numel()
        if self.hist is not None:
            hip.cfg_multistep_step(eps, self.latents, self.x2, self.hist, self.xsave, self.coefs, self.step, self.noise,
                                   self.guidance, self.cfg, n)
        else:
            hip.cfg_ddim_step(eps, self.latents, self.x2, self.coefs, self.step, self.noise, self.guidance, self.cfg, n)
        hip.step_counter_add(self.step, 1)


class StepGraphCache:
    """Denoise steps by ``StepKey``, most recently used last.  ``release(nimg)`` frees the engine's per-batch-size buffers."""

    def __init__(self, release: Optional[Callable[[int], None]] = None, cuda=torch.cuda):
        self.release, self.cuda = release, cuda
        self.bound = 4                     # LRU bound on cached steps (all share ONE private pool, which only shrinks when every graph is dropped)
        self.last_build: Dict[str, float] = {}
        self._steps: Dict[StepKey, DenoiseStep] = {}
        self._pool = None                  # the private memory pool every captured step allocates from (see _capture)

    def __len__(self):
        return len(self._steps)

    def __iter__(self):
        """The cached steps, most recently used last."""
        return iter(self._steps.values())

    def holds(self, nimg: int) -> bool:
        return any(k.nimg == nimg for k in self._steps)

    def step(self, key: StepKey, make: Callable[[], DenoiseStep], capture: bool) -> DenoiseStep:
        """The step of ``key``, built by ``make()`` on a miss (after the LRU made room for it)."""
        step = self._steps.pop(key, None)
        if step is None:
            while len(self._steps) >= self.bound:              # bound the static buffers + cross-attention K / V^T sets kept alive
                self.evict(next(iter(self._steps)), running=key.nimg)
            step = make()
            # The step is captured right AFTER its first eager execution - which is the first REAL denoise step of the first call
            # at this key (lazy allocations / attribute sets happen there), not a throw-away warm-up on zero-filled buffers.
            step.capture_pending = capture
        elif capture and step.graph is None and not step.capture_failed:
            # a step made while graphs were off is captured behind its next eager step once they are on again - otherwise it would
            # run eagerly for ever; one whose capture failed is not tried again
            step.capture_pending = True
        self._steps[key] = step                                # most recently used last
        return step

    def run(self, step: DenoiseStep):
        if step.graph is not None:
            step.graph.replay()
        else:
            step.body()
            if step.capture_pending:
                self._capture(step)

    def padded_batch(self, key: StepKey, B: int) -> Optional[int]:
        """A ragged last batch (``B`` frames, ``key``) may replay a cached step that differs from ``key`` in nothing but a larger
        batch, padded with copies of its last frame: a second capture would own a second multi-GB private pool for one call.
        The smallest such step, and only while the padding is at most a quarter of it - 60 frames replayed as 128 would pay for
        128 - and no step of the exact size is cached.  Returns that step's frame count, or None."""
        if key in self._steps:
            return None
        mult = key.nimg // B
        bigger = [k.nimg // mult for k in self._steps if k.nimg > key.nimg and k._replace(nimg=key.nimg) == key]
        if bigger and 4 * (min(bigger) - B) <= min(bigger):
            return min(bigger)
        return None

    # -- the one eviction path -----------------------------------------------------------------
    def evict(self, key: StepKey, running: Optional[int] = None):
        """Drop the step of ``key``.  The cross-attention K / V^T buffers of the text context are kept per batch size because
        captured graphs hold raw pointers into them: once no cached step runs at that batch size any more they go too (a resumed
        walk with many short runs would otherwise leave one set per distinct batch size behind) - except at ``running``, the
        size the caller is about to run, whose buffers ``prepare_context`` has already filled."""
        del self._steps[key]
        if key.nimg != running and not self.holds(key.nimg):
            self.release(key.nimg)

    def drop_schedule(self, schedule: tuple):
        """Captured steps bake in the pointers of their schedule's coefficient / time-embedding tables."""
        for key in [k for k in self._steps if k.schedule == schedule]:
            self.evict(key)

    def clear(self):
        for key in list(self._steps):
            self.evict(key)

    # -- capture ---------------------------------------------------------------------------------
    def _capture(self, step: DenoiseStep):
        """Capture ``step``'s body into a hipGraph (nothing executes: the static buffers keep the state the eager step
        left).  Not through the ``torch.cuda.graph`` context manager: its ``__enter__`` runs ``torch.cuda.empty_cache()``, which
        hands every cached block of the allocator back to the driver - 0.9 s for a 16-frame capture that followed a 60-frame call,
        1.7 s of the 2.15 s "cold start" the round-4 bench line showed (profiles/round5_cold_start_probe_before.txt); the capture
        itself is 14 ms.  All captured steps share ONE private memory pool: their intermediates are dead when a replay ends and
        two steps never run concurrently, so a new batch size costs the pool only what it needs beyond the largest so far."""
        t0 = time.perf_counter()
        cuda = self.cuda
        # The shared pool lives as long as one graph captured into it does: once every captured step has been dropped (fp8 counter
        # switch, LRU eviction of the last one, a caller clearing the cache) PyTorch forgets the pool, and capturing into the stale
        # handle trips an internal assert of its caching allocator.
        if self._pool is None or not any(s.graph is not None for s in self._steps.values()):
            self._pool = cuda.graph_pool_handle()
        g = cuda.CUDAGraph()
        # with a process group alive its watchdog thread may touch the runtime while this thread captures: only this
        # thread's calls (kernel launches through the C ABI) need to be capture-safe
        mode = "thread_local" if parallel.world()[1] > 1 else "global"
        side = cuda.Stream(device=step.latents.device)
        side.wait_stream(cuda.current_stream())
        # No garbage collection while the stream captures: an unreachable graph the collector finds (steps themselves are freed by
        # reference count, a caller's objects may not be) would be destroyed in the middle of the capture, and destroying a graph /
        # returning its blocks is not a capturable call (seen as a crash inside the first captured launch late in a long test
        # session; ``torch.cuda.graph`` runs a full ``gc.collect()`` up front for the same reason - switching the collector off
        # for the ~10 ms of the capture costs nothing).
        gc_was_on = gc.isenabled()
        gc.disable()
        step.capture_pending = False            # whatever happens below, the capture is not retried on every following step
        err = None
        try:
            with cuda.stream(side):
                g.capture_begin(pool=self._pool, capture_error_mode=mode)
                try:
                    step.body()
                except BaseException as e:      # keep the ORIGINAL error: capture_end() on a broken capture raises one of its own
                    err = e
                try:
                    g.capture_end()
                except BaseException as e:
                    if err is None:
                        err = e
        finally:
            if gc_was_on:
                gc.enable()
            cuda.current_stream().wait_stream(side)
        if err is not None:
            step.capture_failed = True          # this step keeps running eagerly
            raise err
        step.graph = g
        self.last_build = {"capture_s": time.perf_counter() - t0}
