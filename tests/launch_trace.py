"""Launch traces of the UNet's transformer block and of whole engine calls (UNet forward in bf16 and fp8, VAE decode, CLIP text and
vision): WHICH kernel runs, with which operands, at which size.

Every launch of the hot path is a ``torch.ops.sdv.k_*`` op with a Meta kernel, so an engine built with ``device="meta"`` runs its
forward without a GPU and without the shared library, and a ``TorchDispatchMode`` sees every op it dispatches.  The trace of a case
is the list of those ops: an ``sdv`` op with a canonical description of all its arguments (dtype / shape / stride / storage offset of
every tensor, every integer, every float bit for bit), any other op by name - a ``copy_`` or ``cat`` that a change of the engine
adds shows up like a changed launch does.  tests/golden/launch_trace.json holds, per case, the op names and a short hash of each
launch's description (tests/golden/make_golden_launch_trace.py writes it, tests/test_launch_trace_cpu.py compares; one case per
engine runs again on the device, tests/test_model_gpu.py).  The CLIP engines check their inputs on the host before they launch
anything, which a meta tensor cannot answer: their ``clip_call/*`` entries are recorded on the device, and the meta device runs the
part behind those checks, whose ``sdv`` ops must be the entry's (``sdv_ops``).

What the trace cannot see: WHICH tensor of a given dtype and shape an operand is - two same-shaped weights swapped leave it
unchanged; the block-wise parity tests on the GPU catch that."""
from __future__ import annotations

import contextlib
import hashlib
import json
import os
from collections import OrderedDict
from pathlib import Path

import torch
from torch.utils._python_dispatch import TorchDispatchMode

from stable_diffusion_videos_amd import config as cfgs
from stable_diffusion_videos_amd import engine as eng_mod
from stable_diffusion_videos_amd import hip, text, vision, weights

GOLDEN_FILE = Path(__file__).resolve().parent / "golden" / "launch_trace.json"
BF16 = torch.bfloat16
LC = 77

# Ops that move no data and start no kernel: allocations and pure views.  Everything else is recorded.
SKIP = frozenset({"aten::empty", "aten::empty_like", "aten::empty_strided", "aten::new_empty", "aten::new_empty_strided",
                  "aten::view", "aten::_unsafe_view", "aten::reshape", "aten::slice", "aten::select", "aten::as_strided",
                  "aten::alias", "aten::detach", "aten::permute", "aten::transpose", "aten::t", "aten::expand", "aten::unsqueeze",
                  "aten::squeeze"})


def _describe(a):
    if isinstance(a, torch.Tensor):
        return ["T", str(a.dtype), list(a.shape), list(a.stride()), a.storage_offset()]
    if isinstance(a, bool) or a is None or isinstance(a, int):
        return a
    if isinstance(a, float):
        return a.hex()
    if isinstance(a, (list, tuple)):
        return [_describe(v) for v in a]
    raise TypeError(f"launch trace: no canonical form for an argument of type {type(a).__name__}")


class Recorder(TorchDispatchMode):
    """``trace``: one (op name, argument description or None) per dispatched op that is not in ``SKIP``."""

    def __init__(self):
        super().__init__()
        self.trace = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = func._schema.name
        if name.startswith("sdv::"):
            self.trace.append((name[5:], [_describe(a) for a in args] + [[k, _describe(v)] for k, v in sorted(kwargs.items())]))
        elif name not in SKIP:
            self.trace.append((name, None))
        return func(*args, **kwargs)


def digest(trace):
    """The form the golden file holds: op names, and per op the hash of its description (None for an op recorded by name only)."""
    return {"ops": [n for n, _ in trace],
            "args": [None if d is None else hashlib.sha1(json.dumps(d).encode()).hexdigest()[:10] for _, d in trace]}


def first_difference(trace, want):
    """None when ``trace`` is what the golden entry ``want`` describes, else a message with the first differing op."""
    got = digest(trace)
    n = min(len(trace), len(want["ops"]))
    for i in range(n):
        if got["ops"][i] != want["ops"][i] or got["args"][i] != want["args"][i]:
            return (f"op {i}: expected {want['ops'][i]} {want['args'][i]}, got {got['ops'][i]} {got['args'][i]}\n"
                    f"  now: {json.dumps(trace[i][1])}")
    if len(trace) != len(want["ops"]):
        more = trace[n][0] if len(trace) > n else want["ops"][n]
        return f"{len(trace)} ops, expected {len(want['ops'])}: the first {n} agree, then comes {more}"
    return None


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
# one transformer block: name -> (C, heads, side, nimg, shared prefix); rows of the whole call M = nimg * side^2
BLOCKS = OrderedDict([
    ("c320_s16_n2", (320, 8, 16, 2, False)),               # M 512: V^T form, feed-forward as two launches
    ("c320_s16_n2_shared", (320, 8, 16, 2, True)),
    ("c320_s6_n2", (320, 8, 6, 2, False)),                 # M 72: HW % 128 != 0, row-major [Q | K | V]
    ("c320_s64_n4_shared", (320, 8, 64, 4, True)),         # M 16384: exactly hip.PANEL_MIN_ROWS_FFN
    ("c320_s64_n3", (320, 8, 64, 3, False)),               # M 12288: just below it
    ("c640_s8_n2_shared", (640, 8, 8, 2, True)),           # M 128: all igemm, the batch-2 stride-0 launches
    ("c640_s32_n8", (640, 8, 32, 8, False)),               # M 8192: proj_in and attn2.to_q on the panel, Q K V on the igemm
    ("c640_s64_n8", (640, 8, 64, 8, False)),               # M 32768: all three on the panel
    ("c1280_s4_n2", (1280, 8, 4, 2, False)),               # M 32: igemm only
])
FORCED = ("c320_s16_n2", "c640_s8_n2_shared")                                  # again with hip.FORCE_TILE = 6
KNOBS_OFF = OrderedDict([("c320_s64_n4_shared", ("LINEAR320", "FFN_FUSED", "QKV_VT")),      # one knob off, set before construction
                         ("c640_s64_n8", ("LINEAR320", "LINEAR640"))])
CHUNKED = "c320_s16_chunk_2_of_4"                          # images [2, 4) of a 4-image batch: out= and ctx_of=(4, 2)

# a whole UNetEngine.forward: (nimg, side, cfg_shared, SDV_CHUNK_ROWS)
ENGINE_SIZES = ((2, 16, False, 0), (4, 16, True, 0), (6, 16, True, 512), (8, 64, True, 0))
ENGINES = OrderedDict([("tiny", ENGINE_SIZES), ("sd14", ENGINE_SIZES), ("sd21", ENGINE_SIZES[3:])])
UNET_CONFIGS = {"tiny": cfgs.tiny_unet, "sd14": cfgs.sd14_unet, "sd21": cfgs.sd21_unet}
TILED = ("tiny", ENGINE_SIZES[1])                          # unet/<case>_tiled: circular padding in every conv
# an fp8 UNetEngine with fixed scales (``on_meta`` stands in for the weight quantiser), and one forward that calibrates
FP8_ENGINES = OrderedDict([("tiny", ENGINE_SIZES[1:3]), ("sd14", ENGINE_SIZES[1:3])])
FP8_CALIBRATING = ("tiny", ENGINE_SIZES[1])                # unet_fp8/<case>_calibrating: one more bf16 GroupNorm per norm

# VAEDecoderEngine.decode: (images, latent side, want_float, images per score chunk of the mid-block attention or 0, tiled)
VAE_CONFIGS = {"tiny_vae": cfgs.tiny_vae, "sd_vae": cfgs.sd_vae}
VAE_CASES = OrderedDict([("n1_s8", (1, 8, False, 0, False)),
                         ("n3_s16_float", (3, 16, True, 0, False)),
                         ("n3_s16_scorechunk2", (3, 16, False, 2, False)),      # chunks of 2 + 1 images: x_off / w_off / out_off
                         ("n1_s8_tiled", (1, 8, False, 0, True))])

# a whole text_encoder(ids) at L = 77 / vision(patches, n) call: (engine kind, config, batch)
CLIP_CALLS = OrderedDict([("tiny_text_b2", ("text", cfgs.tiny_text, 2)),
                          ("sd14_text_b1", ("text", cfgs.sd14_text, 1)),
                          ("tiny_vision_n2", ("vision", cfgs.tiny_vision, 2))])


def engine_case_name(arch, size):
    nimg, side, shared, chunk = size
    return f"{arch}_n{nimg}_s{side}" + ("_shared" if shared else "") + (f"_chunk{chunk}" if chunk else "")


def _meta_state_dict(shapes):
    sd = OrderedDict((k, torch.empty(s, device="meta")) for k, s in shapes.items())
    for k in ("conv_in.weight", "decoder.conv_in.weight", "embeddings.patch_embedding.weight"):        # (padded on the host)
        if k in sd:
            sd[k] = torch.zeros(shapes[k])
    return sd


def _meta_quant_w(w):
    """engine._quant_w without the amax it cannot read on meta: e4m3 bytes of w's shape and a scale that depends on the shape."""
    return torch.empty(w.shape, dtype=hip.FP8, device=w.device), 2.0 ** -(6 + w.shape[0] // 64 % 3)


def _meta_act_scale(y, prev):
    """engine._act_scale likewise: a calibration sample's scale from its width, the running maximum kept."""
    s = y.shape[1] / 8192.0
    return s if prev is None else max(s, prev)


@contextlib.contextmanager
def on_meta():
    """What an engine on the meta device cannot call, replaced while one is built or run there: ``hip.load`` (no library is needed)
    and the two host-synchronising helpers of the fp8 mode."""
    saved = [(hip, "load", hip.load), (eng_mod, "_quant_w", eng_mod._quant_w), (eng_mod, "_act_scale", eng_mod._act_scale)]
    hip.load, eng_mod._quant_w, eng_mod._act_scale = (lambda *a, **k: None), _meta_quant_w, _meta_act_scale
    try:
        yield
    finally:
        for obj, attr, value in saved:
            setattr(obj, attr, value)


def trace_block(C, heads, side, nimg, shared, chunk_of=None):
    """prepare_context at Lc = 77 and one call of one block on the meta device; ``chunk_of=(total, first)``: the call handles
    images [first, first + nimg) of a batch of ``total`` and writes into ``out=``."""
    shapes = OrderedDict()
    weights._transformer(shapes, "blk", C, 768, False)
    t = eng_mod._Transformer(_meta_state_dict(shapes), "blk", "meta", heads, 32)
    total = chunk_of[0] if chunk_of else nimg
    nb = nimg // 2 if shared else nimg
    x = torch.empty((nb * side * side, C), dtype=BF16, device="meta")
    kw = {}
    if chunk_of:
        kw = dict(out=torch.empty((total * side * side, C), dtype=BF16, device="meta")[chunk_of[1] * side * side:][:nimg * side * side],
                  ctx_of=chunk_of)
    with Recorder() as rec:
        t.prepare_context(torch.empty((total * LC, 768), dtype=BF16, device="meta"), total, LC)
        t(x, nimg, side, side, shared_prefix=shared, **kw)
    return rec.trace


def trace_block_case(name, monkeypatch_setattr):
    """The trace of a named block case; ``monkeypatch_setattr(obj, attr, value)`` is how the knobs of ``hip`` are set (the caller
    undoes them).  Names: a key of BLOCKS, ``<key>@force6``, ``<key>@<KNOB>=0``, CHUNKED."""
    if name == CHUNKED:
        return trace_block(320, 8, 16, 2, False, chunk_of=(4, 2))
    key, _, mod = name.partition("@")
    if mod == "force6":
        monkeypatch_setattr(hip, "FORCE_TILE", 6)
    elif mod:
        monkeypatch_setattr(hip, mod[:-2], False)
    return trace_block(*BLOCKS[key])


def block_case_names():
    return (list(BLOCKS) + [CHUNKED] + [f"{k}@force6" for k in FORCED] + [f"{k}@{knob}=0" for k, knobs in KNOBS_OFF.items() for knob in knobs])


def build_engine(arch, device, tiled=False, fp8=False):
    """The UNetEngine of ``arch``: on "meta" from shapes alone (inside ``on_meta``), on a GPU from the seeded synthetic weights the
    parity tests use.  An fp8 engine gets fixed activation scales, different from one ResBlock to the next."""
    c = UNET_CONFIGS[arch]()
    shapes = weights.unet_shapes(c)
    sd = _meta_state_dict(shapes) if str(device) == "meta" else weights.synthetic_state_dict(shapes, seed=0)
    engine = eng_mod.UNetEngine(c, sd, device, tiled=tiled, fp8=fp8)
    if fp8:
        engine.set_fp8_scales([(2.0 ** -(3 + i % 3), 2.0 ** -(4 + i % 2)) for i in range(len(engine.res))])
    return engine


def trace_engine(engine, nimg, side, cfg_shared, chunk_rows):
    """prepare_context (bf16 context, Lc = 77) and one forward of ``engine`` at this size."""
    c, dev = engine.cfg, engine.device
    engine.prepare_timesteps([981, 961])
    x = torch.zeros((nimg * side * side, c.in_channels), dtype=BF16, device=dev)
    ctx = torch.zeros((nimg, LC, c.cross_attention_dim), dtype=BF16, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    before = os.environ.get("SDV_CHUNK_ROWS")
    os.environ["SDV_CHUNK_ROWS"] = str(chunk_rows)
    try:
        with Recorder() as rec:
            engine.prepare_context(ctx)
            engine.forward(x, nimg, side, side, step, cfg_shared=cfg_shared)
    finally:
        engine.release(nimg)          # (the next trace at this batch size allocates its context buffers again, like this one)
        if before is None:
            del os.environ["SDV_CHUNK_ROWS"]
        else:
            os.environ["SDV_CHUNK_ROWS"] = before
    return rec.trace


def trace_engine_calibrating(arch, size):
    """One forward of a fresh fp8 engine on meta (inside ``on_meta``) while ``fp8_calibration`` is on."""
    c = UNET_CONFIGS[arch]()
    engine = eng_mod.UNetEngine(c, _meta_state_dict(weights.unet_shapes(c)), "meta", fp8=True)
    engine.fp8_calibration(True)
    try:
        return trace_engine(engine, *size)
    finally:
        engine.fp8_calibration(False)


def build_vae(arch, device, tiled=False):
    c = VAE_CONFIGS[arch]()
    shapes = weights.vae_decoder_shapes(c)
    sd = _meta_state_dict(shapes) if str(device) == "meta" else weights.synthetic_state_dict(shapes, seed=0)
    return eng_mod.VAEDecoderEngine(c, sd, device, tiled=tiled)


def trace_vae(engine, nimg, side, want_float, per_chunk):
    """One decode of ``nimg`` latents of side x side; ``per_chunk`` images per score chunk of the mid-block attention (0: the engine's
    own limit, which holds all of them)."""
    lat = torch.zeros((nimg, side, side, engine.cfg.latent_channels), dtype=torch.float32, device=engine.device)
    before = engine.score_chunk_bytes
    if per_chunk:
        engine.score_chunk_bytes = per_chunk * 6 * side ** 4
    try:
        with Recorder() as rec:
            engine.decode(lat, want_float=want_float)
    finally:
        engine.score_chunk_bytes = before
    return rec.trace


def trace_clip_call(name, device):
    """The whole call of a CLIP engine on a GPU - host-side checks included - on seeded synthetic weights."""
    kind, cfg, n = CLIP_CALLS[name]
    c = cfg()
    if kind == "text":
        engine = text.build_text_encoder(c, None, seed=0).to(device)
        arg = (torch.arange(n * LC, device=device).reshape(n, LC) % c.vocab_size,)
    else:
        sd = weights.synthetic_safety_checker(c, seed=0)
        engine = vision.CLIPVisionEngine(c, sd).to(device)
        arg = (torch.zeros((n * (c.num_tokens - 1), hip.patch_kpad(c.patch_size)), dtype=BF16, device=device), n)
    with Recorder() as rec:
        engine(*arg)
    return rec.trace


def trace_clip_on_meta(name):
    """The same call on the meta device (inside ``on_meta``), from shapes alone: the text engine from behind its id-range check,
    the vision engine whole but for its residency check."""
    kind, cfg, n = CLIP_CALLS[name]
    c = cfg()
    if kind == "text":
        engine = text.CLIPTextEngine(c, _meta_state_dict(weights.clip_text_shapes(c)))
        call, arg = engine._forward, (torch.empty((n, LC), dtype=torch.int64, device="meta"),)
    else:
        engine = vision.CLIPVisionEngine(c, _meta_state_dict(weights.vision_shapes(c)))
        engine._need_gpu = lambda t: None
        call, arg = engine, (torch.empty((n * (c.num_tokens - 1), hip.patch_kpad(c.patch_size)), dtype=BF16, device="meta"), n)
    engine._w = engine._prepare("meta")
    with Recorder() as rec:
        call(*arg)
    return rec.trace


def sdv_ops(entry):
    """The launches of a golden entry or of ``digest(trace)``, without the ops recorded by name only."""
    return [(n, a) for n, a in zip(entry["ops"], entry["args"]) if "::" not in n]
