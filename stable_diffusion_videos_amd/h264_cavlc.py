"""Entropy-coded H.264 video samples from frames that are already in HBM (csrc/sdv_h264.hip): the compressed counterpart of h264.py's
``I_PCM`` pictures, for the mp4 of ``walk()``.

The reference asks libx264 for ``crf 10, yuv420p`` (utils.py:69-128).  This is an all-intra, Constrained-Baseline, CAVLC stream with the
same parameter sets as the ``I_PCM`` track (``h264.sps_pps``): every macroblock ``Intra16x16`` with DC prediction from its left neighbour,
one IDR slice per macroblock row so that every row is an independent bit stream (one wave each on the GPU), ``I_PCM`` where a macroblock
would break the 3200-bit limit of Annex A.3.1.  The stream rule is written down in include/sdv_hip.h and DESIGN.md ("H.264 CAVLC intra
encoder"); tests/h264_ref.py restates it and decodes it.

``gop`` > 1 (opt-in on top of the opt-in; sdv_hip.h and DESIGN.md "H.264 P pictures") makes picture k of a call an IDR picture only when
``k % gop == 0`` and a P picture otherwise: zero-motion inter prediction from the reconstruction of the picture before it, ``P_Skip``
where nothing is left to code.  tests/h264_p_ref.py restates and decodes that stream.  ``gop`` 1 is the code and the bytes described above.

``search`` > 0 (opt-in on top of ``gop`` > 1; include/sdv_hip_ext.h and DESIGN.md "H.264 motion search") gives every macroblock of a P picture
one vector of even whole samples, at most ``search`` luma samples a component, found by an exhaustive search on the source pictures: the
prediction is a displaced copy in luma and chroma.  tests/h264_me_ref.py restates it.  ``search`` 0 is the code and the bytes of ``gop`` alone.

``subpel`` in {1, 2, 4} (opt-in on top of ``search`` > 0; include/sdv_hip_h264_sub.h and DESIGN.md "H.264 sub-sample motion") puts the vectors on
the grid of whole, half or quarter samples: every whole-sample vector, odd ones included, then a half- and a quarter-sample refinement, with
the standard's 6-tap luma and bilinear chroma prediction.  tests/h264_sub_ref.py restates it.  ``subpel`` 0 is the code and the bytes of
``search`` alone.

``intra4`` 1 (opt-in, at any ``gop``; include/sdv_hip_h264_i4.h and DESIGN.md "H.264 Intra4x4") codes every IDR picture of a call with a
kernel of its own that chooses per macroblock between ``I_NxN`` (Intra4x4 prediction, nine modes per 4x4 block) and the Intra16x16 DC
macroblock above; P pictures are untouched.  tests/h264_i4_ref.py restates and decodes it.  ``intra4`` 0 is the code and the bytes of
the other settings alone.

``deblock`` 1 (opt-in, with every other setting; include/sdv_hip_h264_lf.h and DESIGN.md "H.264 deblocking") switches the in-loop
deblocking filter on: the slice headers say so, every picture position goes through a per-position entry point that also leaves one side
information word per macroblock, and a filter launch between two positions rewrites the reconstruction planes in place, so P pictures
predict from filtered pictures.  tests/h264_lf_ref.py restates, decodes and filters it.  ``deblock`` 0 is the code and the bytes of the
other settings alone.

``part`` 1 (opt-in on top of ``gop`` > 1 and ``search`` > 0, with every ``subpel``, ``intra4`` and ``deblock``; include/sdv_hip_h264_part.h and
DESIGN.md "H.264 partitions") gives every inter macroblock four vectors, one per 8x8 quadrant: the search keeps the four quadrant winners
beside the 16x16 one and takes them where they are cheaper by more than their syntax, ``P_8x8`` macroblocks carry them, prediction is per
partition and the loop filter compares the vectors per partition.  tests/h264_part_ref.py restates and decodes it.  ``part`` 0, or ``part``
1 without P pictures or without a search, is the code and the bytes of the other settings alone.

``row_slices`` S in 1 .. 16 (opt-in, with every other setting, ``gop`` 1 included; include/sdv_hip_h264_seg.h and DESIGN.md "H.264 row
slices") cuts every macroblock row into ``segs = max(1, min(S, mbw, 1024 // mbh))`` slices of nearly equal width, each an independent bit
stream with a wave of its own: the GPU then has ``segs`` times as many chains to run side by side, at a few bytes per slice.  A slice start
is a row start; vectors, the loop filter and the search do not stop there.  tests/h264_seg_ref.py restates and decodes it.  ``row_slices``
1, or any S on a frame size with ``segs`` 1, is the code and the bytes of the other settings alone.

Host side here: the workspaces, the copy back of the packed samples and their offsets.  Opt-in (video.py ``SDV_VIDEO_CODEC=h264-cavlc``).
"""
from __future__ import annotations

from typing import Dict, List

import torch

from . import hip

DEFAULT_QP = 16
DEFAULT_GOP = 1                                                                                 # a setting, not a measured optimum
DEFAULT_SEARCH = 0                                                                              # a setting, not a measured optimum
DEFAULT_SUBPEL = 0                                                                              # a setting, not a measured optimum
DEFAULT_INTRA4 = 0                                                                              # a setting, not a measured optimum
DEFAULT_DEBLOCK = 0                                                                             # a setting, not a measured optimum
DEFAULT_PART = 0                                                                                # a setting, not a measured optimum
DEFAULT_ROW_SLICES = 1                                                                          # a setting, not a measured optimum


def check_qp(qp) -> int:
    if isinstance(qp, bool) or not isinstance(qp, int) or not 0 <= qp <= 51:
        raise ValueError(f"h264 qp must be an integer in 0 .. 51, got {qp!r}")
    return qp


def check_gop(gop) -> int:
    if isinstance(gop, bool) or not isinstance(gop, int) or not 1 <= gop <= hip.H264_GOP_MAX:
        raise ValueError(f"h264 gop must be an integer in 1 .. {hip.H264_GOP_MAX}, got {gop!r}")
    return gop


def check_search(search) -> int:
    if isinstance(search, bool) or not isinstance(search, int) or not 0 <= search <= hip.H264_SEARCH_MAX or search % 2:
        raise ValueError(f"h264 search must be an even integer in 0 .. {hip.H264_SEARCH_MAX}, got {search!r}")
    return search


def check_subpel(subpel) -> int:
    if isinstance(subpel, bool) or not isinstance(subpel, int) or subpel not in (0,) + hip.H264_SUBPELS:
        raise ValueError(f"h264 subpel must be one of the integers 0, 1, 2, 4, got {subpel!r}")
    return subpel


def check_intra4(intra4) -> int:
    if isinstance(intra4, bool) or not isinstance(intra4, int) or intra4 not in (0, 1):
        raise ValueError(f"h264 intra4 must be one of the integers 0, 1, got {intra4!r}")
    return intra4


def check_deblock(deblock) -> int:
    if isinstance(deblock, bool) or not isinstance(deblock, int) or deblock not in (0, 1):
        raise ValueError(f"h264 deblock must be one of the integers 0, 1, got {deblock!r}")
    return deblock


def check_part(part) -> int:
    if isinstance(part, bool) or not isinstance(part, int) or part not in (0, 1):
        raise ValueError(f"h264 part must be one of the integers 0, 1, got {part!r}")
    return part


def check_row_slices(row_slices) -> int:
    if isinstance(row_slices, bool) or not isinstance(row_slices, int) or not 1 <= row_slices <= hip.H264_ROW_SLICES_MAX:
        raise ValueError(f"h264 row_slices must be an integer in 1 .. {hip.H264_ROW_SLICES_MAX}, got {row_slices!r}")
    return row_slices


class H264Encoder:
    """``encode(frames_u8, first_index)``: uint8 ``[n, H, W, 3]`` tensor in GPU memory (H, W even) -> ``list[bytes]``, one mp4 sample
    (the picture's length-prefixed slice NAL units) per frame.  Picture k carries ``idr_pic_id = (first_index + k) & 1``.  With ``gop``
    > 1 only the pictures at positions ``k % gop == 0`` of a call are IDR pictures (``last_sync`` lists them after every call); the
    others are P pictures, and every call starts a new GOP.  ``return_recon=True`` returns ``(samples, (ry, rcb, rcr))``, the
    decoder's pictures as padded planes in GPU memory (they belong to the workspace: the next call overwrites them).  ``search`` > 0
    (even, at most 16; no effect with ``gop`` 1, which has no P pictures) motion-compensates the P pictures: one more launch for the
    search over all of them, then one launch per picture position of the GOPs instead of one for all.  ``subpel`` 1, 2 or 4 (no
    effect unless ``gop`` > 1 and ``search`` > 0) runs the same number of launches through the quarter-sample pair of entry points.
    ``intra4`` 1 codes the IDR pictures with Intra4x4 prediction: one launch for all of them, then one launch per P picture position
    (always the per-position entry points, with zero vectors when ``search`` is 0); the workspaces are then those of the GOP path at
    any ``gop``, so ``return_recon`` works at ``gop`` 1 too.  ``deblock`` 1 switches the in-loop deblocking filter on: every picture
    position through a per-position entry point (the IDR pictures through the k = 0 step, or the Intra4x4 launch), and one filter launch
    after each position but the last, whose filtered planes only ``return_recon`` reads (it then runs too); GOP workspaces at any ``gop``.
    ``part`` 1 (no effect unless ``gop`` > 1 and ``search`` > 0) runs the partition search, then every P position - and, without ``intra4``,
    the IDR position - through the four-vector entry points, and the four-vector filter with ``deblock``; the same number of launches.
    ``row_slices`` S (1 .. 16, with every other setting) writes ``segs = max(1, min(S, mbw, 1024 // mbh))`` slices per macroblock row.
    ``segs`` 1 (S = 1, a picture one macroblock wide, a very tall one) takes the route above and writes its bytes.  With ``segs`` > 1 every
    setting combination runs the search (if any; the one-vector searches' result is expanded on the device to the four-vector layout
    in quarter samples), then one seg launch per picture position (the Intra4x4 seg launch for the IDR position with ``intra4``), the
    four-vector filter between positions with ``deblock``, and pack over ``mbh * segs`` slot rows; the single-launch
    ``h264_encode_gops`` and ``h264_encode_rows`` routes are not used, so ``return_recon`` works at ``gop`` 1 too.

    Three entry points on the current stream (planes; rows; pack), then two copies into pinned memory: the n + 1 offsets, then the used
    prefix of the packed buffer - raw frames and planes stay in HBM.  Workspaces are cached per ``(n, H, W)`` and sized by the
    capacity bound of sdv_hip.h, so no batch can fail to fit."""

    def __init__(self, qp: int = DEFAULT_QP, device=None, gop: int = DEFAULT_GOP, search: int = DEFAULT_SEARCH,
                 subpel: int = DEFAULT_SUBPEL, intra4: int = DEFAULT_INTRA4, deblock: int = DEFAULT_DEBLOCK, part: int = DEFAULT_PART,
                 row_slices: int = DEFAULT_ROW_SLICES):
        self.qp = check_qp(qp)
        self.gop = check_gop(gop)
        self.search = check_search(search)
        self.subpel = check_subpel(subpel)
        self.intra4 = check_intra4(intra4)
        self.deblock = check_deblock(deblock)
        self.part = check_part(part)
        self.row_slices = check_row_slices(row_slices)
        self._parted = self.part == 1 and self.gop > 1 and self.search > 0                      # otherwise part 1 is today's route
        self.last_sync: List[int] = []
        self.device = torch.device(device) if device is not None else None
        self._ws: Dict[tuple, dict] = {}
        self.last_bytes_to_host = 0

    def _workspace(self, n: int, mbh: int, mbw: int, device) -> dict:
        key = (n, mbh, mbw, str(device))
        ws = self._ws.get(key)
        if ws is None and hip.h264_row_segments(mbh, mbw, self.row_slices) > 1:
            ws = self._seg_workspace(n, mbh, mbw, device)
            if len(self._ws) >= 4:
                self._ws.pop(next(iter(self._ws)))
            self._ws[key] = ws
        if ws is None:
            gops = self.gop > 1 or self.intra4 == 1 or self.deblock == 1                     # Intra4x4 and the loop filter use the GOP slots at any gop
            cap = hip.h264_gop_out_bytes(n, mbh, mbw) if gops else hip.h264_out_bytes(n, mbh, mbw)
            scratch = hip.h264_gop_scratch_bytes(n, mbh, mbw) if gops else hip.h264_scratch_bytes(n, mbh, mbw)
            ws = dict(y=torch.empty((n, 16 * mbh, 16 * mbw), dtype=torch.uint8, device=device),
                      cb=torch.empty((n, 8 * mbh, 8 * mbw), dtype=torch.uint8, device=device),
                      cr=torch.empty((n, 8 * mbh, 8 * mbw), dtype=torch.uint8, device=device),
                      scratch=torch.empty((scratch,), dtype=torch.uint8, device=device),
                      out=torch.empty((cap,), dtype=torch.uint8, device=device),
                      offsets=torch.zeros((n + 1,), dtype=torch.int64, device=device),
                      offsets_host=torch.empty((n + 1,), dtype=torch.int64, pin_memory=True),
                      out_host=torch.empty((cap,), dtype=torch.uint8, pin_memory=True))
            if gops:                                                                            # the reference pictures stay in HBM
                ws.update(ry=torch.empty_like(ws["y"]), rcb=torch.empty_like(ws["cb"]), rcr=torch.empty_like(ws["cr"]))
                if self._parted:                                                                # four quarter-sample vectors a macroblock
                    ws.update(mv=torch.zeros((n, mbh, mbw, 4, 2), dtype=torch.int16, device=device))
                    if self.deblock:
                        ws.update(mbinfo=torch.zeros((n, mbh, mbw), dtype=torch.int32, device=device))
                elif self.deblock:                                                              # the filter reads the vectors of every picture
                    ws.update(mv=torch.zeros((n, mbh, mbw, 2), dtype=torch.int16, device=device),
                              mbinfo=torch.zeros((n, mbh, mbw), dtype=torch.int32, device=device))
                elif self.search and self.gop > 1:                                              # even samples, or quarter samples with subpel
                    ws.update(mv=torch.empty((n, mbh, mbw, 2), dtype=torch.int16, device=device))
                elif self.intra4 and self.gop > 1:                                              # zero vectors for the per-position entry point
                    ws.update(mv=torch.zeros((n, mbh, mbw, 2), dtype=torch.int16, device=device))
            if len(self._ws) >= 4:                                                              # a walk uses one or two shapes
                self._ws.pop(next(iter(self._ws)))
            self._ws[key] = ws
        return ws

    def _seg_workspace(self, n: int, mbh: int, mbw: int, device) -> dict:
        """``row_slices``: slots of the seg layout, the reconstruction planes, the four-vector tensor of every route (zeros without a
        search), the one-vector tensor a search without ``part`` writes, the side information with ``deblock``."""
        segs = hip.h264_row_segments(mbh, mbw, self.row_slices)
        cap = hip.h264_seg_out_bytes(n, mbh, mbw, segs)
        ws = dict(segs=segs,
                  y=torch.empty((n, 16 * mbh, 16 * mbw), dtype=torch.uint8, device=device),
                  cb=torch.empty((n, 8 * mbh, 8 * mbw), dtype=torch.uint8, device=device),
                  cr=torch.empty((n, 8 * mbh, 8 * mbw), dtype=torch.uint8, device=device),
                  scratch=torch.empty((hip.h264_seg_scratch_bytes(n, mbh, mbw, segs),), dtype=torch.uint8, device=device),
                  out=torch.empty((cap,), dtype=torch.uint8, device=device),
                  offsets=torch.zeros((n + 1,), dtype=torch.int64, device=device),
                  offsets_host=torch.empty((n + 1,), dtype=torch.int64, pin_memory=True),
                  out_host=torch.empty((cap,), dtype=torch.uint8, pin_memory=True),
                  mv=torch.zeros((n, mbh, mbw, 4, 2), dtype=torch.int16, device=device))
        ws.update(ry=torch.empty_like(ws["y"]), rcb=torch.empty_like(ws["cb"]), rcr=torch.empty_like(ws["cr"]))
        if self.search and self.gop > 1 and not self._parted:
            ws.update(mv1=torch.zeros((n, mbh, mbw, 2), dtype=torch.int16, device=device))
        if self.deblock:
            ws.update(mbinfo=torch.zeros((n, mbh, mbw), dtype=torch.int32, device=device))
        return ws

    def _check_device(self, what: str, t):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise hip.SdvHipError(f"H264Encoder.{what}: frames must live in GPU memory (got {getattr(t, 'device', type(t))}); "
                                  "the HIP path has no CPU fallback")
        if self.device is not None and self.device.index is not None and t.device != self.device:
            raise hip.SdvHipError(f"H264Encoder.{what}: frames are on {t.device}, the encoder was made for {self.device}")

    def encode(self, frames_u8: torch.Tensor, first_index: int = 0, return_recon: bool = False):
        self._check_device("encode", frames_u8)
        if frames_u8.dtype != torch.uint8 or frames_u8.ndim != 4 or frames_u8.shape[-1] != 3:
            raise hip.SdvHipError(f"H264Encoder.encode: expected a uint8 [n, H, W, 3] tensor, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        frames_u8 = frames_u8.contiguous()
        n, H, W, _ = frames_u8.shape
        if n == 0:
            self.last_sync = []
            return ([], None) if return_recon else []
        if H % 2 or W % 2 or not (2 <= H <= hip.H264_MAX_DIM and 2 <= W <= hip.H264_MAX_DIM):
            raise hip.SdvHipError(f"H264Encoder.encode: frame size must be even and 2 .. {hip.H264_MAX_DIM}, got {H} x {W}")
        mbh, mbw = hip.h264_mb_grid(H, W)
        with torch.cuda.device(frames_u8.device):
            ws = self._workspace(n, mbh, mbw, frames_u8.device)
            hip.h264_planes(frames_u8, ws["y"], ws["cb"], ws["cr"])
            return self._rows_and_pack(ws, n, mbh, mbw, first_index, return_recon)

    def encode_planes(self, y: torch.Tensor, cb: torch.Tensor, cr: torch.Tensor, first_index: int = 0, return_recon: bool = False):
        """The same from padded planes ``y [n, 16 mbh, 16 mbw]``, ``cb`` / ``cr [n, 8 mbh, 8 mbw]`` (any sample values)."""
        for t in (y, cb, cr):
            self._check_device("encode_planes", t)
        if y.ndim != 3 or y.shape[0] == 0:
            raise hip.SdvHipError(f"H264Encoder.encode_planes: expected y [n >= 1, 16 mbh, 16 mbw], got {tuple(y.shape)}")
        n, mbh, mbw = y.shape[0], y.shape[1] // 16, y.shape[2] // 16
        with torch.cuda.device(y.device):
            ws = dict(self._workspace(n, mbh, mbw, y.device), y=y.contiguous(), cb=cb.contiguous(), cr=cr.contiguous())
            return self._rows_and_pack(ws, n, mbh, mbw, first_index, return_recon)

    def _rows_and_pack(self, ws: dict, n: int, mbh: int, mbw: int, first_index: int, return_recon: bool = False):
        if ws.get("segs", 1) > 1:
            self._seg_steps(ws, n, int(first_index), return_recon)
            hip.h264_pack(ws["scratch"], n, mbh * ws["segs"], hip.h264_seg_slot_mbw(mbw, ws["segs"]), ws["out"], ws["offsets"])
        elif self._parted:
            self._parted_steps(ws, n, int(first_index), return_recon)
            hip.h264_pack(ws["scratch"], n, mbh, hip.h264_gop_slot_mbw(mbw), ws["out"], ws["offsets"])
        elif self.deblock:
            self._deblocked_steps(ws, n, int(first_index), return_recon)
            hip.h264_pack(ws["scratch"], n, mbh, hip.h264_gop_slot_mbw(mbw), ws["out"], ws["offsets"])
        elif self.intra4:
            self._idr4_and_steps(ws, n, int(first_index))
            hip.h264_pack(ws["scratch"], n, mbh, hip.h264_gop_slot_mbw(mbw), ws["out"], ws["offsets"])
        elif self.gop == 1:
            if return_recon:
                raise hip.SdvHipError("H264Encoder: the all-intra path (gop 1) reconstructs only what its chains read; return_recon needs gop > 1")
            hip.h264_encode_rows(ws["y"], ws["cb"], ws["cr"], self.qp, int(first_index), ws["scratch"])
            hip.h264_pack(ws["scratch"], n, mbh, mbw, ws["out"], ws["offsets"])
        elif self.search == 0:
            hip.h264_encode_gops(ws["y"], ws["cb"], ws["cr"], self.qp, self.gop, int(first_index), ws["ry"], ws["rcb"], ws["rcr"], ws["scratch"])
            hip.h264_pack(ws["scratch"], n, mbh, hip.h264_gop_slot_mbw(mbw), ws["out"], ws["offsets"])
        elif self.subpel:
            hip.h264_motion_search_sub(ws["y"], self.qp, self.gop, self.search, self.subpel, ws["mv"])
            for k in range(min(self.gop, n)):
                hip.h264_encode_gop_step_sub(ws["y"], ws["cb"], ws["cr"], self.qp, self.gop, k, self.search, self.subpel, int(first_index), ws["mv"],
                                             ws["ry"], ws["rcb"], ws["rcr"], ws["scratch"])
            hip.h264_pack(ws["scratch"], n, mbh, hip.h264_gop_slot_mbw(mbw), ws["out"], ws["offsets"])
        else:
            hip.h264_motion_search(ws["y"], self.qp, self.gop, self.search, ws["mv"])
            for k in range(min(self.gop, n)):                                                   # the kernel boundary orders picture k - 1 before k
                hip.h264_encode_gop_step(ws["y"], ws["cb"], ws["cr"], self.qp, self.gop, k, self.search, int(first_index), ws["mv"], ws["ry"],
                                         ws["rcb"], ws["rcr"], ws["scratch"])
            hip.h264_pack(ws["scratch"], n, mbh, hip.h264_gop_slot_mbw(mbw), ws["out"], ws["offsets"])
        self.last_sync = list(range(0, n, self.gop))
        ws["offsets_host"].copy_(ws["offsets"], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        offs = ws["offsets_host"].tolist()
        used = offs[n]
        ws["out_host"][:used].copy_(ws["out"][:used], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        payload = ws["out_host"].numpy()
        self.last_bytes_to_host = used + 8 * (n + 1)
        samples = [payload[offs[k]:offs[k + 1]].tobytes() for k in range(n)]
        return (samples, (ws["ry"], ws["rcb"], ws["rcr"])) if return_recon else samples


    def _idr4_and_steps(self, ws: dict, n: int, first_index: int):
        """``intra4``: the IDR pictures of the call in one launch, then the P picture positions in order (the kernel boundaries order
        picture k - 1 before k).  Without a search the P pictures take the whole-sample entry point with its smallest range and zero
        vectors, which is the zero-motion prediction of ``gop`` alone."""
        planes, recon = (ws["y"], ws["cb"], ws["cr"]), (ws["ry"], ws["rcb"], ws["rcr"])
        steps = range(1, min(self.gop, n))
        if steps and self.search and self.subpel:
            hip.h264_motion_search_sub(ws["y"], self.qp, self.gop, self.search, self.subpel, ws["mv"])
        elif steps and self.search:
            hip.h264_motion_search(ws["y"], self.qp, self.gop, self.search, ws["mv"])
        hip.h264_encode_idr4(*planes, self.qp, self.gop, first_index, *recon, ws["scratch"])
        for k in steps:
            if self.search and self.subpel:
                hip.h264_encode_gop_step_sub(*planes, self.qp, self.gop, k, self.search, self.subpel, first_index, ws["mv"], *recon, ws["scratch"])
            else:
                hip.h264_encode_gop_step(*planes, self.qp, self.gop, k, self.search or 2, first_index, ws["mv"], *recon, ws["scratch"])


    def _deblocked_steps(self, ws: dict, n: int, first_index: int, filter_last: bool):
        """``deblock``: every picture position through its per-position entry point with the side information, the filter between two
        positions.  IDR pictures take the Intra4x4 launch with ``intra4`` and the k = 0 step without; without a search the P pictures
        take the whole-sample entry point with its smallest range and zero vectors."""
        planes, recon = (ws["y"], ws["cb"], ws["cr"]), (ws["ry"], ws["rcb"], ws["rcr"])
        last = min(self.gop, n)
        searched = bool(self.search) and self.gop > 1
        sub = self.subpel if searched else 0
        if last > 1 and sub:
            hip.h264_motion_search_sub(ws["y"], self.qp, self.gop, self.search, sub, ws["mv"])
        elif last > 1 and searched:
            hip.h264_motion_search(ws["y"], self.qp, self.gop, self.search, ws["mv"])
        for k in range(last):
            if k == 0 and self.intra4:
                hip.h264_encode_idr4_lf(*planes, self.qp, self.gop, first_index, *recon, ws["scratch"], ws["mbinfo"])
            elif sub:
                hip.h264_encode_gop_step_sub_lf(*planes, self.qp, self.gop, k, self.search, sub, first_index, ws["mv"], *recon, ws["scratch"],
                                                ws["mbinfo"])
            else:
                hip.h264_encode_gop_step_lf(*planes, self.qp, self.gop, k, self.search if searched else 2, first_index, ws["mv"], *recon,
                                            ws["scratch"], ws["mbinfo"])
            if k + 1 < last or filter_last:
                hip.h264_deblock(*recon, self.qp, self.gop, k, sub, ws["mbinfo"], ws["mv"])


    def _parted_steps(self, ws: dict, n: int, first_index: int, filter_last: bool):
        """``part`` (with ``gop`` > 1 and ``search`` > 0): the partition search over all P pictures, then every picture position in order
        through the four-vector entry points (IDR pictures through the Intra4x4 launch with ``intra4``), with the side information and
        the four-vector filter between two positions when ``deblock`` is on."""
        planes, recon = (ws["y"], ws["cb"], ws["cr"]), (ws["ry"], ws["rcb"], ws["rcr"])
        last = min(self.gop, n)
        if last > 1:
            hip.h264_motion_search_part(ws["y"], self.qp, self.gop, self.search, self.subpel, ws["mv"])
        for k in range(last):
            if k == 0 and self.intra4 and self.deblock:
                hip.h264_encode_idr4_lf(*planes, self.qp, self.gop, first_index, *recon, ws["scratch"], ws["mbinfo"])
            elif k == 0 and self.intra4:
                hip.h264_encode_idr4(*planes, self.qp, self.gop, first_index, *recon, ws["scratch"])
            elif self.deblock:
                hip.h264_encode_gop_step_part_lf(*planes, self.qp, self.gop, k, self.search, self.subpel, first_index, ws["mv"], *recon, ws["scratch"],
                                                 ws["mbinfo"])
            else:
                hip.h264_encode_gop_step_part(*planes, self.qp, self.gop, k, self.search, self.subpel, first_index, ws["mv"], *recon, ws["scratch"])
            if self.deblock and (k + 1 < last or filter_last):
                hip.h264_deblock_part(*recon, self.qp, self.gop, k, ws["mbinfo"], ws["mv"])


    def _seg_steps(self, ws: dict, n: int, first_index: int, filter_last: bool):
        """``row_slices`` with more than one slice a row: the search of the settings (if any) over all P pictures, its one-vector result
        written four times in quarter samples, then every picture position in order through the seg entry points (IDR pictures through
        the Intra4x4 seg launch with ``intra4``, the k = 0 step without), and with ``deblock`` the four-vector filter between two
        positions - it filters across slice boundaries as it does across rows.  Without a search the vectors are zeros and the step takes
        its smallest range."""
        planes, recon, segs = (ws["y"], ws["cb"], ws["cr"]), (ws["ry"], ws["rcb"], ws["rcr"]), ws["segs"]
        last = min(self.gop, n)
        searched = bool(self.search) and self.gop > 1
        search, sub = (self.search, self.subpel) if searched else (2, 0)
        if last > 1 and self._parted:
            hip.h264_motion_search_part(ws["y"], self.qp, self.gop, self.search, self.subpel, ws["mv"])
        elif last > 1 and searched:
            if sub:
                hip.h264_motion_search_sub(ws["y"], self.qp, self.gop, self.search, sub, ws["mv1"])
                ws["mv"].copy_(ws["mv1"][:, :, :, None, :].expand(-1, -1, -1, 4, -1))             # quarter samples already
            else:
                hip.h264_motion_search(ws["y"], self.qp, self.gop, self.search, ws["mv1"])
                ws["mv"].copy_((ws["mv1"] * 4)[:, :, :, None, :].expand(-1, -1, -1, 4, -1))       # whole samples -> quarter samples
        for k in range(last):
            if k == 0 and self.intra4 and self.deblock:
                hip.h264_encode_idr4_seg_lf(*planes, self.qp, self.gop, first_index, *recon, ws["scratch"], ws["mbinfo"], segs)
            elif k == 0 and self.intra4:
                hip.h264_encode_idr4_seg(*planes, self.qp, self.gop, first_index, *recon, ws["scratch"], segs)
            elif self.deblock:
                hip.h264_encode_gop_step_seg_lf(*planes, self.qp, self.gop, k, search, sub, first_index, ws["mv"], *recon, ws["scratch"],
                                                ws["mbinfo"], segs)
            else:
                hip.h264_encode_gop_step_seg(*planes, self.qp, self.gop, k, search, sub, first_index, ws["mv"], *recon, ws["scratch"], segs)
            if self.deblock and (k + 1 < last or filter_last):
                hip.h264_deblock_part(*recon, self.qp, self.gop, k, ws["mbinfo"], ws["mv"])


_encoders: Dict[tuple, H264Encoder] = {}


def encoder_for(qp: int, device, gop: int = DEFAULT_GOP, search: int = DEFAULT_SEARCH, subpel: int = DEFAULT_SUBPEL,
                intra4: int = DEFAULT_INTRA4, deblock: int = DEFAULT_DEBLOCK, part: int = DEFAULT_PART,
                row_slices: int = DEFAULT_ROW_SLICES) -> H264Encoder:
    """One cached encoder (and its workspaces) per quality setting, GOP length, search range, vector grid, intra setting, loop filter
    setting, partition setting, row slice setting and device."""
    key = (check_qp(qp), str(device), check_gop(gop), check_search(search), check_subpel(subpel), check_intra4(intra4), check_deblock(deblock),
           check_part(part), check_row_slices(row_slices))
    if key not in _encoders:
        _encoders[key] = H264Encoder(qp, device, gop, search, subpel, intra4, deblock, part, row_slices)
    return _encoders[key]
