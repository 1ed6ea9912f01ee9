"""PNG encoding of frames that are already in HBM (csrc/sdv_png.hip): ``.png`` frame files without the raw frames ever crossing to the
host.

Replaces the host-side compression of the reference's ``image.save(frame_filepath)`` (stable_diffusion_pipeline.py:553) for the default
``.png`` ``image_file_ext``.  The visible contract is what ``PIL.Image.save`` gives for this extension - an 8-bit RGB PNG that decodes
to exactly the frame - only the byte stream differs: per-row adaptive filtering by libpng's heuristic, then Huffman-only deflate
(no LZ77 matches) with one dynamic block per stripe of rows, every stripe byte-aligned, so that each is an independent bit stream
(one wave each on the GPU).

Host side here: the header (constant for one ``(H, W)``), the workspaces, the copy back and the CRC-32 of the IDAT chunk.  Opt-in
(``PngEncoder(matches=True)``): LZ77 matches in the deflate stage and the CRC-32 on the GPU as well.
"""
from __future__ import annotations

import struct
import zlib
from typing import Dict, List, Optional

import torch

from . import hip

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PREFIX = 33 + 8 + 2            # signature + IHDR chunk | IDAT length + tag | 78 01
_SUFFIX = 2 + 4 + 4 + 12        # 03 00 | Adler-32 | IDAT CRC | IEND chunk


def png_header(H: int, W: int) -> bytes:
    """Signature | IHDR chunk (W, H, bit depth 8, colour type 2 = RGB, compression 0, filter 0, no interlace): the 33 bytes that open
    every file of one frame size."""
    H, W = int(H), int(W)
    if not (1 <= H <= hip.PNG_MAX_DIM and 1 <= W <= hip.PNG_MAX_DIM):
        raise ValueError(f"PNG frame size must be 1..{hip.PNG_MAX_DIM}, got {H} x {W}")
    ihdr = b"IHDR" + struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    return SIGNATURE + struct.pack(">I", 13) + ihdr + struct.pack(">I", zlib.crc32(ihdr))


def default_stripe_rows(H: int, W: int) -> int:
    """Rows per deflate block: as many filtered rows as fit 32 KiB, at least one, at most the frame (21 at W = 512, 5 at W = 2048)."""
    return max(1, min(int(H), 32768 // (1 + 3 * int(W))))


class PngEncoder:
    """``encode(frames_u8)``: uint8 ``[n, H, W, 3]`` tensor in GPU memory -> ``list[bytes]``, one complete PNG file per frame.

    Two entry points on the current stream (filter; deflate + packing), then two copies into pinned memory: the n + 1 offsets (with
    the needed size behind them), then the used prefix of the packed payload - the raw frames stay in HBM.  The CRC-32 of each IDAT
    chunk is computed here, over the bytes that came back.  Workspaces are cached per ``(n, H, W)``; the payload buffer starts at half
    the raw size and grows to what the kernel asked for when a batch does not fit (one retry, nothing was written past the
    capacity).

    ``matches=True`` (opt-in): the deflate stage looks for LZ77 matches (sdv_hip.h "Matching mode": nine candidates per position, a
    match is taken when the literals it replaces cost more bits; greedy parse) - smaller files for flat and smooth frames, more
    kernel time, and a token scratch of 4 bytes per filtered byte.  ``gpu_crc`` (default: as ``matches``): the IDAT CRC-32 is
    computed on the GPU as well (``sdv_png_crc32``), so no byte of the payload is touched on the host before it is cut into
    files; with ``matches=False`` the files are byte for byte those of the host CRC."""

    def __init__(self, device=None, stripe_rows: Optional[int] = None, matches: bool = False, gpu_crc: Optional[bool] = None):
        self.device = torch.device(device) if device is not None else None
        self.stripe_rows = None if stripe_rows is None else int(stripe_rows)
        if self.stripe_rows is not None and self.stripe_rows < 1:
            raise ValueError(f"stripe_rows must be >= 1, got {stripe_rows!r}")
        self.matches = bool(matches)
        self.gpu_crc = self.matches if gpu_crc is None else bool(gpu_crc)
        self._ws: Dict[tuple, dict] = {}
        self.retries = 0
        self.last_bytes_to_host = 0

    def _workspace(self, n: int, H: int, W: int, device) -> dict:
        key = (n, H, W, str(device))
        ws = self._ws.get(key)
        if ws is None:
            sr = min(self.stripe_rows, H) if self.stripe_rows is not None else default_stripe_rows(H, W)
            stripes = hip.png_stripes(H, W, sr)
            header = png_header(H, W)
            # the fixed bytes of every file and stripe (138 of table, 4 of stored block, the odd bits) + half the raw size
            cap = n * (_PREFIX + _SUFFIX + stripes * 148) + n * H * (1 + 3 * W) // 2
            ws = dict(stripe_rows=sr, stripes=stripes, header=torch.frombuffer(bytearray(header), dtype=torch.uint8).to(device),
                      filtered=torch.empty((n, H, 1 + 3 * W), dtype=torch.uint8, device=device),
                      adler=torch.empty((n, H, 2), dtype=torch.int32, device=device),
                      lengths=torch.empty((n, stripes, 257), dtype=torch.uint8, device=device),
                      scratch=torch.empty((hip.png_scratch_bytes(n, H, sr),), dtype=torch.uint8, device=device),
                      out=torch.empty((cap,), dtype=torch.uint8, device=device),
                      meta=torch.zeros((n + 2,), dtype=torch.int64, device=device),          # offsets [n + 1] | needed
                      meta_host=torch.empty((n + 2,), dtype=torch.int64, pin_memory=True),
                      out_host=torch.empty((cap,), dtype=torch.uint8, pin_memory=True))
            if self.matches:
                ws.update(lz_scratch=torch.empty((hip.png_lz_scratch_bytes(n, H, W, sr),), dtype=torch.uint8, device=device),
                          ll_lengths=torch.empty((n, stripes, 286), dtype=torch.uint8, device=device),
                          d_lengths=torch.empty((n, stripes, 30), dtype=torch.uint8, device=device))
            if self.gpu_crc:
                ws["crc_acc"] = torch.empty((n,), dtype=torch.int32, device=device)
            if len(self._ws) >= 4:                                                              # a walk uses one or two shapes
                self._ws.pop(next(iter(self._ws)))
            self._ws[key] = ws
        return ws

    def _pack(self, ws: dict, n: int, return_tables: bool):
        offsets, needed = ws["meta"][:n + 1], ws["meta"][n + 1:]
        if self.matches:
            hip.png_deflate_lz_pack(ws["filtered"], ws["adler"], ws["stripe_rows"], ws["header"], ws["scratch"], ws["out"], offsets, needed,
                                    ws["lz_scratch"], *((ws["lengths"], ws["ll_lengths"], ws["d_lengths"]) if return_tables else ()))
        else:
            hip.png_deflate_pack(ws["filtered"], ws["adler"], ws["stripe_rows"], ws["header"], ws["scratch"], ws["out"], offsets, needed,
                                 ws["lengths"] if return_tables else None)
        if self.gpu_crc:
            hip.png_crc32(ws["out"], offsets, needed, ws["crc_acc"])

    def encode(self, frames_u8: torch.Tensor, return_tables: bool = False):
        """``return_tables=True``: ``(files, filtered rows uint8 [n, H, 1 + 3W], code lengths uint8 [n, stripes, 257])``, the two
        tensors as copies in GPU memory.  An encoder with ``matches=True`` returns four more: the tokens int32 ``[n, H (1 + 3W)]``
        (``len << 16 | dist`` or the byte; a stripe's tokens start at the index of its first filtered byte), their count per stripe
        int32 ``[n, stripes]``, and the final literal / length and distance code lengths uint8 ``[n, stripes, 286]`` /
        ``[n, stripes, 30]`` - the 257 lengths in front are then the literal prices the matches were weighed against."""
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
            raise hip.SdvHipError(f"PngEncoder.encode: frames must live in GPU memory (got {getattr(frames_u8, 'device', type(frames_u8))}); "
                                  "the HIP path has no CPU fallback")
        if frames_u8.dtype != torch.uint8 or frames_u8.ndim != 4 or frames_u8.shape[-1] != 3:
            raise hip.SdvHipError(f"PngEncoder.encode: expected a uint8 [n, H, W, 3] tensor, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        if self.device is not None and self.device.index is not None and frames_u8.device != self.device:
            raise hip.SdvHipError(f"PngEncoder.encode: frames are on {frames_u8.device}, the encoder was made for {self.device}")
        frames_u8 = frames_u8.contiguous()
        n, H, W, _ = frames_u8.shape
        if n == 0:
            empty = (None,) * (6 if self.matches else 2)
            return ([],) + empty if return_tables else []
        if not (1 <= H <= hip.PNG_MAX_DIM and 1 <= W <= hip.PNG_MAX_DIM):
            raise hip.SdvHipError(f"PngEncoder.encode: frame size must be 1 .. {hip.PNG_MAX_DIM}, got {H} x {W}")
        with torch.cuda.device(frames_u8.device):
            ws = self._workspace(n, H, W, frames_u8.device)
            hip.png_filter(frames_u8, ws["filtered"], ws["adler"])
            for attempt in range(2):
                self._pack(ws, n, return_tables)
                ws["meta_host"].copy_(ws["meta"], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                needed = int(ws["meta_host"][n + 1])
                if needed <= ws["out"].numel():
                    break
                if attempt == 1:
                    raise hip.SdvHipError(f"PngEncoder.encode: {needed} bytes needed after a retry with the size the kernel reported")
                self.retries += 1
                ws["out"] = torch.empty((needed,), dtype=torch.uint8, device=frames_u8.device)
                ws["out_host"] = torch.empty((needed,), dtype=torch.uint8, pin_memory=True)
            ws["out_host"][:needed].copy_(ws["out"][:needed], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        offs = ws["meta_host"][:n + 1].tolist()
        payload = ws["out_host"].numpy()
        files: List[bytes] = []
        for k in range(n):
            lo, hi = offs[k], offs[k + 1]
            if not self.gpu_crc:
                crc = zlib.crc32(payload[lo + 37:hi - 16])                                      # IDAT tag + data
                payload[hi - 16:hi - 12] = list(crc.to_bytes(4, "big"))
            files.append(payload[lo:hi].tobytes())
        self.last_bytes_to_host = needed + 8 * (n + 2)
        if not return_tables:
            return files
        tables = (files, ws["filtered"].clone(), ws["lengths"].clone())
        if self.matches:
            words = ws["lz_scratch"].view(torch.int32)
            total, S = n * H * (1 + 3 * W), n * ws["stripes"]
            tables += (words[:total].view(n, -1).clone(), words[total:total + S].view(n, -1).clone(), ws["ll_lengths"].clone(),
                       ws["d_lengths"].clone())
        return tables


_encoders: Dict[tuple, PngEncoder] = {}


def encoder_for(device, matches: bool = False) -> PngEncoder:
    """One cached encoder (and its workspaces) per device and mode."""
    key = (str(device), bool(matches))
    if key not in _encoders:
        _encoders[key] = PngEncoder(device, matches=matches)
    return _encoders[key]
