"""Baseline JPEG encoding of frames that are already in HBM (csrc/sdv_jpeg.hip): ``.jpg`` frame files and Motion-JPEG tracks
without the raw frames ever crossing to the host.

Replaces the host-side compression of the reference's ``image.save(frame_filepath)`` (stable_diffusion_pipeline.py:553) for a
``.jpg`` / ``.jpeg`` ``image_file_ext`` and of the frame encode inside ``make_video_pyav`` (utils.py:69-128) where this package writes a
Motion-JPEG track.  The visible contract is what ``PIL.Image.save`` gives for these extensions - a baseline 4:2:0 JPEG with the
Annex K tables scaled for the quality (libjpeg's rule) and the Annex K Huffman tables - only the byte stream differs: one restart
interval per MCU row, which makes every MCU row an independent Huffman stream (one wave each on the GPU).

Host side here: the tables, the header (constant for one ``(H, W, quality)``), the workspaces and the copy back.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from . import hip

# ITU-T T.81 Annex K.1 / K.2, natural (row-major) order
_K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# zigzag sequence: natural index of the k-th coefficient (T.81 figure A.6)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# Annex K.3 - K.6: (Tc << 4 | Th, BITS, HUFFVAL) in the order they are written - the tables csrc/sdv_jpeg.hip codes with
_DC_VALS = bytes(range(12))
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_TABLES = ((0x00, bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), _DC_VALS),
                  (0x10, bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]), _AC_LUMA_VALS),
                  (0x01, bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), _DC_VALS),
                  (0x11, bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]), _AC_CHROMA_VALS))


def quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    """(luma, chroma): the Annex K tables scaled by libjpeg's rule (``jpeg_quality_scaling``), int64 [64] in natural order - the tables
    ``PIL.Image.save(quality=quality)`` writes."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be 1..100, got {quality!r}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(t, dtype=np.int64) * s + 50) // 100, 1, 255) for t in (_K1_LUMA, _K2_CHROMA))


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def jfif_header(H: int, W: int, quality: int) -> bytes:
    """SOI | APP0 (JFIF 1.01, density 1:1) | DQT x2 | SOF0 (8 bit, 3 components, Y 2x2, Cb 1x1, Cr 1x1) | DHT x4 | DRI (one MCU row) | SOS."""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"JPEG frame size must be 1..65535, got {H} x {W}")
    ql, qc = quant_tables(quality)
    zz = list(ZIGZAG)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _segment(0xDB, bytes([0]) + bytes(ql[zz].tolist())) + _segment(0xDB, bytes([1]) + bytes(qc[zz].tolist()))
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in HUFFMAN_TABLES:
        out += _segment(0xC4, bytes([tc_th]) + bits + vals)
    out += _segment(0xDD, ((W + 15) // 16).to_bytes(2, "big"))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


class JpegEncoder:
    """``encode(frames_u8)``: uint8 ``[n, H, W, 3]`` tensor in GPU memory -> ``list[bytes]``, one complete JFIF file per frame.

    Two launches' worth of entry points on the current stream (transform; entropy coding + packing), then two copies into pinned
    memory: the n + 1 offsets (with the needed size behind them), then the used prefix of the packed payload - the raw frames stay in
    HBM.  Workspaces are cached per ``(n, H, W)``; the payload buffer starts at half the raw size and grows to what the kernel asked
    for when a batch does not fit (one retry, nothing was written past the capacity)."""

    def __init__(self, quality: int = 75, device=None):
        self.quality = int(quality)
        self.tables = quant_tables(self.quality)
        self.device = torch.device(device) if device is not None else None
        self._ws: Dict[tuple, dict] = {}
        self.retries = 0

    def _workspace(self, n: int, H: int, W: int, device) -> dict:
        key = (n, H, W, str(device))
        ws = self._ws.get(key)
        if ws is None:
            rows, cols = hip.jpeg_mcu_grid(H, W)
            header = jfif_header(H, W, self.quality)
            cap = n * (len(header) + rows * cols * 384 + 2 * rows)
            ws = dict(header_bytes=header, header=torch.frombuffer(bytearray(header), dtype=torch.uint8).to(device),
                      coef=torch.empty((n, rows, cols, 6, 64), dtype=torch.int16, device=device),
                      scratch=torch.empty((hip.jpeg_scratch_bytes(n, H),), dtype=torch.uint8, device=device),
                      out=torch.empty((cap,), dtype=torch.uint8, device=device),
                      meta=torch.zeros((n + 2,), dtype=torch.int64, device=device),          # offsets [n + 1] | needed
                      meta_host=torch.empty((n + 2,), dtype=torch.int64, pin_memory=True),
                      out_host=torch.empty((cap,), dtype=torch.uint8, pin_memory=True))
            if len(self._ws) >= 4:                                                              # a walk uses one or two shapes
                self._ws.pop(next(iter(self._ws)))
            self._ws[key] = ws
        return ws

    def encode(self, frames_u8: torch.Tensor, return_coefficients: bool = False):
        if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
            raise hip.SdvHipError(f"JpegEncoder.encode: frames must live in GPU memory (got {getattr(frames_u8, 'device', type(frames_u8))}); "
                                  "the HIP path has no CPU fallback")
        if frames_u8.dtype != torch.uint8 or frames_u8.ndim != 4 or frames_u8.shape[-1] != 3:
            raise hip.SdvHipError(f"JpegEncoder.encode: expected a uint8 [n, H, W, 3] tensor, got {frames_u8.dtype} {tuple(frames_u8.shape)}")
        if self.device is not None and self.device.index is not None and frames_u8.device != self.device:
            raise hip.SdvHipError(f"JpegEncoder.encode: frames are on {frames_u8.device}, the encoder was made for {self.device}")
        frames_u8 = frames_u8.contiguous()
        n, H, W, _ = frames_u8.shape
        if n == 0:
            return ([], None) if return_coefficients else []
        with torch.cuda.device(frames_u8.device):
            ws = self._workspace(n, H, W, frames_u8.device)
            hip.jpeg_transform(frames_u8, self.tables[0], self.tables[1], out=ws["coef"])
            for attempt in range(2):
                hip.jpeg_entropy_pack(ws["coef"], H, W, ws["header"], ws["scratch"], ws["out"], ws["meta"][:n + 1], ws["meta"][n + 1:])
                ws["meta_host"].copy_(ws["meta"], non_blocking=True)
                torch.cuda.current_stream().synchronize()
                needed = int(ws["meta_host"][n + 1])
                if needed <= ws["out"].numel():
                    break
                if attempt == 1:
                    raise hip.SdvHipError(f"JpegEncoder.encode: {needed} bytes needed after a retry with the size the kernel reported")
                self.retries += 1
                ws["out"] = torch.empty((needed,), dtype=torch.uint8, device=frames_u8.device)
                ws["out_host"] = torch.empty((needed,), dtype=torch.uint8, pin_memory=True)
            ws["out_host"][:needed].copy_(ws["out"][:needed], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        offs = ws["meta_host"][:n + 1].tolist()
        payload = ws["out_host"].numpy()
        files: List[bytes] = [payload[offs[k]:offs[k + 1]].tobytes() for k in range(n)]
        self.last_bytes_to_host = needed + 8 * (n + 2)
        if return_coefficients:
            return files, ws["coef"].clone()
        return files


_encoders: Dict[tuple, JpegEncoder] = {}


def encoder_for(quality: int, device) -> JpegEncoder:
    """One cached encoder (and its workspaces) per quality and device."""
    key = (int(quality), str(device))
    if key not in _encoders:
        _encoders[key] = JpegEncoder(quality, device)
    return _encoders[key]
