"""Baseline-JPEG frame decoding on the MI355X, bit for bit what Pillow gives: ``np.asarray(Image.open(f).convert("RGB"))``.

The reference starts both of its frame-encoding paths from JPEG files on disk (extraction/video_features/
extract_features.py:45-49 ``preprocess(Image.open(image))``; inference_video_retrieval.py:35-46 ``--raw_frame``
``Image.open(p).convert('RGB')``), written by extract_frames.py's ``cv2.imwrite`` (baseline, 4:2:0, q95).

    frames = jpeg.decode(paths_or_bytes)          # uint8 [B,H,W,3] cuda (one size) or a list of [H,W,3]
    frames = jpeg.read_frame_dir(video_dir)       # <video>/*.jpg in extract_features.py's integer order
    jpeg.last_fallbacks                           # [(index, reason), ...] of the last call's host-decoded files
    frames = jpeg.decode(files, entropy="chunked")   # many lanes per image in the entropy stage: same bits

Files are read on a pool of at most 16 threads and parsed on the host (``hirest_jpeg_parse``); the compressed bytes go to
the device in one pinned copy and ``hirest_jpeg_decode`` (entropy decode, IDCT, upsampling + colour) writes the frames.
Files outside the supported subset (progressive, arithmetic, 12-bit, CMYK / RGB, multi-scan, odd sampling, truncated) and
files whose entropy decode reports an anomaly are decoded by Pillow on the host and uploaded: the result is Pillow's in
every case, Pillow's exceptions included.  The device path never falls back silently: ``last_fallbacks`` names every file
that took the host path and why.

The entropy stage has two forms with the same output: ``"lanes"`` gives each image one lane
(``hirest_jpeg_decode``), ``"chunked"`` gives each image a workgroup of up to 1024 lanes that find the block boundaries by
self-synchronisation (``hirest_jpeg_decode_chunked``), so that its rate does not depend on the number of images in the call.
``"chunked"`` is the default: it was the faster one at every size and batch measured.
``Decoder(entropy=..., chunk_bytes=...)``, the same keywords on ``decode`` / ``read_frame_dir``, and ``HIREST_JPEG_ENTROPY``
for the callers that use the module's own decoder (``extract_frame_dir``, ``JpegFrameSource``, ``evaluate_clip_score``).
"""
from __future__ import annotations

import ctypes as C
import glob
import io
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, ops

IO_THREADS = 16                       # file reads / host fallback: a command gets 16 CPUs, never size this from os.cpu_count()
WORKSPACE_BYTES = 10 << 30            # coefficient + plane workspace cap (1024 1080p frames: 9.6 GB); larger batches go in sub-batches
_ALIGN = 256
ENTROPY_MODES = ("lanes", "chunked")
DEFAULT_ENTROPY = "chunked"           # at least as fast on every measured row; HIREST_JPEG_ENTROPY overrides it

last_fallbacks: List[Tuple[int, str]] = []

Source = Union[bytes, bytearray, memoryview, str, os.PathLike]


def _read(src) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, "rb") as f:
        return f.read()


def _pool_map(fn, items):
    items = list(items)
    if len(items) <= 1:
        return [fn(x) for x in items]
    with ThreadPoolExecutor(max_workers=min(IO_THREADS, len(items))) as ex:
        return list(ex.map(fn, items))


def parse(data: bytes) -> Tuple[_lib.JpegImage, _lib.JpegTables]:
    """``hirest_jpeg_parse`` of one file: (descriptor, raw tables).  ``desc.supported`` says whether the device decodes it."""
    lib = _lib.load()
    img, tab = _lib.JpegImage(), _lib.JpegTables()
    buf = np.frombuffer(data, dtype=np.uint8)
    _lib.check(lib.hirest_jpeg_parse(buf.ctypes.data if buf.size else None, buf.size, C.byref(img), C.byref(tab)), "hirest_jpeg_parse")
    return img, tab


def decode_host(data: bytes) -> Tuple[np.ndarray, int]:
    """``hirest_jpeg_decode_host``: the device's arithmetic on the CPU -> (uint8 [H,W,3], status); status != 0 means the file
    is unsupported (HIREST_JPEG_ST_UNSUPPORTED) or its entropy decode reported an anomaly, and the array is then empty."""
    lib = _lib.load()
    img, tab = parse(data)
    if not img.supported:
        return np.zeros((0, 0, 3), np.uint8), 16
    out = np.empty((img.height, img.width, 3), np.uint8)
    buf = np.frombuffer(data, dtype=np.uint8)
    st = C.c_int32(0)
    _lib.check(lib.hirest_jpeg_decode_host(C.byref(img), C.byref(tab), buf.ctypes.data, out.ctypes.data, C.byref(st)), "hirest_jpeg_decode_host")
    return (out if st.value == 0 else np.zeros((0, 0, 3), np.uint8)), st.value


def decode_host_chunked(data: bytes, chunk_bytes: int = 0, scan: bytes = None) -> Tuple[np.ndarray, int, int]:
    """``hirest_jpeg_decode_host_chunked``: ``decode_host`` with the chunked entropy stage, the lanes run one after another
    -> (uint8 [H,W,3], status, sync rounds).  The file must have no restart interval.  ``scan`` (optional) is decoded in
    place of ``data`` with the descriptor and tables parsed from ``data``: a test's way to change bytes behind the parser."""
    lib = _lib.load()
    img, tab = parse(data)
    if not img.supported:
        return np.zeros((0, 0, 3), np.uint8), 16, 0
    out = np.empty((img.height, img.width, 3), np.uint8)
    buf = np.frombuffer(data if scan is None else scan, dtype=np.uint8)
    st, rounds = C.c_int32(0), C.c_int32(0)
    _lib.check(lib.hirest_jpeg_decode_host_chunked(C.byref(img), C.byref(tab), buf.ctypes.data, int(chunk_bytes), out.ctypes.data, C.byref(st),
                                                   C.byref(rounds)), "hirest_jpeg_decode_host_chunked")
    return (out if st.value == 0 else np.zeros((0, 0, 3), np.uint8)), st.value, rounds.value


def _pillow(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _fail_reason(img) -> str:
    return _lib.JPEG_REASONS.get(img.reason, f"reason {img.reason}")


def _status_reason(st: int) -> str:
    return ", ".join(v for k, v in _lib.JPEG_STATUS.items() if st & k) or f"status {st}"


class Decoder:
    """Reusable device decoder: keeps its pinned staging buffer, device buffers and workspace between calls.
    ``entropy``: "lanes" (one lane per image) or "chunked" (many lanes per image, ``chunk_bytes`` per lane, 0 = chosen per
    image); None takes ``HIREST_JPEG_ENTROPY``, else the default.  The frames are the same."""

    def __init__(self, workspace_bytes: int = WORKSPACE_BYTES, entropy: str = None, chunk_bytes: int = 0):
        entropy = entropy or os.environ.get("HIREST_JPEG_ENTROPY") or DEFAULT_ENTROPY
        if entropy not in ENTROPY_MODES:
            raise ValueError(f"entropy must be one of {ENTROPY_MODES}, not {entropy!r}")
        if int(chunk_bytes) < 0:
            raise ValueError("chunk_bytes must be >= 0")
        self.workspace_bytes = int(workspace_bytes)
        self.entropy = entropy
        self.chunk_bytes = int(chunk_bytes)
        self._chunk_info = None              # device int32 [m, 4] of the last chunked call, rows in launch order
        self.last_fallbacks: List[Tuple[int, str]] = []
        self._pinned = None
        self._dev = {}

    def _buffer(self, name: str, nbytes: int, device) -> torch.Tensor:
        t = self._dev.get((name, str(device)))
        if t is None or t.numel() < nbytes:
            t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
            self._dev[(name, str(device))] = t
        return t

    def _staging(self, nbytes: int) -> torch.Tensor:
        if self._pinned is None or self._pinned.numel() < nbytes:
            self._pinned = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, pin_memory=True)
        return self._pinned

    @torch.no_grad()
    def decode(self, sources: Sequence[Source], device=None):
        global last_fallbacks
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if device.type != "cuda":
            raise RuntimeError("hirest_amd.jpeg decodes on the MI355X only (device must be a cuda device)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.load()
        blobs = _pool_map(_read, sources)
        n = len(blobs)
        self.last_fallbacks = fallbacks = []
        last_fallbacks = fallbacks
        if n == 0:
            return []
        parsed = [parse(b) for b in blobs]
        dev_idx = [i for i in range(n) if parsed[i][0].supported]
        for i in range(n):
            if not parsed[i][0].supported:
                fallbacks.append((i, _fail_reason(parsed[i][0])))
        host_px = {}
        if fallbacks:                        # Pillow on the host; its exceptions (a truncated file) propagate
            arrs = _pool_map(_pillow, [blobs[i] for i, _ in fallbacks])
            host_px = {i: a for (i, _), a in zip(fallbacks, arrs)}
        shapes = [(parsed[i][0].height, parsed[i][0].width) if parsed[i][0].supported else host_px[i].shape[:2] for i in range(n)]
        same = len(set(shapes)) == 1
        sizes = [h * w * 3 for h, w in shapes]
        offs, o = [], 0
        for s in sizes:
            offs.append(o)
            o += s if same else -(-s // _ALIGN) * _ALIGN
        with torch.cuda.device(device):
            out = torch.empty(max(o, 1), dtype=torch.uint8, device=device)
            if dev_idx:
                self._decode_device(lib, blobs, parsed, dev_idx, offs, out, device, fallbacks, host_px)
            for i, a in host_px.items():
                out[offs[i]:offs[i] + sizes[i]].copy_(torch.from_numpy(np.array(a, copy=True)).reshape(-1))
        fallbacks.sort()
        if same:
            h, w = shapes[0]
            return out[:n * h * w * 3].view(n, h, w, 3)
        return [out[offs[i]:offs[i] + sizes[i]].view(shapes[i][0], shapes[i][1], 3) for i in range(n)]

    def _decode_device(self, lib, blobs, parsed, dev_idx, offs, out, device, fallbacks, host_px):
        # one table set per distinct (quantisation, Huffman) bytes: all frames of a video normally share one
        sets, set_of = [], {}
        for i in dev_idx:
            key = bytes(parsed[i][1])
            if key not in set_of:
                set_of[key] = len(sets)
                sets.append(parsed[i][1])
            parsed[i][0].table_set = set_of[key]
        order = sorted(dev_idx, key=lambda i: parsed[i][0].table_set)     # adjacent table sets: one entropy launch per set
        m = len(order)
        descs = (_lib.JpegImage * m)()
        data_off = 0
        for k, i in enumerate(order):
            d = parsed[i][0]
            d.data_offset = data_off
            d.out_offset = offs[i]
            data_off += -(-len(blobs[i]) // 16) * 16
            descs[k] = d
        # sub-batches of whole 16-image entropy groups under the workspace cap (one group larger than the cap goes alone)
        sz = C.sizeof(_lib.JpegImage)

        def layout(a, b):            # hirest_jpeg_workspace_bytes of descs[a:b] (also writes their offsets)
            return lib.hirest_jpeg_workspace_bytes(C.cast(C.byref(descs, a * sz), C.POINTER(_lib.JpegImage)), b - a)
        step = 16
        batches, s = [], 0
        while s < m:
            e = min(m, s + step)
            while e < m and e - s + step <= 65535 and layout(s, min(m, e + step)) <= self.workspace_bytes:
                e = min(m, e + step)
            batches.append((s, e))
            s = e
        ws_need = max(layout(a, b) for a, b in batches)   # the final layout of every sub-batch
        # one pinned staging buffer -> one copy: descriptors | tables | compressed bytes
        tsz = C.sizeof(_lib.JpegTables)
        o_tab = -(-m * sz // _ALIGN) * _ALIGN
        o_dat = o_tab + -(-len(sets) * tsz // _ALIGN) * _ALIGN
        total = o_dat + data_off
        host = self._staging(total)
        hp = host.data_ptr()
        C.memmove(hp, descs, m * sz)
        for k, t in enumerate(sets):
            C.memmove(hp + o_tab + k * tsz, C.byref(t), tsz)
        for i in order:
            d = parsed[i][0]
            C.memmove(hp + o_dat + d.data_offset, blobs[i], len(blobs[i]))
        stage = self._buffer("stage", total, device)
        stage[:total].copy_(host[:total], non_blocking=True)
        ws = self._buffer("ws", ws_need, device)
        status = torch.empty(m, dtype=torch.int32, device=device)
        base = stage.data_ptr()
        info = None
        if self.entropy == "chunked":
            info = torch.empty((m, 4), dtype=torch.int32, device=device)
        self._chunk_info = info
        for a, b in batches:
            if info is None:
                _lib.check(lib.hirest_jpeg_decode(C.byref(descs, a * sz), base + a * sz, b - a, base + o_tab, base + o_dat, out.data_ptr(),
                                                  status.data_ptr() + 4 * a, ws.data_ptr(), ws.numel(), ops.stream_ptr()), "hirest_jpeg_decode")
                continue
            cws = self._buffer("chunk_ws", lib.hirest_jpeg_chunked_workspace_bytes(b - a), device)
            _lib.check(lib.hirest_jpeg_decode_chunked(C.byref(descs, a * sz), base + a * sz, b - a, base + o_tab, base + o_dat, out.data_ptr(),
                                                      status.data_ptr() + 4 * a, ws.data_ptr(), ws.numel(), self.chunk_bytes, cws.data_ptr(),
                                                      cws.numel(), ops.stream_ptr()), "hirest_jpeg_decode_chunked")
            info[a:b].copy_(cws[:(b - a) * 16].view(torch.int32).view(b - a, 4))
        st = status.cpu().numpy()               # the one device->host read: which images need the host decode
        bad = [(order[k], int(st[k])) for k in range(m) if st[k] != 0]
        if bad:
            arrs = _pool_map(_pillow, [blobs[i] for i, _ in bad])
            for (i, code), arr in zip(bad, arrs):
                fallbacks.append((i, _status_reason(code)))
                host_px[i] = arr


    def chunk_info(self) -> np.ndarray:
        """int32 [images, 4] of the last chunked call: chunk bytes, lanes, sync rounds, blocks found of every image the
        chunked kernel decoded (rows of zeros: unsupported files and files with a restart interval), in launch order."""
        if self._chunk_info is None:
            return np.zeros((0, 4), np.int32)
        return self._chunk_info.cpu().numpy()


_default = {}


def _decoder(entropy: str = None, chunk_bytes: int = 0) -> Decoder:
    """The module's decoder for an entropy mode; without one, ``HIREST_JPEG_ENTROPY`` or the default decides."""
    entropy = entropy or os.environ.get("HIREST_JPEG_ENTROPY") or DEFAULT_ENTROPY
    key = (entropy, int(chunk_bytes))
    if key not in _default:
        _default[key] = Decoder(entropy=entropy, chunk_bytes=chunk_bytes)
    return _default[key]


def decode(sources: Sequence[Source], device=None, entropy: str = None, chunk_bytes: int = 0):
    """Decode JPEG files (paths, bytes or a mix) on the device.  Returns one uint8 ``[B,H,W,3]`` tensor when every image has the
    same size, else a list of ``[H,W,3]`` tensors (views of one buffer).  ``last_fallbacks`` lists the host-decoded files.
    ``entropy`` / ``chunk_bytes``: see ``Decoder``; None takes ``HIREST_JPEG_ENTROPY``, else the default."""
    return _decoder(entropy, chunk_bytes).decode(sources, device)


def frame_index(path: str) -> int:
    """extract_features.py:46: ``int(name.replace(".jpg", "").split("_")[-1])``."""
    return int(os.path.basename(path).replace(".jpg", "").split("_")[-1])


def list_frame_dir(path) -> List[str]:
    """``<path>/*.jpg`` sorted by the integer after the last ``_`` (not lexically), as extract_features.py:45-46 sorts them."""
    files = glob.glob(os.path.join(str(path), "*.jpg"))
    files.sort(key=frame_index)
    return files


def read_frame_dir(path, device=None, entropy: str = None, chunk_bytes: int = 0):
    """All frames of one video directory, decoded on the device (see ``decode``)."""
    return decode(list_frame_dir(path), device, entropy, chunk_bytes)
