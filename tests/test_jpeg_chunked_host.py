"""Chunked entropy decode on the host core (hirest_jpeg_decode_host_chunked): the sync / scan / write sequence of
jpeg_entropy_chunked_kernel run one lane after another must give the bytes of the serial decode (hirest_jpeg_decode_host), and
through it Pillow's, for every chunk size; and a non-zero status for exactly the inputs the serial decode flags."""
import io

import numpy as np
import pytest

PIL = pytest.importorskip("PIL")
from PIL import Image, features  # noqa: E402

if not features.check_feature("libjpeg_turbo"):
    pytest.skip("Pillow is not built on libjpeg-turbo: the bit-exact targets are libjpeg-turbo's", allow_module_level=True)

from hirest_amd import jpeg  # noqa: E402

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
CHUNK_BYTES = [16, 64, 256, 0]
SIZES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 33), (37, 53), (361, 641)]


# the inputs of tests/test_jpeg_host.py, re-stated
def content(kind, h, w, seed=0):
    rng = np.random.default_rng(seed + h * 131 + w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (30, 140, 220), np.uint8)
    if kind == "saturated":
        a = np.zeros((h, w, 3), np.uint8)
        a[:, : w // 2, 0] = 255
        a[h // 2:, :, 2] = 255
        a[: h // 3, :, 1] = 255
        return a
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), ((x + y) * 3) % 256], -1).astype(np.uint8)


def encode(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


def pillow(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def chunks_of(data, chunk_bytes):
    """(number of chunks, chunk bytes used) by the documented rule: a given size as it is, 0 = max(256, ceil(scan / 1024))."""
    img, _ = jpeg.parse(data)
    n = img.scan_end - img.scan_begin
    cb = chunk_bytes or max(256, -(-n // 1024))
    return -(-n // cb), cb


def boundary_in_stuffing(data, chunk_bytes):
    """True when a chunk of this file begins at the 0x00 stuffed after an 0xFF."""
    img, _ = jpeg.parse(data)
    n, cb = chunks_of(data, chunk_bytes)
    return any(data[img.scan_begin + k * cb - 1] == 0xFF and data[img.scan_begin + k * cb] == 0 for k in range(1, n))


def nblocks(data):
    img, _ = jpeg.parse(data)
    per_mcu = img.hs * img.vs + (2 if img.ncomp == 3 else 0)
    return img.mcux * img.mcuy * per_mcu


class Seen:
    """What the clean images of a test exercised, from the input bytes and the returned counters."""

    def __init__(self):
        self.images = self.corrected = self.empty_chunk = self.split_stuffing = 0

    def check(self, data, ref=None):
        """Chunked == serial == Pillow for every chunk size; status 0; rounds within the bound."""
        host, st = jpeg.decode_host(data)
        assert st == 0, st
        if ref is None:
            ref = pillow(data)
        assert np.array_equal(host, ref)
        self.images += 1
        for cb in CHUNK_BYTES:
            got, st, rounds = jpeg.decode_host_chunked(data, cb)
            n, used = chunks_of(data, cb)
            assert st == 0, (cb, st)                       # a clean image is never excused as a fallback
            assert got.shape == ref.shape and np.array_equal(got, ref), (cb, used)
            assert 1 <= rounds <= n, (cb, rounds, n)
            self.corrected += rounds >= 2
            self.empty_chunk += n > nblocks(data)          # more chunks than blocks: some chunk owns none
            self.split_stuffing += boundary_in_stuffing(data, cb)


def matrix(sub):
    """test_jpeg_host.py's rotating product; files with a restart interval are returned apart (kw, bytes)."""
    kinds = ["flat", "gradient", "saturated", "noise"]
    quals = [1, 5, 50, 75, 95, 100]
    extras = [{}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 4}, {"restart_marker_rows": 1}]
    plain, restart = [], []
    for si, (h, w) in enumerate(SIZES):
        for qi, q in enumerate(quals):
            for ki, kind in enumerate(kinds):
                if (si + qi + ki) % 2:
                    continue
                a = content(kind, h, w, seed=qi)
                if sub == "grey":
                    a = a[..., 1]
                kw = dict(extras[(si + qi + ki) % len(extras)], quality=q)
                if sub != "grey":
                    kw["subsampling"] = SUBSAMPLING[sub]
                (restart if any(k.startswith("restart") for k in kw) else plain).append(encode(a, **kw))
    return plain, restart


@pytest.mark.parametrize("sub", ["444", "422", "420", "grey"])
def test_chunked_equals_serial_and_pillow_matrix(sub):
    plain, restart = matrix(sub)
    assert len(plain) >= 35 and len(restart) >= 35
    seen = Seen()
    for data in plain:
        seen.check(data)
    assert seen.corrected > 0
    # restart intervals are not this function's: it says so instead of decoding them its own way
    for data in restart[:3]:
        assert jpeg.parse(data)[0].restart_interval > 0
        with pytest.raises(RuntimeError):
            jpeg.decode_host_chunked(data, 64)


def test_q100_noise_tiny_chunks_empty_lanes_split_stuffing_and_corrections():
    """q100 noise: a block is longer than a 16-byte chunk, so chunks without a block exist (more chunks than blocks), 0xFF 0x00
    pairs are frequent enough for a chunk boundary to fall inside one, and the first guesses are mostly wrong."""
    seen = Seen()
    for seed, (h, w) in enumerate([(64, 64), (120, 200), (33, 47)]):
        a = content("noise", h, w, seed=seed)
        for ss in (0, 1, 2):
            seen.check(encode(a, quality=100, subsampling=ss))
        seen.check(encode(a[..., 0], quality=100))
    assert seen.empty_chunk > 0 and seen.split_stuffing > 0 and seen.corrected > 0, vars(seen)
    # the named case on its own: q100 noise, chunk_bytes = 16
    data = encode(content("noise", 64, 64), quality=100, subsampling=0)
    n, _ = chunks_of(data, 16)
    assert n > nblocks(data)
    got, st, rounds = jpeg.decode_host_chunked(data, 16)
    assert st == 0 and rounds >= 2 and np.array_equal(got, pillow(data))


def test_low_quality_noise_and_optimised_tables():
    seen = Seen()
    for q in (1, 3, 5):
        a = content("noise", 64, 96, seed=q)
        for ss in (0, 2):
            seen.check(encode(a, quality=q, subsampling=ss))
            seen.check(encode(a, quality=q, subsampling=ss, optimize=True))
    assert seen.images == 12


def test_large_frames_and_segments():
    from hirest_amd import synth
    seen = Seen()
    a = synth.rgb_frames("jpeg.host.720", (720, 1280, 3), 3)
    seen.check(encode(a, quality=95, subsampling=2))
    y, x = np.mgrid[0:1080, 0:1920]
    rng = np.random.default_rng(5)
    smooth = np.stack([x // 8, y // 5, (x + y) // 12], -1) + rng.integers(-3, 4, (1080, 1920, 3))
    seen.check(encode(smooth.clip(0, 255).astype(np.uint8), quality=95, subsampling=2))
    ex = Image.Exif()
    ex[0x010F] = "maker"
    ex[0x0110] = "model"
    data = encode(content("gradient", 33, 47), quality=85, exif=ex.tobytes(), comment=b"a comment segment")
    assert b"Exif" in data and b"\xff\xfe" in data
    seen.check(data)
    assert seen.corrected > 0


def corrupt_cases():
    """The byte-flip recipe of test_jpeg_host.py's anomaly test, then scans cut in the middle of a chunk and at a chunk
    boundary (for chunk_bytes 16, 64 and 256: 512 is a boundary of all three, 40 and 1000 of none)."""
    a = content("noise", 48, 64)
    base = encode(a, quality=90, subsampling=2)
    img, _ = jpeg.parse(base)
    b0, b1 = img.scan_begin, img.scan_end
    assert b1 - b0 > 1200
    rng = np.random.default_rng(1)
    cases = []
    for t in range(40):
        d = bytearray(base)
        lo = int(rng.integers(b0, b1 - 8))
        n = int(rng.integers(1, 8))
        d[lo:lo + n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cases.append(bytes(d))
    cases.append(base[:b0] + b"\xff" * 8 + base[b0 + 8:])                  # all-ones: no valid code
    cases.append(base[:b0 + 40] + b"\xff\xd3" + base[b0 + 40:])             # an RSTn where none belongs
    for cut in (40, 1000, 512, 256, 1024, 4):
        cases.append(base[:b0 + cut] + b"\xff\xd9")                         # scan cut short, EOI kept
    return cases


def test_corrupt_scans_are_flagged_exactly_when_the_serial_decode_flags_them():
    flagged = clean = 0
    for data in corrupt_cases():
        img, _ = jpeg.parse(data)
        if not img.supported:
            assert jpeg.decode_host_chunked(data, 16)[1] == 16
            continue
        ref, st = jpeg.decode_host(data)
        for cb in CHUNK_BYTES:
            got, st2, rounds = jpeg.decode_host_chunked(data, cb)
            assert (st2 != 0) == (st != 0), (cb, st, st2)
            assert rounds <= chunks_of(data, cb)[0]
            if st == 0:
                assert np.array_equal(got, ref), cb
        flagged += st != 0
        clean += st == 0
    assert flagged >= 8 and clean >= 1, (flagged, clean)


def test_nothing_outside_the_scan_is_read():
    """Descriptor and tables come from the real file; the decode then runs over a buffer in which every byte outside
    [scan_begin, scan_end) is different.  Status and pixels must not notice, for clean and for corrupt scans (which run past
    their data and get zero bits, not the bytes behind the scan)."""
    rng = np.random.default_rng(7)
    files = corrupt_cases()[::3] + [encode(content("noise", 40, 56), quality=100, subsampling=0)]
    checked = 0
    for data in files:
        img, _ = jpeg.parse(data)
        if not img.supported:
            continue
        other = np.frombuffer(data, np.uint8).copy()
        mask = np.ones(len(data), bool)
        mask[img.scan_begin:img.scan_end] = False
        other[mask] ^= rng.integers(1, 256, int(mask.sum()), dtype=np.uint8)
        for cb in (16, 0):
            a, sa, ra = jpeg.decode_host_chunked(data, cb)
            b, sb, rb = jpeg.decode_host_chunked(data, cb, scan=other.tobytes())
            assert (sa, ra) == (sb, rb) and np.array_equal(a, b)
            checked += 1
    assert checked >= 10
