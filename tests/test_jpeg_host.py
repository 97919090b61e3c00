"""Baseline-JPEG decode on the host core (hirest_jpeg_parse / hirest_jpeg_decode_host): the same arithmetic the gfx950
kernels run, pinned bit for bit against Pillow's Image.open(f).convert("RGB") on libjpeg-turbo."""
import io

import numpy as np
import pytest

PIL = pytest.importorskip("PIL")
from PIL import Image, features  # noqa: E402

if not features.check_feature("libjpeg_turbo"):
    pytest.skip("Pillow is not built on libjpeg-turbo: the bit-exact targets are libjpeg-turbo's", allow_module_level=True)

from hirest_amd import jpeg  # noqa: E402

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


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


def assert_exact(data):
    got, st = jpeg.decode_host(data)
    assert st == 0, st
    ref = pillow(data)
    assert got.shape == ref.shape
    if not np.array_equal(got, ref):
        d = np.abs(got.astype(int) - ref)
        pytest.fail(f"max |diff| {d.max()}, {(d > 0).sum()} samples differ")


def test_parse_geometry_sampling_restart():
    a = content("gradient", 37, 53)
    for name, ss, hv in (("444", 0, (1, 1)), ("422", 1, (2, 1)), ("420", 2, (2, 2))):
        img, _ = jpeg.parse(encode(a, quality=90, subsampling=ss))
        assert img.supported == 1 and img.reason == 0
        assert (img.height, img.width, img.ncomp, (img.hs, img.vs)) == (37, 53, 3, hv), name
        assert (img.mcux, img.mcuy) == (-(-53 // (8 * hv[0])), -(-37 // (8 * hv[1])))
        assert img.restart_interval == 0
        assert 0 < img.scan_begin < img.scan_end
    img, _ = jpeg.parse(encode(a[..., 0], quality=90))
    assert (img.ncomp, img.hs, img.vs, img.supported) == (1, 1, 1, 1)
    img, _ = jpeg.parse(encode(a, quality=90, subsampling=2, restart_marker_blocks=4))
    assert img.restart_interval == 4
    img, _ = jpeg.parse(encode(a, quality=90, subsampling=2, restart_marker_rows=1))
    assert img.restart_interval == img.mcux == 4


def test_parse_marks_unsupported_files():
    a = content("gradient", 40, 48)
    prog = encode(a, quality=80, progressive=True)
    img, _ = jpeg.parse(prog)
    assert (img.supported, img.reason) == (0, 2)
    full = encode(a, quality=80)
    assert full[-2:] == b"\xff\xd9"
    img, _ = jpeg.parse(full[:-2])                          # EOI cut off
    assert (img.supported, img.reason) == (0, 9)
    img, _ = jpeg.parse(full[: len(full) // 2])             # cut inside the scan
    assert (img.supported, img.reason) == (0, 9)
    b = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(b, "JPEG", quality=80)
    img, _ = jpeg.parse(b.getvalue())
    assert (img.supported, img.reason) == (0, 6)
    img, _ = jpeg.parse(b"not a jpeg at all")
    assert (img.supported, img.reason) == (0, 1)
    for data in (prog, full[:-2]):
        out, st = jpeg.decode_host(data)
        assert st == 16 and out.size == 0


SIZES = [(1, 1), (7, 9), (8, 8), (15, 17), (16, 16), (17, 33), (37, 53), (361, 641)]


@pytest.mark.parametrize("sub", ["444", "422", "420", "grey"])
def test_decode_matches_pillow_matrix(sub):
    """sizes x quality x optimize x restart x content, a rotating subset of the product (every value of every axis is
    exercised for every subsampling)."""
    kinds = ["flat", "gradient", "saturated", "noise"]
    quals = [1, 5, 50, 75, 95, 100]
    extras = [{}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_blocks": 4}, {"restart_marker_rows": 1}]
    n = 0
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
                assert_exact(encode(a, **kw))
                n += 1
    assert n >= 90


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5])
def test_low_quality_noise_exercises_the_range_limit(q):
    """quality 1-5 on noise: IDCT outputs far outside 0..255, clamped as libjpeg-turbo clamps them."""
    a = content("noise", 64, 96, seed=q)
    for ss in (0, 2):
        assert_exact(encode(a, quality=q, subsampling=ss))
        assert_exact(encode(a, quality=q, subsampling=ss, optimize=True))


def test_large_frames():
    from hirest_amd import synth
    a = synth.rgb_frames("jpeg.host.720", (720, 1280, 3), 3)
    assert_exact(encode(a, quality=95, subsampling=2))
    assert_exact(encode(a, quality=75, subsampling=1, restart_marker_rows=2))
    y, x = np.mgrid[0:1080, 0:1920]
    rng = np.random.default_rng(5)
    smooth = np.stack([x // 8, y // 5, (x + y) // 12], -1) + rng.integers(-3, 4, (1080, 1920, 3))
    assert_exact(encode(smooth.clip(0, 255).astype(np.uint8), quality=95, subsampling=2))


def test_app_and_com_segments_are_skipped():
    a = content("gradient", 33, 47)
    ex = Image.Exif()
    ex[0x010F] = "maker"
    ex[0x0110] = "model"
    data = encode(a, quality=85, exif=ex.tobytes(), comment=b"a comment segment")
    assert b"Exif" in data and b"\xff\xfe" in data
    assert_exact(data)


def test_garbage_in_the_scan_sets_a_flag_or_decodes_like_pillow():
    """Corrupted entropy-coded bytes: the decoder either reports an anomaly (the caller then takes Pillow's result) or
    decodes exactly what libjpeg-turbo decodes.  It never reads outside [scan_begin, scan_end)."""
    a = content("noise", 48, 64)
    base = encode(a, quality=90, subsampling=2)
    img, _ = jpeg.parse(base)
    b0, b1 = img.scan_begin, img.scan_end
    rng = np.random.default_rng(1)
    flagged = 0
    cases = []
    for t in range(40):
        d = bytearray(base)
        lo = int(rng.integers(b0, b1 - 8))
        n = int(rng.integers(1, 8))
        d[lo:lo + n] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        cases.append(bytes(d))
    cases.append(base[:b0] + b"\xff" * 8 + base[b0 + 8:])                  # all-ones: no valid code
    cases.append(base[:b0 + 40] + b"\xff\xd9")                              # scan cut short, EOI kept
    cases.append(base[:b0 + 40] + b"\xff\xd3" + base[b0 + 40:])             # an RSTn where none belongs
    for data in cases:
        im, _ = jpeg.parse(data)
        got, st = jpeg.decode_host(data)
        if st:
            flagged += 1
            continue
        assert np.array_equal(got, pillow(data))
    assert flagged >= 3
    # out of data at the very end of the buffer: the reader feeds zero bits and raises the flag
    got, st = jpeg.decode_host(base[:b0 + 4] + b"\xff\xd9")
    assert st & 4


def test_restart_markers_out_of_sequence_are_flagged():
    a = content("noise", 32, 64)
    data = bytearray(encode(a, quality=90, subsampling=2, restart_marker_blocks=1))
    img, _ = jpeg.parse(bytes(data))
    i = data.index(b"\xff\xd1", img.scan_begin)
    data[i + 1] = 0xD5
    got, st = jpeg.decode_host(bytes(data))
    assert st & 8


def test_frame_dir_order_is_integer_order(tmp_path):
    for name in ("frame_2.jpg", "frame_10.jpg", "frame_1.jpg", "x_frame_0.jpg"):
        (tmp_path / name).write_bytes(b"")
    got = [p.split("/")[-1] for p in jpeg.list_frame_dir(tmp_path)]
    assert got == ["x_frame_0.jpg", "frame_1.jpg", "frame_2.jpg", "frame_10.jpg"]
