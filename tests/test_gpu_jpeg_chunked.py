"""Chunked entropy decode on the device (hirest_jpeg_decode_chunked, Decoder(entropy="chunked")) against the one-lane-per-image
decoder, the host core and Pillow, and through the frame-directory paths with HIREST_JPEG_ENTROPY=chunked."""
import io

import numpy as np
import pytest
import torch
from PIL import Image, features

from hirest_amd import synth

pytestmark = pytest.mark.gpu

SUBS = {"444": 0, "422": 1, "420": 2, "grey": None}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("Pillow is not built on libjpeg-turbo")


def _content(kind, h, w, seed=0):
    rng = np.random.default_rng(seed + 7 * h + w)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1)
    return (g + rng.integers(-3, 4, (h, w, 3))).clip(0, 255).astype(np.uint8)      # "smooth": a gradient with mild noise


def _enc(a, sub=None, **kw):
    if sub is not None:
        if SUBS[sub] is None:
            a = a[..., 0]
        else:
            kw["subsampling"] = SUBS[sub]
    b = io.BytesIO()
    Image.fromarray(a).save(b, "JPEG", **kw)
    return b.getvalue()


def _pillow(data):
    return torch.from_numpy(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy())


def _check_one(data, chunk_bytes, dev):
    """One image alone: chunked == lanes == host core == Pillow, no fallback; returns the lane statistics row."""
    from hirest_amd import jpeg
    chunked = jpeg.Decoder(entropy="chunked", chunk_bytes=chunk_bytes)
    got = chunked.decode([data], dev)[0].cpu()
    assert chunked.last_fallbacks == [] and jpeg.last_fallbacks == []
    lanes = jpeg.Decoder(entropy="lanes").decode([data], dev)[0].cpu()
    host, st = jpeg.decode_host(data)
    assert st == 0
    assert torch.equal(got, lanes)
    assert torch.equal(got, torch.from_numpy(host))
    assert torch.equal(got, _pillow(data))
    info = chunked.chunk_info()
    assert info.shape == (1, 4)
    return info[0]


@pytest.mark.parametrize("sub", list(SUBS))
def test_single_small_images_one_lane(sub):
    _need_gpu()
    dev = torch.device("cuda:0")
    for k, (h, w) in enumerate([(1, 1), (8, 8), (17, 13), (33, 47)]):
        data = _enc(_content("smooth", h, w, seed=k), sub, quality=75)
        cb, lanes, rounds, found = _check_one(data, 4096, dev)
        assert (lanes, rounds) == (1, 1) and cb == 4096           # the scan is smaller than one chunk: one lane does the work


@pytest.mark.parametrize("chunk_bytes", [16, 64])
def test_blocks_straddling_chunks(chunk_bytes):
    _need_gpu()
    from hirest_amd import jpeg
    dev = torch.device("cuda:0")
    empty = corrected = 0
    for h, w in [(64, 64), (120, 200)]:
        for kind in ("noise", "smooth"):
            data = _enc(_content(kind, h, w), "444", quality=100)
            cb, lanes, rounds, found = _check_one(data, chunk_bytes, dev)
            img, _ = jpeg.parse(data)
            n = img.scan_end - img.scan_begin
            assert cb == max(chunk_bytes, -(-n // 1024)) and lanes == -(-n // cb) and 1 <= rounds <= lanes
            assert rounds == jpeg.decode_host_chunked(data, cb)[2]          # the host model runs the same rounds
            assert found >= img.mcux * img.mcuy * 3
            empty += lanes > img.mcux * img.mcuy * 3                        # more lanes than blocks: some own nothing
            corrected += rounds >= 2
    assert corrected > 0
    if chunk_bytes == 16:
        assert empty > 0


def test_360p_frame_chosen_chunks():
    _need_gpu()
    dev = torch.device("cuda:0")
    frame = synth.rgb_frames("jpeg.chunked.360", (360, 640, 3), 1)
    cb, lanes, rounds, found = _check_one(_enc(frame, "420", quality=95), 0, dev)
    assert cb >= 256 and 1 < lanes <= 1024 and rounds <= lanes


def _mixed_files():
    files = []
    for k, (h, w, sub, q) in enumerate([(40, 56, "444", 90), (37, 53, "422", 50), (120, 160, "420", 95), (17, 33, "grey", 75),
                                         (64, 64, "444", 100), (96, 128, "420", 5)]):
        files.append(_enc(_content("noise" if k % 2 else "smooth", h, w, seed=k), sub, quality=q))
    files.append(_enc(_content("noise", 48, 64, seed=9), "420", quality=90, optimize=True))        # a second Huffman table set
    files.append(_enc(_content("smooth", 48, 64, seed=10), "444", quality=50, optimize=True))      # and a third
    files.append(_enc(_content("noise", 40, 72, seed=11), "420", quality=90, restart_marker_blocks=4))
    files.append(_enc(_content("smooth", 33, 47, seed=12), "422", quality=75, restart_marker_rows=1))
    files.append(_enc(_content("noise", 40, 56, seed=13), "420", quality=80, progressive=True))
    good = _enc(_content("noise", 48, 64, seed=17), "420", quality=90)      # a seed whose corrupted scan Pillow still decodes
    return files, good


def test_mixed_batch_equals_pillow_with_the_lanes_decoders_fallbacks():
    _need_gpu()
    from hirest_amd import jpeg
    dev = torch.device("cuda:0")
    files, good = _mixed_files()
    img, _ = jpeg.parse(good)
    bad = good[:img.scan_begin] + b"\xff" * 8 + good[img.scan_begin + 8:]
    assert jpeg.parse(bad)[0].supported == 1 and jpeg.decode_host(bad)[1] != 0      # reaches the device and is flagged there
    files += [good, bad]
    assert len({bytes(jpeg.parse(f)[1]) for f in files if jpeg.parse(f)[0].supported}) >= 3
    lanes = jpeg.Decoder(entropy="lanes")
    ref = lanes.decode(files, dev)
    for chunk_bytes in (0, 16):
        dec = jpeg.Decoder(entropy="chunked", chunk_bytes=chunk_bytes)
        out = dec.decode(files, dev)
        assert isinstance(out, list) and len(out) == len(files)
        assert dec.last_fallbacks == lanes.last_fallbacks
        assert sorted(i for i, _ in dec.last_fallbacks) == [len(files) - 3, len(files) - 1]       # progressive, corrupt
        for i, data in enumerate(files):
            assert torch.equal(out[i].cpu(), _pillow(data)), i
            assert torch.equal(out[i], ref[i]), i
        info = dec.chunk_info()
        assert info.shape == (len(files) - 1, 4)                  # the progressive file never reaches the device
        assert (info[:, 1] == 0).sum() == 2                       # the restart-interval files took the one-lane kernel
    # the keyword on the module function
    out = jpeg.decode(files, dev, entropy="chunked", chunk_bytes=64)
    assert jpeg.last_fallbacks == lanes.last_fallbacks
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    with pytest.raises(ValueError):
        jpeg.Decoder(entropy="waves")


def test_an_image_alone_and_inside_a_batch_of_16():
    _need_gpu()
    from hirest_amd import jpeg
    dev = torch.device("cuda:0")
    frames = synth.rgb_frames("jpeg.chunked.batch", (16, 120, 160, 3), 2)
    files = [_enc(f, "420", quality=95) for f in frames]
    dec = jpeg.Decoder(entropy="chunked")
    batch = dec.decode(files, dev).clone()
    assert batch.shape == (16, 120, 160, 3) and dec.last_fallbacks == []
    for i in (0, 7, 15):
        alone = dec.decode([files[i]], dev)
        assert torch.equal(alone[0], batch[i]), i
        assert torch.equal(batch[i].cpu(), _pillow(files[i])), i


def _tiny_model(dev):
    import hirest_amd
    model, transform = hirest_amd.build_eva_model_and_transforms("EVA_CLIP_tiny_test", pretrained="synth:11", precision="bf16")
    return model.to(dev).eval(), transform


def test_frame_directory_paths_with_the_environment_switch(tmp_path, monkeypatch):
    _need_gpu()
    from hirest_amd import features as FT
    from hirest_amd import jpeg
    dev = torch.device("cuda:0")
    model, _ = _tiny_model(dev)
    src = tmp_path / "frames"
    for v, (T, h, w) in enumerate([(20, 120, 160), (18, 90, 176)]):
        d = src / f"vid{v}"
        d.mkdir(parents=True)
        fr = synth.rgb_frames(f"jpeg.chunked.vid{v}", (T, h, w, 3), 4 + v)
        for t in range(T):
            (d / f"frame_{t}.jpg").write_bytes(_enc(fr[t], "420", quality=95))
    monkeypatch.delenv("HIREST_JPEG_ENTROPY", raising=False)
    assert jpeg._decoder().entropy == "lanes" or jpeg.DEFAULT_ENTROPY == "chunked"
    names = FT.extract_frame_dir(model, str(src), str(tmp_path / "out_default"))
    frames_default = [jpeg.read_frame_dir(src / n, dev).clone() for n in sorted(names)]
    monkeypatch.setenv("HIREST_JPEG_ENTROPY", "chunked")
    assert jpeg._decoder().entropy == "chunked" and jpeg.Decoder().entropy == "chunked"
    assert FT.extract_frame_dir(model, str(src), str(tmp_path / "out_chunked")) == names
    assert jpeg._decoder().chunk_info()[:, 1].min() >= 1          # the last call did go through the chunked kernel
    for k, n in enumerate(sorted(names)):
        a = torch.load(str(tmp_path / "out_default" / f"{n}.pt"))
        b = torch.load(str(tmp_path / "out_chunked" / f"{n}.pt"))
        assert torch.equal(a, b), n
        got = jpeg.read_frame_dir(src / n, dev)
        assert torch.equal(got, frames_default[k]), n
        assert torch.equal(got, jpeg.read_frame_dir(src / n, dev, entropy="lanes")), n
        paths = jpeg.list_frame_dir(src / n)
        assert torch.equal(got[0].cpu(), _pillow(open(paths[0], "rb").read()))
    monkeypatch.setenv("HIREST_JPEG_ENTROPY", "nonsense")
    with pytest.raises(ValueError):
        jpeg.decode([open(paths[0], "rb").read()], dev)
