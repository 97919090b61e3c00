"""The device loader on the GPU (hirest_amd/dataset.py + csrc/batch.hip): every batch of the REAL reference's loader
(tests/golden/loader_a.*), the index rules over a sweep of lengths, ragged feature widths against hirest_amd.features on the
host, and the same batch through the joint model in the device layout and in the reference's CPU layout.  Everything is a
gather or integer work: every comparison of a batch is torch.equal.  Through train_step, three float atomic sums of csrc/train.hip
that have no fixed order from run to run for any batch are the only exceptions (assert_same_results says which and how bounded)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_dataset_host import Tok, make_dataset, write_corpus  # noqa: E402

from hirest_amd import dataset as ds, features, synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def corpus(golden_dir, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("loader_corpus"))
    assert "train" not in root and "temp" not in root
    g, z = write_corpus(golden_dir, root)
    return root, g, z


def loader_args(root, cfg, max_words):
    return types.SimpleNamespace(data_dir=root, video_feature_dir=os.path.join(root, "feats"), asr_dir=os.path.join(root, "srt"),
                                 asr_feature_dir=os.path.join(root, "asr"), n_model_frames=cfg["n_model_frames"], distributed=False,
                                 end_to_end=cfg["end_to_end"], max_words=max_words)


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    return v


def test_every_golden_batch_equals_the_reference(dev, corpus):
    root, g, z = corpus
    on_device = {"vis_feats", "vis_mask", "moment_mask", "prev_boundary_mask", "asr_feats", "clip_text_ids", "moment_retrieval_start_target",
                 "moment_retrieval_end_target", "moment_segmentation_target"}
    n_batches = 0
    for cfg in g["configs"]:
        what = (cfg["task"], cfg["split"], cfg["n_model_frames"], cfg["batch_size"], cfg["end_to_end"])
        if cfg["split"] == "test":
            loader = ds.get_moment_loader(loader_args(root, cfg, g["max_words"]), "test", cfg["batch_size"], cfg["task"], device=dev, tokenizer=Tok())
        else:           # the train split is shuffled by get_moment_loader: the golden's sequential order needs the loader built by hand
            d = make_dataset(root, cfg, g["max_words"])
            store = ds.get_feature_store(os.path.join(root, "feats"), os.path.join(root, "srt"), os.path.join(root, "asr"), dev)
            loader = ds.MomentLoader(d, store.attach(d), cfg["batch_size"], shuffle=False)
        assert loader.task == cfg["task"] and len(loader) == len(cfg["batches"]) and len(loader.dataset) == len(cfg["examples"]), what
        got_batches = list(loader)
        assert len(got_batches) == len(cfg["batches"]), what
        for bi, (got, want) in enumerate(zip(got_batches, cfg["batches"])):
            assert list(got.keys()) == list(want.keys()), (what, bi)
            for k, w in want.items():
                if "npz" in w:
                    ref = torch.from_numpy(z[w["npz"]])
                    t = got[k]
                    assert torch.is_tensor(t) and t.is_cuda == (k in on_device), (what, bi, k)
                    assert str(t.dtype) == w["dtype"] and list(t.shape) == w["shape"], (what, bi, k, t.dtype, tuple(t.shape))
                    assert torch.equal(t.cpu(), ref), (what, bi, k)
                else:
                    assert plain(got[k]) == w["value"], (what, bi, k)
            if cfg["task"] == "step_captioning":
                assert torch.equal(got.host["moment_mask"], got["moment_mask"].cpu()) and not got.host["moment_mask"].is_cuda
                for name, f in (("input_caption_ids", 5), ("decoder_mask", 6), ("output_caption_ids", 7)):
                    assert got.device[name].cpu().tolist() == [t[f][0] for t in want["target_text"]["value"]], (what, bi, name)
            else:
                assert not got.host
            n_batches += 1
    assert n_batches == sum(len(c["batches"]) for c in g["configs"])
    assert sum(k[0].startswith(root) for k in ds._STORES) == 1       # every task, split and frame count shared one store
    # the shuffled train split: every epoch is a permutation, epochs differ, set_epoch repeats one
    cfg = next(c for c in g["configs"] if c["split"] == "train" and c["n_model_frames"] == 8 and c["batch_size"] == 3)
    loader = ds.get_moment_loader(loader_args(root, cfg, g["max_words"]), "train", 3, cfg["task"], device=dev, tokenizer=Tok())
    key = lambda batches: [(f, t) for b in batches for f, t in zip(b["video_fnames"], b["moment_segmentation_target"].tolist())]
    first, second = key(loader), key(loader)
    assert sorted(first) == sorted(second) == sorted((e["fname"], e["moment_segmentation_target"]) for e in cfg["examples"])
    assert first != second
    loader.set_epoch(0)
    assert key(loader) == first


def test_index_map_sweep(dev, tmp_path):
    """Frame rows for n in 1 .. 400 plus 571, 1855 and 7200 file rows at six frame counts: features.fit_frame_ids, the rule pinned to the
    real dataset (tests/golden/feature_rules.json).  The row values name (video, row), so a wrong source row cannot pass."""
    lengths = list(range(1, 401)) + [571, 1855, 7200]
    feats = tmp_path / "feats"
    feats.mkdir()
    files, split = [], {"p": {}}
    for v, n in enumerate(lengths):
        x = (v * 8192.0 + torch.arange(n, dtype=torch.float32))[:, None] + torch.arange(4, dtype=torch.float32)[None, :] / 4.0
        torch.save(x, feats / f"v{v}.pt")
        files.append(x)
        split["p"][f"v{v}"] = {"relevant": True, "clip": True, "v_duration": 10.0, "bounds": [1, 5], "steps": []}
    json.dump(split, open(tmp_path / "all_data_test.json", "w"))
    store = ds.DeviceFeatureStore(str(feats), device=dev)
    args = types.SimpleNamespace(end_to_end=False)
    for F in (1, 2, 8, 32, 48, 300):
        d = ds.MomentDataset(args, tmp_path / "all_data_test.json", video_feature_dir=str(feats), n_model_frames=F, task="moment_retrieval")
        batch = next(iter(ds.MomentLoader(d, store.attach(d), len(lengths), shuffle=False)))
        want = torch.stack([x[torch.from_numpy(features.fit_frame_ids(x.shape[0], F, "dataset"))] for x in files])
        got = batch["vis_feats"].cpu()
        assert got.shape == (len(lengths), F, 4)
        bad = (got != want).any(dim=-1).any(dim=-1).nonzero().flatten().tolist()
        assert not bad, (F, [lengths[i] for i in bad[:5]])
        assert bool(batch["vis_mask"].all()) and bool(batch["moment_mask"].all()) and "asr_feats" not in batch
    assert store.frames.shape == (sum(lengths), 4)                   # uploaded once for the six datasets


def stamp(sec):
    return f"{sec // 3600:02d}:{sec // 60 % 60:02d}:{sec % 60:02d},250"


@pytest.mark.parametrize("D,Da", [(1024, 384), (20, 6), (1, 1)])
def test_ragged_widths_against_the_host_rules(dev, tmp_path, D, Da):
    """Widths that are whole 16-byte vectors, vectors with every row at another alignment, and single floats; B = 1 and 5; T <= 64;
    n_model_frames -1 (ragged, zero padded) and 24 (sub- and up-sampled): features.fit_frames / fit_asr on the host."""
    gen = torch.Generator().manual_seed(1000 * D + Da)
    lengths = [7, 64, 33, 16, 50]
    for sub in ("feats", "srt", "asr"):
        (tmp_path / sub).mkdir()
    vis, asr, spans, split = [], [], [], {"p": {}}
    for v, n in enumerate(lengths):
        # edge spans first: start == end, running past the end, starting at and after the end, inverted, two that overlap
        sp = [(3, 3), (n - 2, n + 9), (n, n + 4), (n + 1, n + 2), (5, 2), (1, 6), (4, 9)]
        sp += [tuple(sorted(torch.randint(0, n + 6, (2,), generator=gen).tolist())) for _ in range(0 if v == 3 else 70 if v == 1 else 5)]
        if v == 3:
            sp = []                                                  # a video without subtitles
        x, y = torch.randn(n, D, generator=gen), torch.randn(len(sp), Da, generator=gen)
        torch.save(x, tmp_path / "feats" / f"v{v}.mp4.pt")
        torch.save(y, tmp_path / "asr" / f"v{v}.pt")
        with open(tmp_path / "srt" / f"v{v}.srt", "w") as f:
            f.write("".join(f"{i + 1}\n{stamp(s)} --> {stamp(e)}\ntext\n\n" for i, (s, e) in enumerate(sp)))
        vis.append(x); asr.append(y); spans.append(sp)
        split["p"][f"v{v}.mp4"] = {"relevant": True, "clip": True, "v_duration": float(n), "bounds": [0, 3], "steps": []}
    json.dump(split, open(tmp_path / "all_data_test.json", "w"))
    store = ds.DeviceFeatureStore(str(tmp_path / "feats"), str(tmp_path / "srt"), str(tmp_path / "asr"), device=dev)
    args = types.SimpleNamespace(end_to_end=False)
    for F in (-1, 24):
        d = ds.MomentDataset(args, tmp_path / "all_data_test.json", video_feature_dir=str(tmp_path / "feats"), asr_dir=str(tmp_path / "srt"),
                             asr_feature_dir=str(tmp_path / "asr"), n_model_frames=F, task="moment_retrieval")
        assert d.videoid2asr == {f"v{v}": spans[v] for v in range(5)}
        tables = store.attach(d)
        fitted = [features.fit_frames(x, F, "dataset") for x in vis]
        warped = [features.fit_asr(asr[v], spans[v], fitted[v], F) for v in range(5)]
        for B in (1, 5):
            for bi, batch in enumerate(ds.MomentLoader(d, tables, B, shuffle=False)):
                members = list(range(bi * B, bi * B + B))
                T = max(fitted[v].shape[0] for v in members)
                pad = lambda t: torch.cat([t, torch.zeros(T - t.shape[0], t.shape[1])])
                assert torch.equal(batch["vis_feats"].cpu(), torch.stack([pad(fitted[v]) for v in members])), (F, B, bi)
                assert torch.equal(batch["asr_feats"].cpu(), torch.stack([pad(warped[v]) for v in members])), (F, B, bi)
                want_mask = torch.stack([(torch.arange(T) < fitted[v].shape[0]).long() for v in members])
                assert torch.equal(batch["vis_mask"].cpu(), want_mask) and torch.equal(batch["moment_mask"].cpu(), want_mask)


class ModelArgs:
    clip_model_name = "EVA_CLIP_tiny_e1024_test"
    clip_pretrained = "synth:11"
    visual_num_hidden_layers = 2
    moment_segmentation_difference_threshold = 0.5
    moment_segmentation_max_iterations = 20


@pytest.fixture(scope="module")
def model_and_corpus(dev, golden_dir, tmp_path_factory):
    """The synthetic joint model of the existing joint tests (with its tiny text tower), and the golden's split over feature files of
    the model's widths (1024 / 384)."""
    import hirest_amd
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(golden_dir, "joint_schema.json"))).items()}
    sd = synth.joint_state_dict(shapes, 31)
    sd["clip4cap_model.decoder.classifier.cls.predictions.bias"][102] += 1.5
    model = hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=ModelArgs())
    model.load_state_dict(sd, strict=False)
    model = model.to(dev).eval()
    root = str(tmp_path_factory.mktemp("loader_model_corpus"))
    g, _ = write_corpus(golden_dir, root)
    gen = torch.Generator().manual_seed(5)
    for name, n in g["videos"].items():
        x = torch.randn(n, 1024, generator=gen)
        torch.save(x / x.norm(dim=-1, keepdim=True), os.path.join(root, "feats", f"{name}.pt"))
    for vid, sp in g["spans"].items():
        torch.save(0.05 * torch.randn(len(sp), 384, generator=gen), os.path.join(root, "asr", f"{vid}.pt"))
    return model, root, g


def cpu_layout(batch):
    """The same batch as the reference's collate_fn hands it over: a plain dict of CPU tensors and lists."""
    return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in batch.items()}


def first_batches(root, g, dev, cache_text=None, batch_size=3):
    out = {}
    for name, task, split in (("retrieval", "moment_retrieval", "test"), ("segmentation_train", "moment_segmentation", "train"),
                              ("segmentation", "moment_segmentation", "test"), ("captioning", "step_captioning", "test")):
        cfg = {"n_model_frames": 48, "end_to_end": False}
        loader = ds.get_moment_loader(loader_args(root, cfg, 12), split, batch_size, task, cache_text=cache_text, device=dev, tokenizer=Tok(), seed=3)
        out[name] = next(iter(loader))
    return out


TIED = "clip4cap_model.decoder.embeddings.word_embeddings.weight"


def run_model(model, batches):
    """test_step of the three tasks and train_step (loss and every gradient) of the three tasks on `batches`."""
    res = {}
    for name in ("retrieval", "segmentation", "captioning"):
        kw = {"num_beams": 3} if name == "captioning" else {}
        res["test." + name] = model.test_step(batches[name], **kw)["prediction"]
    for name in ("retrieval", "segmentation_train", "captioning"):
        for p in model.parameters():
            p.grad = None
        loss = model.train_step(batches[name])["loss"]
        loss.backward()
        res["loss." + name] = loss.detach().cpu()
        res["grad." + name] = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}
    for p in model.parameters():
        p.grad = None
    return res


def assert_same_results(a, b, caption_rows):
    """Bit equality of everything the kernels compute in a fixed order.  Two quantities are float atomic sums in csrc/train.hip whose
    order is not fixed from run to run, for ANY batch layout: the captioning loss (ce_rows_kernel: one atomicAdd per row) and the
    embedding share of the tied word-embedding gradient (an atomic scatter-add; tests/test_gpu_train.py gives it the same
    exemption and bound).  Reordering a sum of n non-negative fp32 terms moves it by at most 2 (n - 1) 2^-24 of the sum."""
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("grad."):
            assert a[k].keys() == b[k].keys() and len(a[k]) > 10, k
            for n in a[k]:
                if n == TIED and k == "grad.captioning":
                    assert torch.allclose(a[k][n], b[k][n], rtol=1e-4, atol=1e-8), (k, n)
                else:
                    assert torch.equal(a[k][n], b[k][n]), (k, n)
        elif k == "loss.captioning":
            assert bool(torch.isfinite(a[k])) and abs(float(a[k]) - float(b[k])) <= 2 * (caption_rows - 1) * 2.0 ** -24 * abs(float(a[k])), (k, a[k], b[k])
        elif k.startswith("loss."):
            assert torch.equal(a[k], b[k]) and bool(torch.isfinite(a[k])), (k, float(a[k]).hex(), float(b[k]).hex())
        else:
            assert a[k] == b[k] and len(a[k]) == 2, k


def test_device_batches_through_the_models_equal_the_cpu_layout(dev, model_and_corpus):
    """B = 2: the masked cross-entropy of segmentation training adds one term per sample to the loss with atomicAdd (ce_masked_kernel);
    two terms commute, three need not, so at B = 2 every loss but the captioning one is defined bit for bit."""
    model, root, g = model_and_corpus
    batches = first_batches(root, g, dev, batch_size=2)
    assert all(isinstance(b, ds.DeviceBatch) and b["vis_feats"].is_cuda and b["vis_feats"].shape == (2, 48, 1024) for b in batches.values())
    assert "text_feat" not in batches["retrieval"]
    on_device = run_model(model, batches)
    on_host = run_model(model, {k: cpu_layout(b) for k, b in batches.items()})
    assert_same_results(on_device, on_host, caption_rows=2 * 12)


def test_text_cache_equals_the_clip_text_ids_path(dev, model_and_corpus):
    model, root, g = model_and_corpus
    plain_batches = first_batches(root, g, dev, batch_size=2)
    cached = first_batches(root, g, dev, cache_text=model, batch_size=2)
    for name, b in cached.items():
        ids = plain_batches[name]["clip_text_ids"]
        assert torch.equal(b["clip_text_ids"], ids) and b["text_feat"].is_cuda and b["text_feat"].shape == (2, 1024)
        assert list(b.keys()) == list(plain_batches[name].keys()) + ["text_feat"]
        # one tower call per distinct prompt of the split, gathered by row == the tower on the batch's own ids
        assert torch.equal(b["text_feat"], model.clip_model.encode_text(ids).float()), name
    assert_same_results(run_model(model, cached), run_model(model, plain_batches), caption_rows=2 * 12)
