"""Host side of the device loader (hirest_amd/dataset.py) against the REAL reference's loader (tests/golden/loader_a.*, made by
make_loader_golden.py): the example lists with their masks, MultitaskLoader's task orders, the SRT reader on hand-written
transcripts (the ``srt`` package is not available offline, so nothing else pins it) and the feature-length check."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

from hirest_amd import dataset as ds


class Tok:
    """The BertTokenizer stand-in the golden was made with: whitespace words, every word unknown."""
    vocab = {"[PAD]": 0, "[UNK]": 100, "[CLS]": 101, "[SEP]": 102}

    def tokenize(self, text):
        return text.split()

    def convert_tokens_to_ids(self, toks):
        return [self.vocab.get(t, 100) for t in toks]


def write_corpus(golden_dir, root):
    """The golden's data directory: both split files, the feature files, the transcripts and the ASR feature files."""
    g = json.load(open(os.path.join(golden_dir, "loader_a.json")))
    z = np.load(os.path.join(golden_dir, "loader_a.npz"))
    g["configs"] = json.loads(z["configs.json"].tobytes().decode())
    for sub in ("feats", "srt", "asr"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for name in g["videos"]:
        torch.save(torch.from_numpy(z[f"feat.{name}"]), os.path.join(root, "feats", f"{name}.pt"))
    for vid, text in g["srt"].items():
        with open(os.path.join(root, "srt", f"{vid}.srt"), "w") as f:
            f.write(text)
        torch.save(torch.from_numpy(z[f"asr.{vid}"]), os.path.join(root, "asr", f"{vid}.pt"))
    for sp in ("train", "test"):
        json.dump(g["split"], open(os.path.join(root, f"all_data_{sp}.json"), "w"))
    return g, z


def make_dataset(root, cfg, max_words):
    args = types.SimpleNamespace(end_to_end=cfg["end_to_end"], max_words=max_words)
    return ds.MomentDataset(args, os.path.join(root, f"all_data_{cfg['split']}.json"), video_dir=None,
                            video_feature_dir=os.path.join(root, "feats"), asr_dir=os.path.join(root, "srt"),
                            asr_feature_dir=os.path.join(root, "asr"), n_model_frames=cfg["n_model_frames"], task=cfg["task"], tokenizer=Tok())


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    return v


@pytest.fixture(scope="module")
def corpus(golden_dir, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("loader_corpus"))
    assert "train" not in root and "temp" not in root
    g, z = write_corpus(golden_dir, root)
    return root, g, z


def test_example_lists_and_masks_equal_the_reference(corpus):
    root, g, _ = corpus
    assert len(g["configs"]) == 26
    for cfg in g["configs"]:
        d = make_dataset(root, cfg, g["max_words"])
        what = (cfg["task"], cfg["split"], cfg["n_model_frames"], cfg["end_to_end"])
        assert len(d) == len(cfg["examples"]) and d.task == cfg["task"], what
        for i, want in enumerate(cfg["examples"]):
            got = d.data[i]
            for k, v in want.items():
                if k == "video_mask":
                    assert v == [1] * got["n_frames"], (what, i)
                elif k == "moment_mask":
                    assert d.moment_mask(i).tolist() == v, (what, i, got["mask_range"])
                elif k == "prev_boundary_mask":
                    assert d.prev_boundary_mask(i).tolist() == v, (what, i)
                else:
                    assert plain(got[k]) == v and type(plain(got[k])) is type(v), (what, i, k, got[k], v)
            lo, hi, one = got["mask_range"]
            assert 0 <= lo <= hi <= got["n_frames"] and -1 <= one < got["n_frames"]
    assert d.videoid2asr == {k: [tuple(p) for p in v] for k, v in g["spans"].items()}


def test_multitask_loader_task_orders_equal_the_reference(corpus):
    g = corpus[1]

    class Loader:
        def __init__(self, task, n):
            self.task, self.n, self.epochs = task, n, []

        def __len__(self):
            return self.n

        def set_epoch(self, e):
            self.epochs.append(e)

        def __iter__(self):
            return iter([self.task] * 100)
    for sampling in ("roundrobin", "balanced"):
        loaders = [Loader(t, n) for t, n in zip(ds.TASKS, g["multitask_lengths"])]
        ml = ds.MultitaskLoader(loaders, sampling=sampling, verbose=False)
        for epoch in range(3):
            ml.set_epoch(epoch)
            want = g["multitask"][sampling][epoch]
            assert ml.epoch_tasks == want and len(ml) == len(want), (sampling, epoch)
            assert list(iter(ml)) == want[::-1]                     # tasks are popped from the end
            assert len(ml) == 0
        assert loaders[0].epochs == [0, 0, 1, 2]                    # the constructor sets epoch 0 itself
    assert len(g["multitask"]["balanced"][0]) == 3 * (sum(g["multitask_lengths"]) // 3)
    unshuffled = ds.MultitaskLoader([Loader(t, n) for t, n in zip(ds.TASKS, (1, 2, 1))], shuffle=False, verbose=False)
    assert unshuffled.epoch_tasks == [ds.TASKS[0], ds.TASKS[1], ds.TASKS[1], ds.TASKS[2]]
    assert len(ds.MultitaskLoader([Loader("a", 4), Loader("b", 1)], sampling="balanced", n_batches=7, verbose=False)) == 14


def test_srt_reader_on_hand_written_transcripts():
    text = ("1\n00:00:01,000 --> 00:00:04,999\nHello there\n\n"
            "2\n00:00:04,200 --> 00:01:10,001\ntwo lines\nof content\n\n\n\n"
            "3\n01:02:03,500 --> 01:02:03,900\n- 00:00 is not a timing line\n\n"
            "4\n25:00:07,000 --> 26:10:00,000\nmore than a day wraps like timedelta.seconds\n")
    want = [(1, 4), (4, 70), (3723, 3723), (3607, 7800)]
    assert ds.read_srt_spans(text) == want
    assert ds.read_srt_spans("\ufeff" + text.replace("\n", "\r\n")) == want
    assert ds.read_srt_spans("") == [] and ds.read_srt_spans("\n\n") == []
    assert ds.read_srt_spans("7\n00:00:09.5 --> 00:00:11 X1:10 X2:20\ntext") == [(9, 11)]      # '.' fractions, trailing coordinates
    assert ds.read_srt_spans("1\n00:00:05,000 --> 00:00:02,000\ninverted\n") == [(5, 2)]


def test_feature_file_of_another_length_is_refused_at_store_build(corpus, tmp_path):
    root, g, z = corpus
    cfg = next(c for c in g["configs"] if c["task"] == "moment_retrieval" and c["n_model_frames"] == -1)
    feats = tmp_path / "feats"
    feats.mkdir()
    for name in g["videos"]:
        x = torch.from_numpy(z[f"feat.{name}"])
        torch.save(x[:-1] if name == "v30.mp4" else x, feats / f"{name}.pt")
    args = types.SimpleNamespace(end_to_end=False, max_words=g["max_words"])
    path = os.path.join(root, "all_data_test.json")
    short = ds.MomentDataset(args, path, video_feature_dir=str(feats), n_model_frames=-1, task="moment_retrieval")
    with pytest.raises(ValueError, match=r"v30\.mp4.*trim_to_duration"):
        ds.DeviceFeatureStore(str(feats), device="cpu").attach(short)
    fitted = ds.MomentDataset(args, path, video_feature_dir=str(feats), n_model_frames=8, task="moment_retrieval")
    tables = ds.DeviceFeatureStore(str(feats), device="cpu").attach(fitted)          # a fixed frame count fits any file length
    assert tables.N == len(cfg["examples"]) and tables.store.frame_len.tolist()[:2] == [5, 29]
    with pytest.raises(ValueError, match="tokenizer"):
        ds.MomentDataset(args, path, video_feature_dir=str(feats), n_model_frames=8, task="step_captioning")


def test_batch_assemble_checks_its_argument_block_without_gpu():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    X = 1 << 20
    a = _lib.BatchArgs()
    assert lib.hirest_batch_assemble(None, None) == -1 and lib.hirest_batch_assemble(ctypes.byref(a), None) == -1      # struct_size 0
    a.struct_size = ctypes.sizeof(_lib.BatchArgs)
    assert ctypes.sizeof(_lib.BatchGather) == 32 and _lib.BATCH_GATHER_MAX == 8
    assert lib.hirest_batch_assemble(ctypes.byref(a), None) == 0                     # B = 0 with the library's own struct size: nothing to do
    a.B, a.T, a.D, a.n_examples = 2, 8, 16, 4
    assert lib.hirest_batch_assemble(ctypes.byref(a), None) == -1                    # NULL tables
    for name in ("index", "frames", "frame_off", "ex_video", "ex_len", "ex_range", "vis", "vis_mask", "moment_mask"):
        setattr(a, name, X)
    for field, bad in (("T", 0), ("D", 0), ("n_examples", 0), ("n_gather", 9), ("n_gather", -1), ("n_model_frames", 7)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.hirest_batch_assemble(ctypes.byref(a), None) == -1, field
        setattr(a, field, keep)
    a.asr_rows = X                                                                   # ASR rows without their tables / output
    assert lib.hirest_batch_assemble(ctypes.byref(a), None) == -1
    a.asr_rows = None
    a.prev_boundary_mask = X                                                         # a boundary mask without the lists
    assert lib.hirest_batch_assemble(ctypes.byref(a), None) == -1
    a.prev_boundary_mask = None
    a.n_gather = 1                                                                   # a gather without its table
    assert lib.hirest_batch_assemble(ctypes.byref(a), None) == -1
