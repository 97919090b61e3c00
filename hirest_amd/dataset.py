"""The joint model's loader (hirest_dataset.py:71-693) with the batch built on the device.

The reference's ``MomentDataset.__getitem__`` + ``collate_fn`` run, per sample and per step, a ``torch.load`` of a feature
file, two Python loops (row-by-row up-sampling, subtitle warp), ``deepcopy`` / ``torch.stack`` and a pageable host->device copy
of ``[B, T, 1024 + 384]`` floats.  Here the host side keeps integers only:

    MomentDataset        the same example list in the same order (skip rules, bins, targets), masks kept as ranges and lists
    DeviceFeatureStore   every feature file the example lists use, uploaded ONCE: fp32 ``[sum n, D]`` frame rows and
                         ``[sum s, Da]`` ASR rows with per-video offset tables, plus per-dataset example tables
    MomentLoader         one ``hirest_batch_assemble`` launch (csrc/batch.hip) per batch, driven by a device vector of example
                         numbers; the batch is a dict with exactly ``collate_fn``'s keys
    get_moment_loader / MultitaskLoader   the reference's entry points, so ``run.py`` switches by one import

What is pinned to the real reference (tests/golden/loader_a.*, made by tests/golden/make_loader_golden.py): the example lists,
every tensor and list of every batch.  What is not: the subtitle reader (the ``srt`` package is not available offline; see
``read_srt_spans``) and the shuffle order (the reference's depends on the global RNG state).
"""
from __future__ import annotations

import ctypes as C
import json
import random
import re
from copy import deepcopy
from pathlib import Path
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .timeline import frame_index_to_timestamp, timestamp_to_frame_index
from .tokenizer import tokenize

TASKS = ["moment_retrieval", "moment_segmentation", "step_captioning"]

_SRT_TIMING = re.compile(r"^[ \t]*(\d+):(\d+):(\d+)(?:[,.]\d*)?[ \t]*-->[ \t]*(\d+):(\d+):(\d+)(?:[,.]\d*)?[^\n]*$", re.M)


def read_srt_spans(text: str) -> List[Tuple[int, int]]:
    """One ``(start.seconds, end.seconds)`` pair per subtitle of an SRT transcript, in file order: what
    ``[(s.start.seconds, s.end.seconds) for s in srt.parse(text)]`` gives (hirest_dataset.py:106-109, :378).  ``timedelta.seconds``
    drops the fraction and leaves out whole days, so a pair is ``(h * 3600 + m * 60 + s) % 86400`` of either end.  A block is
    recognised by its timing line ``H:MM:SS,mmm --> H:MM:SS,mmm``; index lines, (multi-line) content, blank lines, a byte-order
    mark and CRLF line ends do not matter.

    The ``srt`` package is not available where this project is built, so this reader is NOT pinned to it: only hand-written
    transcripts in tests/test_dataset_host.py check it."""
    text = text.lstrip("\ufeff").replace("\r\n", "\n").replace("\r", "\n")
    out = []
    for m in _SRT_TIMING.finditer(text):
        h0, m0, s0, h1, m1, s1 = (int(g) for g in m.groups())
        out.append(((h0 * 3600 + m0 * 60 + s0) % 86400, (h1 * 3600 + m1 * 60 + s1) % 86400))
    return out


def load_subtitle_spans(asr_dir) -> Dict[str, List[Tuple[int, int]]]:
    """``{video id: spans}`` for every ``*.srt`` of a directory (hirest_dataset.py:100-109)."""
    out = {}
    for path in Path(asr_dir).glob("*.srt"):
        with open(path, "r", encoding="utf-8-sig") as f:
            out[path.stem] = read_srt_spans(f.read())
    return out


def _token_ids(tokenizer, words_or_text, is_text: bool) -> List[int]:
    if is_text:
        if hasattr(tokenizer, "tokenize_ids"):                       # hirest_amd.wordpiece.WordPieceTokenizer
            return list(tokenizer.tokenize_ids(words_or_text))
        return list(tokenizer.convert_tokens_to_ids(tokenizer.tokenize(words_or_text)))
    if hasattr(tokenizer, "vocab") and not hasattr(tokenizer, "convert_tokens_to_ids"):
        return [tokenizer.vocab[w] for w in words_or_text]
    return list(tokenizer.convert_tokens_to_ids(words_or_text))


def clip4cap_get_text(tokenizer, caption: str, max_words: int):
    """The 9-tuple of hirest_dataset.py:533-580 for one caption: field 0 the ids of ``[CLS] [SEP]``, fields 5, 6, 7 the decoder
    input ids ``[CLS] w1 .. wn``, the decoder mask and the output ids ``w1 .. wn [SEP]``, each ``[1, max_words]`` int64 and
    zero-padded; the caption is cut to ``max_words - 1`` word pieces."""
    cls_id, sep_id = _token_ids(tokenizer, ["[CLS]", "[SEP]"], False)
    room = max_words - 1
    pairs_text = np.zeros((1, max_words), dtype=np.int64)
    pairs_text[0, :2] = [cls_id, sep_id]
    words = _token_ids(tokenizer, caption, True)[:room]
    inp = np.zeros((1, max_words), dtype=np.int64)
    out = np.zeros((1, max_words), dtype=np.int64)
    mask = np.zeros((1, max_words), dtype=np.int64)
    inp[0, :len(words) + 1] = [cls_id] + words
    out[0, :len(words) + 1] = words + [sep_id]
    mask[0, :len(words) + 1] = 1
    return pairs_text, np.array([]), np.array([]), np.array([]), np.array([]), inp, mask, out, []


def _slice_range(lo: int, hi: int, n: int) -> Tuple[int, int]:
    """[lo:hi] of a length-n axis as a half-open range (Python slice semantics for non-negative bounds)."""
    lo, hi = min(max(lo, 0), n), min(max(hi, 0), n)
    return (lo, hi) if lo < hi else (0, 0)


class MomentDataset:
    """hirest_dataset.py:71-316 without the tensors: ``.data`` is the reference's example list (same order, same scalar keys);
    the masks are ``mask_range = (lo, hi, one)`` (ones on ``[lo, hi)`` and at ``one``, -1 = none) over ``n_frames`` slots and
    ``prev_boundary_frames`` (a list), not ``[n_frames]`` tensors.  Features are not read here: a ``DeviceFeatureStore`` holds
    them, and ``MomentLoader`` builds the batches."""

    def __init__(self, args, data_path, video_dir=None, video_feature_dir=None, asr_dir=None, asr_feature_dir=None, n_model_frames=-1,
                 task=None, tokenizer=None):
        with open(data_path, "r") as f:
            prompt2video_anns = json.load(f)
        self.args = args
        self.video_dir = Path(video_dir) if video_dir is not None else None
        self.video_feature_dir = Path(video_feature_dir) if video_feature_dir is not None else None
        if self.video_feature_dir is not None and not self.video_feature_dir.exists():
            raise AssertionError(f"video_feature_dir {self.video_feature_dir} does not exist")
        self.asr_dir = self.asr_feature_dir = None
        self.videoid2asr: Dict[str, List[Tuple[int, int]]] = {}
        if asr_dir is not None:
            self.asr_dir, self.asr_feature_dir = Path(asr_dir), Path(asr_feature_dir)
            assert self.asr_dir.exists(), self.asr_dir
            assert self.asr_feature_dir.exists(), self.asr_feature_dir
            self.videoid2asr = load_subtitle_spans(self.asr_dir)
        self._all_prompts = list(prompt2video_anns.keys())
        self.n_model_frames = n_model_frames
        self.tasks = list(TASKS)
        self.task = task
        self.tokenizer = tokenizer if tokenizer is not None else getattr(args, "tokenizer", None)
        if self.tokenizer is None and task == "step_captioning":
            vocab = getattr(args, "bert_vocab_file", None)
            if vocab is None:
                raise ValueError("step_captioning needs a BERT tokenizer: pass tokenizer=, or set args.tokenizer / args.bert_vocab_file "
                                 "(a bert-base-uncased vocab.txt for hirest_amd.wordpiece.WordPieceTokenizer)")
            from .wordpiece import WordPieceTokenizer
            self.tokenizer = WordPieceTokenizer.from_file(vocab)
        end_to_end = bool(getattr(args, "end_to_end", False))
        train_path = "train" in str(data_path)
        data = []
        for prompt, video_anns in prompt2video_anns.items():
            for fname, ann in video_anns.items():
                if not ann["relevant"] or not ann["clip"]:
                    continue
                duration = round(ann["v_duration"])
                n = n_model_frames if n_model_frames > 0 else duration
                base = {"fname": fname, "prompt": prompt, "video_duration": duration, "n_model_frames": n_model_frames}
                frame = lambda ts: timestamp_to_frame_index(ts, video_duration=duration, n_frames=n)
                second = lambda fr: frame_index_to_timestamp(fr, video_duration=duration, n_frames=n)
                if task == "moment_retrieval":
                    s, e = ann["bounds"][0], ann["bounds"][1]
                    sf, ef = frame(s), frame(e)
                    data.append(dict(base, task=task, moment_retrieval_start_target=sf, moment_retrieval_end_target=ef,
                                     original_bounds=[[s, e]], approximate_bounds=[[second(sf), second(ef)]],
                                     n_frames=n, mask_range=(0, n, -1)))
                elif task == "moment_segmentation":
                    if not end_to_end and len(ann["steps"]) == 0:
                        continue
                    bounds = sorted({b for step in ann["steps"] for b in step["absolute_bounds"]})
                    bound_frames = [frame(b) for b in bounds]
                    ms, me = ann["bounds"][0], ann["bounds"][1]
                    msf, mef = frame(ms), frame(me)
                    common = dict(base, task=task, moment_bound_timestamps=[ms, me], moment_bound_frames=[msf, mef], n_frames=n)
                    if train_path:                               # one teacher-forced example per consecutive pair of boundaries
                        if len(bounds) <= 2:
                            continue
                        for i in range(len(bounds) - 1):
                            lo, hi = _slice_range(bound_frames[i], mef + 1, n)
                            data.append(dict(deepcopy(common), moment_segmentation_target=bound_frames[i + 1],
                                             prev_boundary_frames=sorted(set(bound_frames[:i + 1])), mask_range=(lo, hi, -1),
                                             all_bound_frames=list(bound_frames)))
                    else:
                        lo, hi = _slice_range(msf, mef + 1, n)
                        data.append(dict(common, mask_range=(lo, hi, -1), all_bound_frames=bound_frames))
                elif task == "step_captioning":
                    if not end_to_end and len(ann["steps"]) == 0:
                        continue
                    ann["steps"][0]["absolute_bounds"][0], ann["steps"][-1]["absolute_bounds"][1]      # the reference's IndexError on no steps
                    max_words = int(getattr(args, "max_words"))
                    for step in ann["steps"]:
                        s, e = step["absolute_bounds"]
                        text = step["heading"].strip()
                        sf, ef = frame(s), frame(e)
                        lo, hi = _slice_range(sf, ef, n)
                        data.append(dict(base, task=task, target_text_raw=text, target_text=clip4cap_get_text(self.tokenizer, text, max_words),
                                         n_frames=n, mask_range=(lo, hi, ef)))
        self.data = data
        print(f"# {task} examples:", len(data))

    def __len__(self):
        return len(self.data)

    def moment_mask(self, index: int) -> torch.Tensor:
        """The ``[n_frames]`` long mask of example `index`, rebuilt from its range (for checks; the loader never needs it)."""
        d = self.data[index]
        m = torch.zeros(d["n_frames"], dtype=torch.long)
        lo, hi, one = d["mask_range"]
        m[lo:hi] = 1
        if one >= 0:
            m[one] = 1
        return m

    def prev_boundary_mask(self, index: int) -> torch.Tensor:
        d = self.data[index]
        m = torch.zeros(d["n_frames"], dtype=torch.long)
        m[d["prev_boundary_frames"]] = 1
        return m


class DeviceBatch(dict):
    """A loader batch: ``collate_fn``'s keys (hirest_dataset.py:409-531).  Float tensors, masks, targets and token ids are on the
    device; ``moment_bound_frames`` / ``moment_bound_timestamps`` are CPU LongTensors (the model calls ``.tolist()`` on them); the
    lists are host lists.  ``host`` holds CPU copies of what the model reads on the host (``moment_mask`` of a captioning batch,
    filled from the ranges), ``device`` what was gathered beyond the reference's keys (the caption id tables)."""
    host: Dict[str, torch.Tensor]
    device: Dict[str, torch.Tensor]

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.host, self.device = {}, {}


class ExampleTables:
    """The per-dataset integer tables of a ``DeviceFeatureStore`` (device int32 / int64 arrays) and the batch assembly."""

    def __init__(self, store: "DeviceFeatureStore", dataset: MomentDataset, text_model=None):
        self.store, self.dataset = store, dataset
        dev = store.device
        data = dataset.data
        N = len(data)
        self.N, self.task, self.F = N, dataset.task, int(dataset.n_model_frames)
        vid = np.array([store.video_index[d["fname"]] for d in data], dtype=np.int32).reshape(N)
        self.ex_video_h = vid
        self.ex_len_h = np.array([d["n_frames"] for d in data], dtype=np.int32).reshape(N)
        self.ex_range_h = np.array([d["mask_range"] for d in data], dtype=np.int32).reshape(N, 3)
        if self.F <= 0:
            # collate_fn pads video_mask (length round(v_duration)) by an amount computed from the feature file's length
            # (hirest_dataset.py:431-453): a file of another length makes torch.stack fail or the widths disagree
            for d, v in zip(data, vid):
                n = int(store.frame_len[v])
                if n != d["n_frames"]:
                    raise ValueError(f"{d['fname']}: the feature file has {n} rows but round(v_duration) = {d['n_frames']}; with "
                                     "n_model_frames <= 0 they must agree (cut the file with hirest_amd.features.trim_to_duration)")
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.ex_video, self.ex_len, self.ex_range = up(vid), up(self.ex_len_h), up(self.ex_range_h)
        self.bound_off = self.bound_val = None
        if N and "prev_boundary_frames" in data[0]:
            lists = [d["prev_boundary_frames"] for d in data]
            off = np.zeros(N + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(l) for l in lists])
            self.bound_off, self.bound_val = up(off), up(np.array([f for l in lists for f in l] + [0], dtype=np.int32))
        # int64 rows gathered per example: (batch key, table [N, w], squeeze)
        self.rows: List[Tuple[str, torch.Tensor, bool, bool]] = []
        for key in ("moment_retrieval_start_target", "moment_retrieval_end_target", "moment_segmentation_target"):
            if N and key in data[0]:
                self.rows.append((key, up(np.array([d[key] for d in data], dtype=np.int64).reshape(N, 1)), True, True))
        self.bounds_h = {}
        for key in ("moment_bound_timestamps", "moment_bound_frames"):
            if N and key in data[0]:
                self.bounds_h[key] = torch.tensor([d[key] for d in data], dtype=torch.long).reshape(N, 2)
        prompts = list(dict.fromkeys(d["prompt"] for d in data))
        where = {p: i for i, p in enumerate(prompts)}
        self.prompt_ids = tokenize(prompts).to(dev) if prompts else torch.zeros((0, 77), dtype=torch.long, device=dev)
        self.ex_prompt = up(np.array([where[d["prompt"]] for d in data], dtype=np.int32).reshape(N))
        self.text_feat = None
        if text_model is not None and prompts:
            clip = getattr(text_model, "clip_model", text_model)
            with torch.no_grad():       # the frozen text tower, once per DISTINCT prompt (batch- and order-invariant bit for bit)
                self.text_feat = torch.cat([clip.encode_text(self.prompt_ids[i:i + 256]).float() for i in range(0, len(prompts), 256)]).contiguous()
        self.caption = None
        if N and "target_text" in data[0]:
            self.caption = {name: up(np.concatenate([np.asarray(d["target_text"][f], dtype=np.int64).reshape(1, -1) for d in data]))
                            for name, f in (("input_caption_ids", 5), ("decoder_mask", 6), ("output_caption_ids", 7))}
        self._host_lists = {k: [d[k] for d in data] for k in ("fname", "prompt", "video_duration", "task")}

    def assemble(self, index: torch.Tensor, index_host: Sequence[int]) -> DeviceBatch:
        """One batch: `index` the example numbers as a device int32 vector, `index_host` the same numbers on the host (list
        entries, the padded length).  One kernel launch on the current stream; nothing is read back."""
        st, data, dev = self.store, self.dataset.data, self.store.device
        idx = np.asarray(index_host, dtype=np.int64)
        B = len(idx)
        T = self.F if self.F > 0 else int(st.frame_len[self.ex_video_h[idx]].max())
        vis = torch.empty((B, T, st.D), dtype=torch.float32, device=dev)
        masks = torch.empty((3 if self.bound_off is not None else 2, B, T), dtype=torch.long, device=dev)
        asr = torch.empty((B, T, st.Da), dtype=torch.float32, device=dev) if st.asr_rows is not None else None
        a = _lib.BatchArgs()
        a.struct_size = C.sizeof(_lib.BatchArgs)
        a.index, a.B, a.T, a.D, a.Da = index.data_ptr(), B, T, st.D, st.Da
        a.n_examples, a.n_model_frames = self.N, self.F
        a.frames, a.frame_off = st.frames.data_ptr(), st.frame_off.data_ptr()
        if asr is not None:
            a.asr_rows, a.sub_off, a.sub_span, a.asr = st.asr_rows.data_ptr(), st.sub_off.data_ptr(), st.sub_span.data_ptr(), asr.data_ptr()
        a.ex_video, a.ex_len, a.ex_range = self.ex_video.data_ptr(), self.ex_len.data_ptr(), self.ex_range.data_ptr()
        a.vis, a.vis_mask, a.moment_mask = vis.data_ptr(), masks[0].data_ptr(), masks[1].data_ptr()
        if self.bound_off is not None:
            a.bound_off, a.bound_val, a.prev_boundary_mask = self.bound_off.data_ptr(), self.bound_val.data_ptr(), masks[2].data_ptr()
        gathered = {}
        g = 0

        def gather(name, table, row_of_example=None):
            nonlocal g
            if g >= _lib.BATCH_GATHER_MAX:
                raise RuntimeError(f"{name}: more than {_lib.BATCH_GATHER_MAX} gathered tables in one batch (HIREST_BATCH_GATHER_MAX)")
            out = torch.empty((B, table.shape[1]), dtype=table.dtype, device=dev)
            it = a.gather[g]
            it.src, it.dst, it.words = table.data_ptr(), out.data_ptr(), table.shape[1] * table.element_size() // 4
            it.row_of_example = row_of_example.data_ptr() if row_of_example is not None else None
            g += 1
            gathered[name] = out
        for key, table, _, _ in self.rows:
            gather(key, table)
        gather("clip_text_ids", self.prompt_ids, self.ex_prompt)
        if self.text_feat is not None:
            gather("text_feat", self.text_feat, self.ex_prompt)
        if self.caption is not None:
            for name, table in self.caption.items():
                gather(name, table)
        a.n_gather = g
        with torch.cuda.device(dev):
            _lib.check(_lib.load().hirest_batch_assemble(C.byref(a), ops.stream_ptr()), "hirest_batch_assemble")
        picked = [data[i] for i in idx]
        out = DeviceBatch()
        if self.caption is not None:
            out["target_text"] = [d["target_text"] for d in picked]
            out["target_text_raw"] = [d["target_text_raw"] for d in picked]
        out["vis_feats"], out["vis_mask"], out["moment_mask"] = vis, masks[0], masks[1]
        for key in ("moment_retrieval_start_target", "moment_retrieval_end_target"):
            if key in gathered:
                out[key] = gathered[key].reshape(B)
        if self.bound_off is not None:
            out["prev_boundary_mask"] = masks[2]
        if "moment_segmentation_target" in gathered:
            out["moment_segmentation_target"] = gathered["moment_segmentation_target"].reshape(B)
        if asr is not None:
            out["asr_feats"] = asr
        tidx = torch.from_numpy(idx)
        for key in ("moment_bound_timestamps", "moment_bound_frames"):
            if key in self.bounds_h:
                out[key] = self.bounds_h[key][tidx]
        if picked and "all_bound_frames" in picked[0]:
            out["all_bound_frames"] = [d["all_bound_frames"] for d in picked]
        hl = self._host_lists
        out["video_duration"] = [hl["video_duration"][i] for i in idx]
        out["video_fnames"] = [hl["fname"][i] for i in idx]
        out["tasks"] = [hl["task"][i] for i in idx]
        out["prompts"] = [hl["prompt"][i] for i in idx]
        out["clip_text_ids"] = gathered["clip_text_ids"]
        if self.text_feat is not None:
            out["text_feat"] = gathered["text_feat"]
        if self.caption is not None:
            out.device = {k: gathered[k] for k in self.caption}
            # the captioning model turns this mask into a row-index table on the host (trim_feats): hand it the host's own copy
            t = np.arange(T, dtype=np.int32)[None, :]
            r, L = self.ex_range_h[idx], self.ex_len_h[idx][:, None]
            m = (((t >= r[:, 0:1]) & (t < r[:, 1:2])) | (t == r[:, 2:3])) & (t < L)
            out.host = {"moment_mask": torch.from_numpy(m.astype(np.int64))}
        return out


class DeviceFeatureStore:
    """Every frame-feature file (and ASR feature file) that the attached datasets use, resident on one device.

        frames     fp32 [sum n_i, D]     the rows of all ``<video>.pt`` files, video after video (fp16 files are widened: exact)
        frame_off  int64 [videos + 1]    row offsets
        asr_rows   fp32 [sum s_i, Da]    row i of ``<video id>.pt`` for subtitle i of the video (the reference indexes by subtitle)
        sub_off    int64 [videos + 1]    subtitle = ASR row offsets
        sub_span   int32 [sum s_i, 2]    (start, end) in whole seconds

    Built once per (feature directory, ASR directories, device) and shared by datasets and tasks: ``attach(dataset)`` uploads what
    the dataset's videos still lack and returns the dataset's ``ExampleTables``."""

    def __init__(self, video_feature_dir, asr_dir=None, asr_feature_dir=None, device=None, sub_spans=None):
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("DeviceFeatureStore needs an MI355X (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.video_feature_dir = Path(video_feature_dir)
        self.asr_feature_dir = Path(asr_feature_dir) if asr_feature_dir is not None else None
        self.sub_spans = sub_spans if sub_spans is not None else (load_subtitle_spans(asr_dir) if asr_dir is not None else {})
        self.has_asr = len(self.sub_spans) > 0                       # hirest_dataset.py:359
        self.video_index: Dict[str, int] = {}
        self.frame_len = np.zeros(0, dtype=np.int64)
        self.sub_len = np.zeros(0, dtype=np.int64)
        self.D = self.Da = 0
        self.frames = self.asr_rows = self.frame_off = self.sub_off = self.sub_span = None

    def ensure(self, fnames: Sequence[str]) -> None:
        """Upload the files of the videos the store does not hold yet.  Every file is read and checked before any state changes,
        so a bad file leaves the store as it was.  Appending to a store that already holds videos concatenates the resident arrays
        with the new block (old + new arrays alive for a moment): attach the largest dataset first, or call ``ensure`` once with all
        the videos, where the corpus is a large part of the memory."""
        new = [f for f in dict.fromkeys(fnames) if f not in self.video_index]
        if not new:
            return
        D, Da = self.D, self.Da
        feats, asr, spans = [], [], []
        for f in new:
            x = torch.load(self.video_feature_dir / f"{f}.pt", map_location="cpu")
            if x.dim() != 2 or x.shape[1] < 1 or (D and x.shape[1] != D):
                raise ValueError(f"{f}: feature file of shape {tuple(x.shape)} (expected [n, {D or 'D'}])")
            D = int(x.shape[1])
            feats.append(x.float())
            if self.has_asr:
                vid = f.replace(".mp4", "")
                if vid not in self.sub_spans:
                    raise KeyError(f"{f}: no transcript {vid}.srt in the ASR directory")
                sp = self.sub_spans[vid]
                path = self.asr_feature_dir / f"{vid}.pt"
                assert path.exists(), path
                y = torch.load(path, map_location="cpu")
                if y.dim() != 2 or y.shape[1] < 1 or (Da and y.shape[1] != Da) or y.shape[0] < len(sp):
                    raise ValueError(f"{f}: ASR feature file of shape {tuple(y.shape)} for {len(sp)} subtitles (expected [>= {len(sp)}, {Da or 'Da'}])")
                Da = int(y.shape[1])
                asr.append(y[:len(sp)].float())
                lim = 2 ** 31 - 1
                spans.append(np.clip(np.array(sp, dtype=np.int64).reshape(len(sp), 2), 0, lim).astype(np.int32))
        # ---- everything is valid: commit
        dev = self.device
        held = int(self.sub_len.sum())                               # ASR rows held so far (0: asr_rows is None or the placeholder row)
        self.D, self.Da = D, Da
        for f in new:
            self.video_index[f] = len(self.video_index)
        self.frame_len = np.concatenate([self.frame_len, np.array([x.shape[0] for x in feats], dtype=np.int64)])
        block = torch.cat(feats).contiguous().to(dev)
        self.frames = block if self.frames is None else torch.cat([self.frames, block])
        self.frame_off = torch.from_numpy(np.concatenate([[0], np.cumsum(self.frame_len)]).astype(np.int64)).to(dev)
        if self.has_asr:
            self.sub_len = np.concatenate([self.sub_len, np.array([y.shape[0] for y in asr], dtype=np.int64)])
            block = torch.cat(asr).contiguous().to(dev)
            sblock = torch.from_numpy(np.concatenate(spans)).to(dev)
            self.asr_rows = block if held == 0 else torch.cat([self.asr_rows, block])
            self.sub_span = sblock if held == 0 else torch.cat([self.sub_span, sblock])
            if self.asr_rows.shape[0] == 0:                          # not one subtitle so far: a placeholder row keeps the pointers valid
                self.asr_rows = torch.zeros((1, self.Da), dtype=torch.float32, device=dev)
                self.sub_span = torch.zeros((1, 2), dtype=torch.int32, device=dev)
            self.sub_off = torch.from_numpy(np.concatenate([[0], np.cumsum(self.sub_len)]).astype(np.int64)).to(dev)

    def attach(self, dataset: MomentDataset, text_model=None) -> ExampleTables:
        self.ensure([d["fname"] for d in dataset.data])
        return ExampleTables(self, dataset, text_model)

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.frames, self.asr_rows) if t is not None)


class MomentLoader:
    """What ``get_moment_loader`` returns: an iterable of ``DeviceBatch`` with ``__len__``, ``.task``, ``.dataset``, ``set_epoch``.
    Shuffled epochs draw ``torch.randperm`` from a generator seeded with (seed, epoch); the order differs from the reference's
    DataLoader, whose shuffle depends on the global RNG state.  ``drop_last`` is False."""

    def __init__(self, dataset: MomentDataset, tables: ExampleTables, batch_size: int, shuffle: bool, seed: int = 0, sampler=None):
        self.dataset, self.tables, self.batch_size, self.shuffle, self.seed, self.sampler = dataset, tables, int(batch_size), shuffle, seed, sampler
        self.task = dataset.task
        self.epoch = 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)
        if self.sampler is not None:
            self.sampler.set_epoch(epoch)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return (n + self.batch_size - 1) // self.batch_size

    def order(self) -> List[int]:
        if self.sampler is not None:
            return list(iter(self.sampler))
        if not self.shuffle:
            return list(range(len(self.dataset)))
        gen = torch.Generator()
        gen.manual_seed(self.seed * 1000003 + self.epoch)
        return torch.randperm(len(self.dataset), generator=gen).tolist()

    def __iter__(self):
        order = self.order()
        if self.sampler is None:
            self.epoch += 1                                          # the next epoch is another permutation, set_epoch or not
        if not order:
            return
        on_device = torch.tensor(order, dtype=torch.int32).to(self.tables.store.device)      # one upload per epoch
        for lo in range(0, len(order), self.batch_size):
            yield self.tables.assemble(on_device[lo:lo + self.batch_size], order[lo:lo + self.batch_size])


_STORES: Dict[tuple, DeviceFeatureStore] = {}


def get_feature_store(video_feature_dir, asr_dir=None, asr_feature_dir=None, device=None) -> DeviceFeatureStore:
    """The process-wide store of (feature directory, ASR directories, device): the three tasks and both splits share one."""
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("the device loader needs an MI355X (no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    key = (str(video_feature_dir), str(asr_dir), str(asr_feature_dir), str(device))
    if key not in _STORES:
        _STORES[key] = DeviceFeatureStore(video_feature_dir, asr_dir, asr_feature_dir, device)
    return _STORES[key]


def get_moment_loader(args, split="train", batch_size=32, task="moment_retrieval", cache_text=None, device=None, tokenizer=None,
                      seed=0) -> MomentLoader:
    """hirest_dataset.py:582-634.  ``cache_text=model``: every distinct prompt is encoded once with the model's frozen
    ``clip_model.encode_text`` and the batches carry ``text_feat`` (which ``MomentModel`` prefers to ``clip_text_ids``)."""
    assert task in TASKS, task
    name = f"temp_data_{split}.json" if "temp" in str(args.data_dir) else f"all_data_{split}.json"
    dataset = MomentDataset(args, data_path=Path(args.data_dir) / name, video_dir=None, video_feature_dir=args.video_feature_dir,
                            asr_dir=getattr(args, "asr_dir", None), asr_feature_dir=getattr(args, "asr_feature_dir", None),
                            n_model_frames=args.n_model_frames, task=task, tokenizer=tokenizer)
    if device is None and cache_text is not None:
        device = next(cache_text.parameters()).device
    store = get_feature_store(args.video_feature_dir, getattr(args, "asr_dir", None), getattr(args, "asr_feature_dir", None), device)
    tables = store.attach(dataset, text_model=cache_text)
    shuffle = split == "train"
    sampler = None
    if getattr(args, "distributed", False):
        sampler = torch.utils.data.distributed.DistributedSampler(range(len(dataset)), shuffle=shuffle)
    return MomentLoader(dataset, tables, batch_size, shuffle, seed=seed, sampler=sampler)


class MultitaskLoader(object):
    """hirest_dataset.py:636-693: one epoch is a task name per batch — every loader's own length under ``roundrobin``, the mean
    length (or ``n_batches``) for each task under ``balanced`` — shuffled with ``random.Random(epoch)`` and consumed from the end."""

    def __init__(self, loaders, shuffle=True, drop_last=False, sampling="roundrobin", n_batches=None, verbose=True):
        self.loaders = loaders
        self.verbose = verbose
        self.task2len = {loader.task: len(loader) for loader in loaders}
        if verbose:
            print("Task2len:", self.task2len)
        self.task2loader = {loader.task: loader for loader in loaders}
        self.shuffle, self.drop_last, self.sampling, self.n_batches = shuffle, drop_last, sampling, n_batches
        self.epoch_tasks = None
        self.set_epoch(0)

    def __iter__(self):
        self.task2iter = {loader.task: iter(loader) for loader in self.loaders}
        return self

    def set_epoch(self, epoch):
        for loader in self.loaders:
            if hasattr(loader, "set_epoch"):
                loader.set_epoch(epoch)
        tasks = []
        if self.sampling == "roundrobin":
            for task, loader in self.task2loader.items():
                tasks += [task] * len(loader)
        elif self.sampling == "balanced":
            n = self.n_batches if self.n_batches is not None else sum(self.task2len.values()) // len(self.loaders)
            if self.verbose:
                print("# batches:", n)
            for task in self.task2loader:
                tasks += [task] * n
        if self.shuffle:
            random.Random(epoch).shuffle(tasks)
        self.epoch_tasks = tasks
        if self.verbose:
            print("# epoch_tasks:", len(tasks))

    def __next__(self):
        if len(self.epoch_tasks) > 0:
            return next(self.task2iter[self.epoch_tasks.pop()])
        raise StopIteration

    def __len__(self):
        return len(self.epoch_tasks)
