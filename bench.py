#!/usr/bin/env python3
"""Headline benchmark: encoded frames/sec of the EVA-CLIP-g/14 frame encoder (224^2, bf16 MFMA)
on N MI355X, BASELINE.json configs[1]: a 1024-frame synthetic batch per GPU per step.

One step = the hot path over one batch: 32 videos x 32 frames -> encode_image (40-layer ViT-g)
-> mean-pool + L2 -> all-gather of the [V,1024] rows over RCCL (identity at N=1) -> 546-query
cosine matrix -> top-10.  Inputs (bf16 NCHW frames, token ids) are resident in HBM before the
timed region; weights are random-init of the real architecture (no checkpoints offline).

    python bench.py [--gpus N] [--steps K] [--warmup W]          N > 1: re-executes itself as N ranks (one per GPU)
    python bench.py ... --dump-outputs DIR                       also writes the last timed step's results as DIR/<name>.npy
    python bench.py ... --full                                   also runs the legs outside the headline (below)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`--gpus N` is binding: run directly it starts N ranks under torch.distributed.run (hirest_amd/launch.py) and fails
loudly when fewer than N GPUs are visible; run under a launcher, WORLD_SIZE must equal N.  The JSON line carries
`rccl_ranks` = the size of the process group the timed all-gather ran on.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the steps,
writes --dump-outputs and prints the line, which carries one extra object:
  roofline      live per-launch timing (hipEvent pairs recorded by the library on the launch
                stream during the timed steps) of the dominant kernel vs the dense bf16 MFMA peak
With --full the line also carries the figures that take runs of their own, after the timed steps:
  matched_recall  R@k against the real reference's rankings on the pinned C3 sub-corpus, the fp32 and bf16x3
                  towers on it, the margin-guarded re-rank and its throughput on a synthetic corpus (rank 0)
  cpu_baseline    the fp32 CPU oracle (oracle/ref_cpu.py, kind "port") timed on this host on a
                  bounded sample of the same workload (rank 0, N=1 only)
  secondary       the joint model, captioning, training step and ASR encoder (tools/secondary_bench.py) and
                  the tower at small call sizes (rank 0, N=1 only)
--no-matched-recall / --no-cpu-baseline / --no-secondary leave single legs out of a --full run.
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from hirest_amd import launch  # noqa: E402  (sets HSA_ENABLE_IPC_MODE_LEGACY=0 before the HIP runtime starts)

import torch  # noqa: E402

FRAMES_PER_STEP = 1024          # configs[1]
FRAMES_PER_VIDEO = 32
N_QUERIES = 546                 # size of the real HiREST test prompt set
TOPK = 10
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense, MI355X_MICROARCH.md
GFLOP_PER_FRAME = 534.06        # algorithmic work of the vision tower when every block runs on all 257 tokens
# Work the tower actually executes since round 3: the last block only serves x[:, 0] (vit_model.py:340-351), so its proj / fc1 /
# fc2 run on the CLS row and its attention on the leading 16-query tile (keys / values still for all tokens):
_D, _DM, _T, _H, _DH = 1408, 6144, 257, 16, 88
GFLOP_PRUNED_PER_FRAME = (2.0 * (_T - 1) * _D * _D + 2 * 2.0 * (_T - 1) * _D * _DM + 4.0 * (_T - 16) * _T * _DH * _H) / 1e9
GFLOP_EXECUTED_PER_FRAME = GFLOP_PER_FRAME - GFLOP_PRUNED_PER_FRAME
PROFILE_ROUNDS = ("r06", "r05", "r04", "r03", "r02", "r01")  # newest first: where roofline.traffic is looked up


def small_calls(model, frames):
    """frames/s of encode_image at the call sizes the reference's own drivers use (inference_video_retrieval.py:59,270: 10 videos x 32
    frames = 320 per call; extract_features.py:15: 256) and below (one 32-frame video, 64 frames).  Outside the timed region; the
    1024-frame headline is the same model and kernels.  Calls of fewer than 64 frames take the unfolded-LayerNorm kernels."""
    flat = frames.reshape(-1, 3, 224, 224)
    out = {}
    for n in (32, 64, 128, 256, 320):
        x = flat[:n]
        reps = max(3, 1024 // n)
        for _ in range(2):
            model.encode_image(x)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            model.encode_image(x)
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / reps
        out[str(n)] = {"frames_per_s": n / dt, "ms_per_call": dt * 1e3}
    return {"unit": "frames/s by frames per encode_image call", "by_frames_per_call": out,
            "note": "below 256 frames the persistent attention walks one head per workgroup (one frame per workgroup left 192 of 256 CUs idle at 64 frames); "
                    "what remains is tile quantisation: a 64-frame call is 65 row panels = 6.09 rounds of 256 x 256 tiles on 256 CUs for fc1, run as 7"}


def matched_recall(model, dev):
    """R@1/5/10 of the GPU path against GT(q) = the real reference's top-1 video on the committed C3 sub-corpus, with the
    margin report that says which disagreements a bf16 encoder is entitled to (evaluate.py:33-81 semantics: ranking by
    (score, name), recall = fraction of queries whose ground-truth video is in the top k)."""
    import numpy as np
    from hirest_amd import retrieval, synth
    path = os.path.join(REPO, "tests", "golden", "eva_g14_c3.npz")
    if not os.path.isfile(path):
        return {"skipped": "tests/golden/eva_g14_c3.npz missing"}
    g = np.load(path)
    V, F, seed = int(g["V"]), int(g["F"]), int(g["seed"])
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.load_state_dict(synth.eva_clip_state_dict(synth.EVA_CLIP_G_14, seed), strict=True)
    fp32 = x3 = None
    try:
        frames = synth.c3_corpus(V, F).to(dev)
        names = synth.c3_names(V)
        tok = torch.from_numpy(g["tokens"].astype(np.int64)).to(dev)
        tie = retrieval.tie_rank_from_names(names, dev)
        pooled = retrieval.encode_videos(model, frames)
        texts = retrieval.encode_texts(model, tok)
        scores, _, idx = retrieval.retrieve(texts, pooled, 10, tie)
        # the same corpus through the reference-precision towers (precision='fp32', csrc/tower_f32.hip): ranks must be the
        # reference's; its frames/s is a separate figure, never the headline (BASELINE configs[1] is bf16)
        model.set_precision("fp32")
        retrieval.encode_videos(model, frames[:8])                    # warm-up (workspace, descriptors)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pooled32 = retrieval.encode_videos(model, frames)
        torch.cuda.synchronize(); dt32 = time.perf_counter() - t0
        texts32 = retrieval.encode_texts(model, tok)
        scores32, _, idx32 = retrieval.retrieve(texts32, pooled32, 10, tie)
        gt_ = torch.from_numpy(g["top10"][:, 0].astype(np.int64))
        idx32 = idx32.cpu().long()
        fp32 = {"frames_per_s": V * F / dt32, "frames": V * F, "dtype": "f32 (v_mfma_f32_32x32x2_f32 GEMMs + fp32 flash attention)",
                "whole_tower_tflops": V * F / dt32 * GFLOP_PER_FRAME / 1e3, "fp32_mfma_peak_tflops": 157.3,
                "whole_tower_frac_of_fp32_peak": V * F / dt32 * GFLOP_PER_FRAME / 1e3 / 157.3,
                **{f"matched_R@{k}": 100.0 * (idx32[:, :k] == gt_[:, None]).any(dim=1).float().mean().item() for k in (1, 5, 10)},
                "top1_flips": int((idx32[:, 0] != gt_).sum()),
                "top10_lists_identical": int((idx32 == torch.from_numpy(g["top10"].astype(np.int64))).all(dim=1).sum()),
                "max_abs_score_error": (scores32.cpu() - torch.from_numpy(g["scores"])).abs().max().item(),
                "pooled_min_cosine_vs_reference": torch.nn.functional.cosine_similarity(
                    pooled32.cpu(), torch.from_numpy(g["pooled"]), dim=-1).min().item()}
        # precision='bf16x3' (csrc/tower_x3.hip): the fp32 forward with the weight GEMMs on bf16 hi + lo splits of both operands — the
        # reference-rank operating point that is not 10x slower.  Its own roofline line: three bf16 MFMAs per product, so the
        # matrix-pipe peak for ALGORITHMIC flops is 2500 / 3 TFLOP/s.
        from hirest_amd import _lib as _l
        lib = _l.load()
        model.set_precision("bf16x3")
        retrieval.encode_videos(model, frames)                        # warm-up at full size: weight split (once), the 17-GB workspace
        torch.cuda.synchronize()
        lib.hirest_profile_enable(1)
        t0 = time.perf_counter()
        pooled3 = retrieval.encode_videos(model, frames)
        torch.cuda.synchronize(); dt3 = time.perf_counter() - t0
        recs = (_l.ProfRecord * 4096)()
        nrec = lib.hirest_profile_collect(recs, len(recs))
        lib.hirest_profile_enable(0)
        fc = [recs[i] for i in range(max(nrec, 0)) if recs[i].kind == 0 and recs[i].d1 == _DM]      # fc1: N = 6144, K = 2 x 1408
        scores3, _, idx3 = retrieval.retrieve(texts32, pooled3, 10, tie)          # (text tower: exact fp32 in this mode)
        idx3 = idx3.cpu().long()
        x3 = {"frames_per_s": V * F / dt3, "frames": V * F,
              "dtype": "bf16 hi + lo splits of fp32 operands, 3 MFMAs per product, fp32 accumulation; fp32 LayerNorm / attention / GELU",
              **{f"matched_R@{k}": 100.0 * (idx3[:, :k] == gt_[:, None]).any(dim=1).float().mean().item() for k in (1, 5, 10)},
              "top1_flips": int((idx3[:, 0] != gt_).sum()),
              "top10_lists_identical": int((idx3 == torch.from_numpy(g["top10"].astype(np.int64))).all(dim=1).sum()),
              "max_abs_score_error": (scores3.cpu() - torch.from_numpy(g["scores"])).abs().max().item(),
              "pooled_min_cosine_vs_reference": torch.nn.functional.cosine_similarity(
                  pooled3.cpu(), torch.from_numpy(g["pooled"]), dim=-1).min().item(),
              "whole_tower_tflops": V * F / dt3 * GFLOP_PER_FRAME / 1e3,
              "whole_tower_frac_of_peak_over_3": V * F / dt3 * GFLOP_PER_FRAME / 1e3 / (MFMA_BF16_PEAK_TFLOPS / 3)}
        if fc:
            ms = sum(r.ms for r in fc) / len(fc)
            tf = 2.0 * fc[0].d0 * fc[0].d1 * (fc[0].d2 // 2) / (ms * 1e-3) / 1e12
            x3["roofline"] = {"bound": "mfma", "kernel": f"gemm_pp256x3<bias+gelu->split hi|lo (HIREST_EPI_BIAS_GELU_SPLIT2)> fc1 M={fc[0].d0} N={fc[0].d1} K={fc[0].d2 // 2} (x2 split columns)",
                              "achieved": tf, "peak": MFMA_BF16_PEAK_TFLOPS / 3, "unit": "TFLOP/s", "frac": tf / (MFMA_BF16_PEAK_TFLOPS / 3),
                              "avg_launch_ms": ms, "launches": len(fc),
                              "note": "algorithmic flops (2 M N K) over the kernel's live hipEvent time; peak = dense bf16 MFMA peak / 3 "
                                      "because every product costs three bf16 MFMAs"}
        # Margin-guarded re-rank (retrieval.rerank_exact, round 6) on the same pinned corpus: the bf16 rows, re-encoded at bf16x3 only where a
        # place in a query's top 10 is within twice the measured score error — gate: the reference's top-1 and top-10 lists
        model.set_precision("bf16")
        src = retrieval.FrameSource(names, frames, videos_per_call=64)
        rows_rx, rep_rx = retrieval.rerank_exact(model, src, texts32, pooled, 10)
        _, _, idx_rx = retrieval.retrieve(texts32, rows_rx, 10, tie)
        idx_rx = idx_rx.cpu().long()
        rank_exact = {**rep_rx, "top1_flips": int((idx_rx[:, 0] != gt_).sum()),
                      "top10_lists_identical": int((idx_rx == torch.from_numpy(g["top10"].astype(np.int64))).all(dim=1).sum()),
                      **{f"matched_R@{k}": 100.0 * (idx_rx[:, :k] == gt_[:, None]).any(dim=1).float().mean().item() for k in (1, 5, 10)}}
    finally:
        model.set_precision("bf16")
        model.load_state_dict(saved, strict=True)
    idx = idx.cpu().long()
    ref_scores = torch.from_numpy(g["scores"])
    gt = torch.from_numpy(g["top10"][:, 0].astype(np.int64))
    margin = torch.from_numpy(g["margin"])
    err = (scores.cpu() - ref_scores).abs()
    res = {f"matched_R@{k}": 100.0 * (idx[:, :k] == gt[:, None]).any(dim=1).float().mean().item() for k in (1, 5, 10)}
    flipped = idx[:, 0] != gt
    res.update({"queries": int(gt.numel()), "videos": V, "frames_per_video": F,
                "max_abs_score_error": err.max().item(), "mean_abs_score_error": err.mean().item(),
                "median_top1_margin": margin.median().item(),
                "top1_flips": int(flipped.sum()),
                "max_margin_of_a_flip": margin[flipped].max().item() if flipped.any() else 0.0,
                "top1_exact_where_margin_gt_2x_error": bool((~flipped | (margin <= 2 * err.max())).all()),
                "pooled_min_cosine_vs_reference": torch.nn.functional.cosine_similarity(
                    pooled.cpu(), torch.from_numpy(g["pooled"]), dim=-1).min().item(),
                "ground_truth": "top-1 of the real reference EVA_CLIP (fp32, CPU) on the same corpus / prompts / synthetic "
                                "weights: tests/golden/eva_g14_c3.npz",
                "precision_fp32": fp32, "precision_bf16x3": x3, "rank_exact_rerank_k10": rank_exact})
    return res


def rank_exact_throughput(model, dev, videos=1024, frames=32):
    """Reference-rank retrieval at close to the bf16 towers' speed (retrieval.run_corpus(rank_exact_k=...)): a synthetic
    corpus of `videos` x `frames` frames (BASELINE configs[2]'s shape, a quarter of its size so the --full run stays short) goes through the
    bf16 tower once; the videos whose place in a query's top k is within twice the measured bf16 score error go through bf16x3 again.
    effective frames/s = corpus frames / (fast pass + measuring eps + re-encoding).  The 4096 x 32 figures (k = 1: 3.7 % re-encoded, 1948
    frames/s, top-1 lists equal to the whole corpus at bf16x3; k = 10: 13 %, 1581) are in profiles/r06/rank_exact_*.json."""
    import json
    from hirest_amd import retrieval, synth
    prompts = json.load(open(os.path.join(REPO, "tests", "golden", "test_prompts.json")))
    ids = synth.c3_device_names(videos)
    src = retrieval.FrameSource(ids, lambda lo, hi: synth.c3_device_block(lo, hi, frames, dev), videos_per_call=32)
    out = {"workload": f"{videos} videos x {frames} frames, {len(prompts)} real test prompts, EVA-CLIP-g/14 synthetic weights"}
    model.set_precision("bf16x3")
    retrieval.encode_videos(model, synth.c3_device_block(0, 32, frames, dev))      # warm-up: weight split, workspace
    model.set_precision("bf16")
    try:
        for k in (1, 10):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = retrieval.run_corpus(model, src, prompts, frames, rank_exact_k=k)
            res.topk(k)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            r = dict(res.rank_exact)
            out[f"k{k}"] = {"effective_frames_per_s": videos * frames / dt, "seconds": dt, "reencoded_fraction": r["reencoded_fraction"],
                            "reencoded": r["reencoded"], "eps": r["eps"], "max_abs_score_error_on_sample": r.get("max_abs_score_error_on_sample")}
    finally:
        model.set_precision("bf16")
    out["rank_exact_effective_frames_per_s"] = out["k1"]["effective_frames_per_s"]
    return out


def _log(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def _cpu_probe_child(threads: int, frames: int = 2, layers: int = 2):
    """Child process of cpu_baseline's pinned probes (python bench.py --cpu-probe N, started with OMP_NUM_THREADS=N OMP_PROC_BIND=close
    OMP_PLACES=cores): the oracle's tower on `layers` of the 40 identical blocks, random weights (the time does not depend on the values),
    extrapolated to 40 blocks.  Prints one JSON line."""
    import copy
    from oracle import ref_cpu
    from hirest_amd import synth
    torch.set_num_threads(threads)
    cfg = copy.deepcopy(synth.EVA_CLIP_G_14)
    L = cfg["vision_cfg"]["layers"]
    cfg["vision_cfg"]["layers"] = layers
    sd = synth.eva_clip_state_dict(cfg, 3, towers=("visual",))
    x = torch.randn(frames, 3, 224, 224)
    with torch.no_grad():
        ref_cpu.eva_encode_image(sd, x[:1], cfg)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref_cpu.eva_encode_image(sd, x, cfg)
            times.append(time.perf_counter() - t0)
    dt = sorted(times)[1]
    print(json.dumps({"threads": threads, "frames_per_s": frames / (dt * L / layers), "seconds_for_the_probe": sum(times),
                      "omp_proc_bind": os.environ.get("OMP_PROC_BIND"), "omp_places": os.environ.get("OMP_PLACES")}), flush=True)


def _pinned_probe(threads: int, timeout_s: float = 150.0):
    """cpu_baseline at `threads` OpenMP threads bound close to each other (one per core): a 2-block probe in a fresh process, because the
    binding has to be in the environment before the OpenMP runtime starts."""
    import subprocess
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads), OMP_PROC_BIND="close", OMP_PLACES="cores")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-probe", str(threads)], capture_output=True, text=True,
                           timeout=timeout_s, env=env)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        return json.loads(line[-1]) if r.returncode == 0 and line else {"threads": threads, "error": (r.stderr or r.stdout)[-300:]}
    except subprocess.TimeoutExpired:
        return {"threads": threads, "error": f"timed out after {timeout_s:.0f} s"}


def cpu_baseline(model, frames, cfg, n):
    """The fp32 CPU oracle (oracle/ref_cpu.py, torch CPU; kind "port") on the first n frames of the same batch.
    Reported at three thread counts: 32, os.cpu_count() and 1.  Only the 32-thread figure is a full measurement
    (1 warm-up frame + 3 timed passes of the whole 40-layer tower, median); torch's CPU kernels collapse far below this
    box's 256 hardware threads and a single thread needs ~15 s per frame, so those two are first PROBED on the first 2 of
    the 40 (identical) blocks and the full 3-pass measurement is only run for a thread count whose probe beats the
    32-thread rate — otherwise the probe's extrapolation (x 40 / 2 layers) is what is reported, and labelled so."""
    from oracle import ref_cpu
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items() if k.startswith("visual.")}
    sample = frames.reshape(-1, 3, 224, 224)[:n].float().cpu()
    ncpu = os.cpu_count() or 1
    L = cfg["vision_cfg"]["layers"]
    spent = 0.0

    def full(threads):
        nonlocal spent
        torch.set_num_threads(threads)
        ref_cpu.eva_encode_image(sd, sample[:1], cfg)       # warm-up
        times, out = [], None
        for _ in range(3):
            t0 = time.perf_counter()
            out = ref_cpu.eva_encode_image(sd, sample, cfg)
            times.append(time.perf_counter() - t0)
        spent += sum(times)
        return n / sorted(times)[1], out

    def probe(threads, layers=2):
        nonlocal spent
        torch.set_num_threads(threads)
        ref_cpu.eva_encode_image(sd, sample[:1], cfg, n_layers=1)
        t0 = time.perf_counter()
        ref_cpu.eva_encode_image(sd, sample[:1], cfg, n_layers=layers)
        dt = time.perf_counter() - t0
        spent += dt
        return 1.0 / (dt * L / layers)
    with torch.no_grad():
        base_threads = min(32, ncpu)
        _log(f"cpu baseline: {base_threads} threads, 3 passes x {n} frames")
        rate32, cpu_out = full(base_threads)
        by_threads = {str(base_threads): {"frames_per_s": rate32, "how": "measured: 3 passes, median"}}
        best_threads, best = base_threads, rate32
        if ncpu != base_threads:
            # all hardware threads: only a full measurement is reported.  A 2-block probe decides whether it is worth the
            # time (torch's CPU kernels collapse far below 256 threads: oversubscription, not a property of the workload);
            # a losing probe is logged, not printed as a rate.
            _log(f"cpu baseline: probing {ncpu} threads on 2 of {L} blocks")
            est = probe(ncpu)
            if est > rate32:
                r, _ = full(ncpu)
                by_threads[str(ncpu)] = {"frames_per_s": r, "how": "measured: 3 passes, median"}
                if r > best:
                    best_threads, best = ncpu, r
            else:
                _log(f"cpu baseline: {ncpu} threads slower than {base_threads} on the probe ({est:.4f} vs {rate32:.4f} frames/s): not measured")
        _log("cpu baseline: probing 1 thread on 2 blocks")
        one = probe(1)
        by_threads["1"] = {"frames_per_s": one, "how": "extrapolated from a 2-block probe of one frame"}
        # 64 / 128 threads with OMP_PROC_BIND=close OMP_PLACES=cores: fresh processes, 2-block probes.  `value` stays
        # the best FULL measurement; a pinned probe that beats it is reported beside it, labelled as what it is.
        for t in (64, 128):
            if t < ncpu:
                _log(f"cpu baseline: {t} threads pinned (OMP_PROC_BIND=close), 2-block probe in a child process")
                pr = _pinned_probe(t)
                by_threads[f"{t}_pinned"] = ({"frames_per_s": pr["frames_per_s"], "how": "extrapolated from a 2-block probe (2 frames, 3 passes, median) in a "
                                              "child process with OMP_PROC_BIND=close OMP_PLACES=cores", "beats_the_32_thread_measurement": pr["frames_per_s"] > rate32}
                                             if "frames_per_s" in pr else {"error": pr.get("error")})
    torch.set_num_threads(base_threads)
    # same kernels as the timed path: tower calls of >= 64 frames fold the LayerNorms into the GEMMs, so encode 64+ and keep n
    gpu_out = model.encode_image(frames.reshape(-1, 3, 224, 224)[:max(n, 64)])[:n].float().cpu()
    cos = torch.nn.functional.cosine_similarity(cpu_out, gpu_out, dim=-1).min().item()
    return {"value": best, "unit": "frames/s", "cores": best_threads, "kind": "port", "by_threads": by_threads,
            "single_thread": one, "host_cpus": ncpu,
            "sample": f"{n} frames of the same synthetic batch, full 40-layer EVA-CLIP-g/14 fp32 (oracle/ref_cpu.py, torch "
                      f"CPU), 1 warm-up frame + 3 timed passes (median) at {base_threads} threads; 1 thread probed on 2 of the 40 "
                      f"blocks; {ncpu} threads measured only if a probe beats {base_threads} (see by_threads); {spent:.1f} s of timed CPU work",
            "min_cosine_gpu_vs_cpu_on_sample": cos}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(outdir, rows, scores, val, idx):
    """--dump-outputs: the last timed step's results as float32 / float64 .npy files, so two builds can be compared output
    for output.  video_rows [V, E] and scores [Q, V] grow with the corpus: past DUMP_MAX_BYTES in all they are cut to a fixed,
    seeded sample of videos, whose corpus indices go to video_index.npy."""
    import numpy as np
    V = rows.shape[0]
    per_video = 4 * (rows.shape[1] + scores.shape[0]) + 8             # + its video_index entry when sampled
    keep = max(1, (DUMP_MAX_BYTES - 4096 - 12 * val.numel()) // per_video)   # 4096: the .npy headers
    out = {"topk_values": val.float(), "topk_indices": idx.double()}
    if keep < V:
        sel = torch.randperm(V, generator=torch.Generator().manual_seed(0))[:keep].sort().values
        out["video_index"] = sel.double()
        rows, scores = rows[sel.to(rows.device)], scores[:, sel.to(scores.device)]
    out["video_rows"], out["scores"] = rows.float(), scores.float()
    os.makedirs(outdir, exist_ok=True)
    for name, t in out.items():
        np.save(os.path.join(outdir, f"{name}.npy"), t.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--cpu-probe", type=int, default=0, help="internal: child process of cpu_baseline's pinned thread-count probes")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", type=int, default=FRAMES_PER_STEP, help="frames per GPU per step")
    ap.add_argument("--chunk", type=int, default=1024, help="frames per tower call (micro-batch)")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run the matched-R@k, CPU-baseline and secondary legs "
                    "(a plain run reports the headline and its roofline only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU-baseline leg")
    ap.add_argument("--cpu-frames", type=int, default=4, help="frames per timed pass of the CPU oracle (3 passes per thread count)")
    ap.add_argument("--no-matched-recall", action="store_true", help="with --full: skip the matched-R@k leg (reference-pinned sub-corpus)")
    ap.add_argument("--gemm-kernel", type=int, default=0, help="0 auto, 1 force t128, 2 force t256 (A/B timing)")
    ap.add_argument("--no-ln-fold", action="store_true", help="A/B: run the LayerNorm passes instead of folding them into the GEMMs")
    ap.add_argument("--no-prune", action="store_true", help="A/B: run the last block on every token (results identical)")
    ap.add_argument("--no-profile", action="store_true", help="A/B: no per-launch hipEvent pairs inside the timed region (the line then "
                    "carries no roofline; profiles/r04/README.md holds the comparison)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the joint-model / captioning / training / ASR figures")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"), help="nccl = RCCL over xGMI (the measured path); gloo: functional tests")
    ap.add_argument("--share-gpu", action="store_true", help="FUNCTIONAL TEST ONLY (needs --backend gloo): rank r runs on device r %% device_count, "
                    "so the N-rank code path — launcher, timing protocol, gather, rank-0 report — runs on a one-GPU box.  The line is marked INVALID")
    ap.add_argument("--gemm-dbg", type=int, default=0, help="hirest_gemm_debug_mode bits: TIMING EXPERIMENTS ONLY, the line is not a valid result")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one returned (gathered video rows, "
                    "scores, top-k values and indices) as DIR/<name>.npy; same arguments, same inputs")
    args = ap.parse_args()
    if args.cpu_probe > 0:
        _cpu_probe_child(args.cpu_probe)
        return
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")

    if args.frames % FRAMES_PER_VIDEO != 0:
        raise SystemExit(f"--frames must be a multiple of {FRAMES_PER_VIDEO} (whole videos): a remainder would be counted "
                         "in frames/s without being encoded")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the measured path)")
    if args.share_gpu and args.backend != "gloo":
        raise SystemExit("--share-gpu needs --backend gloo (RCCL refuses two ranks on one device)")
    launch.ensure_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:],
                        visible_devices=None if args.share_gpu else torch.cuda.device_count())
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dev_index = local_rank % torch.cuda.device_count() if args.share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    import torch.distributed as dist
    rank, local_rank, world = launch.init_ranks(args.gpus, args.backend, device=dev)   # "nccl" is RCCL on ROCm
    assert world == args.gpus and (world == 1 or dist.get_world_size() == args.gpus)

    import hirest_amd
    from hirest_amd import _lib, retrieval, synth
    lib = _lib.load()
    lib.hirest_gemm_select_kernel(args.gemm_kernel)
    lib.hirest_gemm_debug_mode(args.gemm_dbg)

    cfg = synth.EVA_CLIP_G_14
    model = hirest_amd.EVA_CLIP(**cfg).to(dev).eval()
    model.init_random_(seed=1234)
    model.visual.max_frames_per_call = args.chunk
    if args.no_ln_fold:
        model.visual.fold_layernorm = False
    if args.no_prune:
        model.visual.prune_last_block = False
    # the pruned last block exists in the folded form of the tower (calls of >= 64 frames)
    gflop_frame = GFLOP_EXECUTED_PER_FRAME if (not args.no_prune and not args.no_ln_fold and args.chunk >= 64) else GFLOP_PER_FRAME

    V_local = args.frames // FRAMES_PER_VIDEO
    gen = torch.Generator(device=dev)
    gen.manual_seed(99 + rank)
    frames = torch.randn((V_local, FRAMES_PER_VIDEO, 3, 224, 224), device=dev, dtype=torch.float32, generator=gen).to(torch.bfloat16)
    tokens = synth.tokens("bench.queries", N_QUERIES, 5).to(dev)
    text_n = retrieval.encode_texts(model, tokens)            # queries encoded once, outside the frame metric
    V_total = V_local * world
    gather = retrieval.RowGather()                                          # receive buffer allocated once, reused every step

    def step():
        pooled = retrieval.encode_videos(model, frames)                     # [V_local, 1024]
        allv = gather(pooled, V_total)                                      # RCCL all-gather (no-op at N=1)
        scores, val, idx = retrieval.retrieve(text_n, allv, min(TOPK, V_total))
        return allv, scores, val, idx

    tinfo = {}
    elapsed, last = launch.timed_steps(step, args.warmup, args.steps, torch.cuda.synchronize,
                                       on_timed_start=(None if args.no_profile else (lambda: lib.hirest_profile_enable(1))), reduce_device=dev,
                                       info=tinfo)
    # per-launch records of the timed steps (this rank)
    recs = (_lib.ProfRecord * 200000)()
    nrec = lib.hirest_profile_collect(recs, len(recs))
    lib.hirest_profile_enable(0)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, *last)

    out = None
    if rank == 0:
        frames_total = V_local * FRAMES_PER_VIDEO * world * args.steps
        value = frames_total / elapsed
        # ---- roofline of the dominant kernel, from the live records
        groups = {}
        kinds = {0: "gemm", 1: "attention", 2: "layernorm"}
        for i in range(max(nrec, 0)):
            r = recs[i]
            key = (r.kind, r.tag, r.d0, r.d1, r.d2)
            g = groups.setdefault(key, [0, 0.0])
            g[0] += 1
            g[1] += r.ms
        total_ms = sum(g[1] for g in groups.values()) or 1.0
        breakdown = []
        for (kind, tag, d0, d1, d2), (cnt, ms) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
            ent = {"kernel": kinds.get(kind, str(kind)), "tag": tag, "dims": [d0, d1, d2], "launches": cnt,
                   "avg_ms": ms / cnt, "share": ms / total_ms}
            if kind == 0:
                ent["tflops"] = 2.0 * d0 * d1 * d2 / (ms / cnt * 1e-3) / 1e12
            elif kind == 1:
                ent["tflops"] = 4.0 * d0 * d1 * d1 * d2 / (ms / cnt * 1e-3) / 1e12   # QK^T + PV, algorithmic
            breakdown.append(ent)
        dom = next((e for e in breakdown if e["kernel"] == "gemm"), None)
        roofline = None
        traffic = None
        if dom:
            # HBM-side bytes per launch of this kernel from the committed rocprofv3 PMC profile (FETCH_SIZE + WRITE_SIZE,
            # separate passes, gfx950 correction; tools/pmc_traffic.sh).  bench.py cannot sample counters on itself.
            try:
                prof_path = next(p for p in (os.path.join(REPO, "profiles", r, "pmc_traffic.json") for r in PROFILE_ROUNDS)
                                 if os.path.isfile(p))
                prof = json.load(open(prof_path))
                same_tag = [e for e in breakdown if e["kernel"] == "gemm" and e["tag"] == dom["tag"]
                            and e["launches"] == dom["launches"]]
                same_tag.sort(key=lambda e: -e["dims"][0] * e["dims"][2])            # more operand bytes first
                cands = [k for k in prof["kernels"] if (f"gemm_p256<{dom['tag']}," in k["kernel"] or f"gemm_pp256<{dom['tag']}>" in k["kernel"] or f"gemm_pp256<{dom['tag']}," in k["kernel"]
                                                          or f"gemm_pq256<{dom['tag']}>" in k["kernel"])
                         and k["launches"] * args.steps in (dom["launches"], dom["launches"] - args.steps)]
                cands.sort(key=lambda k: -k["fetch_bytes_per_launch"])
                which = same_tag.index(dom)
                if which < len(cands):
                    traffic = cands[which]["traffic_bytes_per_launch"]
            except (OSError, ValueError, KeyError, StopIteration):
                traffic = None
        if dom:
            epi = {0: "bias", 1: "bias+gelu", 2: "bias+quickgelu", 3: "bias+residual", 4: "bias->f32", 5: "patch+pos",
                   6: "bias+residual+ln-stats", 7: "ln-fold+bias", 8: "ln-fold+bias+gelu",
                   10: "bias+residual(hi+lo)+ln-stats"}
            roofline = {"bound": "mfma", "achieved": dom["tflops"], "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": dom["tflops"] / MFMA_BF16_PEAK_TFLOPS, "traffic": traffic,
                        "traffic_missing": traffic is None,      # loud: no committed profile matches the kernels this run dispatched
                        "traffic_note": "bytes per launch through the L2's memory side (Infinity-Cache hits included), from the "
                                        "newest committed profiles/rNN/pmc_traffic.json (rocprofv3 PMC passes of this same "
                                        "command; tests/test_abi_and_host.py checks its kernel names against the current "
                                        "dispatch); null if no matching profile",
                        "kernel": f"gemm<{epi.get(dom['tag'], dom['tag'])}> M={dom['dims'][0]} N={dom['dims'][1]} K={dom['dims'][2]}",
                        "avg_launch_ms": dom["avg_ms"], "launches": dom["launches"],
                        "algorithmic_flops_per_launch": 2.0 * dom["dims"][0] * dom["dims"][1] * dom["dims"][2],
                        # the tower fraction counts EXECUTED work (the pruned last block is not credited); the figure on the
                        # unpruned 534.06 GFLOP/frame is given beside it for comparison with rounds 1-2
                        "whole_tower_tflops": value / world * gflop_frame / 1e3,
                        "whole_tower_frac": value / world * gflop_frame / 1e3 / MFMA_BF16_PEAK_TFLOPS,
                        "executed_gflop_per_frame": gflop_frame, "unpruned_gflop_per_frame": GFLOP_PER_FRAME,
                        "whole_tower_frac_on_unpruned_flops": value / world * GFLOP_PER_FRAME / 1e3 / MFMA_BF16_PEAK_TFLOPS,
                        "breakdown": breakdown[:12]}
        out = {"metric": "encoded frames/sec (EVA-CLIP-g/14 224^2)", "value": value, "unit": "frames/s",
               "n_gpus": world, "rccl_ranks": dist.get_world_size() if world > 1 else 1, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": elapsed / args.steps * 1e3,
               # every rank's own time per step up to its own device sync, before the closing barrier (ms_per_step is their MAX + the barrier):
               # the first real N-GPU run shows skew between ranks, not just a sum
               "ms_per_step_by_rank": [t / args.steps * 1e3 for t in tinfo.get("per_rank_s", [])],
               "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "config": {"workload": "EVA-CLIP-g/14 frame encoder, 1024-frame synthetic batch bf16 per GPU per step "
                                      "(BASELINE configs[1]) as 32 videos x 32 frames -> mean-pool+L2 -> all-gather "
                                      "[V,1024] rows -> 546-query cosine top-10; random-init weights",
                          "frames_per_gpu_per_step": args.frames, "global_batch": args.frames * world,
                          "micro_batch": args.chunk, "parallelism": f"dp{world}",
                          "arithmetic": "bf16 MFMA products, fp32 accumulation / LayerNorm statistics / softmax / pooling / scoring; residual "
                                        "stream between the blocks held as bf16 hi + bf16 lo (16 significand bits; HIREST_F32_RESIDUAL=1: fp32 array)"},
               "roofline": roofline}
        if args.no_profile:
            out["profile"] = "off (--no-profile: no per-launch event pairs in the timed region, hence no roofline in this line)"
        if args.share_gpu or args.backend != "nccl":
            out["INVALID"] = f"functional run of the N-rank path: backend {args.backend}" + (", ranks sharing the GPU(s)" if args.share_gpu else "")
        if args.gemm_dbg & ~512:                       # bit 9 only switches the kernels' walk direction off (A/B), results unchanged
            out["INVALID"] = f"timing experiment: hirest_gemm_debug_mode({args.gemm_dbg})"

    # ---- everything below runs with --full only: a plain run ends with the headline line.
    # matched R@k at EVA-CLIP-g/14 scale (BASELINE.json's "at matched R@1"), outside the timed region, rank 0:
    # the sub-corpus and the 546 real prompts whose rankings the REAL reference produced in the build container
    # (tests/golden/eva_g14_c3.npz, made by tests/golden/make_golden.py gen_c3) are re-encoded here by the same kernels
    # the timed step ran (one >= 64-frame tower call) and ranked; GT(q) = the reference's top-1.
    if rank == 0 and args.full and not args.no_matched_recall:
        _log("matched R@k leg: synthetic checkpoint of the reference-pinned sub-corpus")
        out["matched_recall"] = matched_recall(model, dev)
        _log("rank-exact retrieval: margin-guarded re-rank on a synthetic corpus of 32-frame videos")
        out["matched_recall"]["rank_exact_throughput"] = rank_exact_throughput(model, dev, videos=1024 if args.frames >= 1024 else 256)
        _log("matched R@k leg done")

    # ---- CPU baseline: the fp32 oracle on this host's cores, bounded sample (rank 0, N=1 only)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(model, frames, cfg, args.cpu_frames)
    # ---- the other rows of SURVEY 8 (configs[3], configs[4], f4) at the reference's operating point, outside the timed
    # region, rank 0, N = 1: value + roofline fraction + CPU oracle each (tools/secondary_bench.py)
    if rank == 0 and world == 1 and args.full and not args.no_secondary:
        small = small_calls(model, frames)
        del frames
        model.visual._workspace = None
        torch.cuda.empty_cache()
        sys.path.insert(0, os.path.join(REPO, "tools"))
        import secondary_bench
        out["secondary"] = secondary_bench.measure(dev, cpu=not args.no_cpu_baseline, log=_log)
        out["secondary"]["tower_small_calls"] = small
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()                 # rank 0's untimed legs (matched R@k) are done before anyone tears the group down
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
