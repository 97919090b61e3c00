"""Numpy restatement of the word alignment: the alignment matrix, the median filter, dynamic time warping and the word
logic of ``find_alignment``.  Written from the definitions in the design section (OpenAI's whisper/timing.py is not in this tree), in
fp64 unless a dtype is passed — the fp32 forms are the yardstick's error and, for ``dtw``, the bit-exact reference."""
import itertools

import numpy as np


def median_filter(x, width):
    """median of ``width`` (odd) along the last axis, reflect padding of width // 2; unfiltered when the axis has <= width // 2 elements"""
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    padded = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    windows = np.lib.stride_tricks.sliding_window_view(padded, width, axis=-1)
    return np.sort(windows, axis=-1)[..., pad]


def head_weights(queries, cross_kv, pairs, n_keys, qk_scale, dtype):
    """steps 1 and 2: [n_sel, T, n_keys] softmax over the first n_keys keys, normalised per key over the tokens"""
    out = []
    for layer, head in pairs:
        q = np.asarray(queries[layer], dtype=dtype)[:, 64 * head:64 * head + 64]
        D = queries[layer].shape[1]
        k = np.asarray(cross_kv[layer], dtype=dtype)[:n_keys, :D][:, 64 * head:64 * head + 64]
        s = (q @ k.T) * dtype(0.125 * qk_scale)
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        out.append(e / e.sum(axis=-1, keepdims=True))
    w = np.stack(out)
    mean, std = w.mean(axis=1, keepdims=True, dtype=dtype), w.std(axis=1, keepdims=True, dtype=dtype)
    if dtype == np.float64:                                           # no column is excused: every one has a spread worth dividing by
        assert (std > 1e-3 * np.abs(w).mean(axis=1, keepdims=True)).all(), "a column's standard deviation is below 1e-3 of its mean weight"
    return ((w - mean) / std).astype(dtype)


def alignment_matrix(queries, cross_kv, pairs, n_keys, qk_scale=1.0, medfilt_width=7, row0=0, n_rows=None, dtype=np.float64):
    w = head_weights(queries, cross_kv, pairs, n_keys, qk_scale, dtype)
    w = median_filter(w, medfilt_width)
    m = w.mean(axis=0, dtype=dtype)
    return m[row0:(None if n_rows is None else row0 + n_rows)]


def dtw(x, dtype=np.float64, return_cost=False):
    """the recurrence and the backtrace as DESIGN 4.19 states them; every cell one addition in ``dtype``"""
    x = np.asarray(x, dtype=dtype)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=dtype)
    trace = -np.ones((N + 1, M + 1), dtype=np.int64)
    cost[0, 0] = 0
    for i in range(1, N + 1):
        row, above, xi = cost[i], cost[i - 1], x[i - 1]
        for j in range(1, M + 1):
            c0, c1, c2 = above[j - 1], above[j], row[j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            row[j] = xi[j - 1] + c
            trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j, path = N, M, []
    while i > 0 or j > 0:
        path.append((i - 1, j - 1))
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    path = np.array(path[::-1], dtype=np.int64).reshape(-1, 2)
    return (path[:, 0], path[:, 1]) + ((cost[1:, 1:],) if return_cost else ())


def monotone_paths(N, M):
    """every path from (0, 0) to (N - 1, M - 1) by steps (1, 1), (1, 0), (0, 1)"""
    def walk(i, j):
        if (i, j) == (N - 1, M - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < N and j + dj < M:
                for rest in walk(i + di, j + dj):
                    yield [(i, j)] + rest
    return list(walk(0, 0))


def path_cost(x, path):
    return sum(x[i, j] for i, j in path)


def words_from_path(words, word_tokens, text_indices, time_indices, token_probs):
    """(word, tokens, start, end, probability) of every word but the last (eot's)"""
    lengths = [len(t) for t in word_tokens[:-1]]
    bounds = [0] + list(itertools.accumulate(lengths))
    jumps = [k for k in range(len(text_indices)) if k == 0 or text_indices[k] != text_indices[k - 1]]
    times = [time_indices[k] / 50 for k in jumps]
    return [(words[n], list(word_tokens[n]), float(times[bounds[n]]), float(times[bounds[n + 1]]), float(np.mean(token_probs[bounds[n]:bounds[n + 1]])))
            for n in range(len(lengths))]
