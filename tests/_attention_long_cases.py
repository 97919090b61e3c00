"""Shapes and seeds shared by tests/test_attention_long_host.py (which proves the input families' guarantees for exactly these cases on the
CPU) and tests/test_gpu_attention_long.py (which runs them).  Not a test module."""
import _exact_inputs as X

H, DH = X.ATTN_H, 64
# first length the short kernels refuse, whole 64-key tiles, one key past them, ViT-L/14@336px, many tiles + 1
LENGTHS = [273, 320, 321, 577, 1025]
BATCHES = [1, 3]
# (B, N, seed) of the selector family: every one has selector_gap > 64 (test_attention_long_host.py), none needs excusing
SELECTOR_CASES = [(B, N, 0) for N in LENGTHS for B in BATCHES]
Q_ROWS = [1, 17]
SHORT_MAX = 272                      # hirest_attention_bf16 / _rows hold at most this many tokens on chip
LONG_MAX = 4096


def tower_takes_long_entry(T, head_dim):
    """csrc/tower.hip, vision_attention_long: the vision call sites take hirest_attention_bf16_long exactly then."""
    return T > SHORT_MAX and head_dim == 64
