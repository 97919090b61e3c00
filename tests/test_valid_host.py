"""CPU-side checks of the validation kernels' entry points (csrc/valid.hip): every documented argument error is refused before
anything is enqueued (the placeholder pointer is never dereferenced), and the wrappers reject bad shapes with ValueError."""
import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_argument_errors_without_gpu(lib):
    X, BAD, SHAPE, WS = 1 << 20, -1, -2, -3
    mv = lambda *p, B=2, T=300: lib.hirest_moment_valid_f32(*p[:5], B, T, -1e10, *p[5:], None)
    for i in range(7):
        assert mv(*[None if j == i else X for j in range(7)]) == BAD
    assert mv(*[X] * 7, B=0) == BAD and mv(*[X] * 7, T=0) == BAD and mv(*[X] * 7, B=1025) == BAD
    assert lib.hirest_lm_head_ce_workspace_bytes(200, 30524) == 200 * 60 * 16          # one 16-byte partial per (row, 512-column slice)
    assert lib.hirest_lm_head_ce_workspace_bytes(1, 17) == 16 and lib.hirest_lm_head_ce_workspace_bytes(3, 513) == 3 * 2 * 16
    assert lib.hirest_lm_head_ce_workspace_bytes(0, 17) == 0 and lib.hirest_lm_head_ce_workspace_bytes(4, 0) == 0
    big = 1 << 30

    def ce(ptrs=(X,) * 7, ldh=768, ldw=768, R=4, V=20, K=768, n_valid=4, ws=big):
        h, w, b, t, nll, loss, wsp = ptrs
        return lib.hirest_lm_head_ce_f32(h, ldh, w, ldw, b, t, R, V, K, n_valid, nll, loss, wsp, ws, None)
    for i in range(7):
        assert ce(tuple(None if j == i else X for j in range(7))) == BAD
    assert ce(R=0) == BAD and ce(V=0) == BAD and ce(K=0) == BAD and ce(n_valid=-1) == BAD
    assert ce(ldh=764) == BAD and ce(ldw=767) == BAD and ce(ldh=770) == BAD         # shorter than a row / rows not 16-byte aligned
    assert ce(K=512, ldh=512, ldw=512) == SHAPE
    assert ce(ws=4 * 16 - 1) == WS


def test_wrappers_reject_bad_shapes_before_any_launch():
    from hirest_amd import ops
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    with pytest.raises(ValueError):
        ops.lm_head_ce(z(4, 768), z(20, 512), z(20), z(4, dt=torch.int32))
    with pytest.raises(ValueError):
        ops.lm_head_ce(z(4, 768), z(20, 768), z(21), z(4, dt=torch.int32))
    with pytest.raises(ValueError):
        ops.lm_head_ce(z(4, 768), z(20, 768), z(20), z(5, dt=torch.int32))
    with pytest.raises(ValueError):
        ops.lm_head_ce(z(0, 768), z(20, 768), z(20), z(0, dt=torch.int32))
    with pytest.raises(ValueError):
        ops.moment_valid(z(2, 11), z(2, 6, dt=torch.int32), z(2, 6, dt=torch.int32), z(2, dt=torch.int32), z(2, dt=torch.int32))
    with pytest.raises(ValueError):
        ops.moment_valid(z(2, 12), z(2, 6, dt=torch.int32), z(2, 5, dt=torch.int32), z(2, dt=torch.int32), z(2, dt=torch.int32))
    with pytest.raises(ValueError):
        ops.moment_valid(z(2, 12), z(2, 6, dt=torch.int32), z(2, 6, dt=torch.int32), z(3, dt=torch.int32), z(2, dt=torch.int32))


def test_causal_mask_rule_and_targets_on_the_host():
    """MomentModel.valid_step's mask rule: the causal penalty alone is exact where no target position has a padded key at or before it."""
    from hirest_amd import MomentModel, synth
    tt = synth.caption_targets("host.cap", 3, 48, 5)
    inp, mask, out = MomentModel._caption_targets({"target_text": tt})
    assert inp.shape == mask.shape == out.shape == (3, 48) and inp.dtype == np.int64
    assert MomentModel._causal_mask_is_exact(mask, out)                   # the loader's masks: ones, then zeros
    holed = mask.copy()
    holed[1, 1] = 0
    assert not MomentModel._causal_mask_is_exact(holed, out)             # a padded key in front of a target
    late = mask.copy()
    late[2, 47] = 0 if out[2, 47] < 0 else late[2, 47]
    late[0, int((out[0] >= 0).sum()):] = 0                               # zeros only behind the last target: still exact
    assert MomentModel._causal_mask_is_exact(late, out)
    assert MomentModel._causal_mask_is_exact(np.zeros_like(mask), np.full_like(out, -1))      # no target at all
