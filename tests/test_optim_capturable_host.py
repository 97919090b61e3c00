"""CPU-side checks of hirest_amd.optim.AdamW(capturable=True) (csrc/optim_capturable.hip): what the constructor accepts and refuses in
either mode, that a scheduler drives a tensor lr in place, that the new entry points refuse bad arguments before any launch, and that
the new kernels neither spill nor use scratch memory."""
import ctypes
import os

import pytest
import torch

from test_code_objects import kernel_notes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSAL = r"tensor lr / betas \(capturable\) are not implemented"


@pytest.fixture(scope="module")
def lib():
    from hirest_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture
def cpu_params(monkeypatch):
    """Parameters on the CPU stand in for device ones: the constructor's device check is switched off, nothing is launched."""
    from hirest_amd import optim
    monkeypatch.setattr(optim, "_check_param", lambda p: None)
    return [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(3))]


def test_capturable_constructs_with_tensor_lr_and_a_scheduler_fills_it(cpu_params):
    from hirest_amd import optim
    lrs = [torch.tensor(1e-3), torch.tensor([3e-3])]
    opt = optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(cpu_params, lrs)], capturable=True, max_grad_norm=1.0)
    assert all(g["capturable"] and g["lr"] is lr for g, lr in zip(opt.param_groups, lrs))
    assert opt._step_supports_amp_scaling is True
    # get_linear_schedule_with_warmup is a LambdaLR: the group's tensor keeps its identity (its address is what a graph recorded)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: min(1.0, (e + 1) / 4))
    for e in range(1, 4):
        sched.step()
        for g, lr, base in zip(opt.param_groups, lrs, (1e-3, 3e-3)):
            assert g["lr"] is lr and lr.dtype == torch.float32 and lr.item() == (torch.tensor(base) * ((e + 1) / 4)).item()
    assert optim.AdamW(cpu_params, lr=torch.tensor(1e-3), capturable=True).param_groups[0]["lr"].numel() == 1     # a default lr tensor
    assert optim.AdamW(cpu_params, lr=1e-3, capturable=True).param_groups[0]["lr"] == 1e-3                        # floats stay floats
    for bad in (torch.tensor(1e-3, dtype=torch.float64), torch.tensor([1e-3, 1e-3])):
        with pytest.raises(ValueError):
            optim.AdamW(cpu_params, lr=bad, capturable=True)
    with pytest.raises(ValueError, match=REFUSAL):
        optim.AdamW(cpu_params, betas=(torch.tensor(0.9), 0.999), capturable=True)                                # tensor betas: out of scope


def test_default_mode_still_refuses_tensor_lr_and_has_no_amp_hook(cpu_params):
    from hirest_amd import optim
    with pytest.raises(ValueError, match=REFUSAL):
        optim.AdamW(cpu_params, lr=torch.tensor(1e-3))
    with pytest.raises(ValueError, match=REFUSAL):
        optim.AdamW(cpu_params, lr=torch.tensor(1e-3), capturable=False)
    opt = optim.AdamW(cpu_params, lr=1e-3)
    assert not getattr(opt, "_step_supports_amp_scaling", False) and opt.param_groups[0]["capturable"] is False
    assert getattr(optim.AdamW(cpu_params, capturable=True), "_step_supports_amp_scaling", False)


@pytest.mark.parametrize("capturable", [False, True])
def test_amsgrad_and_maximize_are_refused_in_both_modes(cpu_params, capturable):
    from hirest_amd import optim
    with pytest.raises(ValueError, match="amsgrad / maximize"):
        optim.AdamW(cpu_params, amsgrad=True, capturable=capturable)
    with pytest.raises(ValueError, match="amsgrad / maximize"):
        optim.AdamW(cpu_params, maximize=True, capturable=capturable)


def _items(count, **over):
    from hirest_amd._lib import OptimItem
    arr = (OptimItem * count)()
    X = 1 << 20                    # placeholder addresses: every call below is refused by its argument checks, none is dereferenced
    for i, it in enumerate(arr):
        it.p, it.g, it.m, it.v, it.n = X, X, X, X, 100 + i
        for k, v in over.items():
            setattr(it, k, v)
    return arr


def _steps(count, hole=None):
    arr = (ctypes.c_void_p * count)(*[1 << 20] * count)
    if hole is not None:
        arr[hole] = None
    return arr


def test_new_entry_points_refuse_bad_arguments_without_gpu(lib):
    from hirest_amd._lib import OPTIM_GROUP_MAX
    BAD, X = -1, 1 << 20
    hp = (0.9, 0.999, 1e-8, 0.01)                   # beta1, beta2, eps, weight_decay

    def update(items, steps, count, betas=hp[:2]):
        return lib.hirest_adamw_capturable_grouped_f32(items, steps, count, None, None, 1e-3, None, None, *betas, *hp[2:], None)
    ok, big = _items(3), _items(OPTIM_GROUP_MAX + 1)
    for items, count in ((None, 3), (ok, 0), (ok, -1), (big, OPTIM_GROUP_MAX + 1)):           # the item table
        assert lib.hirest_grad_sqnorm_scaled_grouped_f32(items, count, None, X, None) == BAD
        assert update(items, _steps(max(count, 1)), count) == BAD
    for count in (0, -1, OPTIM_GROUP_MAX + 1):                                                # the steps table
        assert lib.hirest_optim_step_advance_f32(_steps(OPTIM_GROUP_MAX + 1), count, None, None) == BAD
    assert lib.hirest_optim_step_advance_f32(None, 3, None, None) == BAD
    assert lib.hirest_optim_step_advance_f32(_steps(3, hole=1), 3, None, None) == BAD
    assert update(ok, None, 3) == BAD
    assert update(ok, _steps(3, hole=2), 3) == BAD
    assert lib.hirest_grad_sqnorm_scaled_grouped_f32(ok, 3, None, None, None) == BAD           # no partials array
    for args in ((None, 4, X, X), (X, 4, None, X), (X, 4, X, None), (X, 0, X, X)):            # the clip bound on the device
        assert lib.hirest_clip_coef_dev_f32(*args, None) == BAD
    for field in ("p", "g", "m", "v"):                                                        # a NULL tensor, a non-positive length
        assert update(_items(2, **{field: None}), _steps(2), 2) == BAD
    assert update(_items(2, n=0), _steps(2), 2) == BAD
    assert lib.hirest_grad_sqnorm_scaled_grouped_f32(_items(2, g=None), 2, None, X, None) == BAD
    assert lib.hirest_grad_sqnorm_scaled_grouped_f32(_items(2, n=-5), 2, None, X, None) == BAD
    assert update(ok, _steps(3), 3, betas=(1.0, 0.999)) == BAD and update(ok, _steps(3), 3, betas=(0.9, -0.1)) == BAD


def test_capturable_kernels_do_not_spill(lib, tmp_path):
    """Like the kernels they sit beside: 8 waves per SIMD, no spilled register, no scratch memory, the double pow included."""
    notes = kernel_notes(os.path.join(REPO, "hirest_amd", "lib", "optim_capturable.o"), str(tmp_path))
    wanted = ("grad_sqnorm_scaled_kernel", "clip_coef_dev_kernel", "step_advance_kernel", "adamw_capturable_kernel")
    assert len(notes) == 4 and all(any(k in name for name in notes) for k in wanted), sorted(notes)
    for k, v in notes.items():
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
        assert v["vgpr_count"] <= 64, (k, v)
