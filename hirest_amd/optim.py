"""Native optimizer step for the joint model's training loop: ``AdamW`` below does what the reference's
``clip_grad_norm_(model.parameters(), c)`` + ``torch.optim.AdamW.step()`` (run.py:264-295, trainer_base.py:55-61) do, in the kernels
of csrc/optim.hip: per-chunk sums of squared gradients -> total norm and clip coefficient (device floats) -> one read-modify-write
pass over p, exp_avg, exp_avg_sq with the coefficient applied to the gradient on the fly.  Nothing is read back: ``step()`` never
synchronises.  The state layout is torch.optim.AdamW's, so state dicts load either way.  ``capturable=True`` moves every per-step
scalar (step counts, learning rate, a loss scaler's scale and verdict) to the device: the kernels of csrc/optim_capturable.hip.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops

OPTIM_CHUNK = _lib.OPTIM_CHUNK
OPTIM_GROUP_MAX = _lib.OPTIM_GROUP_MAX
_UNSET = object()


def chunk_map(sizes, chunk: int = OPTIM_CHUNK):
    """Which workgroup handles what: [(item, start, count)] in workgroup order for tensors of ``sizes`` elements.  Item i is cut into
    ceil(n_i / chunk) chunks; a chunk never spans two tensors.  A pure function of the sizes (the kernels compute the same map from
    the item table: hirest_optim_partials_count is its length)."""
    out = []
    for i, n in enumerate(sizes):
        if n <= 0:
            raise ValueError(f"tensor {i} has {n} elements")
        out.extend((i, s, min(chunk, n - s)) for s in range(0, n, chunk))
    return out


def group_ranges(n_items: int, group_max: int = OPTIM_GROUP_MAX):
    """[(lo, hi)]: the item ranges of the launches that cover ``n_items`` tensors, at most ``group_max`` per launch."""
    return [(lo, min(lo + group_max, n_items)) for lo in range(0, n_items, group_max)]


def hyperparameters(step: int, lr: float, betas, eps: float, weight_decay: float):
    """The scalars of one update, in double precision from the step count exactly as torch.optim.AdamW derives them (its default
    path): bias corrections, step size, sqrt of the second correction, decay factor and the two complements."""
    beta1, beta2 = betas
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    return {"bc1": bc1, "bc2_sqrt": bc2 ** 0.5, "step_size": lr / bc1, "decay": 1 - lr * weight_decay,
            "one_minus_beta1": 1 - beta1, "beta2": beta2, "one_minus_beta2": 1 - beta2, "eps": eps}


def _check_lr(lr):
    if lr.dtype != torch.float32 or lr.numel() != 1:
        raise ValueError(f"hirest_amd.optim.AdamW: a tensor lr must be one fp32 element, got {lr.dtype} with {lr.numel()}")


def _device_scalar(x, device, what):
    """Address of a 1-element fp32 tensor on ``device`` (lr, grad_scale, found_inf); None stays None."""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.numel() != 1 or x.device != device:
        raise ValueError(f"hirest_amd.optim.AdamW: {what} must be a 1-element fp32 tensor on {device}")
    return x.data_ptr()


def _check_param(p):
    if not isinstance(p, torch.Tensor):
        raise ValueError(f"hirest_amd.optim.AdamW: parameters must be tensors, got {type(p).__name__}")
    if p.dtype != torch.float32:
        raise ValueError(f"hirest_amd.optim.AdamW: fp32 parameters only, got {p.dtype}")
    if not p.is_cuda:
        raise ValueError(f"hirest_amd.optim.AdamW: parameters must be on the GPU, got {p.device}")
    if p.is_sparse or not p.is_contiguous():
        raise ValueError("hirest_amd.optim.AdamW: parameters must be dense and contiguous")


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (decoupled weight decay, bias-corrected, no amsgrad) with gradient-norm clipping folded in.

    ``max_grad_norm=c`` clips the gradients of ALL param groups together to total 2-norm ``c`` as
    ``clip_grad_norm_(model.parameters(), c)`` does, without writing them: the update uses ``coef * grad``.  ``None``: no clipping
    (and no norm is computed).  ``step(max_grad_norm=x)`` overrides it for one call.  ``grad_norm`` is a 0-dim device tensor with the
    last pre-clip total norm (what clip_grad_norm_ returns); reading it is the caller's synchronisation, ``step()`` has none.

    ``capturable=True`` keeps everything that changes from step to step on the device, so that ``step()`` can be recorded into a
    hipGraph (``torch.cuda.graph``) and replayed, and can sit behind ``torch.amp.GradScaler`` without a host read:

    * ``state[p]["step"]`` is a 0-dim fp32 device tensor (torch's capturable layout); a kernel advances it and every workgroup of the
      update derives the bias corrections from it.  A state loaded from a non-capturable optimizer is moved over by
      ``load_state_dict``.
    * a group's ``lr`` may be a 1-element fp32 device tensor, which schedulers fill in place (``LambdaLR`` does).
    * ``_step_supports_amp_scaling`` is set: ``GradScaler.step`` leaves ``grad_scale`` and ``found_inf`` on the instance.  Gradients
      count as ``g * (1 / grad_scale)``, the clip norm is that of the unscaled gradients, gradients are never written, and a step
      whose ``found_inf`` is non-zero changes neither parameters, moments nor step counts.

    The capture contract: run one eager ``step()`` first (it creates the state and the workspaces), then capture.  A replay repeats
    the recorded launches on the recorded addresses, so gradients must live at fixed addresses (``zero_grad(set_to_none=False)``, or
    fill them in place), the set of parameters that have a gradient is frozen at capture, and ``lr`` must be a tensor if it is to
    change between replays; so must ``max_grad_norm`` (a 1-element fp32 device tensor is accepted in this mode).  Floats, ``betas``,
    ``eps`` and ``weight_decay`` among them, are recorded by value.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 max_grad_norm=None, capturable=False):
        if amsgrad or maximize:
            raise ValueError("hirest_amd.optim.AdamW: amsgrad / maximize are not implemented")
        if (isinstance(lr, torch.Tensor) and not capturable) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("hirest_amd.optim.AdamW: tensor lr / betas (capturable) are not implemented")
        if isinstance(lr, torch.Tensor):
            _check_lr(lr)
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        self._scalars = None          # device floats [total_norm, coef]
        self._partials = None         # one float per chunk
        self._norm_valid = False
        self._capturable = bool(capturable)
        if capturable:
            self._step_supports_amp_scaling = True    # torch.amp.GradScaler.step: sets grad_scale / found_inf and calls step() itself
        # the keys torch.optim.AdamW keeps in a param group, with its defaults: a state dict saved here loads there as AdamW
        # (without decoupled_weight_decay torch's __setstate__ would fall back to Adam's L2 penalty)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=bool(capturable), differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        params = param_group["params"]
        params = [params] if isinstance(params, torch.Tensor) else list(params)
        for p in params:
            _check_param(p)
        super().add_param_group({**param_group, "params": params})

    @property
    def grad_norm(self):
        """0-dim device tensor: total gradient norm before clipping of the last step that clipped; None before the first one."""
        return self._scalars[0] if self._norm_valid else None

    @property
    def clip_coef(self):
        """0-dim device tensor: the coefficient the last clipping step multiplied the gradients by."""
        return self._scalars[1] if self._norm_valid else None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._capturable:                              # the mode is the instance's, whatever saved the state: step counts live on
            for group in self.param_groups:               # the device, moved here once (outside any capture)
                group["capturable"] = True
                for p in group["params"]:
                    st = self.state.get(p)
                    if st and not st["step"].is_cuda:
                        st["step"] = st["step"].to(device=p.device, dtype=torch.float32)

    def _collect(self):
        """[(group, [(p, grad, state)])] for the parameters that have a gradient; creates missing state like torch (lazily)."""
        work, device = [], None
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize") or (group.get("capturable") and not self._capturable) or \
                    not group.get("decoupled_weight_decay", True):
                raise ValueError("hirest_amd.optim.AdamW: amsgrad / maximize / capturable / coupled weight decay are not implemented")
            entries = []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise ValueError("hirest_amd.optim.AdamW does not support sparse gradients")
                _check_param(p)
                if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise ValueError("hirest_amd.optim.AdamW: a gradient must match its parameter's dtype, device and shape")
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise ValueError("hirest_amd.optim.AdamW: all parameters of one step must be on one device")
                if not g.is_contiguous():
                    g = g.contiguous()
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if self._capturable else \
                        torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                else:
                    m, v = st["exp_avg"], st["exp_avg_sq"]
                    if self._capturable:
                        if st["step"].device != device or st["step"].dtype != torch.float32:     # a state put in place by hand
                            st["step"] = st["step"].to(device=device, dtype=torch.float32)
                    elif st["step"].is_cuda:               # a state saved by a fused / capturable torch optimizer: counted on the host here
                        st["step"] = st["step"].cpu()
                    if m.dtype != torch.float32 or v.dtype != torch.float32 or m.device != device or v.device != device or \
                            m.shape != p.shape or v.shape != p.shape or not m.is_contiguous() or not v.is_contiguous():
                        raise ValueError("hirest_amd.optim.AdamW: exp_avg / exp_avg_sq must be contiguous fp32 tensors of the parameter's shape and device")
                entries.append((p, g, st))
            if entries:
                work.append((group, entries))
        return work, device

    @staticmethod
    def _table(entries):
        arr = (_lib.OptimItem * len(entries))()
        for it, (p, g, st) in zip(arr, entries):
            it.p, it.g, it.m, it.v, it.n = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
        return arr

    @torch.no_grad()
    def step(self, closure=None, max_grad_norm=_UNSET):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        max_norm = self.max_grad_norm if max_grad_norm is _UNSET else max_grad_norm
        work, device = self._collect()
        if not work:
            return loss
        lib = _lib.load()
        item_size = C.sizeof(_lib.OptimItem)
        with torch.cuda.device(device):
            stream = ops.stream_ptr()
            tables = [(group, entries, self._table(entries)) for group, entries in work]
            scale_ptr = inf_ptr = coef_ptr = None
            if self._capturable:
                scale_ptr = _device_scalar(getattr(self, "grad_scale", None), device, "grad_scale")
                inf_ptr = _device_scalar(getattr(self, "found_inf", None), device, "found_inf")
            if max_norm is not None:
                if self._scalars is None or self._scalars.device != device:
                    self._scalars = torch.zeros(2, dtype=torch.float32, device=device)
                n_chunks = sum(-(-p.numel() // OPTIM_CHUNK) for _, entries, _ in tables for p, _, _ in entries)
                if self._partials is None or self._partials.numel() < n_chunks or self._partials.device != device:
                    self._partials = torch.empty(n_chunks, dtype=torch.float32, device=device)
                done = 0
                for _, entries, arr in tables:                    # the norm is over every group together: one partials array
                    for lo, hi in group_ranges(len(entries)):
                        items, partials = C.addressof(arr) + lo * item_size, self._partials.data_ptr() + 4 * done
                        if self._capturable:
                            _lib.check(lib.hirest_grad_sqnorm_scaled_grouped_f32(items, hi - lo, scale_ptr, partials, stream), "grad_sqnorm")
                        else:
                            _lib.check(lib.hirest_grad_sqnorm_grouped_f32(items, hi - lo, partials, stream), "grad_sqnorm")
                        done += sum(-(-entries[k][0].numel() // OPTIM_CHUNK) for k in range(lo, hi))
                if self._capturable and isinstance(max_norm, torch.Tensor):      # a bound that changes between replays
                    _lib.check(lib.hirest_clip_coef_dev_f32(self._partials.data_ptr(), n_chunks, _device_scalar(max_norm, device, "a tensor max_grad_norm"),
                                                            self._scalars.data_ptr(), stream), "clip_coef")
                else:
                    _lib.check(lib.hirest_clip_coef_f32(self._partials.data_ptr(), n_chunks, float(max_norm), self._scalars.data_ptr(), stream),
                               "clip_coef")
                self._norm_valid = True
                coef_ptr = self._scalars.data_ptr() + 4
            for group, entries, arr in tables:
                if self._capturable:
                    # the step counts and the bias corrections stay on the device: one launch advances the counts of a range of
                    # tensors (unless found_inf), the update's workgroups read them, so tensors whose counts differ share a launch
                    lr, (beta1, beta2) = group["lr"], group["betas"]
                    lr_ptr = _device_scalar(lr, device, "a tensor lr") if isinstance(lr, torch.Tensor) else None
                    steps = (C.c_void_p * len(entries))(*[st["step"].data_ptr() for _, _, st in entries])
                    for lo, hi in group_ranges(len(entries)):
                        items, sp = C.addressof(arr) + lo * item_size, C.addressof(steps) + lo * C.sizeof(C.c_void_p)
                        _lib.check(lib.hirest_optim_step_advance_f32(sp, hi - lo, inf_ptr, stream), "step_advance")
                        _lib.check(lib.hirest_adamw_capturable_grouped_f32(items, sp, hi - lo, coef_ptr, lr_ptr, 0.0 if lr_ptr else lr,
                                                                           scale_ptr, inf_ptr, beta1, beta2, group["eps"],
                                                                           group["weight_decay"], stream), "adamw_capturable")
                    continue
                steps = [st["step"] for _, _, st in entries]
                torch._foreach_add_(steps, 1.0)
                counts = [int(s) for s in steps]
                # one launch sequence per distinct step count (parameters that once had no gradient lag behind the others)
                runs, lo = [], 0
                for k in range(1, len(counts) + 1):
                    if k == len(counts) or counts[k] != counts[lo]:
                        runs.append((lo, k))
                        lo = k
                for rlo, rhi in runs:
                    h = hyperparameters(counts[rlo], group["lr"], group["betas"], group["eps"], group["weight_decay"])
                    for lo, hi in group_ranges(rhi - rlo):
                        _lib.check(lib.hirest_adamw_grouped_f32(C.addressof(arr) + (rlo + lo) * item_size, hi - lo, coef_ptr, h["decay"],
                                                                h["one_minus_beta1"], h["beta2"], h["one_minus_beta2"], h["step_size"],
                                                                h["bc2_sqrt"], h["eps"], stream), "adamw")
            # the kernels write through raw pointers: tell autograd (and the model's caches of fused weights, which key on
            # Parameter._version) that the parameters and moments have changed in place
            torch.autograd.graph.increment_version([t for _, entries in work for p, _, st in entries
                                                    for t in (p, st["exp_avg"], st["exp_avg_sq"])])
        return loss
