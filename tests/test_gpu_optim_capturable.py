"""hirest_amd.optim.AdamW(capturable=True) (csrc/optim_capturable.hip) on the GPU: step counts, learning rates, the loss scale and the
scaler's verdict all live on the device.  The problem and the bars are those of tests/test_gpu_optim.py (fp64 CPU reference, torch's
fp32 clip_grad_norm_ + for-each AdamW as yardstick), cut down to the sizes at which these kernels can go wrong:

    norm      |grad_norm - norm64| <= 1e-5 norm64
    coef      min(1, max_norm / (grad_norm + 1e-6)) in fp32 from the kernel's own grad_norm, within 2 ulp
    update    E_native <= 2 E_torch32 + 2^-23 max|x64|,  E = max|x - x64|, for p, exp_avg, exp_avg_sq of every tensor

The learning rate of step s is the fp32-rounded warm-up value base (s + 1) / STEPS: the capturable runs hold it in a device tensor,
every other run (fp64 included) gets the same rounded value as a float.  Everything else (scaling, skipping, GradScaler, graph replay)
is compared bit for bit against ONE eager capturable run, made once per module and only read afterwards."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 5
FACTORS = [2.0, 0.5, 0.5, 2.0, 0.5]           # max_grad_norm / fp64 norm of each step: no clip (coef == 1) and clip
BASE_LR = (1e-3, 3e-3)                        # group 0 (weight_decay 0.01), group 1 (weight_decay 0)
WD = (0.01, 0.0)
MISALIGNED, NO_GRAD, ZERO_GRAD = "misaligned", "no_grad", "zero_grad"
KEYS = ("p", "exp_avg", "exp_avg_sq")


def lr_of(gi, s):
    """The warm-up learning rate of group gi at step s as the fp32 value a device tensor holds."""
    return float(np.float32(BASE_LR[gi] * (s + 1) / STEPS))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def problem():
    from hirest_amd.optim import OPTIM_CHUNK as c
    shapes = [(n,) for n in (1, 3, 65, 1025, c - 1, c + 1, 3 * c + 5)] + [(37, 53), (1001,), (100,), (300,)]
    kinds = [None] * 8 + [MISALIGNED, NO_GRAD, ZERO_GRAD]
    gen = torch.Generator().manual_seed(4321)
    scales = np.logspace(-4, 2, len(shapes))
    init = [torch.randn(s, generator=gen) for s in shapes]
    grads = []
    for s in range(STEPS):
        row = []
        for shape, kind, scale in zip(shapes, kinds, scales):
            g = torch.randn(shape, generator=gen) * float(scale)
            row.append(None if kind == NO_GRAD else torch.zeros(shape) if kind == ZERO_GRAD else g)
        grads.append(row)
    norm64 = [float(torch.sqrt(sum((g.double() ** 2).sum() for g in row if g is not None))) for row in grads]
    return {"shapes": shapes, "kinds": kinds, "init": init, "grads": grads, "norm64": norm64, "group": [i % 2 for i in range(len(shapes))]}


def _leaf(x, kind, device, dtype):
    """A leaf tensor holding x; the MISALIGNED one is a view that starts one element into a larger buffer."""
    x = x.to(device=device, dtype=dtype)
    if kind == MISALIGNED:
        buf = torch.zeros(x.numel() + 8, device=device, dtype=dtype)
        buf[1:1 + x.numel()] = x.flatten()
        x = buf[1:1 + x.numel()].view(x.shape)
        assert dtype != torch.float32 or x.data_ptr() % 16 == 4
    return x.detach()


class Run:
    """One optimizer on one copy of the problem.  kind: 'f64' (CPU, double), 'torch32' (GPU, torch's for-each AdamW), 'native'
    (hirest_amd, host step counts), 'cap' (hirest_amd, capturable: tensor lr).  gmul multiplies every gradient (a loss scale);
    static keeps one gradient buffer per parameter and copies into it (what a graph replay needs)."""

    def __init__(self, kind, problem, dev, gmul=1.0, static=False, tensor_max_norm=False):
        from hirest_amd import optim
        self.kind, self.pb, self.gmul, self.static = kind, problem, gmul, static
        self.device, self.dtype = (torch.device("cpu"), torch.float64) if kind == "f64" else (dev, torch.float32)
        self.params = [_leaf(x, k, self.device, self.dtype).requires_grad_() for x, k in zip(problem["init"], problem["kinds"])]
        lr0 = [torch.zeros((), device=dev) if kind == "cap" else 0.0 for _ in (0, 1)]
        groups = [{"params": [p for p, g in zip(self.params, problem["group"]) if g == gi], "lr": lr0[gi], "weight_decay": WD[gi]}
                  for gi in (0, 1)]
        self.opt = optim.AdamW(groups, capturable=kind == "cap") if kind in ("native", "cap") else torch.optim.AdamW(groups)
        self.max_norm = torch.zeros((), device=dev) if tensor_max_norm else None
        self.norms, self.coefs = [], []
        if static:
            for p, g, k in zip(self.params, problem["grads"][0], problem["kinds"]):
                p.grad = None if g is None else _leaf(torch.zeros_like(g), k, self.device, self.dtype)

    def set_grads(self, s):
        for p, g, k in zip(self.params, self.pb["grads"][s], self.pb["kinds"]):
            if self.static and g is not None:
                p.grad.copy_(g * self.gmul)
            else:
                p.grad = None if g is None else _leaf(g * self.gmul, k, self.device, self.dtype)

    def set_scalars(self, s):
        """The step's learning rates and clip bound, in place where they are device tensors; returns the bound to pass to step()."""
        for gi, group in enumerate(self.opt.param_groups):
            if isinstance(group["lr"], torch.Tensor):
                group["lr"].fill_(lr_of(gi, s))
            else:
                group["lr"] = lr_of(gi, s)
        max_norm = FACTORS[s] * self.pb["norm64"][s]
        return max_norm if self.max_norm is None else self.max_norm.fill_(max_norm)

    def step(self, s):
        self.set_grads(s)
        max_norm = self.set_scalars(s)
        if self.kind in ("native", "cap"):
            held = [p.grad for p in self.params]
            self.opt.step(max_grad_norm=max_norm)
            self.record()
            for p, g0, g in zip(self.params, held, self.pb["grads"][s]):               # gradients are bit-unchanged, in place
                assert p.grad is g0 and (g is None or torch.equal(p.grad.cpu(), g * self.gmul))
        else:
            self.norms.append(torch.nn.utils.clip_grad_norm_(self.params, max_norm).clone())
            self.opt.step()

    def record(self):
        self.norms.append(self.opt.grad_norm.clone())
        self.coefs.append(self.opt.clip_coef.clone())

    def snapshot(self):
        """p, exp_avg, exp_avg_sq (CPU copies in the run's own dtype) and the step count of every tensor."""
        out = []
        for p in self.params:
            st = self.opt.state.get(p, {})
            out.append({"p": p.detach().cpu().clone(), "exp_avg": st["exp_avg"].cpu().clone() if st else None,
                        "exp_avg_sq": st["exp_avg_sq"].cpu().clone() if st else None, "step": st["step"].cpu().clone() if st else None})
        return out

    def run(self, steps):
        snaps = {}
        for s in steps:
            self.step(s)
            snaps[s] = self.snapshot()
        return snaps


@pytest.fixture(scope="module")
def baseline(problem, dev):
    """The fp64 reference and the torch fp32 yardstick after every step, computed once and only read by the tests."""
    return {k: Run(k, problem, dev).run(range(STEPS)) for k in ("f64", "torch32")}


@pytest.fixture(scope="module")
def eager(problem, dev):
    """The eager capturable run every other test compares against, bit for bit: snapshots, norms and coefficients per step."""
    run = Run("cap", problem, dev)
    snaps = run.run(range(STEPS))
    return {"snaps": snaps, "norms": [n.cpu() for n in run.norms], "coefs": [c.cpu() for c in run.coefs]}


def _check_bar(got, baseline, s, what):
    """E_got <= 2 E_torch32 + 2^-23 max|x64| for every tensor of step s; returns the worst E_got / bar."""
    used = 0.0
    for i, (x, r, y) in enumerate(zip(got, baseline["f64"][s], baseline["torch32"][s])):
        for key in KEYS:
            if r[key] is None:
                assert x[key] is None and key != "p", (what, i, key)
                continue
            e_got, e_y = (x[key].double() - r[key]).abs().max().item(), (y[key].double() - r[key]).abs().max().item()
            bar = 2 * e_y + 2.0 ** -23 * r[key].abs().max().item()
            used = max(used, e_got / bar) if bar > 0 else used
            assert e_got <= bar, (what, f"step {s + 1}", f"tensor {i}", key, e_got, e_y, bar)
    return used


def _same_bits(a, b, what, keys=KEYS + ("step",)):
    for i, (x, y) in enumerate(zip(a, b)):
        for key in keys:
            assert (x[key] is None and y[key] is None) or torch.equal(x[key], y[key]), (what, f"tensor {i}", key)


def test_eager_capturable_vs_fp64(problem, baseline, eager, dev):
    """Measured on an MI355X: norm within 7e-8 of fp64, coefficients exact, at most 0.51 of the update bar; all 31 tensors (p of the 11,
    exp_avg and exp_avg_sq of the 10 with a gradient) bit-identical to the non-capturable native run after 5 steps: device pow against
    host pow made no difference after rounding to fp32 here.  That count is printed, not asserted."""
    used = {s: _check_bar(eager["snaps"][s], baseline, s, "capturable") for s in (0, STEPS - 1)}
    for s in range(STEPS):
        norm64, max_norm = problem["norm64"][s], FACTORS[s] * problem["norm64"][s]
        norm, coef = np.float32(eager["norms"][s].item()), np.float32(eager["coefs"][s].item())
        rel = abs(float(norm) - norm64) / norm64
        expect = np.minimum(np.float32(1), np.float32(max_norm) / (norm + np.float32(1e-6)))
        print(f"step {s + 1}: grad_norm {norm:.8g} (fp64 {norm64:.10g}, rel {rel:.2e}), coef {coef:.8g} (expected {expect:.8g})")
        assert rel <= 1e-5
        assert abs(float(coef) - float(expect)) <= 2 * float(np.spacing(expect))
        assert coef == 1.0 if FACTORS[s] > 1 else coef < 1.0
    # every step count is a 0-dim fp32 tensor holding the number of steps in which the parameter had a gradient
    for s in range(STEPS):
        for x, kind in zip(eager["snaps"][s], problem["kinds"]):
            if kind == NO_GRAD:
                assert x["step"] is None and torch.equal(x["p"], problem["init"][problem["kinds"].index(NO_GRAD)])
            else:
                assert x["step"].dtype == torch.float32 and x["step"].dim() == 0 and x["step"].item() == s + 1
    native = Run("native", problem, dev).run(range(STEPS))[STEPS - 1]
    same = sum(torch.equal(x[k], y[k]) for x, y in zip(eager["snaps"][STEPS - 1], native) for k in KEYS if x[k] is not None)
    total = sum(x[k] is not None for x in native for k in KEYS)
    print(f"worst E / bar: step 1 {used[0]:.3f}, step {STEPS} {used[STEPS - 1]:.3f}; "
          f"bit-identical to the non-capturable native run after {STEPS} steps: {same} of {total} tensors")


def test_step_tensors_live_on_the_device(problem, dev):
    run = Run("cap", problem, dev)
    run.step(0)
    steps = [run.opt.state[p]["step"] for p in run.params if p in run.opt.state]
    assert len(steps) == len(run.params) - 1 and all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 0 for t in steps)
    assert run.opt._step_supports_amp_scaling and all(g["capturable"] for g in run.opt.param_groups)


def test_grad_scale_gives_the_unscaled_bits(problem, eager, dev):
    """grad_scale = 1024 with gradients pre-multiplied by 1024: g * 1024 and (g * 1024) * (1 / 1024) are exact in fp32 (a power of two,
    magnitudes between 1e-11 and 1e3: no overflow, nothing denormal), so all five steps equal the run without scaling, bit for bit."""
    run = Run("cap", problem, dev, gmul=1024.0)
    run.opt.grad_scale = torch.full((), 1024.0, device=dev)
    run.opt.found_inf = torch.zeros((), device=dev)
    snaps = run.run(range(STEPS))                                     # (Run.step asserts that the scaled gradients keep their bits)
    for s in range(STEPS):
        _same_bits(snaps[s], eager["snaps"][s], f"scaled, step {s + 1}")
        assert torch.equal(run.norms[s].cpu(), eager["norms"][s]) and torch.equal(run.coefs[s].cpu(), eager["coefs"][s])


def test_found_inf_leaves_everything_unchanged(problem, eager, dev):
    run = Run("cap", problem, dev)
    run.step(0)
    run.opt.found_inf = torch.ones((), device=dev)
    run.opt.grad_scale = None
    run.step(1)                                                       # (asserts that the gradients keep their bits)
    _same_bits(run.snapshot(), eager["snaps"][0], "found_inf")
    del run.opt.found_inf, run.opt.grad_scale
    run.step(1)                                                       # and the run goes on as if the skipped step had not been
    _same_bits(run.snapshot(), eager["snaps"][1], "after found_inf")


def _scaler_problem(dev):
    from hirest_amd.optim import OPTIM_CHUNK as c
    gen = torch.Generator().manual_seed(99)
    shapes = [(5,), (c + 3,), (37, 53)]
    init = [torch.randn(s, generator=gen) for s in shapes]
    coef = [torch.randn(s, generator=gen).to(dev) for s in shapes]
    max_norm = 0.5 * float(torch.sqrt(sum((x.double() ** 2).sum() for x in coef)))          # clipping is active
    return init, coef, max_norm


def _state(opt, params):
    return [{"p": p.detach().cpu().clone(), **{k: opt.state[p][k].cpu().clone() for k in ("exp_avg", "exp_avg_sq", "step")}} for p in params]


def test_grad_scaler_round_trip(dev):
    """loss = sum(p_i c_i): each gradient is exactly scale * c_i.  Iteration 2 has an inf in c: the scaler's found_inf reaches the
    kernels on the device, nothing moves, the scale halves; the four iterations end on the bits of three unscaled ones."""
    from hirest_amd import optim
    init, coef, max_norm = _scaler_problem(dev)
    bad = [x.clone() for x in coef]
    bad[1][7] = float("inf")
    params = [x.to(dev).clone().requires_grad_() for x in init]
    opt = optim.AdamW(params, lr=1e-2, capturable=True, max_grad_norm=max_norm)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10, growth_interval=1000)
    after = {}
    for it in (1, 2, 3, 4):
        opt.zero_grad()
        loss = sum((p * c).sum() for p, c in zip(params, bad if it == 2 else coef))
        scaler.scale(loss).backward()
        if it != 2:
            assert all(torch.equal(p.grad, scaler.get_scale() * c) for p, c in zip(params, coef))
        scaler.step(opt)
        scaler.update()
        after[it] = _state(opt, params)
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    _same_bits(after[2], after[1], "skipped iteration")
    assert after[1][0]["step"].item() == 1 and after[4][0]["step"].item() == 3 and scaler.get_scale() == 2.0 ** 9
    plain_params = [x.to(dev).clone().requires_grad_() for x in init]
    plain = optim.AdamW(plain_params, lr=1e-2, capturable=True, max_grad_norm=max_norm)
    for _ in range(3):
        for p, c in zip(plain_params, coef):
            p.grad = c.clone()
        plain.step()
    _same_bits(after[4], _state(plain, plain_params), "scaler against plain")
    assert not any(torch.equal(x["p"], y["p"]) for x, y in zip(after[4], after[1]))          # (the finite iterations did move them)


def test_graph_replay_equals_the_eager_run(problem, eager, dev):
    """Eager step 1 creates state and workspaces; one opt.step() is then captured (after a side-stream warm-up, torch's rule) and
    replayed for steps 2 .. 5 with new gradients in the static buffers, new learning rates and a new clip bound in their tensors.  A
    host read inside step() would make the capture raise: this also pins 'no synchronisation'."""
    run = Run("cap", problem, dev, static=True, tensor_max_norm=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run.step(0)                                                   # the warm-up IS step 1
    torch.cuda.current_stream().wait_stream(side)
    _same_bits(run.snapshot(), eager["snaps"][0], "eager step with static buffers")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.opt.step(max_grad_norm=run.max_norm)
    _same_bits(run.snapshot(), eager["snaps"][0], "capture runs nothing")
    for s in range(1, STEPS):
        run.set_grads(s)
        run.set_scalars(s)
        graph.replay()
        _same_bits(run.snapshot(), eager["snaps"][s], f"replay of step {s + 1}")
        assert torch.equal(run.opt.grad_norm.cpu(), eager["norms"][s]) and torch.equal(run.opt.clip_coef.cpu(), eager["coefs"][s])


def test_state_dicts_interchange_with_torch_capturable_and_native(problem, baseline, eager, dev):
    """Two capturable steps, the state dict into torch.optim.AdamW(capturable=True) and back, a third step on each side: all within the
    bar.  A state saved by the non-capturable native optimizer loads into a capturable one: the step count moves to the device."""
    a = Run("cap", problem, dev)
    a.run(range(2))
    sd = a.opt.state_dict()
    assert all(g["capturable"] for g in sd["param_groups"])
    b = Run("torch32", problem, dev)
    c = Run("cap", problem, dev)
    n = Run("native", problem, dev)
    n.run(range(2))
    d = Run("cap", problem, dev)
    for dst, src, state in ((b, a, sd), (d, n, n.opt.state_dict())):
        with torch.no_grad():
            for q, p in zip(dst.params, src.params):
                q.copy_(p)
        dst.opt.load_state_dict(state)
    st = b.opt.state[b.params[0]]["step"]
    assert b.opt.param_groups[0]["capturable"] and st.is_cuda and st.item() == 2
    with torch.no_grad():
        for q, p in zip(c.params, b.params):
            q.copy_(p)
    c.opt.load_state_dict(copy.deepcopy(b.opt.state_dict()))          # and back (a copy, as from a checkpoint: b steps on below)
    st = d.opt.state[d.params[0]]["step"]
    assert st.is_cuda and st.dtype == torch.float32 and st.item() == 2 and all(g["capturable"] for g in d.opt.param_groups)
    i = problem["kinds"].index(NO_GRAD)
    for run, what in ((b, "capturable -> torch capturable"), (c, "torch capturable -> capturable"), (d, "native -> capturable")):
        assert run.params[i] not in run.opt.state
        if run.kind == "torch32":                                     # torch keeps lr as given: a tensor from our state dict
            for gi, group in enumerate(run.opt.param_groups):
                group["lr"] = lr_of(gi, 2)
            run.set_grads(2)
            torch.nn.utils.clip_grad_norm_(run.params, FACTORS[2] * problem["norm64"][2])
            run.opt.step()
        else:
            run.step(2)
        used = _check_bar(run.snapshot(), baseline, 2, what)
        assert run.opt.state[run.params[0]]["step"].item() == 3
        print(f"{what}: worst E / bar after step 3: {used:.3f}")


def test_tensors_whose_step_counts_differ_share_a_launch(dev):
    """A parameter that had no gradient in the first step lags one step behind: every workgroup reads its own tensor's count."""
    from hirest_amd import optim
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(n, generator=gen) for n in (70, 9000)]
    grads = [[torch.randn(n, generator=gen) for n in (70, 9000)] for _ in range(3)]
    runs = {}
    for kind in ("f64", "torch32", "cap"):
        dt, device = (torch.float64, "cpu") if kind == "f64" else (torch.float32, dev)
        ps = [x.to(device=device, dtype=dt).clone().requires_grad_() for x in init]
        opt = optim.AdamW(ps, lr=1e-2, capturable=True) if kind == "cap" else torch.optim.AdamW(ps, lr=1e-2)
        for s in range(3):
            for j, p in enumerate(ps):
                p.grad = None if (s == 0 and j == 1) else grads[s][j].to(device=device, dtype=dt)
            opt.step()
        runs[kind] = [t.detach().double().cpu() for p in ps for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
        if kind == "cap":
            assert [opt.state[p]["step"].item() for p in ps] == [3, 2]
    for x, r, y in zip(runs["cap"], runs["f64"], runs["torch32"]):
        assert (x - r).abs().max().item() <= 2 * (y - r).abs().max().item() + 2.0 ** -23 * r.abs().max().item()
