"""hirest_amd.optim.AdamW (csrc/optim.hip) on the GPU against the same loop in fp64 on the CPU — torch.nn.utils.clip_grad_norm_ +
torch.optim.AdamW on double copies — with torch's own fp32 clip_grad_norm_ + AdamW (for-each) on the same inputs as the yardstick:

    norm      |grad_norm - norm64| <= 1e-5 norm64     (a fixed-order blocked fp32 sum of n squares: ~(log2 n + 2) 2^-24 relative)
    coef      min(1, max_norm / (grad_norm + 1e-6)) in fp32 from the kernel's own grad_norm, within 2 ulp; exactly 1 when not clipping
    update    E_native <= 2 E_torch32 + 2^-23 max|x64|,  E = max|x - x64|, for p, exp_avg, exp_avg_sq of every tensor: the factor 2
              allows for a different order of roundings (contraction, divide vs reciprocal), each worth one rounding

Measured on an MI355X: norm within 3e-8 of fp64; no tensor uses more than 0.64 of the update bar; the plain ratio E_native / E_torch32
reaches 10.2 on exp_avg_sq of the one-element tensor (3.3 - 4.0 on the model's bias tensors), where torch's v * beta2 + (1 - beta2) g g lands within
a fraction of an ulp of fp64 and the contracted fma one ulp away: one rounding, covered by the additive term.

Shapes: every size around the 4-element vector and the chunk, a 2-D tensor, a parameter and gradient that start one element into a
larger buffer, a parameter without gradient, an all-zero gradient; gradient scales 1e-4 .. 1e2; two param groups."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 5
FACTORS = [2.0, 0.5, 0.5, 2.0, 0.5]           # max_grad_norm / fp64 norm of each step: no clip (coef == 1) and clip
BASE_LR = (1e-3, 3e-3)                        # group 0 (weight_decay 0.01), group 1 (weight_decay 0); warm-up: lr_s = base (s + 1) / STEPS
WD = (0.01, 0.0)
MISALIGNED, NO_GRAD, ZERO_GRAD = "misaligned", "no_grad", "zero_grad"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def problem():
    from hirest_amd.optim import OPTIM_CHUNK as c
    shapes = [(n,) for n in (1, 3, 63, 64, 65, 255, 257, 1023, 1025, c - 1, c, c + 1, 3 * c + 5)] + [(37, 53), (1001,), (100,), (300,)]
    kinds = [None] * 14 + [MISALIGNED, NO_GRAD, ZERO_GRAD]
    gen = torch.Generator().manual_seed(1234)
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
    """One optimizer on one copy of the problem.  kind: 'f64' (CPU, double), 'torch32' (GPU, torch's for-each AdamW), 'native'."""

    def __init__(self, kind, problem, dev):
        from hirest_amd import optim
        self.kind, self.pb = kind, problem
        self.device, self.dtype = (torch.device("cpu"), torch.float64) if kind == "f64" else (dev, torch.float32)
        self.params = [_leaf(x, k, self.device, self.dtype).requires_grad_() for x, k in zip(problem["init"], problem["kinds"])]
        groups = [{"params": [p for p, g in zip(self.params, problem["group"]) if g == gi], "lr": BASE_LR[gi], "weight_decay": WD[gi]}
                  for gi in (0, 1)]
        self.opt = optim.AdamW(groups) if kind == "native" else torch.optim.AdamW(groups)
        self.norms, self.coefs = [], []

    def set_grads(self, s):
        for p, g, k in zip(self.params, self.pb["grads"][s], self.pb["kinds"]):
            p.grad = None if g is None else _leaf(g, k, self.device, self.dtype)

    def step(self, s, set_grads=True):
        if set_grads:
            self.set_grads(s)
        for gi, group in enumerate(self.opt.param_groups):
            group["lr"] = BASE_LR[gi] * (s + 1) / STEPS
        max_norm = FACTORS[s] * self.pb["norm64"][s]
        if self.kind == "native":
            self.opt.step(max_grad_norm=max_norm)
            self.norms.append(self.opt.grad_norm.clone())
            self.coefs.append(self.opt.clip_coef.clone())
        else:
            self.norms.append(torch.nn.utils.clip_grad_norm_(self.params, max_norm).clone())
            self.opt.step()

    def snapshot(self):
        out = []
        for p in self.params:
            st = self.opt.state.get(p, {})
            out.append({"p": p.detach().double().cpu().clone(),
                        "exp_avg": st["exp_avg"].double().cpu().clone() if st else None,
                        "exp_avg_sq": st["exp_avg_sq"].double().cpu().clone() if st else None})
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


def _check_bar(got, baseline, s, what):
    """E_got <= 2 E_torch32 + 2^-23 max|x64| for every tensor of step s; returns 'worst E_got / E_torch32 (where), worst E_got / bar'.
    (The plain ratio is large where the yardstick happens to land within a rounding of fp64 on a tensor of a few elements: the
    additive term of the bar is there for that.)"""
    worst, where, used = 0.0, None, 0.0
    for i, (x, r, y) in enumerate(zip(got, baseline["f64"][s], baseline["torch32"][s])):
        for key in ("p", "exp_avg", "exp_avg_sq"):
            if r[key] is None:
                assert x[key] is None and key != "p", (what, i, key)
                continue
            e_got, e_y = (x[key] - r[key]).abs().max().item(), (y[key] - r[key]).abs().max().item()
            bar = 2 * e_y + 2.0 ** -23 * r[key].abs().max().item()
            if e_y > 0 and e_got / e_y > worst:
                worst, where = e_got / e_y, f"{key} of tensor {i}, {r[key].numel()} elements"
            used = max(used, e_got / bar) if bar > 0 else used
            assert e_got <= bar, (what, f"step {s + 1}", f"tensor {i}", key, e_got, e_y, bar)
    return f"{worst:.3f} ({where}); worst E / bar {used:.3f}"


def test_norm_coefficient_and_update_vs_fp64(problem, baseline, dev):
    run = Run("native", problem, dev)
    worst = {}
    for s in range(STEPS):
        run.set_grads(s)
        held = [p.grad for p in run.params]
        run.step(s, set_grads=False)
        for p, g0, g in zip(run.params, held, problem["grads"][s]):                        # gradients are bit-unchanged, in place
            assert p.grad is g0 and (g is None or torch.equal(p.grad.cpu(), g))
        if s in (0, STEPS - 1):
            worst[s] = _check_bar(run.snapshot(), baseline, s, "native")
    for s in range(STEPS):
        norm64, max_norm = problem["norm64"][s], FACTORS[s] * problem["norm64"][s]
        norm = np.float32(run.norms[s].item())
        coef = np.float32(run.coefs[s].item())
        rel = abs(float(norm) - norm64) / norm64
        expect = np.minimum(np.float32(1), np.float32(max_norm) / (norm + np.float32(1e-6)))
        print(f"step {s + 1}: grad_norm {norm:.8g} (fp64 {norm64:.10g}, rel {rel:.2e}; torch fp32 rel "
              f"{abs(baseline_norm(problem, dev, s) - norm64) / norm64:.2e}), coef {coef:.8g} (expected {expect:.8g})")
        assert rel <= 1e-5
        assert abs(float(coef) - float(expect)) <= 2 * float(np.spacing(expect))
        if FACTORS[s] > 1:
            assert coef == 1.0
        else:
            assert coef < 1.0
    print(f"worst E_native / E_torch32: step 1 {worst[0]}, step {STEPS} {worst[STEPS - 1]}")


def baseline_norm(problem, dev, s):
    """torch's fp32 clip_grad_norm_ total norm of step s (printed next to the native one)."""
    gs = [g.to(dev) for g in problem["grads"][s] if g is not None]
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in gs])).item()


def test_parameter_without_gradient_is_skipped(problem, dev):
    run = Run("native", problem, dev)
    i = problem["kinds"].index(NO_GRAD)
    v0 = [p._version for p in run.params]
    run.run(range(2))
    assert torch.equal(run.params[i].detach().cpu(), problem["init"][i])      # bit-unchanged (no weight decay either)
    assert run.params[i] not in run.opt.state and len(run.opt.state) == len(run.params) - 1
    # autograd's in-place bookkeeping follows the raw-pointer writes: one version per step for the updated tensors, none for the skipped
    assert [p._version - v for p, v in zip(run.params, v0)] == [0 if j == i else 2 for j in range(len(run.params))]
    # (it cannot enter the norm: the norm test's fp64 reference is taken over the other tensors)
    for p in run.params:
        if p in run.opt.state:
            st = run.opt.state[p]
            assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["step"].dim() == 0 and st["step"].item() == 2
            assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape


def test_two_fresh_runs_give_the_same_bits(problem, dev):
    a, b = Run("native", problem, dev), Run("native", problem, dev)
    sa, sb = a.run(range(STEPS)), b.run(range(STEPS))
    for x, y in zip(sa[STEPS - 1], sb[STEPS - 1]):
        for key in x:
            assert (x[key] is None and y[key] is None) or torch.equal(x[key], y[key])
    assert all(torch.equal(m, n) for m, n in zip(a.norms, b.norms))


def test_no_clipping_launches_no_norm_and_matches_torch(problem, dev):
    """max_grad_norm=None: coef is 1, grad_norm stays unset; one step equals the bar against plain AdamW in fp64."""
    from hirest_amd import optim
    ps = [_leaf(x, k, dev, torch.float32).requires_grad_() for x, k in zip(problem["init"], problem["kinds"])]
    p64 = [x.double().clone().requires_grad_() for x in problem["init"]]
    p32 = [x.to(dev).clone().requires_grad_() for x in problem["init"]]
    opts = [optim.AdamW(ps, lr=1e-3), torch.optim.AdamW(p64, lr=1e-3), torch.optim.AdamW(p32, lr=1e-3)]
    for plist, dt in ((ps, torch.float32), (p64, torch.float64), (p32, torch.float32)):
        for p, g, k in zip(plist, problem["grads"][0], problem["kinds"]):
            p.grad = None if g is None else _leaf(g, k, p.device, dt)
    for o in opts:
        o.step()
    assert opts[0].grad_norm is None
    for a, r, y in zip(ps, p64, p32):
        e, ey = (a.detach().double().cpu() - r.detach()).abs().max().item(), (y.detach().double().cpu() - r.detach()).abs().max().item()
        assert e <= 2 * ey + 2.0 ** -23 * r.abs().max().item()


def test_refusals_on_the_device(dev):
    from hirest_amd import optim
    with pytest.raises(ValueError):
        optim.AdamW([torch.zeros(8, 8, device=dev).t().requires_grad_()])                  # non-contiguous parameter
    with pytest.raises(ValueError):
        optim.AdamW([torch.zeros(8, device=dev, dtype=torch.bfloat16).requires_grad_()])
    p = torch.zeros(8, 4, device=dev).requires_grad_()
    opt = optim.AdamW([p], lr=0.1, weight_decay=0.0)
    p.grad = torch.sparse_coo_tensor(torch.tensor([[0], [0]]), torch.tensor([1.0]), (8, 4)).to(dev)
    with pytest.raises(ValueError):
        opt.step()
    p.grad = torch.ones(4, 8, device=dev).t()                                               # non-contiguous gradient: made contiguous
    opt.step()
    torch.testing.assert_close(p.detach(), torch.full((8, 4), -0.1, device=dev), rtol=1e-6, atol=0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5)                            # schedulers, zero_grad, add_param_group
    opt.step(); sched.step()
    assert opt.param_groups[0]["lr"] == 0.05
    opt.zero_grad()
    assert p.grad is None
    opt.add_param_group({"params": [torch.zeros(3, device=dev).requires_grad_()], "lr": 0.2})
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["weight_decay"] == 0.0
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.zeros(3).requires_grad_()]})


def test_state_dict_round_trip_with_torch_adamw(problem, baseline, dev):
    """Two steps with one optimizer, its state dict into the other, a third step there: both directions continue within the bar."""
    for first, second in (("native", "torch32"), ("torch32", "native")):
        a = Run(first, problem, dev)
        a.run(range(2))
        b = Run(second, problem, dev)
        with torch.no_grad():
            for q, p in zip(b.params, a.params):
                q.copy_(p)
        b.opt.load_state_dict(a.opt.state_dict())
        group = b.opt.param_groups[0]
        assert group["weight_decay"] == WD[0] and group.get("decoupled_weight_decay", True) and not group["amsgrad"]
        i = problem["kinds"].index(NO_GRAD)
        assert b.params[i] not in b.opt.state
        st = b.opt.state[b.params[0]]
        assert st["step"].item() == 2 and st["step"].device.type == "cpu" and st["exp_avg"].device == b.params[0].device
        b.step(2)
        worst = _check_bar(b.snapshot(), baseline, 2, f"{first} -> {second}")
        assert b.opt.state[b.params[0]]["step"].item() == 3
        print(f"{first} -> {second}: worst E / E_torch32 after step 3: {worst}")


# ---- model level: the 63 M-parameter joint model, one moment-retrieval batch (the _setup recipe of tests/test_gpu_train.py, case a)
def _model_and_batch(golden_dir, dev):
    import hirest_amd
    from hirest_amd import synth
    from hirest_amd.synth import joint_inputs, train_targets, TRAIN_CASES
    B, T = TRAIN_CASES["a"]
    shapes = {k: tuple(v) for k, v in json.load(open(os.path.join(golden_dir, "joint_schema.json"))).items()}
    sd = synth.joint_state_dict(shapes, 31)
    models = []
    for _ in range(2):
        model = hirest_amd.MomentModel(n_frames=-1, asr_dim=384, args=None, clip_model=None)
        model.load_state_dict(sd, strict=False)
        models.append(model.to(dev).eval())
    vis, asr, text, vis_mask, moment_mask, bounds = joint_inputs("train.a", B, T, 53)
    st, et, seg, prev = train_targets("train.a", B, T, 53, bounds)
    batch = {"tasks": ["moment_retrieval"], "vis_feats": vis, "vis_mask": vis_mask, "moment_mask": moment_mask, "asr_feats": asr,
             "text_feat": text, "moment_retrieval_start_target": st, "moment_retrieval_end_target": et}
    return models, batch, sd


def test_model_level_step_vs_fp64_and_training_loop(dev, golden_dir):
    from hirest_amd import optim
    (A, B), batch, sd = _model_and_batch(golden_dir, dev)

    def backward(model):
        for p in model.parameters():
            p.grad = None
        loss = model.train_step(batch)["loss"]
        loss.backward()
        return loss.item()
    first = backward(A)
    names = [n for n, p in A.named_parameters() if p.grad is not None]
    gA = {n: dict(A.named_parameters())[n].grad.clone() for n in names}
    assert abs(backward(B) - first) <= 1e-6 * abs(first)
    nB = dict(B.named_parameters())
    assert all(torch.equal(nB[n].grad, gA[n]) for n in names)                    # identical gradients at step 1
    norm64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in gA.values())))
    start = {n: p.detach().clone() for n, p in A.named_parameters()}
    for c in (5.0, 0.5 * norm64):
        with torch.no_grad():
            for model in (A, B):
                for n, p in model.named_parameters():
                    p.copy_(start[n])
        nA, nB = dict(A.named_parameters()), dict(B.named_parameters())
        for n in names:
            nA[n].grad = gA[n].clone()
        backward(B)
        # fp64: the update from A's gradients, on double copies
        p64 = [start[n].double().requires_grad_() for n in names]
        for p, n in zip(p64, names):
            p.grad = gA[n].double()
        o64 = torch.optim.AdamW(p64, lr=2e-4)
        torch.nn.utils.clip_grad_norm_(p64, c)
        o64.step()
        oA = torch.optim.AdamW([p for p in A.parameters() if p.requires_grad], lr=2e-4)
        totalA = torch.nn.utils.clip_grad_norm_(A.parameters(), c)
        oA.step()
        oB = optim.AdamW([p for p in B.parameters() if p.requires_grad], lr=2e-4, max_grad_norm=c)
        oB.step()
        relA = abs(oB.grad_norm.item() - totalA.item()) / totalA.item()
        assert relA <= 1e-5 and abs(oB.grad_norm.item() - norm64) <= 1e-5 * norm64, (oB.grad_norm.item(), totalA.item(), norm64)
        assert (oB.clip_coef.item() < 1.0) == (c < norm64)
        worst, where, used = 0.0, None, 0.0
        for p, n in zip(p64, names):
            for key in ("p", "exp_avg", "exp_avg_sq"):
                r = p.detach() if key == "p" else o64.state[p][key]
                a = nA[n].detach() if key == "p" else oA.state[nA[n]][key]
                b = nB[n].detach() if key == "p" else oB.state[nB[n]][key]
                e_b, e_a = (b.double() - r).abs().max().item(), (a.double() - r).abs().max().item()
                bar = 2 * e_a + 2.0 ** -23 * r.abs().max().item()
                if e_a > 0 and e_b / e_a > worst:
                    worst, where = e_b / e_a, f"{key} of {n}"
                used = max(used, e_b / bar) if bar > 0 else used
                assert e_b <= bar, (c, n, key, e_b, e_a, bar)
        assert set(oB.state) == {nB[n] for n in names}                             # no state for tensors the backward does not reach
        print(f"c = {c:.4g}: grad_norm {oB.grad_norm.item():.8g} (torch {totalA.item():.8g}, fp64 {norm64:.10g}), "
              f"worst E_native / E_torch32 over {len(names)} tensors: {worst:.3f} ({where}); worst E / bar {used:.3f}")
    # B goes on for three more steps in train mode (dropout on), as test_training_loop_contract_and_dropout does with torch's optimizer
    B.train()
    for _ in range(3):
        oB.zero_grad(set_to_none=True)
        loss = B.train_step(batch)["loss"]
        assert torch.isfinite(loss)
        loss.backward()
        oB.step()
    B.eval()
    last = B.train_step(batch)["loss"].item()
    print(f"eval-mode loss {first:.5f} -> {last:.5f} after 4 native AdamW steps")
    assert last < first
    # the model's caches of fused weights followed the raw-pointer updates: a model that loads B's weights afresh computes the same loss
    A.load_state_dict(B.state_dict(), strict=False)
    assert abs(A.eval().train_step(batch)["loss"].item() - last) <= 1e-6 * abs(last)
