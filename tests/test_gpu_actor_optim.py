"""GPU checks of gymnet_vecenv_actor_apply_gradient (gym.net_amd/csrc/actor_optim.hip) through Actor.ApplyGradient.  The reference is
clip_grad_norm_ + torch.optim.{SGD, Adadelta, Adam} on a float64 CPU copy, the yardstick the same run in float32 on the CPU; after three
updates the weights and every used state row meet, per tensor, the gradient tests' rule max|got - f64| <= 4 max|f32 - f64| + 2^-22 max|f64|
(docs/ledger.md §45, §47).  The hyperparameters reach the reference as the float32 values the C call takes.  Every test fails without the
feature."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RULES = {"sgd": 0, "adadelta": 1, "adam": 2}
COUNTS = (1, 63, 65, 1024, 1025, 8191, 8192)           # one element, a partial wave, a wave plus one, one element a thread, thread 0 with two, the last thread short by one, the maximum
f32 = lambda v: float(np.float32(v))                   # noqa: E731
HP = {"sgd": dict(lr=f32(0.05), momentum=f32(0.8)), "adadelta": dict(lr=f32(0.7), rho=f32(0.85), eps=f32(1e-5)),
      "adam": dict(lr=f32(3e-3), betas=(f32(0.8), f32(0.99)), eps=f32(1e-6))}
DECAY = f32(1e-2)
STATE_KEYS = {"sgd": ("momentum_buffer",), "adadelta": ("square_avg", "acc_delta"), "adam": ("exp_avg", "exp_avg_sq")}
SEED = 0                                               # count = 1: |g| of the three draws is 0.29, 2.18, 0.57 (checked on the CPU): both sides of the clip at 0.5
CASES = [(r, c, mn, s) for r in RULES for c in COUNTS for mn in (0.0, 0.5) for s in ((1, 1000) if r == "adam" else (1,))]


def draws(count, updates=3):
    import torch
    g = torch.Generator().manual_seed(SEED)
    return 0.5 * torch.randn(count, generator=g), [torch.randn(count, generator=g) for _ in range(updates)]


def reference(rule, w0, grads, dtype, max_norm, step):
    """(weights, used state rows, norms before clipping) after one update per gradient, the first of them numbered `step`"""
    import torch
    w = torch.nn.Parameter(w0.to(dtype).clone())
    opt = {"sgd": torch.optim.SGD, "adadelta": torch.optim.Adadelta, "adam": torch.optim.Adam}[rule]([w], weight_decay=DECAY, **HP[rule])
    if rule == "adam":
        opt.state[w] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.zeros_like(w), "exp_avg_sq": torch.zeros_like(w)}
    norms = []
    for g in grads:
        w.grad = g.to(dtype).clone()
        norms.append(float(torch.linalg.vector_norm(w.grad.double())))
        if max_norm:
            torch.nn.utils.clip_grad_norm_([w], max_norm)
        opt.step()
    return w.detach(), [opt.state[w][k] for k in STATE_KEYS[rule]], norms


def held(name, got, a64, a32):
    err, err32, top = float((got.double() - a64).abs().max()), float((a32.double() - a64).abs().max()), float(a64.abs().max())
    bound = 4 * err32 + 2.0 ** -22 * top
    print(f"  {name}: kernel {err:.3e} torch32 {err32:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
    assert err <= bound, (name, err, err32, bound)


@pytest.fixture(scope="module")
def actor(gpu_pkg):
    import torch
    with gpu_pkg.VectorEnv("CartPole-v1", 256, seed=11, auto_reset=True) as e:
        e.ResetDevice()
        torch.manual_seed(167)
        net = torch.nn.Sequential(torch.nn.Linear(16, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, 2))
        yield e, e.Actor(net, history=4), net


def apply(actor, rule, w, g, state, step, max_norm, norm):
    hp = dict(HP[rule])
    return actor.ApplyGradient(w, g, state, rule=rule, step=step, lr=hp.pop("lr"), weight_decay=DECAY, max_grad_norm=max_norm, norm=norm, **hp)


@pytest.mark.parametrize("rule,count,max_norm,step", CASES)
def test_three_updates_against_float64(actor, rule, count, max_norm, step):
    import torch
    e, ac, _ = actor
    w0, grads = draws(count)
    w, state, norm, norms = w0.cuda(), torch.zeros(2, count, device="cuda"), torch.empty(1, device="cuda"), []
    torch.cuda.synchronize()                            # torch's stream is not the handle's
    for k, g in enumerate(grads):
        apply(ac, rule, w, g.cuda(), state, step + k, max_norm, norm)
        e.Sync()
        norms.append(float(norm.cpu()))
    w64, s64, n64 = reference(rule, w0, grads, torch.float64, max_norm, step)
    w32, s32, _ = reference(rule, w0, grads, torch.float32, max_norm, step)
    print(f"{rule} count={count} max_norm={max_norm} step={step}")
    held("weights", w.cpu(), w64, w32)
    for row, (a64, a32) in enumerate(zip(s64, s32)):
        held(STATE_KEYS[rule][row], state[row].cpu(), a64, a32)
    assert all(abs(a - b) <= 2.0 ** -22 * max(1.0, b) for a, b in zip(norms, n64)), (norms, n64)
    if max_norm and count == 1:                         # both sides of the clip within this one case: coef == 1 and coef < 1
        assert min(norms) + 1e-6 < max_norm < max(norms), norms
    if max_norm and count > 1:
        assert min(norms) > max_norm, norms


@pytest.mark.parametrize("rule", RULES)
def test_the_same_bits_twice_and_nothing_else_touched(actor, rule):
    import torch
    e, ac, _ = actor
    count, pad, canary = 1025, 16, -7.25
    w0, (g0,) = draws(count, updates=1)
    out = []
    for max_norm, with_norm in ((0.5, True), (0.5, True), (0.0, True), (0.0, False)):
        w, state = torch.full((1 + count + pad,), canary, device="cuda")[1:], torch.full((1 + 2 * count + pad,), canary, device="cuda")[1:]     # (4-byte aligned, no more)
        w[:count], state[:2 * count], g, norm = w0.cuda(), 0.0, g0.cuda(), torch.full((1,), canary, device="cuda")
        torch.cuda.synchronize()
        apply(ac, rule, w[:count], g, state[:2 * count].view(2, count), 7, max_norm, norm if with_norm else None)
        e.Sync()
        assert bool((w[count:] == canary).all()) and bool((state[2 * count:] == canary).all()) and torch.equal(g.cpu(), g0)
        assert with_norm or float(norm.cpu()) == canary
        out.append([t.cpu().numpy().view(np.uint32).copy() for t in (w, state, norm)])
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1])) and not np.array_equal(out[0][0][:count], w0.numpy().view(np.uint32))
    assert np.array_equal(out[2][0], out[3][0]) and np.array_equal(out[2][1], out[3][1])


def test_policy_gradient_then_the_step_on_a_sequential_with_no_synchronise(actor):
    """a fused rollout's rows, PolicyGradient on the module, ApplyGradient(grad=None) straight behind it: the module's parameters meet the
    float64 step applied to the float64 autograd gradient.  SGD with momentum and a clip: a rule that is linear in the gradient carries
    the gradient kernel's own error, which test_gpu_actor_grad.py bounds, into the weights unamplified."""
    import copy
    import torch
    e, ac, net = actor
    n, T, m, rule = 256, 4, 64, "sgd"
    ac.SetExploration("softmax", 1.0)
    h0 = ac.HistoryDevice()
    obs, done = torch.empty((T, 4, n), dtype=torch.float32, device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
    act = torch.empty((T, n), dtype=torch.int32, device="cuda")
    e.RolloutFusedDevice(None, T, actions="actor", epsilon=1.0, action_seed=5, rec_obs=obs, rec_done=done, rec_actions=act)
    e.Sync()
    idx = torch.arange(0, T * n, T * n // m, device="cuda")
    x, a, coef = e.RolloutInputsDevice(obs, done, h0, history=4, rows=idx), act.view(-1)[idx].contiguous(), torch.randn(m, generator=torch.Generator().manual_seed(1)).cuda()
    dev, state = copy.deepcopy(net).cuda(), torch.zeros(2, ac.Count, device="cuda")
    torch.cuda.synchronize()                            # torch's stream is not the handle's; from here on the handle's alone
    ac.PolicyGradient(dev, x, a, coef)
    assert apply(ac, rule, dev, None, state, 1, 0.5, None) is dev
    e.Sync()
    want = []
    for dtype in (torch.float64, torch.float32):
        ref = copy.deepcopy(net).to(dtype)
        logp = torch.log_softmax(ref(x.cpu().to(dtype)), 1).gather(1, a.cpu().long()[:, None])[:, 0]
        (-(coef.cpu().to(dtype) * logp).mean()).backward()
        flat, grad = (torch.cat([t.detach().reshape(-1) for t in ts]) for ts in (list(ref.parameters()), [p.grad for p in ref.parameters()]))
        want.append(reference(rule, flat, [grad], dtype, 0.5, 1))
    at = 0
    for name, p in dev.named_parameters():
        held(name, p.detach().cpu().reshape(-1), want[0][0][at:at + p.numel()], want[1][0][at:at + p.numel()])
        at += p.numel()


REFUSED = {"weights": dict(w=None), "grad": dict(g=None), "count 0": dict(count=0), "count 8193": dict(count=8193), "rule": dict(rule=3), "state": dict(s=None),
           "sgd state": dict(rule=0, p0=0.5, s=None), "grad in weights": dict(g="w+8"), "state in weights": dict(s="w+32"), "norm in state": dict(n="s+100"),
           "grad in state": dict(g="s+64"), "norm in grad": dict(n="g+0"), "step": dict(step=0), "lr": dict(lr=-1.0), "lr inf": dict(lr=math.inf), "eps": dict(eps=math.nan),
           "decay": dict(wd=-1e-3), "adadelta eps": dict(rule=1, eps=0.0), "p0": dict(p0=1.0), "p0 negative": dict(p0=-0.1), "p1": dict(p1=1.0),
           "max norm": dict(mn=-0.5), "max norm nan": dict(mn=math.nan)}


@pytest.mark.parametrize("what", REFUSED)
def test_refusals_touch_nothing(gpu_pkg, actor, what):
    import ctypes as C
    import torch
    e, ac, _ = actor
    capi, count = gpu_pkg._capi, 16
    t = {k: torch.full((2 * 8193 + 64,), -7.25, device="cuda") for k in "wgsn"}          # (in bounds for every case, were one accepted)
    c = dict(rule=2, w="w+0", g="g+0", s="s+0", n="n+0", count=count, step=1, lr=1e-3, p0=0.9, p1=0.999, eps=1e-8, wd=0.0, mn=0.5)
    c.update(REFUSED[what])
    p = {k: None if c[k] is None else C.c_void_p(t[c[k][0]].data_ptr() + int(c[k][1:])) for k in "wgsn"}
    st = capi.load_library().gymnet_vecenv_actor_apply_gradient(e._h, c["rule"], p["w"], c["count"], p["g"], p["s"], c["step"], c["lr"], c["p0"], c["p1"], c["eps"],
                                                                c["wd"], c["mn"], p["n"])
    e.Sync()
    assert st == capi.ERR_INVALID_ARG and all(bool((v == -7.25).all()) for v in t.values()), (what, st)
