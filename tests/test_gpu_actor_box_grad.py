"""GPU checks of gymnet_vecenv_actor_box_policy_gradient (the Box head of gym.net_amd/csrc/actor_grad.hip) through Actor.BoxPolicyGradient.
The reference is torch float64 autograd on the CPU over the same float32 inputs and the formulas of include/gymnet_amd.h, with ln sigma a
leaf so that autograd gives grad_log_sigma.  Tolerances are test_gpu_actor_grad.py's: a parameter tensor, and grad_log_sigma as a
one-element tensor, may err by 4 x |torch float32 - float64| + 2^-22 x max |ref|; the loss and the logd rows by 2^-18 x max(1, |ref|).  On
these inputs at sigma = 0.5 torch's own float32 loss and logd stay inside half of that (at most 0.10 and 0.41 of the bound over every
case: docs/ledger.md §46).  Asserted on the float64 reference: no hidden pre-activation within 1e-5 of zero, no ratio within 1e-5 of
1 +- clip, and for the clamp head no raw within 1e-5 of a bound and — wherever m >= 15; one row cannot be on both sides — at least a tenth
of the rows outside the bounds and a tenth inside (for that NETS carries a factor on the last layer's weights and a bias in its own's place).
SEEDS holds, per (widths, m), input seeds found on the CPU for which the reference meets these: at m = 8193 a seed per eighth of x's rows.  Every test fails without the feature: the export does not exist."""
import math

import numpy as np
import pytest

from test_gpu_actor_grad import flat_of, make_net, padded

pytestmark = pytest.mark.gpu
MS = (1, 15, 16, 17, 16 * 512 + 1)                     # R - 1, R, R + 1, R * kGradBlocks + 1 (csrc/actor_grad.hpp)
CLIP, SIGMA = 0.2, 0.5
INV_SIGMA, C = float(np.float32(1.0 / SIGMA)), float(np.float32(-math.log(SIGMA) - 0.91893853320467274178))       # box_logd_args
# (env, history, widths, (low, high), (the factor on the last layer's weights, its bias): raw spreads about as wide as the bounds, around 0)
NETS = (("Pendulum-v1", 1, (3, 5, 1), (-2.0, 2.0), (16.0, 4.0)), ("Pendulum-v1", 4, (12, 50, 20, 1), (-2.0, 2.0), (28.0, 1.0)),
        ("MountainCarContinuous-v0", 32, (64, 64, 33, 1), (-1.0, 1.0), (14.0, 0.0)))
FORMS = {"plain": (False, 0.0), "ppo": (True, 0.0), "ppo+entropy": (True, 0.01)}
# (widths, m): (a seed per chunk of rows of x, the other inputs' seed); ((0,), 0) where absent
SEEDS = {((3, 5, 1), 8193): ((0, 1000, 2001, 3000, 4000, 5000, 6000, 7000), 0), ((12, 50, 20, 1), 8193): ((2, 1000, 2000, 3000, 4002, 5003, 6000, 7000), 0),
         ((64, 64, 33, 1), 8193): ((0, 1004, 2009, 3002, 4000, 5000, 6001, 7004), 0)}


def scaled_net(widths, last):
    import torch
    net = make_net(widths, seed=1)
    with torch.no_grad():
        list(net)[-1].weight.mul_(last[0])
        list(net)[-1].bias.fill_(last[1])
    return net


def reference(net, inp, dtype, head, bounds, old=None, ec=0.0):
    """(gradients per parameter tensor and grad_log_sigma [1] last, loss, logd rows, least |hidden pre-activation|, least |ratio - (1 +- clip)|, raw)"""
    import copy
    import torch
    net = copy.deepcopy(net).to(dtype)
    (low, high), h, margin, edge, mods = bounds, inp["x"].to(dtype), math.inf, math.inf, list(net)
    for k, mod in enumerate(mods):
        h = mod(h)
        if isinstance(mod, torch.nn.Linear) and k + 1 < len(mods):
            margin = min(margin, float(h.detach().abs().min()))
    raw = h[:, 0]
    g = raw.clamp(low, high) if head == "clamp" else 0.5 * (low + high) + 0.5 * (high - low) * torch.tanh(raw)
    if "actions" not in inp:                           # the float64 greedy action plus sigma * N(0, 1), clamped, as float32
        inp["actions"] = (g.detach().double() + SIGMA * inp["z"].double()).clamp(low, high).float()
    ls = torch.zeros(1, dtype=dtype, requires_grad=True)             # ln sigma - ln SIGMA: the constants are the float32 ones the library forms
    d = (inp["actions"].to(dtype) - g) * (INV_SIGMA * (-ls).exp())
    logd, coef = -0.5 * d * d + (C - ls), inp["coef"].to(dtype)
    if old is None:
        s = coef * logd
    else:
        r = (logd - old.to(dtype)).exp()
        s = torch.minimum(r * coef, r.clamp(1 - CLIP, 1 + CLIP) * coef)
        edge = float(torch.minimum((r - (1 - CLIP)).abs(), (r - (1 + CLIP)).abs()).min().detach())
    loss = -s.mean() - ec * (ls + math.log(SIGMA) + 0.5 * (1 + math.log(2 * math.pi)))
    loss.backward()
    return [p.grad.detach() for p in net.parameters()] + [ls.grad.detach()], float(loss.detach()), logd.detach(), margin, edge, raw.detach()


def make_case(widths, last, m, head, bounds, ppo):
    """the caller's network, the inputs (float32; actions around the float64 greedy action), logd_old = the reference's logd + N(0, 0.2^2)"""
    import torch
    xs, rest = SEEDS.get((tuple(widths), m), ((0,), 0))
    chunk, g = -(-m // len(xs)), torch.Generator().manual_seed(rest)
    x = torch.cat([torch.randn(min(chunk, m - k * chunk), widths[0], generator=torch.Generator().manual_seed(s)) for k, s in enumerate(xs)])
    inp = {"x": x, "coef": torch.randn(m, generator=g), "z": torch.randn(m, generator=g)}
    noise, net = 0.2 * torch.randn(m, generator=g), scaled_net(widths, last)
    logd = reference(net, inp, torch.float64, head, bounds)[2]
    return net, inp, ((logd + noise.double()).float() if ppo else None)


def check(net, inp, head, bounds, old, ec, got_grad, got_sigma, got_loss, got_rows):
    import torch
    g64, loss64, rows64, margin, edge, raw = reference(net, inp, torch.float64, head, bounds, old, ec)
    g32, loss32, rows32 = reference(net, inp, torch.float32, head, bounds, old, ec)[:3]
    assert margin > 1e-5 and edge > 1e-5, (margin, edge)
    m, (low, high) = raw.numel(), bounds
    if head == "clamp":
        outside = int(((raw < low) | (raw > high)).sum())
        assert float(torch.minimum((raw - low).abs(), (raw - high).abs()).min()) > 1e-5
        assert m < 15 or (10 * outside >= m and 10 * (m - outside) >= m), (m, outside)
    got, at = torch.cat([got_grad, got_sigma]).double(), 0
    for a64, a32 in zip(g64, g32):
        part = got[at:at + a64.numel()].reshape(a64.shape)
        at += a64.numel()
        err, err32, top = float((part - a64).abs().max()), float((a32.double() - a64).abs().max()), float(a64.abs().max())
        bound = 4 * err32 + 2.0 ** -22 * top
        print(f"  {tuple(a64.shape)}: kernel {err:.3e} torch32 {err32:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
        assert err <= bound, (tuple(a64.shape), err, err32, bound)
    assert at == got.numel()
    bl, br = 2.0 ** -18 * max(1.0, abs(loss64)), 2.0 ** -18 * max(1.0, float(rows64.abs().max()))
    el, er = abs(got_loss - loss64), float((got_rows.double() - rows64).abs().max())
    print(f"  loss: kernel {el / bl:.3f} torch32 {abs(loss32 - loss64) / bl:.3f} of the bound; logd: kernel {er / br:.3f} torch32 "
          f"{float((rows32.double() - rows64).abs().max()) / br:.3f}")
    assert abs(loss32 - loss64) <= bl / 2 and float((rows32.double() - rows64).abs().max()) <= br / 2          # the premise of the row bound
    assert el <= bl and er <= br, (el, bl, er, br)


@pytest.fixture(scope="module")
def handles(gpu_pkg):
    """one handle per network, its Box actor holding other weights than the caller's"""
    made = {}

    def get(k, head, sigma=SIGMA):
        env, S, widths = NETS[k][:3]
        if k not in made:
            e = gpu_pkg.VectorEnv(env, 8, seed=3)
            e.ResetDevice()
            made[k] = (e, e.Actor(make_net(widths), history=S))
        made[k][1].SetPolicy(head, "gaussian", sigma)
        return made[k]
    yield get
    for e, _ in made.values():
        e.Close()


def run(actor, net, inp, old, ec, pad=0, sigma_out=True):
    import torch
    m = inp["x"].shape[0]
    rows, gls = torch.empty(m, device="cuda"), torch.full((1,), -7.25, device="cuda") if sigma_out else None
    grad, loss = actor.BoxPolicyGradient(net if hasattr(net, "data_ptr") else flat_of(net), padded(inp["x"], pad), inp["actions"].cuda(), inp["coef"].cuda(),
                                         logd_old=None if old is None else old.cuda(), clip=CLIP, entropy_coef=ec, logd=rows, grad_log_sigma=gls)
    torch.cuda.synchronize()
    return grad.cpu(), (gls.cpu() if sigma_out else None), float(loss.cpu()), rows.cpu()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("head", ("clamp", "tanh"))
@pytest.mark.parametrize("k", range(len(NETS)))
def test_gradients_loss_and_rows_against_float64(handles, k, head, form):
    """On an MI355X every bound holds: the kernel's gradient error is at most 0.24 of its bound over every tensor of every case, its loss
    and logd within 0.007 and 0.012 of theirs.  (a - g) / sigma^2 carries the error of the greedy action into every gradient, which is
    why the Box head forms raw and the head in float64: with both in float32 ten of these cases missed the bound (docs/ledger.md §46)."""
    env, S, widths, bounds, last = NETS[k]
    e, actor = handles(k, head)
    ppo, ec = FORMS[form]
    for j, m in enumerate(MS):
        if k == 2 and m == MS[-1] and form != "ppo+entropy":          # the large network at the large m: once per head
            continue
        net, inp, old = make_case(widths, last, m, head, bounds, ppo)
        print(f"{env} {widths} {head} {form} m={m}")
        check(net, inp, head, bounds, old, ec, *run(actor, net, inp, old, ec, pad=3 * (j % 2)))          # a padded x stride in every other case


def test_same_bits_twice_and_without_the_sigma_output(handles):
    _, actor = handles(1, "tanh")
    net, inp, old = make_case(NETS[1][2], NETS[1][4], MS[-1], "tanh", NETS[1][3], True)
    a, b, c = (run(actor, net, inp, old, 0.01, sigma_out=s) for s in (True, True, False))
    bits = lambda t: np.asarray(t, dtype=np.float32).view(np.uint32)          # noqa: E731
    assert all(np.array_equal(bits(a[i]), bits(b[i])) for i in range(4)) and bits(a[0]).any() and float(a[1]) != -7.25
    assert all(np.array_equal(bits(a[i]), bits(c[i])) for i in (0, 2, 3))


def test_a_nan_action_poisons_its_row_only(handles):
    _, actor = handles(1, "clamp")
    net, inp, _ = make_case(NETS[1][2], NETS[1][4], 40, "clamp", NETS[1][3], False)
    good = run(actor, net, inp, None, 0.0)
    inp["actions"][17] = math.nan
    grad, gls, loss, rows = run(actor, net, inp, None, 0.0)
    keep = np.arange(40) != 17
    assert math.isnan(loss) and bool(grad.isnan().all()) and bool(gls.isnan().all()) and math.isnan(rows[17])
    assert np.array_equal(rows.numpy()[keep].view(np.uint32), good[3].numpy()[keep].view(np.uint32)) and math.isfinite(good[2])


def test_logd_over_a_fused_rollouts_rows_is_rec_logd(gpu_pkg):
    import torch
    n, T, widths = 256, 4, (12, 50, 20, 1)
    net = make_net(widths, seed=5)
    with gpu_pkg.VectorEnv("Pendulum-v1", n, seed=11, auto_reset=True) as e:
        e.ResetDevice()
        actor = e.Actor(net, history=4)
        actor.SetPolicy("tanh", "gaussian", SIGMA)
        h0 = actor.HistoryDevice()
        obs, done = torch.empty((T, 3, n), dtype=torch.float32, device="cuda"), torch.empty((T, n), dtype=torch.uint8, device="cuda")
        act, rec = torch.empty((T, n), dtype=torch.float32, device="cuda"), torch.empty((T, n), dtype=torch.float32, device="cuda")
        e.RolloutFusedDevice(None, T, actions="actor", epsilon=1.0, action_seed=5, rec_obs=obs, rec_done=done, rec_actions=act, rec_logd=rec)
        x = e.RolloutInputsDevice(obs, done, h0, history=4, rows=torch.arange(T * n, device="cuda"))
        logd = torch.empty(T * n, device="cuda")
        actor.BoxPolicyGradient(flat_of(net), x, act.view(-1), torch.ones(T * n, device="cuda"), logd_old=rec.view(-1), logd=logd)
        e.Sync()
        old = rec.view(-1).cpu()
        assert bool(((logd.cpu() - old).abs() <= 2.0 ** -18 * old.abs().clamp(min=1.0)).all()) and len(old.unique()) > T * n // 4


@pytest.mark.parametrize("what", ("discrete", "sigma", "actions"))
def test_new_refusals_touch_nothing(gpu_pkg, what):
    import ctypes as C
    import torch
    capi, widths = gpu_pkg._capi, (16, 4, 2) if what == "discrete" else (3, 4, 1)
    with gpu_pkg.VectorEnv("CartPole-v1" if what == "discrete" else "Pendulum-v1", 8, seed=1) as e:
        e.ResetDevice()
        actor = e.Actor(make_net(widths), history=4 if what == "discrete" else 1)
        if what == "actions":
            actor.SetPolicy("clamp", "gaussian", SIGMA)                # ("sigma": a fresh actor's is 0)
        count = sum(a * b + b for a, b in zip(widths, widths[1:]))
        t = {k: torch.full((max(count, 80),), -7.25, device="cuda") for k in ("weights", "x", "actions", "coef", "grad")}
        p = {k: C.c_void_p(None if k == what else v.data_ptr()) for k, v in t.items()}
        st = capi.load_library().gymnet_vecenv_actor_box_policy_gradient(e._h, p["weights"], count, p["x"], 16, 5, p["actions"], p["coef"], None, 0.2, 0.0,
                                                                         p["grad"], None, None, None)
        e.Sync()
        assert st == capi.ERR_INVALID_ARG and bool((t["grad"] == -7.25).all()), (what, st)
