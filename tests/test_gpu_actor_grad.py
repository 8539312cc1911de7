"""GPU checks of gymnet_vecenv_actor_policy_gradient / _value_gradient (gym.net_amd/csrc/actor_grad.hip) through Actor.PolicyGradient /
Actor.ValueGradient.  The reference is torch float64 autograd on the CPU over the same float32 inputs and the same loss formulas.  The
tolerance is relative to what torch's own float32 autograd loses on the same inputs: per parameter tensor the kernel's max |g - g64| may
be 4 x max |g32 - g64| (another summation order over at most m rows) plus 2^-22 x max |g64| (tensors where float32 torch happens to be
exact).  Asserted on the float64 reference: no hidden pre-activation within 1e-5 of zero (a ReLU mask that float32 could flip), no ratio
within 1e-5 of 1 +- clip; SEEDS holds, per (widths, m), a seed found on the CPU for which the reference meets both (for 795 000
pre-activations no single seed was found in four million: that x is eight chunks of rows, a seed each).  m runs over 1, R - 1,
R, R + 1 and R * kGradBlocks + 1 (one workgroup takes two tiles, the others one).  Every test fails without the feature."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
R, BLOCKS = 16, 512                                    # csrc/actor_grad.hpp kGradRows, kGradBlocks
MS = (1, R - 1, R, R + 1, R * BLOCKS + 1)
CLIP = 0.2
# (env, history, widths): the widest action space an env ships is 3 (MountainCar, Acrobot), so the 64-wide network ends in 3, not 8
POLICY = (("CartPole-v1", 4, (16, 50, 20, 2)), ("Acrobot-v1", 4, (24, 50, 20, 3)), ("CartPole-v1", 1, (4, 2)), ("MountainCar-v0", 32, (64, 64, 33, 3)))
CRITIC = (("CartPole-v1", 4, (16, 50, 20, 1)), ("Pendulum-v1", 1, (3, 5, 1)))
FORMS = {"plain": (False, 0.0), "ppo": (True, 0.0), "ppo+entropy": (True, 0.01)}
SEEDS = {((16, 50, 20, 2), 8193): 172676, ((24, 50, 20, 3), 8193): 15930, ((16, 50, 20, 1), 8193): 172676,
         ((64, 64, 33, 3), 8193): (76, 1004, 2121, 3054, 4284, 5031, 6006, 7004)}            # 0 where absent


def make_net(widths, seed=0):
    import torch
    torch.manual_seed(seed)                            # torch's default init
    mods = []
    for k in range(len(widths) - 1):
        mods += [torch.nn.Linear(widths[k], widths[k + 1])] + ([torch.nn.ReLU()] if k + 2 < len(widths) else [])
    return torch.nn.Sequential(*mods)


def make_inputs(widths, m):
    import torch
    seeds = SEEDS.get((tuple(widths), m), 0)                         # one seed, or one per chunk of rows of x (the 64-wide network at m = 8193)
    gens = [torch.Generator().manual_seed(s) for s in (seeds if isinstance(seeds, tuple) else (seeds,))]
    chunk, g = -(-m // len(gens)), gens[0]
    x = torch.cat([torch.randn(min(chunk, m - k * chunk), widths[0], generator=gk) for k, gk in enumerate(gens)])
    return {"x": x, "coef": torch.randn(m, generator=g),
            "actions": torch.randint(0, widths[-1], (m,), generator=g, dtype=torch.int32), "noise": 0.2 * torch.randn(m, generator=g),
            "target": torch.randn(m, generator=g)}


def reference(net, inp, dtype, policy, old=None, ec=0.0, tau=1.0):
    """(gradients per parameter tensor, loss, per-row logp / value, least |hidden pre-activation|, least |ratio - (1 +- clip)|)"""
    import copy
    import torch
    net = copy.deepcopy(net).to(dtype)
    h, margin = inp["x"].to(dtype), math.inf
    mods = list(net)
    for k, mod in enumerate(mods):
        h = mod(h)
        if isinstance(mod, torch.nn.Linear) and k + 1 < len(mods):
            margin = min(margin, float(h.detach().abs().min()))
    edge = math.inf
    if policy:
        logp_all = torch.log_softmax(h / tau, dim=1)
        rows = logp_all.gather(1, inp["actions"].long()[:, None])[:, 0]
        ent = -(logp_all.exp() * logp_all).sum(1)
        coef = inp["coef"].to(dtype)
        if old is None:
            s = coef * rows
        else:
            r = (rows - old.to(dtype)).exp()
            s = torch.minimum(r * coef, r.clamp(1 - CLIP, 1 + CLIP) * coef)
            edge = float(torch.minimum((r - (1 - CLIP)).abs(), (r - (1 + CLIP)).abs()).min().detach())
        loss = -(s + ec * ent).mean()
    else:
        rows = h[:, 0]
        loss = 0.5 * ((rows - inp["target"].to(dtype)) ** 2).mean()
    loss.backward()
    return [p.grad.detach() for p in net.parameters()], float(loss.detach()), rows.detach(), margin, edge


def logp_old_of(net, inp):
    """the reference's logp plus N(0, 0.2^2) noise, float32: some rows clip on either side"""
    import torch
    return (reference(net, inp, torch.float64, True)[2] + inp["noise"].double()).float()


def check(net, inp, got_grad, got_loss, got_rows, policy, old=None, ec=0.0):
    import torch
    g64, loss64, rows64, margin, edge = reference(net, inp, torch.float64, policy, old, ec)
    g32 = reference(net, inp, torch.float32, policy, old, ec)[0]
    assert margin > 1e-5 and edge > 1e-5, (margin, edge)
    at = 0
    for a64, a32 in zip(g64, g32):
        got = got_grad[at:at + a64.numel()].double().reshape(a64.shape)
        at += a64.numel()
        err, err32, top = float((got - a64).abs().max()), float((a32.double() - a64).abs().max()), float(a64.abs().max())
        bound = 4 * err32 + 2.0 ** -22 * top
        print(f"  {tuple(a64.shape)}: kernel {err:.3e} torch32 {err32:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
        assert err <= bound, (tuple(a64.shape), err, err32, bound)
    assert at == got_grad.numel()
    assert abs(got_loss - loss64) <= 2.0 ** -18 * max(1.0, abs(loss64)), (got_loss, loss64)
    assert float((got_rows.double() - rows64).abs().max()) <= 2.0 ** -18 * max(1.0, float(rows64.abs().max()))


def flat_of(net):
    import torch
    return torch.cat([t.detach().reshape(-1) for t in net.parameters()]).cuda()


def new(m):
    import torch
    return torch.empty(m, dtype=torch.float32, device="cuda")


def padded(x, pad):
    """x's rows on the device at a stride of width + pad floats, the floats between rows NaN"""
    import torch
    full = torch.full((x.shape[0], x.shape[1] + pad), math.nan, dtype=torch.float32, device="cuda")
    full[:, :x.shape[1]] = x.cuda()
    return full[:, :x.shape[1]]


@pytest.fixture(scope="module")
def handles(gpu_pkg):
    """one handle per (env, history, widths), each with an actor; a critic's handle gets an actor of its input width"""
    made = {}

    def get(env, S, widths, critic=False):
        key = (env, S, tuple(widths), critic)
        if key not in made:
            e = gpu_pkg.VectorEnv(env, 8, seed=3)
            e.ResetDevice()
            actor = e.Actor(make_net((widths[0], 1 if env == "Pendulum-v1" else 2) if critic else widths), history=S)
            if critic:
                actor.SetCritic(make_net(widths))
            made[key] = (e, actor)
        return made[key]
    yield get
    for e, _ in made.values():
        e.Close()


CASES = [(env, S, w, form) for env, S, w in POLICY for form in FORMS] + [(env, S, w, "value") for env, S, w in CRITIC]


@pytest.mark.parametrize("env,S,widths,form", CASES)
def test_gradient_loss_and_rows_against_float64(handles, env, S, widths, form):
    policy = form != "value"
    e, actor = handles(env, S, widths, critic=not policy)
    net = make_net(widths, seed=1)                                   # not the weights the handle holds: the caller's
    ppo, ec = FORMS.get(form, (False, 0.0))
    for k, m in enumerate(MS):
        inp = make_inputs(widths, m)
        old = logp_old_of(net, inp) if ppo else None
        x, rows = padded(inp["x"], 3 * (k % 2)), new(m)               # x_stride > widths[0] in half the cases
        if policy:
            grad, loss = actor.PolicyGradient(flat_of(net), x, inp["actions"].cuda(), inp["coef"].cuda(), logp_old=None if old is None else old.cuda(),
                                              clip=CLIP, entropy_coef=ec, logp=rows)
        else:
            grad, loss = actor.ValueGradient(flat_of(net), x, inp["target"].cuda(), value=rows)
        e.Sync()
        print(f"{env} {widths} {form} m={m}")
        check(net, inp, grad.cpu(), float(loss.cpu()), rows.cpu(), policy, old, ec)


@pytest.mark.parametrize("policy", (True, False))
def test_the_same_inputs_give_the_same_bits(handles, policy):
    widths = POLICY[0][2] if policy else CRITIC[0][2]
    e, actor = handles("CartPole-v1", 4, widths, critic=not policy)
    inp, net, out = make_inputs(widths, MS[-1]), make_net(widths, seed=1).cuda(), []
    old = logp_old_of(make_net(widths, seed=1), inp).cuda() if policy else None
    for _ in range(2):
        if policy:
            g, l = actor.PolicyGradient(net, inp["x"].cuda(), inp["actions"].cuda(), inp["coef"].cuda(), logp_old=old, entropy_coef=0.01)
        else:
            g, l = actor.ValueGradient(net, inp["x"].cuda(), inp["target"].cuda())
        e.Sync()
        out.append((g.cpu().numpy().view(np.uint32).copy(), l.cpu().numpy().view(np.uint32).copy()))
        assert all(p.grad is not None and p.grad.shape == p.shape for p in net.parameters())           # the Sequential form sets .grad
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][0].any()


def test_the_public_loop_end_to_end(gpu_pkg):
    """softmax exploration at epsilon = 1, a fused rollout with its records, RolloutInputsDevice over every row, PolicyGradient with the
    loaded weights: logp is rec_logp to rounding, and with logp_old = rec_logp, coef = 1 the gradient meets the float64 reference"""
    import torch
    n, T, widths = 256, 4, (16, 50, 20, 2)
    net = make_net(widths, seed=167)                                 # (of seeds 2 .. 200 the ones that meet the reference's conditions: 69, 77, 83, 167)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=11, auto_reset=True) as e:
        e.ResetDevice()
        actor = e.Actor(net, history=4)
        actor.SetExploration("softmax", 1.0)
        h0 = actor.HistoryDevice()
        obs, rec_logp = torch.empty((T, 4, n), dtype=torch.float32, device="cuda"), new(T * n).view(T, n)
        done, act = torch.empty((T, n), dtype=torch.uint8, device="cuda"), torch.empty((T, n), dtype=torch.int32, device="cuda")
        e.RolloutFusedDevice(None, T, actions="actor", epsilon=1.0, action_seed=5, rec_obs=obs, rec_done=done, rec_actions=act, rec_logp=rec_logp)
        x = e.RolloutInputsDevice(obs, done, h0, history=4, rows=torch.arange(T * n, device="cuda"))
        logp, coef = new(T * n), torch.ones(T * n, dtype=torch.float32, device="cuda")
        grad, loss = actor.PolicyGradient(flat_of(net), x, act.view(-1), coef, logp_old=rec_logp.view(-1), clip=CLIP, logp=logp)
        e.Sync()
        old = rec_logp.view(-1).cpu()
        assert bool(((logp.cpu() - old).abs() <= 2.0 ** -18 * old.abs().clamp(min=1.0)).all())
        inp = {"x": x.cpu(), "actions": act.view(-1).cpu(), "coef": coef.cpu()}
        check(net, inp, grad.cpu(), float(loss.cpu()), logp.cpu(), True, old)


@pytest.mark.parametrize("what", ("box", "count", "m", "x_stride", "weights", "x", "actions", "coef", "grad", "clip", "entropy", "no critic", "target", "no actor"))
def test_refusals_touch_nothing(gpu_pkg, what):
    import ctypes as C
    import torch
    capi, box, m = gpu_pkg._capi, what == "box", 5
    widths = (3, 4, 1) if box else (16, 50, 20, 2)
    with gpu_pkg.VectorEnv("Pendulum-v1" if box else "CartPole-v1", 8, seed=1) as e:
        e.ResetDevice()
        actor = None if what == "no actor" else e.Actor(make_net(widths), history=1 if box else 4)
        if what == "target":
            widths = (16, 4, 1)
            actor.SetCritic(make_net(widths))
        count = sum(a * b + b for a, b in zip(widths, widths[1:]))
        t = {k: torch.full((max(count, 16 * m),), -7.25, device="cuda") for k in ("weights", "x", "actions", "coef", "old", "grad")}     # (a refused call reads none)
        p = {k: C.c_void_p(None if k == what else v.data_ptr()) for k, v in t.items()}
        if what in ("no critic", "target"):
            st = capi.load_library().gymnet_vecenv_actor_value_gradient(e._h, p["weights"], count, p["x"], 16, m, None if what == "target" else p["coef"], p["grad"], None, None)
        else:
            st = capi.load_library().gymnet_vecenv_actor_policy_gradient(
                e._h, p["weights"], count + (what == "count"), p["x"], 15 if what == "x_stride" else 16, 0 if what == "m" else m, p["actions"], p["coef"],
                p["old"], 1.0 if what == "clip" else 0.2, math.inf if what == "entropy" else 0.0, p["grad"], None, None)
        e.Sync()
        assert st == capi.ERR_INVALID_ARG and bool((t["grad"] == -7.25).all()), (what, st)


def test_an_action_outside_the_space_poisons_its_row_only(handles):
    widths, m = POLICY[0][2], 40
    e, actor = handles("CartPole-v1", 4, widths)
    flat, inp, out = flat_of(make_net(widths, seed=1)), make_inputs(widths, m), []
    for bad in (None, 2, -1):
        actions, logp = inp["actions"].clone(), new(m)
        if bad is not None:
            actions[17] = bad
        grad, loss = actor.PolicyGradient(flat, inp["x"].cuda(), actions.cuda(), inp["coef"].cuda(), logp=logp)
        e.Sync()
        out.append((logp.cpu().numpy(), float(loss.cpu()), grad.cpu().numpy()))
    keep = np.arange(m) != 17
    for logp, loss, grad in out[1:]:
        assert math.isnan(loss) and np.isnan(logp[17]) and np.isnan(grad).all()
        assert np.array_equal(logp[keep].view(np.uint32), out[0][0][keep].view(np.uint32))
    assert math.isfinite(out[0][1]) and np.isfinite(out[0][0]).all()
