"""GPU checks of gymnet_vecenv_actor_q_gradient (gym.net_amd/csrc/actor_grad.hip, the Q head and its target passes) through Actor.QGradient.
The reference is torch float64 on the CPU over the same float32 inputs and the header's formulas; the tolerances are test_gpu_actor_grad's:
per parameter tensor max |g - g64| <= 4 x max |g32 - g64| + 2^-22 x max |g64| with g32 torch's float32 autograd, and loss, y, q within
2^-18 x max(1, |ref|).  Asserted on the float64 reference at 1e-5: no hidden pre-activation of Q(x) near zero (x and the online network
are that file's, so its SEEDS carry over), no ||td| - delta| near zero, and for the double form no two leading entries of Q(x_next) of a
live row near each other.  QSEEDS holds, per (widths, m), a seed of this file's generator found on the CPU for which the reference meets
them in every form.  m runs over 1, R - 1, R, R + 1 and, for the first and the widest network, R * kGradBlocks + 1: one workgroup walks
two tiles in every pass.  x_next of every done row is NaN.  Every test fails without the feature: the export does not exist."""
import math

import numpy as np
import pytest

from test_gpu_actor_grad import POLICY, flat_of, handles, make_inputs, make_net, new, padded  # noqa: F401  (handles: a fixture)

pytestmark = pytest.mark.gpu
R, BLOCKS, GAMMA = 16, 512, float(np.float32(0.99))    # (the float32 the call receives)
BIG = R * BLOCKS + 1
FORMS = {"dqn": (True, 1.0, False), "double": (True, 1.0, True), "shared-mse": (False, math.inf, False)}       # (a target network, delta, double)
QSEEDS = {((16, 50, 20, 2), BIG): 1, ((64, 64, 33, 3), BIG): 1}
E2E_SEED = 12           # the end-to-end test's networks (of seeds 0 .. 24 the rollout's rows meet the three conditions for 12, 14 and 24)                    # 0 where absent


def make_q_inputs(widths, m):
    import torch
    inp = make_inputs(widths, m)
    g = torch.Generator().manual_seed(QSEEDS.get((tuple(widths), m), 0))
    done = torch.where(torch.rand(m, generator=g) < 0.25, torch.randint(1, 4, (m,), generator=g), 0).to(torch.uint8)
    x_next = torch.randn(m, widths[0], generator=g)
    x_next[done != 0] = math.nan
    return {"x": inp["x"], "actions": inp["actions"], "x_next": x_next, "reward": torch.randn(m, generator=g), "done": done}


def reference(net, tnet, inp, dtype, delta, double):
    """(gradients per parameter tensor, loss, y, q, least |hidden pre-activation| of Q(x), least ||td| - delta|, least top-two gap of Q(x_next))"""
    import copy
    import torch
    net, tnet = copy.deepcopy(net).to(dtype), copy.deepcopy(tnet).to(dtype)
    h, margin, gap = inp["x"].to(dtype), math.inf, math.inf
    mods = list(net)
    for k, mod in enumerate(mods):
        h = mod(h)
        if isinstance(mod, torch.nn.Linear) and k + 1 < len(mods):
            margin = min(margin, float(h.detach().abs().min()))
    live = inp["done"] == 0
    with torch.no_grad():
        x_next, reward = inp["x_next"].to(dtype), inp["reward"].to(dtype)
        qn = tnet(x_next).max(1).values
        if double:
            online = net(x_next)
            qn = tnet(x_next).gather(1, online.argmax(1)[:, None])[:, 0]
            top = online[live].topk(2, dim=1).values
            gap = float((top[:, 0] - top[:, 1]).min()) if top.numel() else math.inf
        y = torch.where(live, reward + GAMMA * qn, reward)
    q = h.gather(1, inp["actions"].long()[:, None])[:, 0]
    td = q - y
    term = 0.5 * td * td if math.isinf(delta) else torch.nn.functional.huber_loss(q, y, delta=delta, reduction="none")
    term.mean().backward()
    edge = float((td.detach().abs() - delta).abs().min())
    return [p.grad.detach() for p in net.parameters()], float(term.mean().detach()), y, q.detach(), margin, edge, gap


def check(net, tnet, inp, got, delta, double):
    import torch
    grad, loss, y, q = got
    g64, loss64, y64, q64, margin, edge, gap = reference(net, tnet, inp, torch.float64, delta, double)
    g32 = reference(net, tnet, inp, torch.float32, delta, double)[0]
    assert margin > 1e-5 and edge > 1e-5 and gap > 1e-5, (margin, edge, gap)
    at = 0
    for a64, a32 in zip(g64, g32):
        have = grad[at:at + a64.numel()].double().reshape(a64.shape)
        at += a64.numel()
        err, err32, top = float((have - a64).abs().max()), float((a32.double() - a64).abs().max()), float(a64.abs().max())
        bound = 4 * err32 + 2.0 ** -22 * top
        print(f"  {tuple(a64.shape)}: kernel {err:.3e} torch32 {err32:.3e} bound {bound:.3e} ratio {err / bound if bound else 0:.3f}")
        assert err <= bound, (tuple(a64.shape), err, err32, bound)
    assert at == grad.numel()
    assert abs(loss - loss64) <= 2.0 ** -18 * max(1.0, abs(loss64)), (loss, loss64)
    for have, want in ((y, y64), (q, q64)):
        assert float((have.double() - want).abs().max()) <= 2.0 ** -18 * max(1.0, float(want.abs().max()))
    done = inp["done"] != 0
    assert np.array_equal(y[done].numpy().view(np.uint32), inp["reward"][done].numpy().view(np.uint32))              # a select: bit for bit


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("env,S,widths", POLICY)
def test_gradient_loss_y_and_q_against_float64(handles, env, S, widths, form):
    e, actor = handles(env, S, widths)
    net, tnet = make_net(widths, seed=1), make_net(widths, seed=2)                      # the caller's, not the weights the handle holds
    has_target, delta, double = FORMS[form]
    for k, m in enumerate((1, R - 1, R, R + 1) + ((BIG,) if widths in (POLICY[0][2], POLICY[-1][2]) else ())):
        inp = make_q_inputs(widths, m)
        x, x_next, y, q = padded(inp["x"], 3 * (k % 2)), padded(inp["x_next"], 3 * ((k + 1) % 2)), new(m), new(m)
        grad, loss = actor.QGradient(flat_of(net), x, inp["actions"].cuda(), inp["reward"].cuda(), inp["done"].cuda(), x_next,
                                     target_net=flat_of(tnet) if has_target else None, gamma=GAMMA, huber_delta=delta, double=double, y=y, q=q)
        e.Sync()
        print(f"{env} {widths} {form} m={m}")
        check(net, tnet if has_target else net, inp, (grad.cpu(), float(loss.cpu()), y.cpu(), q.cpu()), delta, double)


def test_the_same_inputs_give_the_same_bits(handles):
    widths = POLICY[0][2]
    e, actor = handles("CartPole-v1", 4, widths)
    inp, net, tnet, out = make_q_inputs(widths, BIG), make_net(widths, seed=1).cuda(), make_net(widths, seed=2).cuda(), []
    for _ in range(2):
        y = new(BIG)
        g, l = actor.QGradient(net, inp["x"].cuda(), inp["actions"].cuda(), inp["reward"].cuda(), inp["done"].cuda(), inp["x_next"].cuda(),
                               target_net=tnet, gamma=GAMMA, double=True, y=y)
        e.Sync()
        out.append([t.cpu().numpy().view(np.uint32).copy() for t in (g, l, y)])
        assert all(p.grad is not None and p.grad.shape == p.shape for p in net.parameters())           # the Sequential form sets .grad on net ...
        assert all(p.grad is None for p in tnet.parameters())                                          # ... and never on target_net
    assert all(np.array_equal(a, b) and a.any() for a, b in zip(*out))


REFUSALS = ("box", "count", "m", "x_stride", "x_next_stride", "weights", "x", "x_next", "actions", "reward", "done", "y", "grad", "gamma above",
            "gamma nan", "delta zero", "delta nan", "overflow", "no actor")


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_touch_nothing(gpu_pkg, what):
    import ctypes as C
    import torch
    capi, box, m = gpu_pkg._capi, what == "box", 5
    widths = (3, 4, 1) if box else (16, 50, 20, 2)
    with gpu_pkg.VectorEnv("Pendulum-v1" if box else "CartPole-v1", 8, seed=1) as e:
        e.ResetDevice()
        if what != "no actor":
            e.Actor(make_net(widths), history=1 if box else 4)
        count = sum(a * b + b for a, b in zip(widths, widths[1:]))
        names = ("weights", "target", "x", "x_next", "actions", "reward", "done", "y", "grad")
        t = {k: torch.full((max(count, 16 * m),), -7.25, device="cuda") for k in names}                # (a refused call reads none)
        p = {k: C.c_void_p(None if k == what else v.data_ptr()) for k, v in t.items()}
        st = capi.load_library().gymnet_vecenv_actor_q_gradient(
            e._h, p["weights"], p["target"], count + (what == "count"), p["x"], 15 if what == "x_stride" else 16, p["x_next"],
            15 if what == "x_next_stride" else 16, {"m": 0, "overflow": 2 ** 62}.get(what, m), p["actions"], p["reward"], p["done"],
            {"gamma above": 1.5, "gamma nan": math.nan}.get(what, GAMMA), {"delta zero": 0.0, "delta nan": math.nan}.get(what, 1.0), 0,
            p["y"], p["grad"], None, None)
        e.Sync()
        assert st == capi.ERR_INVALID_ARG and bool((t["grad"] == -7.25).all()) and bool((t["y"] == -7.25).all()), (what, st)


def test_an_action_outside_the_space_poisons_its_row_only(handles):
    widths, m = POLICY[0][2], 40
    e, actor = handles("CartPole-v1", 4, widths)
    flat, target, inp, out = flat_of(make_net(widths, seed=1)), flat_of(make_net(widths, seed=2)), make_q_inputs(widths, m), []
    for bad in (None, widths[-1], -1):
        actions, y, q = inp["actions"].clone(), new(m), new(m)
        if bad is not None:
            actions[17] = bad
        grad, loss = actor.QGradient(flat, inp["x"].cuda(), actions.cuda(), inp["reward"].cuda(), inp["done"].cuda(), inp["x_next"].cuda(),
                                     target_net=target, double=True, y=y, q=q)
        e.Sync()
        out.append((q.cpu().numpy(), float(loss.cpu()), grad.cpu().numpy(), y.cpu().numpy()))
    keep = np.arange(m) != 17
    for q, loss, grad, y in out[1:]:
        assert math.isnan(loss) and np.isnan(q[17]) and np.isnan(grad).all()
        assert np.array_equal(q[keep].view(np.uint32), out[0][0][keep].view(np.uint32)) and np.array_equal(y.view(np.uint32), out[0][3].view(np.uint32))
    assert math.isfinite(out[0][1]) and np.isfinite(out[0][0]).all() and np.isfinite(out[0][3]).all()


def test_the_public_loop_end_to_end(gpu_pkg):
    """an epsilon-greedy fused rollout with its records, x and x_next from RolloutInputsDevice at idx and idx + n over the rows of the
    first T - 1 steps, QGradient (double) with a second network as the target: the gradient meets the float64 reference"""
    import torch
    n, T, widths = 256, 4, (16, 50, 20, 2)
    net, tnet = make_net(widths, seed=E2E_SEED), make_net(widths, seed=E2E_SEED + 1000)
    with gpu_pkg.VectorEnv("CartPole-v1", n, seed=11, auto_reset=True) as e:
        e.ResetDevice()
        actor = e.Actor(net, history=4)
        h0 = actor.HistoryDevice()
        obs, rew = torch.empty((T, 4, n), dtype=torch.float32, device="cuda"), new(T * n).view(T, n)
        done, act = torch.empty((T, n), dtype=torch.uint8, device="cuda"), torch.empty((T, n), dtype=torch.int32, device="cuda")
        e.RolloutFusedDevice(None, T, actions="actor", epsilon=0.5, action_seed=5, rec_obs=obs, rec_done=done, rec_reward=rew, rec_actions=act)
        idx = torch.arange((T - 1) * n, device="cuda")
        x, x_next = (e.RolloutInputsDevice(obs, done, h0, history=4, rows=rows) for rows in (idx, idx + n))
        rows = {"actions": act.view(-1)[idx], "reward": rew.view(-1)[idx], "done": done.view(-1)[idx]}
        y, q = new(idx.numel()), new(idx.numel())
        grad, loss = actor.QGradient(flat_of(net), x, rows["actions"], rows["reward"], rows["done"], x_next, target_net=flat_of(tnet), gamma=GAMMA,
                                     double=True, y=y, q=q)
        e.Sync()
        inp = dict({k: v.cpu() for k, v in rows.items()}, x=x.cpu(), x_next=x_next.cpu())
        check(net, tnet, inp, (grad.cpu(), float(loss.cpu()), y.cpu(), q.cpu()), 1.0, True)
