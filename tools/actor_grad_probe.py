"""Times Actor.PolicyGradient / Actor.ValueGradient / Actor.BoxPolicyGradient (csrc/actor_grad.hip) against what a caller does today on the
same device and rows: torch float32 forward, the same loss, backward().  CartPole's 16-50-20-2 actor and 16-50-20-1 critic, then Pendulum's
12-50-20-1 Box actor under both heads (sigma 0.5, ln sigma a leaf on torch's side), at m = 2^12, 2^16, 2^20; HIP events around batches of calls, medians, and the whole measurement run twice, alternating the two sides, so that drift shows as a spread between
the passes.  Writes one line per (call, m, pass).

    python tools/actor_grad_probe.py [--out profiles/actor_grad_probe.txt]
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, batches=9):
    """median over `batches` of the mean time of `reps` back-to-back calls, microseconds"""
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return statistics.median(out)


def main():
    import torch
    import __graft_entry__ as ge
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = ge.load_package()
    lines = []

    def mlp(widths):
        mods = []
        for k in range(len(widths) - 1):
            mods += [torch.nn.Linear(widths[k], widths[k + 1])] + ([torch.nn.ReLU()] if k + 2 < len(widths) else [])
        return torch.nn.Sequential(*mods).cuda()

    def both(name, m, a, b):
        reps = {12: 1000, 16: 300, 20: 40}[m.bit_length() - 1]              # every timed window is tens of milliseconds or more
        for p in (1, 2):                                                   # the whole measurement twice, alternating the sides
            ta, tb = timed(a, reps), timed(b, reps)
            lines.append(f"{name:9s} m=2^{m.bit_length() - 1:<2d} pass {p}: hip {ta:9.1f} us   torch fwd+loss+backward {tb:9.1f} us   torch/hip {tb / ta:6.2f}")
            print(lines[-1], flush=True)

    torch.manual_seed(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), pkg.VectorEnv("CartPole-v1", 64, seed=1, stream=stream.cuda_stream) as env:          # the handle works on torch's stream: one timeline
        env.ResetDevice()
        pnet, vnet = mlp((16, 50, 20, 2)), mlp((16, 50, 20, 1))
        actor = env.Actor(pnet, history=4)
        actor.SetCritic(vnet)
        pflat = torch.cat([p.detach().reshape(-1) for p in pnet.parameters()])
        vflat = torch.cat([p.detach().reshape(-1) for p in vnet.parameters()])
        for m in (1 << 12, 1 << 16, 1 << 20):
            x = torch.randn(m, 16, device="cuda")
            act = torch.randint(0, 2, (m,), device="cuda", dtype=torch.int32)
            coef, target = torch.randn(m, device="cuda"), torch.randn(m, device="cuda")
            old = torch.log_softmax(pnet(x), 1).gather(1, act.long()[:, None])[:, 0].detach() + 0.2 * torch.randn(m, device="cuda")
            pgrad, vgrad = torch.empty_like(pflat), torch.empty_like(vflat)

            def hip_policy():
                actor.PolicyGradient(pflat, x, act, coef, logp_old=old, clip=0.2, entropy_coef=0.01, grad=pgrad)

            def torch_policy():
                pnet.zero_grad(set_to_none=True)
                lp_all = torch.log_softmax(pnet(x), 1)
                lp = lp_all.gather(1, act.long()[:, None])[:, 0]
                r = (lp - old).exp()
                s = torch.minimum(r * coef, r.clamp(0.8, 1.2) * coef)
                (-(s - 0.01 * (lp_all.exp() * lp_all).sum(1)).mean()).backward()

            def hip_value():
                actor.ValueGradient(vflat, x, target, grad=vgrad)

            def torch_value():
                vnet.zero_grad(set_to_none=True)
                (0.5 * ((vnet(x)[:, 0] - target) ** 2).mean()).backward()

            both("policy", m, hip_policy, torch_policy)
            both("value", m, hip_value, torch_value)
    with torch.cuda.stream(stream), pkg.VectorEnv("Pendulum-v1", 64, seed=1, stream=stream.cuda_stream) as env:
        env.ResetDevice()
        bnet = mlp((12, 50, 20, 1))
        actor = env.Actor(bnet, history=4)
        bflat, sigma = torch.cat([p.detach().reshape(-1) for p in bnet.parameters()]), 0.5
        c = -math.log(sigma) - 0.5 * math.log(2 * math.pi)
        ls = torch.zeros(1, device="cuda", requires_grad=True)             # ln sigma - ln 0.5
        for head in ("clamp", "tanh"):
            actor.SetPolicy(head, "gaussian", sigma)

            def greedy(raw):
                return raw.clamp(-2.0, 2.0) if head == "clamp" else 2.0 * torch.tanh(raw)

            for m in (1 << 12, 1 << 16, 1 << 20):
                x, coef = torch.randn(m, 12, device="cuda"), torch.randn(m, device="cuda")
                with torch.no_grad():
                    g0 = greedy(bnet(x)[:, 0])
                    act = (g0 + sigma * torch.randn(m, device="cuda")).clamp(-2.0, 2.0)
                    old = -0.5 * ((act - g0) / sigma) ** 2 + c + 0.2 * torch.randn(m, device="cuda")
                bgrad, bsig = torch.empty_like(bflat), torch.empty(1, device="cuda")

                def hip_box():
                    actor.BoxPolicyGradient(bflat, x, act, coef, logd_old=old, clip=0.2, entropy_coef=0.01, grad=bgrad, grad_log_sigma=bsig)

                def torch_box():
                    bnet.zero_grad(set_to_none=True)
                    ls.grad = None
                    d = (act - greedy(bnet(x)[:, 0])) * ((1.0 / sigma) * (-ls).exp())
                    r = (-0.5 * d * d + (c - ls) - old).exp()
                    s = torch.minimum(r * coef, r.clamp(0.8, 1.2) * coef)
                    (-s.mean() - 0.01 * (ls + math.log(sigma) + 0.5 * (1 + math.log(2 * math.pi)))).sum().backward()

                both("box " + head, m, hip_box, torch_box)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/actor_grad_probe.py: CartPole 16-50-20-2 / 16-50-20-1, Pendulum 12-50-20-1 (Box, sigma 0.5), PPO clip 0.2 + entropy 0.01; HIP events, median of 9 batches\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
