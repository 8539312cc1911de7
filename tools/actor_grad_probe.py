"""Times Actor.PolicyGradient / Actor.ValueGradient (csrc/actor_grad.hip) against what a caller does today on the same device and rows:
torch float32 forward, the same loss, backward().  CartPole's 16-50-20-2 actor and 16-50-20-1 critic at m = 2^12, 2^16, 2^20; HIP events
around batches of calls, medians, and the whole measurement run twice, alternating the two sides, so that drift shows as a spread between
the passes.  Writes one line per (call, m, pass).

    python tools/actor_grad_probe.py [--out profiles/actor_grad_probe.txt]
"""
import argparse
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

            reps = {12: 1000, 16: 300, 20: 40}[m.bit_length() - 1]          # every timed window is tens of milliseconds or more
            for name, a, b in (("policy", hip_policy, torch_policy), ("value", hip_value, torch_value)):
                for p in (1, 2):                                       # the whole measurement twice, alternating the sides
                    ta, tb = timed(a, reps), timed(b, reps)
                    lines.append(f"{name:6s} m=2^{m.bit_length() - 1:<2d} pass {p}: hip {ta:9.1f} us   torch fwd+loss+backward {tb:9.1f} us   torch/hip {tb / ta:6.2f}")
                    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/actor_grad_probe.py: CartPole 16-50-20-2 / 16-50-20-1, PPO clip 0.2 + entropy 0.01; HIP events, median of 9 batches\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
