"""Times Actor.QGradient (csrc/actor_grad.hip, the Q head and its target passes) against what a caller does today on the same device and
rows: torch float32, two no_grad forwards over x_next (one for the plain form), the forward over x, huber_loss, backward().  CartPole's
16-50-20-2 network with a distinct target network, forms dqn and double, at m = 2^12, 2^16, 2^20; Actor.ValueGradient of a 16-50-20-1
critic at the same m in the same run, since the expectation is its time plus one forward-only pass per target pass.  HIP events around
batches of calls, medians, and the whole measurement run twice, alternating the two sides, so that drift shows as a spread between the
passes.  Writes one line per (call, m, pass).

    python tools/actor_q_grad_probe.py [--out profiles/actor_q_grad_probe.txt]
"""
import argparse
import os
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
from actor_grad_probe import timed  # noqa: E402


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
        qnet, tnet, vnet = mlp((16, 50, 20, 2)), mlp((16, 50, 20, 2)), mlp((16, 50, 20, 1))
        actor = env.Actor(qnet, history=4)
        actor.SetCritic(vnet)
        flat = lambda net: torch.cat([p.detach().reshape(-1) for p in net.parameters()])        # noqa: E731
        qflat, tflat, vflat = flat(qnet), flat(tnet), flat(vnet)
        for m in (1 << 12, 1 << 16, 1 << 20):
            x, x_next = torch.randn(m, 16, device="cuda"), torch.randn(m, 16, device="cuda")
            act = torch.randint(0, 2, (m,), device="cuda", dtype=torch.int32)
            reward, done = torch.randn(m, device="cuda"), (torch.rand(m, device="cuda") < 0.25).to(torch.uint8)
            qgrad, vgrad, y = torch.empty_like(qflat), torch.empty_like(vflat), torch.empty(m, device="cuda")
            act64, live = act.long()[:, None], done == 0

            def hip_value():
                actor.ValueGradient(vflat, x, reward, grad=vgrad)

            def torch_value():
                vnet.zero_grad(set_to_none=True)
                (0.5 * ((vnet(x)[:, 0] - reward) ** 2).mean()).backward()

            both("value", m, hip_value, torch_value)
            for double in (False, True):
                def hip_q():
                    actor.QGradient(qflat, x, act, reward, done, x_next, target_net=tflat, gamma=0.99, huber_delta=1.0, double=double, grad=qgrad, y=y)

                def torch_q():
                    qnet.zero_grad(set_to_none=True)
                    with torch.no_grad():
                        qt = tnet(x_next)
                        qn = qt.gather(1, qnet(x_next).argmax(1)[:, None])[:, 0] if double else qt.max(1).values
                        target = torch.where(live, reward + 0.99 * qn, reward)
                    torch.nn.functional.huber_loss(qnet(x).gather(1, act64)[:, 0], target, delta=1.0).backward()

                both("double" if double else "dqn", m, hip_q, torch_q)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/actor_q_grad_probe.py: CartPole 16-50-20-2 online + target network, Huber delta 1, gamma 0.99, a quarter of the rows done; "
                    "value: the 16-50-20-1 critic's ValueGradient at the same m; HIP events, median of 9 batches\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
