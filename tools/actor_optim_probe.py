"""Times Actor.ApplyGradient (csrc/actor_optim.hip) against what a torch caller does today on the same flat device tensor:
torch.nn.utils.clip_grad_norm_ (where clipping is on) followed by the matching torch.optim step, in torch's default form and, where torch
offers it, fused=True.  CartPole's 16-50-20-2 (1 912 parameters) and an 8 192-parameter vector; every rule with and without clipping; then
a whole minibatch update at m = 2^12, PolicyGradient + ApplyGradient against PolicyGradient + the torch step.  HIP events around batches of
calls, medians, and the whole measurement run twice, alternating the sides, so that drift shows as a spread between the passes.  Writes one
line per (case, pass).

    python tools/actor_optim_probe.py [--out profiles/actor_optim_probe.txt]
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
    hp = {"sgd": dict(lr=1e-2, momentum=0.9), "adadelta": dict(lr=1.0, rho=0.9, eps=1e-6), "adam": dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8)}
    optim = {"sgd": torch.optim.SGD, "adadelta": torch.optim.Adadelta, "adam": torch.optim.Adam}

    def torch_sides(rule, count, clip):
        """{form: step function} over a flat parameter of its own"""
        sides = {}
        for form in ("default", "fused"):
            p = torch.nn.Parameter(0.5 * torch.randn(count, device="cuda"))
            p.grad = torch.randn(count, device="cuda")
            try:
                opt = optim[rule]([p], **hp[rule], **({"fused": True} if form == "fused" else {}))
            except (TypeError, RuntimeError):              # this torch has no fused form of the rule
                continue

            def step(p=p, opt=opt):
                if clip:
                    torch.nn.utils.clip_grad_norm_([p], clip)
                opt.step()
            sides[form] = step
        return sides

    def report(name, reps, hip, sides):
        for pas in (1, 2):                                 # the whole measurement twice, alternating the sides
            t = {"hip": timed(hip, reps)}
            for form, fn in sides.items():
                t[form] = timed(fn, reps)
            lines.append(f"{name:34s} pass {pas}: hip {t['hip']:8.1f} us   " + "   ".join(f"torch {k} {v:8.1f} us ({v / t['hip']:5.2f}x)" for k, v in t.items() if k != "hip"))
            print(lines[-1], flush=True)

    torch.manual_seed(0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), pkg.VectorEnv("CartPole-v1", 64, seed=1, stream=stream.cuda_stream) as env:          # the handle works on torch's stream: one timeline
        env.ResetDevice()
        mods = [torch.nn.Linear(16, 50), torch.nn.ReLU(), torch.nn.Linear(50, 20), torch.nn.ReLU(), torch.nn.Linear(20, 2)]
        pnet = torch.nn.Sequential(*mods).cuda()
        actor = env.Actor(pnet, history=4)
        for count in (actor.Count, 8192):
            for rule in ("sgd", "adadelta", "adam"):
                for clip in (0.0, 0.5):
                    w, g, state = 0.5 * torch.randn(count, device="cuda"), torch.randn(count, device="cuda"), torch.zeros(2, count, device="cuda")
                    kw = dict(hp[rule])

                    def hip(w=w, g=g, state=state, rule=rule, clip=clip, kw=kw):
                        actor.ApplyGradient(w, g, state, rule=rule, step=3, max_grad_norm=clip, **kw)
                    report(f"{rule:8s} count={count:<5d} clip={clip:<3}", 2000, hip, torch_sides(rule, count, clip))
        # a whole minibatch update of the policy: the gradient call, then the step
        m = 1 << 12
        x, act = torch.randn(m, 16, device="cuda"), torch.randint(0, 2, (m,), device="cuda", dtype=torch.int32)
        coef, old = torch.randn(m, device="cuda"), -0.7 + 0.2 * torch.randn(m, device="cuda")
        flat = torch.cat([p.detach().reshape(-1) for p in pnet.parameters()])
        grad, state = torch.empty_like(flat), torch.zeros(2, flat.numel(), device="cuda")

        def gradient():
            actor.PolicyGradient(flat, x, act, coef, logp_old=old, clip=0.2, entropy_coef=0.01, grad=grad)

        def hip_update():
            gradient()
            actor.ApplyGradient(flat, grad, state, rule="adam", step=3, max_grad_norm=0.5, **hp["adam"])

        sides = {}
        for form, kw in (("default", {}), ("fused", {"fused": True})):
            p = torch.nn.Parameter(flat.clone())
            p.grad = grad
            opt = torch.optim.Adam([p], **hp["adam"], **kw)

            def torch_update(p=p, opt=opt):
                gradient()
                torch.nn.utils.clip_grad_norm_([p], 0.5)
                opt.step()
            sides[form] = torch_update
        report("policy update adam clip m=2^12", 1000, hip_update, sides)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/actor_optim_probe.py: ApplyGradient against clip_grad_norm_ + torch.optim step on one flat tensor; HIP events, median of 9 batches\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
