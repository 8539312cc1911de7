"""GPU checks of WHERE and WHEN the device path runs (tests/_stream_contract.py holds the table, the gate and the runner): every *_device
call and every handle-less export, on a caller's torch stream that a gate keeps busy while the calls are issued.

  ordered       a handle on the caller's stream under the gate, no synchronise between calls, against a second handle of the same seed on the
                library's own stream with a synchronise after every call (the arrangement the rest of the suite holds to the twins and the
                oracle): every output, the state, done bytes, tick, counters, attachment state and episode records (as sets), bit for bit,
                on a cold run (first-use allocations under the gate) and a warm one
  non-blocking  the warm run's readings: after every call the stream still has the gate in it (query() is False) and the host clock stands
                below half the gate — a reading taken later than that is void and FAILS
  two streams   two handles (two sets of handle-less calls) on two streams, gated independently and issued alternately, cold and warm, each
                pass equal to its solo run and the warm pass issued entirely while both gates held: no hidden process-wide scratch
  capturable    the handle-less rows captured into one linear torch.cuda.graph on the caller's stream and replayed three times over inputs
                rewritten in place, against _advantage_twin, _rollout_inputs_twin and _space_sampling_ref each time
  the yardstick the same runner with the copy of one value input issued on another stream behind a longer gate: the comparison must fail

Shapes (_stream_contract.py): 2051 lanes (two workgroups of 256 threads x 4 lanes and a tail of 3), T = 5, ring 2; gae at 1030 lanes and at
the smallest wide count with T = 2U + 1; the smallest dense and gathered rollout-input shapes that span two blocks; samplers at 37 elements
and at 1027 from lane offset 2^32 + 5.  Every run prints its calibration, gate and per-call readings (pytest -s shows them)."""
import ctypes as C
import time

import numpy as np
import pytest

import _advantage_twin as gtwin
import _rollout_inputs_twin as itwin
import _space_sampling_ref as R
import _stream_contract as sc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

HANDLE_VARIANTS = [v for v in sc.VARIANTS if v != "free"]
_outcomes = {}


def _outcome(pkg, variant):
    """reference (cold, warm) and gated (cold, warm) runs of one variant, made once and shared by the ordered and the non-blocking test"""
    if variant in _outcomes:
        return _outcomes[variant]
    import torch
    S = sc.streams(torch)[0]
    seq = sc.VARIANTS[variant]["seq"]
    ref, got = sc.Ctx(pkg, torch, variant, None), sc.Ctx(pkg, torch, variant, S)
    out = {"runs": [], "host": ref.host}
    try:
        gate = sc.gate_for(torch, S)
        sc.record(f"[{variant}] gate calibration: {gate.mode}, {gate.rate:.1f} units/ms, trials {[(u, round(ms, 3)) for u, ms in gate.trials]}")
        for temperature in ("cold", "warm"):
            want, _, ref_ms = sc.run(ref, seq)
            length = sc.gate_ms(ref_ms)
            have, readings, host_ms = sc.run_gated(got, seq, length)
            out["runs"].append({"temperature": temperature, "want": want, "have": have, "readings": readings, "gate_ms": length, "ref_ms": ref_ms, "host_ms": host_ms})
            sc.record(f"[{variant}] {temperature}: reference host time {ref_ms:.2f} ms -> gate {length:.1f} ms; the gated sequence was issued in {host_ms:.2f} ms")
            for key, done, ms in readings:
                sc.record(f"[{variant}] {temperature}   {key:44s} query={done!s:5s} host={ms:8.3f} ms")
    finally:
        ref.close()
        got.close()
    _outcomes[variant] = out
    return out


@pytest.mark.parametrize("variant", HANDLE_VARIANTS)
def test_ordered_on_the_callers_stream(gpu_pkg, variant):
    out = _outcome(gpu_pkg, variant)
    for run in out["runs"]:
        bad = sc.differences(run["have"], run["want"])
        assert not bad, (variant, run["temperature"], f"{len(bad)} of {len(run['want'])} outputs differ from the synchronised run", bad[:12])
        assert len(run["want"]) >= len(sc.VARIANTS[variant]["seq"]) // 2                                  # the comparison is not empty
    # the sequence did something: episodes ended, and the two runs of a handle are not one another's copy
    assert any(k.startswith("after: ") for k in out["runs"][0]["want"])
    assert sc.differences(out["runs"][0]["want"], out["runs"][1]["want"])


@pytest.mark.parametrize("variant", HANDLE_VARIANTS + ["free"])
def test_non_blocking_under_the_gate(gpu_pkg, variant):
    out = _outcome(gpu_pkg, variant)
    warm = out["runs"][1]
    half = warm["gate_ms"] / 2.0
    blocked, void = [], []
    for key, done, ms in warm["readings"]:
        row = sc.ROWS[key]
        if row["blocks"] is not None:
            sc.record(f"[{variant}] {key} is documented to block ({row['blocks']!r}): query={done} at {ms:.3f} ms")
            continue
        if ms >= half:
            void.append((key, round(ms, 3)))
        elif done:
            blocked.append((key, round(ms, 3)))
    assert not void, (f"{variant}: readings at or past half the {warm['gate_ms']:.1f} ms gate are void — the call before blocked, or the host was too slow "
                      f"for this gate (reference host time {warm['ref_ms']:.2f} ms)", void[:8])
    assert not blocked, (f"{variant}: the stream had drained after these calls, within {half:.1f} ms of a {warm['gate_ms']:.1f} ms gate", blocked[:8])


def test_the_handle_less_rows_are_ordered(gpu_pkg):
    out = _outcome(gpu_pkg, "free")
    for run in out["runs"]:
        bad = sc.differences(run["have"], run["want"])
        assert not bad, (run["temperature"], bad[:12])
    # ... and the synchronised run itself has the twins' bits (gae and the rollout inputs; the samplers are held in the capture test)
    want = out["runs"][0]["want"]
    ctx_rows = out["host"]                                            # the static inputs the run uploaded (the gathered rows among them)
    for k, (steps, n) in enumerate(sc.gae_shapes()):
        c = gtwin.case(steps, n, 3)
        adv, ret = gtwin.gae(c["r"], c["d"], c["v"][:steps], c["v"][steps], c["boot"])
        for name, twin in ((f"g{k}_adv", adv), (f"g{k}_ret", ret)):
            label = [key for key in want if key.endswith(name)][0]
            assert np.array_equal(want[label], twin.view(np.uint8).reshape(-1)), name
    for k, (obs, hist, steps, n, m) in enumerate(sc.inputs_shapes()):
        c = itwin.case(obs, hist, steps, n, "bernoulli", seed=3)
        x = itwin.gathered(c["x"], ctx_rows[f"i{k}_rows"]) if m else c["x"]
        for name, twin in ((f"i{k}_x", x), (f"i{k}_hout", c["history_out"])):
            label = [key for key in want if key.endswith(name)][0]
            assert np.array_equal(want[label], np.ascontiguousarray(twin).view(np.uint8).reshape(-1)), name


@pytest.mark.parametrize("variant", ["core-f32", "attach-f32", "free"])
def test_two_streams_interleaved_equal_their_solo_runs(gpu_pkg, variant):
    """Two passes, as in the ordered test: the cold one does the first-use allocations (a handle's first rollout with episode records drains
    its stream), the warm one issues EVERY call of both sequences while both gates are still in their streams — which its readings must
    show.  Each pass's gate is gate_ms() of the slower of the two solo runs of that pass; both passes equal their solo runs."""
    import torch
    S = sc.streams(torch)
    seq = sc.VARIANTS[variant]["seq"]
    seeds = (3, 4)
    refs, ctxs = [], []
    try:
        refs = [sc.Ctx(gpu_pkg, torch, variant, None, seed=seed) for seed in seeds]
        ctxs = [sc.Ctx(gpu_pkg, torch, variant, S[j], seed=seed) for j, seed in enumerate(seeds)]
        for temperature in ("cold", "warm"):
            solos = [sc.run(ref, seq) for ref in refs]
            assert sc.differences(solos[0][0], solos[1][0])                                              # the two have different inputs
            ref_ms = max(solo[2] for solo in solos)
            length = sc.gate_ms(ref_ms)
            t0 = time.perf_counter()
            results, readings = sc.run_interleaved(ctxs, [seq, seq], length)
            sc.record(f"[two streams, {variant}] {temperature}: reference host time {ref_ms:.2f} ms -> gates {length:.1f} ms; {len(seq)} calls on each of "
                      f"two streams, drained after {(time.perf_counter() - t0) * 1e3:.1f} ms")
            for j in range(2):
                bad = sc.differences(results[j], solos[j][0])
                assert not bad, (variant, temperature, f"stream {j}", f"{len(bad)} outputs differ from the solo run", bad[:12])
                late = [(key, done, round(ms, 3)) for key, done, ms in readings[j] if sc.ROWS[key]["blocks"] is None and (done or ms >= length / 2.0)]
                sc.record(f"[two streams, {variant}] {temperature}, stream {j}: last reading {readings[j][-1][2]:.3f} ms; readings with a drained stream or "
                          f"past half the gate: {late[:6]}")
                if temperature == "warm":
                    assert not late, (f"{variant}, stream {j}: these calls were not issued while both {length:.1f} ms gates held their streams", late[:8])
    finally:
        for c in refs + ctxs:
            c.close()


def test_the_yardstick_sees_a_misplaced_copy(gpu_pkg):
    """The runner itself, held to a planted mis-ordering that no library call takes part in: the torch copy that writes gae's rewards is
    issued on ANOTHER torch stream behind a gate twice as long, with no event, so the kernel on the caller's stream reads the zero-filled
    buffer.  The comparison with the synchronised run must fail, on exactly the outputs computed from that input; with the copy in its
    place the same runner passes."""
    import torch
    S = sc.streams(torch)
    seq = ["gae_device"]
    ref, got = sc.Ctx(gpu_pkg, torch, "free", None), sc.Ctx(gpu_pkg, torch, "free", S[0])
    want, _, ref_ms = sc.run(ref, seq)
    length = min(sc.gate_ms(ref_ms), sc.GATE_CAP_MS / 2.0)
    have, readings, _ = sc.run_gated(got, seq, length)
    assert not sc.differences(have, want) and readings[0][1] is False
    want2 = sc.run(ref, seq)[0]
    have2 = sc.run_gated(got, seq, length, misplace=("g0_r", S[2], 2.0 * length))[0]
    bad = sc.differences(have2, want2)
    sc.record(f"[yardstick] a copy misplaced behind a {2.0 * length:.0f} ms gate on another stream: {bad}")
    assert sorted(k.split()[-1] for k in bad) == ["g0_adv", "g0_ret"], bad
    # what the kernel read was the zero-filled buffer: its outputs are those of all-zero rewards
    c = gtwin.case(*sc.gae_shapes()[0], 3)
    steps = sc.gae_shapes()[0][0]
    adv0, _ = gtwin.gae(np.zeros_like(c["r"]), c["d"], c["v"][:steps], c["v"][steps], c["boot"])
    label = [k for k in have2 if k.endswith("g0_adv")][0]
    assert np.array_equal(have2[label], adv0.view(np.uint8).reshape(-1))


# ---- capture ---------------------------------------------------------------------------------------------------------------------------------
def _rewrite(ctx, torch, replay):
    """new values for every device input of the handle-less rows, written IN PLACE (the graph holds the addresses), outputs poisoned"""
    rng = np.random.default_rng(100 + replay)
    new = {}
    for k, (steps, n) in enumerate(sc.gae_shapes()):
        c = gtwin.case(steps, n, 50 + replay)
        new.update({f"g{k}_r": c["r"], f"g{k}_d": c["d"], f"g{k}_v": c["v"], f"g{k}_boot": c["boot"]})
    for k, (obs, hist, steps, n, m) in enumerate(sc.inputs_shapes()):
        c = itwin.case(obs, hist, steps, n, "runs", seed=50 + replay)
        new.update({f"i{k}_obs": c["rec_obs"], f"i{k}_done": c["rec_done"], f"i{k}_h0": c["history0"]})
        if m:
            new[f"i{k}_rows"] = rng.integers(0, steps * n, m).astype(np.int64)
    for k, (count, _) in enumerate(sc.SAMPLER_COUNTS):
        new[f"smask{k}"] = rng.integers(0, 2, (count, 5)).astype(np.uint8)
    new["box_low"] = np.array([-1.0 - replay, -np.inf, -np.inf], np.float32)
    new["box_high"] = np.array([2.0 + replay, np.inf, 5.0 + replay], np.float32)
    new["peer_src"] = itwin.random_bits(ctx.spec["peer_src"][0], rng)
    for name, a in new.items():
        ctx.b[name].copy_(torch.from_numpy(np.array(a)))
    for name, (_, _, role, _) in ctx.spec.items():
        if role == "out":
            sc._poison(torch, ctx.b[name])
    torch.cuda.synchronize()
    return new


def _check_replay(ctx, oracle, new, seed, tick):
    got = {name: t.cpu().numpy() for name, t in ctx.b.items() if ctx.spec[name][2] == "out"}
    bits = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    for k, (steps, n) in enumerate(sc.gae_shapes()):
        adv, ret = gtwin.gae(new[f"g{k}_r"], new[f"g{k}_d"], new[f"g{k}_v"][:steps], new[f"g{k}_v"][steps], new[f"g{k}_boot"])
        assert np.array_equal(bits(got[f"g{k}_adv"]), bits(adv)) and np.array_equal(bits(got[f"g{k}_ret"]), bits(ret)), ("gae_device", k)
    for k, (obs, hist, steps, n, m) in enumerate(sc.inputs_shapes()):
        x, hout = itwin.inputs(new[f"i{k}_obs"], new[f"i{k}_done"], new[f"i{k}_h0"])
        want = itwin.gathered(x, new[f"i{k}_rows"]) if m else x
        assert np.array_equal(bits(got[f"i{k}_x"]), bits(want)) and np.array_equal(bits(got[f"i{k}_hout"]), bits(hout)), ("rollout_inputs_device", k)
    for k, (count, off) in enumerate(sc.SAMPLER_COUNTS):
        a, b = R.words(oracle, seed, off, tick, count)
        assert np.array_equal(got[f"sd{k}"], R.discrete_sample(a, 37, 10)), ("sample_discrete_device", k)
        assert np.array_equal(got[f"sm{k}"], R.discrete_sample_masked(a, new[f"smask{k}"], 5, 3)), ("sample_discrete_masked_device", k)
        assert np.array_equal(bits(got[f"sb{k}"]), bits(oracle.box_uniform_sample(seed, off, tick, -2.0, 2.0, count))), ("sample_box_device", k)
        rows = got[f"se{k}"]
        assert np.isfinite(rows).all()
        for e, (low, high) in enumerate(zip(new["box_low"], new["box_high"])):
            ea, eb = R.words(oracle, seed, off, tick, count, element=e)
            ref = R.box_sample(low, high, ea, eb)
            err = np.abs(rows[:, e].astype(np.float64) - ref)
            if np.isfinite(low) and np.isfinite(high):
                want = oracle.box_uniform_sample(R.element_key(seed, e), off, tick, float(low), float(high), count)
                assert np.array_equal(bits(rows[:, e]), bits(want)), ("sample_box_elementwise_device", k, e)
            elif not np.isfinite(low) and not np.isfinite(high):
                assert (err <= R.UNBOUNDED_BOUND).all(), ("sample_box_elementwise_device", k, e, err.max())
            else:
                assert (err <= R.one_sided_bound(ea, ref)).all(), ("sample_box_elementwise_device", k, e, err.max())
    assert np.array_equal(bits(got["peer_dst"]), bits(new["peer_src"])), "push_obs_device"


def test_the_handle_less_rows_are_captured_and_replayed(gpu_pkg, oracle):
    """one linear chain of every capturable row on the caller's stream, captured with the default capture_error_mode ("global": any
    allocation, copy or synchronise on any thread would end the capture with an error), replayed three times"""
    import torch
    S = sc.streams(torch)[0]
    seq = sc.FREE_SEQUENCE
    assert all(sc.ROWS[sc.resolve(e)[0]["key"]]["capturable"] is True for e in seq)
    ctx = sc.Ctx(gpu_pkg, torch, "free", S, seed=9)
    ctx.round = 21                                                     # the samplers' tick: a kernel argument, frozen at capture
    sc.prepare(ctx)
    with torch.cuda.stream(S):                                         # everything is allocated and every kernel has run once before the capture
        sc.stage(ctx, seq)
        for entry in seq:
            r, a, _, _ = sc.resolve(entry)
            r["call"](ctx, a)
    S.synchronize()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    t0 = time.perf_counter()
    with torch.cuda.graph(g, stream=S):
        for entry in seq:
            r, a, _, _ = sc.resolve(entry)
            r["call"](ctx, a)
    sc.record(f"[capture] {len(seq)} handle-less calls captured into one graph in {(time.perf_counter() - t0) * 1e3:.1f} ms: "
              + ", ".join(sorted({sc.resolve(e)[0]['export'] for e in seq})))
    for replay in range(3):
        new = _rewrite(ctx, torch, replay)
        with torch.cuda.stream(S):
            g.replay()
        S.synchronize()
        _check_replay(ctx, oracle, new, 9, 21)
        sc.record(f"[capture] replay {replay}: every output has the reference's bits for this replay's inputs")
