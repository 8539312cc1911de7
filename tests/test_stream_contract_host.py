"""CPU checks of tests/_stream_contract.py: the table against the header's exports, name for name; the `blocks` sentences against the header
and the docstrings, word for word; the gate's calibration arithmetic under a fake timer; and that every index-bearing input of every row, in
every sequence that uses it, is a buffer uploaded before the gate."""
import os
import re

import numpy as np
import pytest

import _stream_contract as sc

pytestmark = pytest.mark.timeout(120)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gymnet_amd.h")
DOCSTRINGS = os.path.join(ROOT, "gym.net_amd", "vector_env.py")


def _declarations():
    """{export: its parameter list} of every `int gymnet_*(...)` the header declares (comments removed first)"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(gymnet_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def device_path_exports(decls):
    """every export whose name ends in _device, and every handle-less export that takes a `void *stream`"""
    return {name for name, params in decls.items()
            if name.endswith("_device") or ("void *stream" in params and "gymnet_vecenv *" not in params and "gymnet_group *" not in params)}


def test_every_device_path_export_is_a_row_or_excluded_with_a_reason():
    decls = _declarations()
    assert len(decls) > 100 and "gymnet_vecenv_step_device" in decls and "gymnet_gae_device" in decls         # the parser sees the header
    want = device_path_exports(decls)
    rows = {r["export"] for r in sc.ROWS.values()}
    assert not rows - set(decls), f"rows name exports the header lacks: {sorted(rows - set(decls))}"
    assert not set(sc.EXCLUDED) - set(decls), f"EXCLUDED names exports the header lacks: {sorted(set(sc.EXCLUDED) - set(decls))}"
    assert not rows & set(sc.EXCLUDED), sorted(rows & set(sc.EXCLUDED))
    missing = want - rows - set(sc.EXCLUDED)
    assert not missing, f"device-path exports with neither a row nor an EXCLUDED entry: {sorted(missing)}"
    assert not (rows | set(sc.EXCLUDED)) - want, f"not device-path exports: {sorted((rows | set(sc.EXCLUDED)) - want)}"
    assert all(isinstance(reason, str) and len(reason) > 20 for reason in sc.EXCLUDED.values())


def test_the_check_fails_when_a_row_is_removed(monkeypatch):
    """what "Done when" asks of this file: a _device export dropped from ROWS without an EXCLUDED entry is seen"""
    rows = dict(sc.ROWS)
    del rows["actor_history_device"]
    monkeypatch.setattr(sc, "ROWS", rows)
    with pytest.raises(AssertionError, match="gymnet_vecenv_actor_history_device"):
        test_every_device_path_export_is_a_row_or_excluded_with_a_reason()


def test_every_row_runs_in_a_sequence_and_is_complete():
    used = {sc.resolve(e)[0]["key"] for v in sc.VARIANTS.values() for e in v["seq"]}
    assert used == set(sc.ROWS), sorted(set(sc.ROWS) - used)
    for r in sc.ROWS.values():
        assert r["kind"] in ("core", "attach", "box", "free") and callable(r["call"])
        assert r["blocks"] is None or isinstance(r["blocks"], str)
        assert r["capturable"] in (True, False), (r["key"], "the committed table holds no probe")
        assert r["capturable"] is False or r["kind"] == "free", (r["key"], "handle calls keep host-side counters: the caller does not capture them")


def _norm(text):
    """one line, the comment prefixes of continuation lines (" * ", "# ") and every run of whitespace removed"""
    return " ".join(re.sub(r"^\s*(\*|#)\s?", " ", text, flags=re.M).split())


def test_blocks_sentences_are_the_documents_own_words():
    norm = _norm
    docs = norm(open(HEADER).read()) + " " + norm(open(DOCSTRINGS).read())
    for r in sc.ROWS.values():
        if r["blocks"] is not None:
            assert norm(r["blocks"]) in docs, (r["key"], r["blocks"])


CAPTURABLE = "capturable (no allocation, copy or synchronise)"


def _comment_before(text, export):
    """the comment block that ends right before the declaration of `export` (nothing but whitespace in between), normalised"""
    m = re.search(r"\bint\s+" + export + r"\s*\(", text)
    assert m, export
    head = text[:m.start()]
    assert head.rstrip().endswith("*/"), (export, "no comment directly before the declaration")
    return _norm(head[head.rindex("/*"):])


def test_the_header_says_what_the_table_says_about_capture():
    """export by export: the comment block directly before the declaration of a handle-less export carries the phrase exactly when its rows
    are capturable; no handle call's own comment carries it, and the device path's opening paragraph forbids capturing them"""
    text = open(HEADER).read()
    by_export = {}
    for r in sc.ROWS.values():
        by_export.setdefault(r["export"], set()).add(r["capturable"])
    for export, verdicts in by_export.items():
        assert len(verdicts) == 1, (export, "rows of one export disagree")
        handle = "gymnet_vecenv_" in export
        m = re.search(r"\bint\s+" + export + r"\s*\(", text)
        directly = text[:m.start()].rstrip().endswith("*/")
        if verdicts == {True}:
            assert not handle and CAPTURABLE in _comment_before(text, export), (export, "its comment does not say that it is capturable")
        else:
            assert handle, (export, "a handle-less export whose rows are not capturable must say why")
            assert not directly or CAPTURABLE not in _comment_before(text, export), (export, "its comment says capturable, the table does not")
    assert {e for e, v in by_export.items() if v == {True}} == {e for e in by_export if "gymnet_vecenv_" not in e}
    path = _norm(text[text.index("---- device-resident path"):text.index("int gymnet_vecenv_reset_device")])
    assert "Handle calls must not be captured by the caller" in path and "are capturable" in path


def test_the_capture_check_sees_a_sentence_that_moved():
    """the phrase deleted at gymnet_push_obs_device and duplicated elsewhere is seen"""
    text = open(HEADER).read()
    assert CAPTURABLE in _comment_before(text, "gymnet_push_obs_device")
    start = text.rindex("/*", 0, text.index("int gymnet_push_obs_device"))
    moved = text[:start] + text[start:].replace("capturable (no allocation, copy or synchronise)", "ordered", 1)
    moved = moved.replace("stream-ordered, non-blocking, capturable", "stream-ordered, non-blocking, capturable (no allocation, copy or synchronise), capturable", 1)
    assert moved.count(CAPTURABLE) >= text.count(CAPTURABLE) - 1 and CAPTURABLE not in _comment_before(moved, "gymnet_push_obs_device")


def test_index_bearing_inputs_are_uploaded_before_the_gate():
    for name, v in sc.VARIANTS.items():
        spec = sc.buffers(v["kind"], "f64" if v["kw"].get("dtype") is np.float64 else "f32")
        for entry in v["seq"]:
            r, a, outs, idx = sc.resolve(entry)
            for buf in sc.output_names(outs):
                assert spec[buf][2] == "out", (name, r["key"], buf)
            for buf in idx:
                assert spec[buf][2] == "static", (name, r["key"], buf)
        # and the other way round: a buffer of indices (int64), a mask (uint8 input) or weights is never a value input
        for buf, (_, dt, role, _) in spec.items():
            if role == "value":
                assert dt != "i64" and "mask" not in buf and "weights" not in buf and "rows" not in buf, (name, buf)


def test_the_gate_length():
    assert sc.gate_ms(0.0) == 50.0 and sc.gate_ms(2.4) == 50.0 and sc.gate_ms(2.5) == 50.0        # the floor
    assert sc.gate_ms(5.0) == 100.0 and sc.gate_ms(19.99) == pytest.approx(399.8)
    assert sc.gate_ms(20.0) == 400.0 and sc.gate_ms(1e6) == 400.0                                    # the cap


class FakeTimer:
    def __init__(self, per_ms, overhead_ms=0.0, lie=None):
        self.per_ms, self.overhead_ms, self.lie, self.calls = per_ms, overhead_ms, lie or {}, []

    def __call__(self, units):
        self.calls.append(units)
        return self.lie.get(units, units / self.per_ms + self.overhead_ms)


def test_the_rate_is_derived_from_two_trials():
    sleep, chain = FakeTimer(100_000.0), FakeTimer(2.0)
    mode, rate, trials = sc.calibrate(sleep, chain)
    assert mode == "sleep" and rate == pytest.approx(100_000.0) and sleep.calls == list(sc.TRIAL_CYCLES) and chain.calls == []
    assert sc.units_for(rate, 50.0) == 5_000_000 and sc.units_for(rate, 0.0) == 1
    # a launch overhead that does not move the two rates apart by 2 x is tolerated, and the longer trial's rate is taken
    mode, rate, _ = sc.calibrate(FakeTimer(100_000.0, overhead_ms=2.0), chain)
    assert mode == "sleep" and rate == pytest.approx(sc.TRIAL_CYCLES[1] / (sc.TRIAL_CYCLES[1] / 100_000.0 + 2.0))
    assert sc.derive_rate([(10, 1.0), (40, 2.0)]) == 20.0 and sc.derive_rate([(10, 1.0), (40, 1.99)]) is None      # exactly 2 x is still one rate


def test_trials_that_disagree_fall_back_to_the_chain():
    for lie in ({sc.TRIAL_CYCLES[0]: 0.0}, {sc.TRIAL_CYCLES[1]: -1.0}, {sc.TRIAL_CYCLES[0]: 100.0}, {sc.TRIAL_CYCLES[1]: sc.TRIAL_CYCLES[1] / 100_000.0 / 4.1}):
        chain = FakeTimer(2.0)
        mode, rate, trials = sc.calibrate(FakeTimer(100_000.0, lie=lie), chain)
        assert mode == "chain" and rate == pytest.approx(2.0) and chain.calls == list(sc.TRIAL_OPS) and len(trials) == 4
        assert sc.units_for(rate, 400.0) == 800
    with pytest.raises(RuntimeError, match="cannot be calibrated"):
        sc.calibrate(FakeTimer(100_000.0, lie={sc.TRIAL_CYCLES[0]: 0.0}), FakeTimer(2.0, lie={sc.TRIAL_OPS[1]: 0.0}))


def test_shapes_are_the_ones_the_forms_tables_name():
    import _advantage_forms as aforms
    import _advantage_twin as atwin
    assert sc.gae_shapes() == ((2 * aforms.U[1] + 1, 1030), (2 * aforms.U[4] + 1, min(atwin.WIDE_NS)))
    assert sc.gae_shapes()[1][1] >= aforms.NARROW_BELOW and sc.gae_shapes()[0][1] < aforms.NARROW_BELOW            # both forms are reached
    (o, s, t, n, m), gathered = sc.inputs_shapes()
    assert m == 0 and gathered[4] > 0 and n > 4 * 256                                                                # dense and gathered, two blocks
    assert sc.N == 2 * 4 * 256 + 3 and sc.NPAD % 4 == 0 and sc.NPAD >= sc.N
    assert sc.SAMPLER_COUNTS == ((37, 0), (1027, 2 ** 32 + 5))
