#!/usr/bin/env python3
"""Generates tests/golden/reference_text_facts.json: what the tests need to know about the reference's source text, as data
only, so that they run from the repository alone.  Nothing of the text itself is stored:

  step_digests / machine_digest  SHA-256 of each CartPoleEnv.Step assignment's canonical token stream (and of the reward /
                                 steps_beyond_done machine), as oracle/check_against_reference.py reduces them
  integrator                     the kinematics integrator the text selects
  constants                      the `private const float` initialisers evaluated in binary32
  reset                          Reset()'s steps_beyond_done and the three arguments of random.uniform
  obs_high, action_n             the observation-space bound and the Discrete action count the ctor builds
  discrete_contains              Discrete.Contains(x) evaluated from its text for N in (1, 2, 3, 7), x in [-3, N + 3)

    python tests/golden/make_reference_text_facts.py REFERENCE_ROOT
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import check_against_reference as chk  # noqa: E402
from oracle.evaluate_reference_text import Parser, Value, _strip_comments, _tokens, load_reference, reference_constants  # noqa: E402

OUT = os.path.join(HERE, "reference_text_facts.json")


def digest(tokens):
    return hashlib.sha256(" ".join(tokens).encode()).hexdigest()


def facts(root):
    cs = open(os.path.join(root, chk.REL), encoding="utf-8-sig").read()
    steps, machine, integ = chk.reference_step(cs)
    out = {"step_digests": {v: digest(steps[v]) for v in chk.STEP_VARS}, "machine_digest": digest(machine), "integrator": integ,
           "constants": {k: float(v) for k, v in chk.reference_constants(cs).items()}}
    text = load_reference(root)
    body = text[text.index("public override NDArray Reset()"):]
    body = body[:body.index("return")]
    sbd0 = Parser(_tokens(re.search(r"steps_beyond_done = ([^;]+);", body).group(1)), {}).expr()
    low, high, count = (Parser(_tokens(a), {}).expr() for a in re.search(r"state = random\.uniform\(([^;]*)\);", body).group(1).split(","))
    assert count.t == "int"
    out["reset"] = {"steps_beyond_done": int(sbd0.v), "low": float(low.v), "high": float(high.v), "count": int(count.v)}
    env = reference_constants(text)
    high_v = []
    for a in re.search(r"var high = np\.array\(([^;]*)\);", text).group(1).split(","):
        a = a.strip()
        if a == "float.MaxValue":
            high_v.append(float(np.finfo(np.float32).max))
        else:
            v = Parser(_tokens(a), env).expr()
            assert v.t == "float"
            high_v.append(float(v.v))
    out["obs_high"] = high_v
    out["action_n"] = int(re.search(r"ActionSpace = new Discrete\((\d+)\);", text).group(1))
    dtext = _strip_comments(open(os.path.join(root, "src", "Gym", "Spaces", "Discrete.cs"), encoding="utf-8-sig").read())
    toks = _tokens(re.search(r"public bool Contains\(int x\)\s*\{\s*return ([^;]+);\s*\}", dtext).group(1))
    rows = {"n": [], "x": [], "contains": []}
    for n in (1, 2, 3, 7):
        for x in range(-3, n + 3):
            r = Parser(toks, {"x": Value(x, "int"), "N": Value(n, "int"), "Start": Value(0, "int")}).expr()
            assert r.t == "bool"
            rows["n"].append(n)
            rows["x"].append(x)
            rows["contains"].append(bool(r.v))
    out["discrete_contains"] = rows
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    with open(OUT, "w") as f:
        json.dump(facts(sys.argv[1]), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
