"""Edge-state tables of Pendulum, MountainCar and Acrobot, and the Acrobot domain search (helper module, not a conftest).

A table is a deterministic list of named rows: a float32 state, an action, what the row probes, and the facts the step's result must
satisfy — derived by hand from the upstream algorithm, without running either oracle.  tests/test_env_edge_tables_host.py holds both
oracles (float64 upstream semantics, float32 kernel semantics) to the facts and to each other; tests/test_gpu_env_edges.py tiles
the tables into batches and holds every kernel form to the twin bit for bit, to the facts and to the float64 bars.

Facts (value literals are cast to the dtype of the oracle under test: -1.2 is -1.2f for the twin and the double -1.2 for float64):
  ("eq", k, v)        component k of the new state equals v exactly         ("nan", k)   component k is NaN
  ("le", k, v)        |component k| <= v                                    ("gt", k, v) |component k| > v
  ("pos", k) / ("neg", k)   component k is > 0 / < 0                        ("finite",)  every component, and the reward, is finite
  ("done", b)         the termination flag                                 ("reward", v) / ("reward_nan",) / ("reward_in", lo, hi)
  ("same_as", name)   state, reward and flag equal those of row `name` bit for bit (an action beyond a bound acts like the bound)
  ("twin", *fact)     a fact of the kernel's evaluation order only (held against the twin and the GPU, not against float64)
Row flags: finite — no NaN / inf anywhere in the input; upstream — the row lies where the kernel's contract promises upstream's
result (inside the env's state bounds, or outside them where nothing but the bounds was assumed), so it is compared with float64;
facts of a row that is not `upstream` are held against the twin only.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

f32 = np.float32
INF, NAN = float("inf"), float("nan")
PI32 = f32(np.pi)                                   # 3.14159274: the kernels' PI, one half-ulp ABOVE pi
MV1, MV2 = f32(4.0) * PI32, f32(9.0) * PI32         # Acrobot's velocity clamps as the kernel forms them (4.0f * PI, 9.0f * PI)
TWO_PI32 = f32(2.0) * PI32


def up(x, k=1):
    """x moved |k| float32 ulps towards +inf (k > 0) or -inf (k < 0)."""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(INF if k > 0 else -INF), dtype=f32)
    return x


def _row(name, state, action, probes, facts, upstream=True):
    state = tuple(f32(v) for v in state)
    finite = bool(np.isfinite(np.array(state, f32)).all()) and (isinstance(action, (int, np.integer)) or bool(np.isfinite(f32(action))))
    return dict(name=name, state=state, action=action, probes=probes, facts=tuple(facts), finite=finite, upstream=upstream and finite)


# ---------------------------------------------------------------------------------------------------------------------------------
# Pendulum-v1: state (theta, theta_dot), action = torque (float32).  u = clip(a, -2, 2); cost = norm(theta)^2 + 0.1 thdot^2 + 0.001 u^2;
# thdot' = clip(thdot + (15 sin theta + 3 u) 0.05, -8, 8); theta' = theta + 0.05 thdot'; never done.
# ---------------------------------------------------------------------------------------------------------------------------------
PENDULUM_COST_MAX = float(np.pi) ** 2 + 0.1 * 100.0 ** 2 + 0.001 * 4.0      # the largest cost of a finite row (|thdot| <= 100 in this table)


def pendulum_table():
    rows = []
    never = ("done", False)
    fin = (("finite",), never, ("le", 1, 8.0), ("reward_in", -PENDULUM_COST_MAX * 1.001, 0.0))
    # --- torque
    base = (1.0, 0.5)
    rows.append(_row("torque=+2", base, 2.0, "upper torque bound itself: not clamped", fin))
    rows.append(_row("torque=-2", base, -2.0, "lower torque bound itself: not clamped", fin))
    rows.append(_row("torque=+2-1ulp", base, up(2.0, -1), "one ulp inside the upper bound", fin))
    rows.append(_row("torque=+2+1ulp", base, up(2.0, 1), "one ulp outside the upper bound: clamped", fin + (("same_as", "torque=+2"),)))
    rows.append(_row("torque=-2+1ulp", base, up(-2.0, 1), "one ulp inside the lower bound", fin))
    rows.append(_row("torque=-2-1ulp", base, up(-2.0, -1), "one ulp outside the lower bound: clamped", fin + (("same_as", "torque=-2"),)))
    rows.append(_row("torque=+50", base, 50.0, "far beyond: clamped", fin + (("same_as", "torque=+2"),)))
    rows.append(_row("torque=-50", base, -50.0, "far beyond: clamped", fin + (("same_as", "torque=-2"),)))
    rows.append(_row("torque=+inf", base, INF, "infinite torque clamps to +2 (inf > 2)", (never, ("le", 1, 8.0), ("same_as", "torque=+2"))))
    rows.append(_row("torque=-inf", base, -INF, "infinite torque clamps to -2", (never, ("le", 1, 8.0), ("same_as", "torque=-2"))))
    rows.append(_row("torque=nan", base, NAN, "NaN passes both compares of the clamp: it reaches the cost and the velocity",
                     (never, ("nan", 0), ("nan", 1), ("reward_nan",))))
    rows.append(_row("torque=-0", base, -0.0, "negative zero torque", fin + (("same_as", "torque=+0"),)))
    rows.append(_row("torque=+0", base, 0.0, "zero torque (the partner of torque=-0)", fin))
    # --- theta_dot at and beyond its clamp
    rows.append(_row("thdot=+8,accelerating", (0.3, 8.0), 0.0, "8 + 0.75 sin(0.3) > 8: upper clamp", fin + (("eq", 1, 8.0),)))
    rows.append(_row("thdot=-8,accelerating", (-0.3, -8.0), 0.0, "lower clamp", fin + (("eq", 1, -8.0),)))
    rows.append(_row("thdot=+8,braking", (-0.3, 8.0), -2.0, "8 - 0.75 sin(0.3) - 0.3 < 8: no clamp", fin + (("pos", 1),)))
    rows.append(_row("thdot=+100", (0.3, 100.0), 0.0, "beyond the clamp (SetState)", fin + (("eq", 1, 8.0),)))
    rows.append(_row("thdot=-100", (0.3, -100.0), 0.0, "beyond the clamp (SetState)", fin + (("eq", 1, -8.0),)))
    rows.append(_row("thdot lands on +8", (0.0, 8.0), 0.0, "sin 0 = 0 and u = 0: the new velocity is 8 exactly, unclamped", fin + (("eq", 1, 8.0),)))
    rows.append(_row("thdot lands on -8", (0.0, -8.0), -0.0, "the new velocity is -8 exactly, unclamped", fin + (("eq", 1, -8.0),)))
    # --- theta near multiples of 2 pi (the normalisation's floored modulus), both signs
    for sgn, tag in ((1, "+"), (-1, "-")):
        for d in (-1, 0, 1):
            rows.append(_row(f"theta={tag}pi{d:+d}ulp", (up(sgn * PI32, d), 0.25), 0.5, "theta + pi next to 0 / 2 pi", fin))
    for k in (1, 7, 1000, 10000):
        for sgn, tag in ((1, "+"), (-1, "-")):
            for d in (-3, -1, 0, 1, 3):
                rows.append(_row(f"theta={tag}2pi*{k}{d:+d}ulp", (up(f32(sgn * 2.0 * np.pi * k), d), -0.5), -1.0,
                                 "the neighbourhood of a multiple of 2 pi: a truncated quotient off by one shows here", fin))
    # --- very large theta: the switch of sincos_f32 to the device library, the fallback of fmod_2pi, and beyond
    big = f32(65536.0)
    fb = f32(4194304.0) * TWO_PI32                           # fmod_2pi: !(|a| < 2^22 * 2 pi) takes fmodf
    for sgn, tag in ((1, "+"), (-1, "-")):
        for d in (-1, 0, 1):
            rows.append(_row(f"theta={tag}65536{d:+d}ulp", (up(sgn * big, d), 1.0), 1.0, "sincos_f32 switches to the library above 65536", fin))
            rows.append(_row(f"theta={tag}2^22*2pi{d:+d}ulp", (up(sgn * fb, d), 1.0), 1.0, "fmod_2pi falls back to fmodf from here on", fin))
        rows.append(_row(f"theta={tag}1e30", (sgn * 1e30, 1.0), 1.0, "|thdot' dt| <= 0.4 is far below an ulp of 1e30: theta stays",
                         fin + (("eq", 0, sgn * float(f32(1e30))),)))
        rows.append(_row(f"theta={tag}inf", (sgn * INF, 1.0), 1.0, "sin(inf) and fmod(inf) are NaN",
                         (never, ("nan", 0), ("nan", 1), ("reward_nan",))))
    rows.append(_row("theta=nan", (NAN, 1.0), 1.0, "NaN angle", (never, ("nan", 0), ("nan", 1), ("reward_nan",))))
    rows.append(_row("thdot=nan", (1.0, NAN), 1.0, "NaN velocity passes the clamp", (never, ("nan", 0), ("nan", 1), ("reward_nan",))))
    rows.append(_row("thdot=+inf", (1.0, INF), 1.0, "clamped to 8, so theta' is finite; the cost is infinite",
                     (never, ("eq", 1, 8.0), ("reward", -INF))))
    rows.append(_row("thdot=-inf", (1.0, -INF), 1.0, "clamped to -8; the cost is infinite", (never, ("eq", 1, -8.0), ("reward", -INF))))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# MountainCar-v0: state (p, v), action in {0, 1, 2} (unvalidated: any int).  v' = clip(v + (a - 1) 0.001 - 0.0025 cos 3p, +-0.07);
# p' = clip(p + v', -1.2, 0.6); p' == -1.2 and v' < 0 -> v' = 0; done = p' >= 0.5 and v' >= 0; reward -1.
# At p = -1.2 the slope term is -0.0025 cos(-3.6) = +0.002242; at p = 0.5 it is -0.0025 cos(1.5) = -0.000177.
# ---------------------------------------------------------------------------------------------------------------------------------
def mountaincar_table():
    rows = []
    rw = ("reward", -1.0)
    fin = (("finite",), rw, ("le", 1, 0.07), ("le", 0, 1.2))
    wall = fin + (("eq", 0, -1.2), ("eq", 1, 0.0), ("done", False))
    L = f32(-1.2)
    # --- left wall
    rows.append(_row("wall,v<0", (L, -0.01), 0, "-0.01 - 0.001 + 0.00224 < 0: pushed into the wall, the velocity is zeroed", wall))
    rows.append(_row("wall,v=+0,a=0", (L, 0.0), 0, "0 - 0.001 + 0.00224 > 0: leaves the wall", fin + (("pos", 1), ("done", False))))
    rows.append(_row("wall,v=-0,a=0", (L, -0.0), 0, "the same from negative zero", fin + (("same_as", "wall,v=+0,a=0"),)))
    rows.append(_row("wall,v>0", (L, 0.01), 2, "moving right off the wall", fin + (("pos", 1), ("done", False))))
    rows.append(_row("wall,v=-0.07", (L, -0.07), 0, "at the lower velocity clamp into the wall", wall))
    rows.append(_row("crosses wall from -1.19", (-1.19, -0.05), 0, "p + v' = -1.2388 crosses -1.2", wall))
    rows.append(_row("crosses wall from -1.2+1ulp", (up(L, 1), -0.004), 0, "-0.004 - 0.001 + 0.00224 = -0.00276: crosses by a hair's start", wall))
    rows.append(_row("stops short of wall", (-1.15, -0.04), 1, "p + v' = -1.1878 stays right of the wall", fin + (("neg", 1), ("done", False))))
    rows.append(_row("left of the wall", (-1.5, -0.01), 1, "p beyond the bound (SetState): clamped to the wall", wall))
    # --- right clamp
    rows.append(_row("right clamp", (0.59, 0.07), 2, "p + v' = 0.66 > 0.6", fin + (("eq", 0, 0.6), ("eq", 1, 0.07), ("done", True))))
    rows.append(_row("right of the clamp", (0.9, 0.01), 1, "p beyond the bound (SetState)", (("finite",), rw, ("eq", 0, 0.6), ("pos", 1), ("done", True))))
    # --- goal: 0.5 and one ulp below, v = +0, -0, -tiny; a = 2 gives v' = v + 0.000823 > 0 (done), a = 1 gives v' < 0 (not done)
    tiny = -float(np.finfo(f32).tiny)
    for pname, p in (("0.5", f32(0.5)), ("0.5-1ulp", up(0.5, -1))):
        for vname, v in (("+0", 0.0), ("-0", -0.0), ("-tiny", tiny)):
            rows.append(_row(f"goal,p={pname},v={vname},a=2", (p, v), 2, "crosses the flag moving right", fin + (("pos", 1), ("done", True))))
            rows.append(_row(f"goal,p={pname},v={vname},a=1", (p, v), 1, "the slope alone pulls it back: v' < 0, and p' < 0.5",
                             fin + (("neg", 1), ("done", False))))
    rows.append(_row("past the flag moving left", (0.55, -0.01), 0, "p' >= 0.5 but v' < 0: not done", fin + (("neg", 1), ("done", False))))
    # --- velocity at and beyond its clamp
    rows.append(_row("v=+0.07,a=2", (-0.5, 0.07), 2, "0.07 + 0.001 - 0.000177 > 0.07: upper clamp", fin + (("eq", 1, 0.07), ("done", False))))
    rows.append(_row("v=-0.07,a=0", (-0.5, -0.07), 0, "lower clamp", fin + (("eq", 1, -0.07), ("done", False))))
    rows.append(_row("v=+1", (-0.5, 1.0), 1, "beyond the clamp (SetState)", fin + (("eq", 1, 0.07), ("done", False))))
    rows.append(_row("v=-1", (-0.5, -1.0), 1, "beyond the clamp (SetState)", fin + (("eq", 1, -0.07), ("done", False))))
    # --- actions outside Discrete(3), unvalidated: (a - 1) * 0.001
    rows.append(_row("a=-1", (-0.5, 0.0), -1, "force -0.002", fin + (("neg", 1), ("done", False))))
    rows.append(_row("a=3", (-0.5, 0.0), 3, "force +0.002", fin + (("pos", 1), ("done", False))))
    rows.append(_row("a=7", (-0.5, 0.0), 7, "force +0.006", fin + (("pos", 1), ("done", False))))
    # --- non-finite state components
    allnan = (rw, ("nan", 0), ("nan", 1), ("done", False))
    rows.append(_row("p=nan", (NAN, 0.01), 1, "cos(NaN): everything NaN, every compare false", allnan))
    rows.append(_row("p=+inf", (INF, 0.01), 1, "cos(inf) = NaN", allnan))
    rows.append(_row("p=-inf", (-INF, 0.01), 1, "cos(-inf) = NaN", allnan))
    rows.append(_row("v=nan", (-0.5, NAN), 1, "NaN passes both clamps", allnan))
    rows.append(_row("v=+inf", (-0.5, INF), 1, "clamped to 0.07: finite again", (rw, ("eq", 1, 0.07), ("finite",), ("done", False))))
    rows.append(_row("v=-inf", (-0.5, -INF), 1, "clamped to -0.07: finite again", (rw, ("eq", 1, -0.07), ("finite",), ("done", False))))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# Acrobot-v1: state (th1, th2, dth1, dth2), action in {0, 1, 2}: torque a - 1.  One RK4 step of 0.2 s, angles wrapped to [-pi, pi],
# velocities clamped to +-4 pi / +-9 pi, done = -cos th1' - cos(th1' + th2') > 1, reward 0 if done else -1.
# ---------------------------------------------------------------------------------------------------------------------------------
# The worst states of the domain search (test_env_edge_tables_host.py finds them again): the largest angle before the wrap, the
# largest angle handed to sin / cos by an RK4 stage, and a state that needs the FIFTH subtraction (with four, the stored angle is
# outside [-pi, pi]: the named state of the k = 4 check).
ACROBOT_WORST = {
    "largest pre-wrap angle": ((-3.1415927, -1.9535553, -12.566371, -28.274334), 0),       # th1 before the wrap: -29.724
    "largest stage angle": ((-1.5980719, 1.9804358, 12.566371, 28.274334), 2),              # the largest |angle| of its four stages: 33.317
    "needs the fifth subtraction": ((3.1142824, 1.9374146, 12.566371, 28.26685), 1),
}
# One state per wrap depth that the grid of clamped velocities below does not reach by itself (found by the same search)
ACROBOT_WRAP_DEPTH = {
    "th1 wraps twice": ((-3.028529, -2.1512387, -12.566371, -19.6573), 1),                 # th1 before the wrap: -10.85
    "th1 wraps three times": ((3.0827537, -2.1019156, -12.566371, -26.726942), 2),         # -16.58
    "th2 wraps three times": ((1.7946897, -1.0544254, -12.566371, -27.554853), 2),         # th2 before the wrap: -18.09
}
# Termination on both sides of the threshold, at least 1e-3 away from it in float64 (the CPU test asserts the margins)
ACROBOT_TERMINATION = (
    ("just terminal", (2.2, 0.0, 0.0, 0.0), 1, True),
    ("just not terminal", (2.0, 0.0, 0.0, 0.0), 1, False),
    ("terminal while swinging", (1.8, 0.6, 2.0, -1.0), 2, True),
    ("not terminal while swinging", (1.5, 0.6, 2.0, -1.0), 0, False),
)


def acrobot_table():
    rows = []
    inb = (("finite",), ("le", 0, float(np.pi)), ("le", 1, float(np.pi)), ("le", 2, 4.0 * float(np.pi)), ("le", 3, 9.0 * float(np.pi)))
    # (upstream writes the gravity terms as cos(th - pi/2), 6e-17 at th = 0 in float64: the fixed point is exact in the kernel's sin(th))
    rows.append(_row("hanging at rest", (0.0, 0.0, 0.0, 0.0), 1, "a fixed point: every term of dsdt is zero",
                     inb + tuple(("le", c, 1e-15) for c in range(4)) + tuple(("twin", "eq", c, 0.0) for c in range(4))
                     + (("done", False), ("reward", -1.0))))
    # --- the velocity clamps, each alone and together, over a grid of angles
    grid = (-PI32, f32(-1.5707964), f32(0.0), f32(1.5707964), PI32)
    k = 0
    for v1, v2, tag in ((MV1, 0, "dth1=+4pi"), (-MV1, 0, "dth1=-4pi"), (0, MV2, "dth2=+9pi"), (0, -MV2, "dth2=-9pi"),
                        (MV1, MV2, "dth=(+4pi,+9pi)"), (MV1, -MV2, "dth=(+4pi,-9pi)"), (-MV1, MV2, "dth=(-4pi,+9pi)"),
                        (-MV1, -MV2, "dth=(-4pi,-9pi)")):
        for i, t1 in enumerate(grid):
            for j, t2 in enumerate(grid):
                rows.append(_row(f"{tag},th=({i - 2},{j - 2})*pi/2", (t1, t2, v1, v2), k % 3, "velocities on their clamps", inb))
                k += 1
    for name, (s, a) in ACROBOT_WORST.items():
        rows.append(_row(name, s, a, "worst state of the domain search", inb))
    for name, (s, a) in ACROBOT_WRAP_DEPTH.items():
        rows.append(_row(name, s, a, "a wrap depth of its own", inb))
    # --- theta = +-pi
    rows.append(_row("th1=+pi at rest", (PI32, 0.0, 0.0, 0.0), 1, "upright (an unstable equilibrium): height 2", inb + (("done", True), ("reward", 0.0))))
    rows.append(_row("th1=-pi at rest", (-PI32, 0.0, 0.0, 0.0), 1, "upright", inb + (("done", True), ("reward", 0.0))))
    rows.append(_row("th2=+pi at rest", (0.0, PI32, 0.0, 0.0), 1, "lower link folded back: height 0", inb + (("done", False), ("reward", -1.0))))
    rows.append(_row("th2=-pi at rest", (0.0, -PI32, 0.0, 0.0), 1, "lower link folded back", inb + (("done", False), ("reward", -1.0))))
    for name, s, a, d in ACROBOT_TERMINATION:
        rows.append(_row(name, s, a, "termination, at least 1e-3 from the threshold", inb + (("done", d), ("reward", 0.0 if d else -1.0))))
    # --- outside the bounds through SetState.  Velocities: the clamps bring them back, the angles they produce stay below 13 pi
    # (|th| + 0.2 * 100 + ... ); angles: 3.2 and 24 are wrapped like any other (24 + 0.2 * 0 < 13 pi), 100 is beyond six subtractions
    velonly = (("finite",), ("le", 2, 4.0 * float(np.pi)), ("le", 3, 9.0 * float(np.pi)))
    for v in (13.0, -13.0, 100.0, -100.0):
        rows.append(_row(f"dth1={v:+g}", (0.5, -0.5, v, 0.0), 1, "beyond the clamp (SetState)", inb if abs(v) < 50 else velonly, upstream=abs(v) < 50))
    for v in (29.0, -29.0, 100.0, -100.0):
        # (at 100 rad/s the centrifugal terms, ~ dth^2, throw the angles thousands of radians in one step: only the clamps are promised)
        rows.append(_row(f"dth2={v:+g}", (0.5, -0.5, 0.0, v), 1, "beyond the clamp (SetState)", inb if abs(v) < 50 else velonly, upstream=abs(v) < 50))
    for t in (3.2, -3.2, 24.0, -24.0):
        rows.append(_row(f"th1={t:+g}", (t, 0.3, 0.0, 0.0), 1, "beyond [-pi, pi] (SetState): wrapped", inb))
        rows.append(_row(f"th2={t:+g}", (0.3, t, 0.0, 0.0), 1, "beyond [-pi, pi] (SetState): wrapped", inb))
    for t in (100.0, -100.0):
        # from rest the angle moves by less than a radian in one step: 100 - 6 * 2 pi = 62.3 is what the bounded wrap leaves
        rows.append(_row(f"th1={t:+g}", (t, 0.3, 0.0, 0.0), 1, "beyond 13 pi: six subtractions leave it outside [-pi, pi]",
                         (("finite",), ("gt", 0, 60.0), ("le", 0, 64.0), ("le", 1, float(np.pi))), upstream=False))
        rows.append(_row(f"th2={t:+g}", (0.3, t, 0.0, 0.0), 1, "beyond 13 pi: six subtractions leave it outside [-pi, pi]",
                         (("finite",), ("gt", 1, 60.0), ("le", 1, 64.0), ("le", 0, float(np.pi))), upstream=False))
    # --- non-finite components: sin / cos of the first stage (angles) or of the second (velocities: th + 0.1 * inf) are NaN, and
    # NaN reaches every component through the coupled accelerations; every compare is false: never done
    allnan = (("nan", 0), ("nan", 1), ("nan", 2), ("nan", 3), ("done", False), ("reward", -1.0))
    base = [0.5, 0.4, 1.0, -1.0]
    for c, cname in enumerate(("th1", "th2", "dth1", "dth2")):
        for v, vname in ((NAN, "nan"), (INF, "+inf"), (-INF, "-inf")):
            s = list(base)
            s[c] = v
            rows.append(_row(f"{cname}={vname}", s, c % 3, "non-finite component", allnan))
    return rows


TABLES = {"Pendulum-v1": pendulum_table, "MountainCar-v0": mountaincar_table, "Acrobot-v1": acrobot_table}
STATE_DIM = {"Pendulum-v1": 2, "MountainCar-v0": 2, "Acrobot-v1": 4}


def table_arrays(env):
    """(rows, state float32 [S, R], action [R]) of one env's table."""
    rows = TABLES[env]()
    s = np.array([r["state"] for r in rows], f32).T.copy()
    a = np.array([r["action"] for r in rows], f32 if env == "Pendulum-v1" else np.int32)
    assert len({r["name"] for r in rows}) == len(rows), "row names must be unique"
    return rows, s, a


# ---------------------------------------------------------------------------------------------------------------------------------
# fact checking
# ---------------------------------------------------------------------------------------------------------------------------------
def check_facts(rows, state, reward, done, dtype, which, only=None):
    """Holds the result of ONE step of the table (state [S, R], reward [R], done [R], in table order) to every row's facts.
    which: "f64" (rows that are not `upstream` are skipped: the contract promises upstream's result only there) or "twin" / "gpu"."""
    index = {r["name"]: i for i, r in enumerate(rows)}
    cast = (lambda v: np.float64(v)) if dtype == np.float64 else (lambda v: f32(v))
    bad = []
    for i, r in enumerate(rows):
        if which == "f64" and not r["upstream"]:
            continue
        if only is not None and not only[i]:
            continue
        for f in r["facts"]:
            if f[0] == "twin":
                if which == "f64":
                    continue
                f = f[1:]
            kind = f[0]
            if kind == "eq":
                ok = state[f[1], i] == cast(f[2])
            elif kind == "nan":
                ok = np.isnan(state[f[1], i])
            elif kind == "le":
                ok = abs(state[f[1], i]) <= cast(f[2])
            elif kind == "gt":
                ok = abs(state[f[1], i]) > cast(f[2])
            elif kind == "pos":
                ok = state[f[1], i] > 0
            elif kind == "neg":
                ok = state[f[1], i] < 0
            elif kind == "finite":
                ok = np.isfinite(state[:, i]).all() and np.isfinite(reward[i])
            elif kind == "done":
                ok = bool(done[i]) == f[1]
            elif kind == "reward":
                ok = reward[i] == cast(f[1])
            elif kind == "reward_nan":
                ok = np.isnan(reward[i])
            elif kind == "reward_in":
                ok = f[1] <= reward[i] <= f[2]
            elif kind == "same_as":
                j = index[f[1]]
                ok = (np.array_equal(state[:, i], state[:, j], equal_nan=True) and np.array_equal(reward[i], reward[j], equal_nan=True)
                      and bool(done[i]) == bool(done[j]))
            else:
                raise AssertionError(f"unknown fact {f}")
            if not ok:
                bad.append((r["name"], f, state[:, i].tolist(), float(reward[i]), bool(done[i])))
    assert not bad, (which, bad[:6])


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 bars (those of tests/test_gpu_other_envs.py), shared by the CPU test of the twin and the GPU test of the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def ulp32(x):
    """The float32 ulp at |x| (float64 array in, float64 out)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.spacing(np.abs(np.asarray(x, np.float64)).astype(f32)).astype(np.float64)


def circle(a, b):
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, np.float64) - np.asarray(b, np.float64)))))


def acrobot_errors(got, want):
    """(angle error on the circle [2, n], velocity error [2, n]) against a float64 state."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return circle(got[:2], want[:2]), np.abs(got[2:] - want[2:])


LIBRARY_SINCOS_BOUND = 4 * 2.0 ** -24      # 4 ulp of a value <= 1: the project's bound for the math library (tests/_actor_box_policy_twin.py)


def check_float64_bars(env, s, want, got, use, literal=None):
    """got (dict s2 / obs / reward / done of the twin or of a kernel, float32) against want (the same of the float64 oracle) on the
    lanes `use` (finite rows where the contract promises upstream's result).  Integer outputs are equal on every such lane.
      Pendulum     velocity, and its copy in the observation, 1e-5.  theta' 1e-5 plus half a float32 ulp of theta' itself — beyond
                   |theta| = 128 the format cannot hold it closer — and as much for cos / sin theta', which inherit the angle's
                   rounding.  Reward 1e-4 of its range (16.3, or |reward| where larger), plus, beyond |theta| = 100, what rounding
                   theta + pi to float32 does to the cost's normalised angle: one ulp of that sum times d(x^2)/dx <= 2 pi.
                   The observation is also within LIBRARY_SINCOS_BOUND of the float64 cos / sin of the float32 angle it was taken of.
      MountainCar  state 1e-6, reward equal.
      Acrobot      the literal float32 transcription of upstream is the yardstick: no worse than it at the median and the 99th
                   percentile (+25 %), within 4 x at the worst lane; the observation within 1.2e-7 of cos / sin of the stored angles."""
    use = np.asarray(use, bool)
    g2, w2 = np.asarray(got["s2"], np.float64)[:, use], np.asarray(want["s2"], np.float64)[:, use]
    go, wo = np.asarray(got["obs"], np.float64)[:, use], np.asarray(want["obs"], np.float64)[:, use]
    gr, wr = np.asarray(got["reward"], np.float64)[use], np.asarray(want["reward"], np.float64)[use]
    assert np.array_equal(np.asarray(got["done"]).astype(bool)[use], np.asarray(want["done"]).astype(bool)[use])
    if env == "Pendulum-v1":
        th = np.asarray(s, np.float64)[0, use]
        th_bar = 1e-5 + 0.5 * ulp32(w2[0])
        r_bar = 1e-4 * np.maximum(16.3, np.abs(wr)) + 2.0 * np.pi * ulp32(np.abs(th) + np.pi) * (np.abs(th) > 100)
        assert (np.abs(g2[1] - w2[1]) <= 1e-5).all() and (np.abs(go[2] - wo[2]) <= 1e-5).all()
        assert (np.abs(g2[0] - w2[0]) <= th_bar).all()
        assert (np.abs(go[:2] - wo[:2]) <= th_bar).all()
        assert (np.abs(gr - wr) <= r_bar).all()
        assert np.abs(go[0] - np.cos(g2[0])).max() <= LIBRARY_SINCOS_BOUND and np.abs(go[1] - np.sin(g2[0])).max() <= LIBRARY_SINCOS_BOUND
    elif env == "MountainCar-v0":
        assert np.abs(g2 - w2).max() <= 1e-6 and np.array_equal(gr, wr)
    else:
        assert np.array_equal(gr, wr)
        dang, dvel = acrobot_errors(g2, w2)
        lang, lvel = acrobot_errors(np.asarray(literal)[:, use], w2)
        for q in (0.5, 0.99):
            assert np.quantile(dang, q) <= 1.25 * np.quantile(lang, q) and np.quantile(dvel, q) <= 1.25 * np.quantile(lvel, q), q
        assert dang.max() <= 4 * lang.max() and dvel.max() <= 4 * lvel.max(), (dang.max(), lang.max(), dvel.max(), lvel.max())
        assert np.abs(go[0] - np.cos(g2[0])).max() <= 1.2e-7 and np.abs(go[1] - np.sin(g2[0])).max() <= 1.2e-7
        assert np.abs(go[2] - np.cos(g2[1])).max() <= 1.2e-7 and np.abs(go[3] - np.sin(g2[1])).max() <= 1.2e-7


# ---------------------------------------------------------------------------------------------------------------------------------
# branches: which paths of the step a row takes, read off the step's inputs and results in the dtype of the oracle that ran it
# ---------------------------------------------------------------------------------------------------------------------------------
PENDULUM_BRANCHES = {"torque<-2", "torque>2", "torque inside", "thdot clamp -", "thdot clamp +", "thdot unclamped", "theta+pi<0",
                     "theta+pi>=0", "sincos library", "sincos kernel", "fmod fallback", "fmod fast"}
# ("wall with v >= 0" — p' == -1.2 reached with a velocity that is not negative — would need p + v' to land on the bound exactly from
# the right: no float64 row can be built for it, so it is reported by mountaincar_branches but not required)
MOUNTAINCAR_BRANCHES = {"v clamp -", "v clamp +", "v unclamped", "p clamp left", "p clamp right", "p unclamped", "wall zeroes v",
                        "done", "not done", "p>=0.5 with v<0"}
# (inside the state box th1 takes up to five subtractions and th2 up to four: the search of test_env_edge_tables_host.py)
ACROBOT_BRANCHES = ({f"wrap th1 x{k}" for k in range(6)} | {f"wrap th2 x{k}" for k in range(5)}
                    | {"dth1 clamp -", "dth1 clamp +", "dth1 unclamped", "dth2 clamp -", "dth2 clamp +", "dth2 unclamped", "done", "not done"})


def pendulum_branches(s, a, s2, dtype):
    """Sets of branch names per row.  The unclamped new velocity is recomputed in `dtype` from the oracle's own result where the clamp
    did not bind, and from the inputs' sign where it did."""
    out = []
    for i in range(s.shape[1]):
        b = set()
        th, act = float(s[0, i]), float(a[i])
        if np.isfinite(th) and np.isfinite(s[1, i]) and not np.isnan(act):
            b.add("torque<-2" if act < -2 else ("torque>2" if act > 2 else "torque inside"))
            u = min(max(act, -2.0), 2.0)
            raw = float(s[1, i]) + (15.0 * np.sin(th) + 3.0 * u) * 0.05            # (decides the SIDE only; rows sit far from a tie or on it exactly)
            if s2[1, i] == -8 and raw < -8:
                b.add("thdot clamp -")
            elif s2[1, i] == 8 and raw > 8:
                b.add("thdot clamp +")
            else:
                b.add("thdot unclamped")
            b.add("theta+pi<0" if dtype(th) + dtype(np.pi) < 0 else "theta+pi>=0")
            b.add("sincos library" if abs(th) > 65536.0 else "sincos kernel")
            b.add("fmod fast" if abs(dtype(th) + dtype(np.pi)) < 4194304.0 * float(TWO_PI32) else "fmod fallback")
        out.append(b)
    return out


def mountaincar_branches(s, a, s2, done, dtype):
    out = []
    lo, hi, vm = dtype(-1.2), dtype(0.6), dtype(0.07)
    for i in range(s.shape[1]):
        b = set()
        if np.isfinite(s2[:, i]).all() and np.isfinite(s[0, i]):
            p2, v2 = s2[0, i], s2[1, i]
            raw_sign = float(s[1, i]) + (int(a[i]) - 1) * 0.001 - 0.0025 * np.cos(3.0 * float(s[0, i]))
            if p2 == lo and v2 == 0 and raw_sign < 0:
                b.add("wall zeroes v")
                b.add("v clamp -" if raw_sign < -0.07 else "v unclamped")
            else:
                b.add("v clamp -" if (v2 == -vm and raw_sign < -0.07) else ("v clamp +" if (v2 == vm and raw_sign > 0.07) else "v unclamped"))
            pre = float(s[0, i]) + float(v2 if "wall zeroes v" not in b else raw_sign)
            b.add("p clamp left" if (p2 == lo and pre < -1.2) else ("p clamp right" if (p2 == hi and pre > 0.6) else "p unclamped"))
            if p2 == lo and "wall zeroes v" not in b:
                b.add("wall with v>=0")
            b.add("done" if done[i] else "not done")
            if p2 >= dtype(0.5) and v2 < 0:
                b.add("p>=0.5 with v<0")
        out.append(b)
    return out


def acrobot_branches(s2, done, wraps, dtype):
    out = []
    m1, m2 = (MV1, MV2) if dtype == f32 else (4.0 * np.pi, 9.0 * np.pi)
    for i in range(s2.shape[1]):
        b = set()
        if np.isfinite(s2[:, i]).all():
            b.add(f"wrap th1 x{int(wraps[0, i])}")
            b.add(f"wrap th2 x{int(wraps[1, i])}")
            for c, m, nm in ((2, m1, "dth1"), (3, m2, "dth2")):
                b.add(f"{nm} clamp -" if s2[c, i] == -m else (f"{nm} clamp +" if s2[c, i] == m else f"{nm} unclamped"))
            b.add("done" if done[i] else "not done")
        out.append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# The Acrobot domain search: the closed state box |th| <= pi, |dth1| <= 4 pi, |dth2| <= 9 pi (float32 bounds as the kernel forms them)
# ---------------------------------------------------------------------------------------------------------------------------------
SINCOS_SMALL_SWEEP = 36.5          # rad: how far tests/test_oracle.py sweeps sincos_small — the measured stage maximum (33.32) plus pi
ACROBOT_BOX = np.array([PI32, PI32, MV1, MV2], f32)
SEARCH_RANDOM = 1 << 24
_CHUNK = 1 << 19


def acrobot_corner_states():
    """All 3^4 corner / centre combinations x 3 actions."""
    g = np.array(np.meshgrid(*[[-1.0, 0.0, 1.0]] * 4, indexing="ij")).reshape(4, -1)
    s = (g * ACROBOT_BOX[:, None].astype(np.float64)).astype(f32)
    s = np.tile(s, (1, 3))
    a = np.repeat(np.arange(3, dtype=np.int32), 81)
    return s, a


def acrobot_random_states(chunk, n=_CHUNK):
    """Chunk `chunk` of the random search: uniform in the box, one quarter with dth1 pinned to a clamp, one with dth2, one with both."""
    rng = np.random.default_rng([20240611, chunk])
    s = (rng.uniform(-1.0, 1.0, (4, n)) * ACROBOT_BOX[:, None].astype(np.float64)).astype(f32)
    q = n // 4
    s[2, :q] = np.where(rng.random(q) < 0.5, -MV1, MV1)
    s[3, q:2 * q] = np.where(rng.random(q) < 0.5, -MV2, MV2)
    s[2, 2 * q:3 * q] = np.where(rng.random(q) < 0.5, -MV1, MV1)
    s[3, 2 * q:3 * q] = np.where(rng.random(q) < 0.5, -MV2, MV2)
    return s, rng.integers(0, 3, n).astype(np.int32)


def acrobot_search(oracle, visit, n_random=SEARCH_RANDOM, climb_rounds=40, keep=32):
    """Runs the probe over corners, random states and a hill-climb from the worst points; `visit(states, actions, probe)` sees every
    evaluated batch.  Returns dict(pre=(value, state, action), stage=(value, state, action))."""
    best = {"pre": [], "stage": []}

    def note(s, a, o):
        for key, val in (("pre", np.abs(o["pre64"][:2]).max(0)), ("stage", o["pre64"][2])):
            top = np.argsort(val)[-keep:]
            best[key] += [(float(val[i]), tuple(float(x) for x in s[:, i]), int(a[i])) for i in top]
            best[key] = sorted(set(best[key]))[-keep:]

    def run(s, a):
        o = oracle.acrobot_domain_probe(s, a)
        visit(s, a, o)
        note(s, a, o)

    run(*acrobot_corner_states())
    chunks = n_random // _CHUNK
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:                  # (ctypes releases the GIL inside the probe)
        for s, a, o in pool.map(lambda c: (lambda s, a: (s, a, oracle.acrobot_domain_probe(s, a)))(*acrobot_random_states(c)), range(chunks)):
            visit(s, a, o)
            note(s, a, o)
    rng = np.random.default_rng(7)
    for r in range(climb_rounds):
        scale = 0.25 * 0.8 ** r
        for key in ("pre", "stage"):
            seeds = np.array([b[1] for b in best[key]], np.float64).T                       # [4, keep]
            acts = np.array([b[2] for b in best[key]], np.int32)
            cand = np.repeat(seeds, 64, axis=1) + rng.normal(0.0, scale, (4, seeds.shape[1] * 64)) * ACROBOT_BOX[:, None]
            # half of the candidates keep the velocities where they were (the maxima sit ON the clamps)
            cand[2:, ::2] = np.repeat(seeds, 64, axis=1)[2:, ::2]
            cand = np.clip(cand, -ACROBOT_BOX[:, None].astype(np.float64), ACROBOT_BOX[:, None].astype(np.float64)).astype(f32)
            run(cand, np.repeat(acts, 64))
    return {k: v[-1] for k, v in best.items()}
