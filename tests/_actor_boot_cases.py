"""What the boot tests share (helper module, not a conftest): the recipe table of actor_boot.hip's 20 fused forms, the per-lane table of
running episode lengths that staggers the time limits, the NumPy statement of the definition, and the coverage count every test that uses
the table asserts.

actor_boot.hip compiles actor_value_boot_rollout_kernel<Env, AUTORESET, RECORDS> for CartPole, MountainCar and Acrobot and
actor_box_boot_rollout_kernel<Env, AUTORESET, RECORDS> for Pendulum and MountainCarContinuous: bookkeeping forms only (a time limit needs
episode_stats), 20 kernels.  Each row of FORMS names one the way the assembly demangles it and says how to reach it through the public
API: the env, the handle's auto_reset, and whether the rollout call carries an episodes= dict.

Staggering.  After Reset() every lane's episode length is 0, so a small max_episode_steps alone would truncate all lanes in the same steps
and none in the others.  lengths(n) gives lane i its running episode length at the start of the T = 12 measured steps, with LIMIT = 7:
    wave w = i // 64 with w % 4 == 0:  0 for every lane      all of the wave truncates at step 6, none of it in any other step
                           w % 4 == 2:  3 for every lane      all at steps 3 and 10
                           otherwise :  i % 7                 a few lanes in every step: mixed
(with auto_reset; without it a lane stays finished once its length reaches LIMIT, so "all" holds from that step on and "none" before
it).  goal_lanes(n) are the lanes of the mixed waves with i % 3 == 0: on MountainCar, MountainCarContinuous and Acrobot they are put
where the next step is terminal (tests/test_gpu_actor_softmax.py _at_the_goal's states), so d == 1 rows occur, and those of them whose
length is LIMIT - 1 (lane 69 is the first) end with d == 3.  The "all" and "none" waves hold no goal lane, so their pattern stands."""
import numpy as np

import _actor_twin as twin

F32 = np.float32
LIMIT, T, S = 7, 12, 2
N, N_ATT = 321, 257
WAVE = 64
DISCRETE = {"CartPole": "CartPole-v1", "MountainCar": "MountainCar-v0", "Acrobot": "Acrobot-v1"}
BOX = {"Pendulum": "Pendulum-v1", "MountainCarContinuous": "MountainCarContinuous-v0"}
OBS = {"CartPole-v1": 4, "MountainCar-v0": 2, "Acrobot-v1": 6, "Pendulum-v1": 3, "MountainCarContinuous-v0": 2}
GOAL_ENVS = ("MountainCar-v0", "MountainCarContinuous-v0", "Acrobot-v1")      # envs whose goal lanes terminate in the first step
POISON = 7.25                                      # what a boot buffer holds before the launch


def _b(v):
    return "true" if v else "false"


FORMS = [dict(kernel=f"{'actor_box_boot' if gym in BOX.values() else 'actor_value_boot'}_rollout_kernel<{env},{_b(ar)},{_b(rec)}>", env=gym, auto_reset=ar,
              records=rec, box=gym in BOX.values())
         for env, gym in {**DISCRETE, **BOX}.items() for ar in (True, False) for rec in (False, True)]
# the kernel that serves the same handle and call without rec_boot (actor_value.hip / actor_box_logd.hip)
SIBLING = {row["kernel"]: (f"actor_box_logd_rollout_kernel<{env},{_b(row['auto_reset'])},true,{_b(row['records'])}>" if row["box"] else
                           f"actor_value_rollout_kernel<{env},{_b(row['auto_reset'])},true,{_b(row['records'])}>")
           for row in FORMS for env in [row["kernel"].split("<")[1].split(",")[0]]}


def form_id(row):
    return row["kernel"]


def handle_kwargs(auto_reset, **more):
    return dict(auto_reset=auto_reset, episode_stats=True, max_episode_steps=LIMIT, **more)


def lengths(n):
    """int32 [n]: lane i's running episode length before the first measured step"""
    i = np.arange(n)
    w = (i // WAVE) % 4
    return np.where(w == 0, 0, np.where(w == 2, 3, i % LIMIT)).astype(np.int32)


def goal_lanes(n):
    i = np.arange(n)
    return ((i // WAVE) % 2 == 1) & (i % 3 == 0)


def at_the_goal(name, state):
    """state [S, n] with the goal lanes moved where their next step is terminal (a copy); CartPole and Pendulum have no such place"""
    s = np.array(state, copy=True)
    g = goal_lanes(s.shape[1])
    if OBS[name] == 2:
        s[0, g], s[1, g] = 0.49, 0.05
    elif OBS[name] == 6:
        s[:, g] = np.array([np.pi, 0.0, 0.0, 0.0], s.dtype)[:, None]
    return s


def place(env, name):
    """the table, on a handle: goal lanes moved, running lengths set.  The caller refills the actor's history afterwards (actor.Reset())"""
    if name in GOAL_ENVS:
        env.SetState(at_the_goal(name, env.GetState()))
    env.SetArray("episode_length", lengths(env.NumberOfEnvironments))


def done_bytes(terminated, length, auto_reset):
    """The engine's bookkeeping for one step (step_kernels.hpp): (done bytes uint8 [n], the lengths after the step)."""
    length = length + 1
    done = (np.asarray(terminated) != 0).astype(np.uint8) | np.where(length >= LIMIT, 2, 0).astype(np.uint8)
    if auto_reset:
        length = np.where(done != 0, 0, length)
    return done, length.astype(np.int32)


def coverage(done):
    """dict of counts over done uint8 [T, n]: rows with d == 1, 2, 3, and (wave, step) pairs in which all / none / some but not all of the
    wave's lanes have bit 1 set (the last wave may be partial: its lanes in range count)"""
    done = np.asarray(done, np.uint8)
    n = done.shape[1]
    out = {f"d{k}": int((done == k).sum()) for k in (1, 2, 3)}
    out.update(all=0, none=0, mixed=0)
    for w0 in range(0, n, WAVE):
        tr = (done[:, w0:w0 + WAVE] & 2) != 0
        k = tr.sum(axis=1)
        out["all"] += int((k == tr.shape[1]).sum())
        out["none"] += int((k == 0).sum())
        out["mixed"] += int(((k > 0) & (k < tr.shape[1])).sum())
    return out


def assert_covered(cov, name):
    """every path the table is there for occurs: a case table that stopped covering one fails rather than passes"""
    need = ["d2", "all", "none", "mixed"] + (["d1", "d3"] if name in GOAL_ENVS else [])
    assert all(cov[k] > 0 for k in need), (name, cov)


def critic(name, deep, seed=11):
    """(widths, flat, pairs) of one of the two critics of tests/test_gpu_actor_value.py for this env: [2 O, 13, 7, 1] or [2 O, 16, 1]"""
    O = OBS[name]
    return twin.net(np.random.default_rng([seed, O, int(deep)]), [S * O, 13, 7, 1] if deep else [S * O, 16, 1])


def want_boot(critic, history_before_push, terminal_obs, done):
    """The definition: float32 [n].  history_before_push [n, S, O] oldest first (the input the step's action was chosen from),
    terminal_obs [n, O] (the post-step observation before any reset), done uint8 [n].  Rows with bit 1: the critic over the history's rows
    1 .. S-1 followed by the terminal observation; every other row +0."""
    w, flat, _ = critic
    hist = np.asarray(history_before_push, F32)
    n = len(hist)
    x = np.concatenate([hist[:, 1:].reshape(n, -1), np.asarray(terminal_obs).astype(F32).reshape(n, -1)], axis=1)
    v = twin.forward(w, flat, np.ascontiguousarray(x))[0][:, 0]
    return np.where((np.asarray(done) & 2) != 0, v, F32(0.0)).astype(F32)
