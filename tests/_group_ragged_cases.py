"""Case table of tests/test_gpu_group_ragged.py: groups of logical members whose size is NOT a multiple of four lanes.

Row = (env, dtype, G, lanes per member, overlap, forced lanes per thread or None).  What the sizes reach:

  - n_local % 4 in {1, 2, 3} (and one aligned row): a member's rows sit at replica + (m * D + k) * n_local elements, so with a
    ragged n_local every row but the first is off a 16-byte line, and for D = 3, n_local = 2 (mod 4) odd members START 8 bytes off;
    default_policy() must resolve such a float32 member to one lane per thread, a float64 member with odd n_local likewise, a
    float64 member with even n_local to the two-lane form;
  - n_local on both sides of kSmallHostPath = 4096: group_copy_out()'s host-mapped export (<= 4096) and pack + memcpy (> 4096);
  - D in {2, 3, 4, 6}; alias envs (CartPole, MountainCar[Continuous]: state rows ARE the replica slice) and non-alias envs
    (Pendulum, Acrobot: observation rows in the replica, state rows in the library's allocation) with an odd ext_obs_stride;
  - members whose first global lane is 1, 2 or 3 (mod 4): the Philox lane groups of a reset straddle member boundaries;
  - G = 16 (kMaxPeers + 1): every push carries 15 destinations;
  - the gather's push: a CartPole slice is 16 * n_local bytes (float64: 32), always on a line and without a tail; Pendulum 4 x 7,
    3 x 1002 and 2 x 4099, MountainCar 3 x 1001, Acrobot 3 x 333 and MountainCarContinuous 3 x 1003 have D * n_local % 4 != 0 and
    slices that start 4, 8 or 12 bytes off a line: the dwordx4 branch with its tail loop on the members that start on a line,
    the scalar branch on the others, in one gather.

The two forced rows put a wide form beside the fallbacks: CartPole float32 at 1024 lanes with vec = 4 on every member (dwordx4
stores into replica slices), Acrobot at 4098 lanes with vec = 2 (rows alternately on and 8 bytes off a 16-byte line).
"""
import numpy as np

F32, F64 = np.float32, np.float64

#        env                          dtype G   n_local overlap force_vec
CASES = [
    ("CartPole-v1",              F32, 3,  1,    False, None),
    ("CartPole-v1",              F32, 2,  3,    True,  None),
    ("CartPole-v1",              F32, 5,  63,   True,  None),
    ("CartPole-v1",              F32, 3,  1001, True,  None),
    ("CartPole-v1",              F32, 2,  4097, False, None),
    ("CartPole-v1",              F32, 16, 65,   False, None),
    ("CartPole-v1",              F32, 2,  1024, True,  4),
    ("CartPole-v1",              F64, 3,  5,    True,  None),
    ("CartPole-v1",              F64, 2,  1002, True,  None),
    ("CartPole-v1",              F64, 2,  4097, False, None),
    ("Pendulum-v1",              F32, 4,  7,    False, None),
    ("Pendulum-v1",              F32, 3,  1002, True,  None),
    ("Pendulum-v1",              F32, 2,  4099, False, None),
    ("MountainCar-v0",           F32, 5,  2,    False, None),
    ("MountainCar-v0",           F32, 3,  1001, True,  None),
    ("Acrobot-v1",               F32, 3,  333,  True,  None),
    ("Acrobot-v1",               F32, 2,  4098, False, None),
    ("Acrobot-v1",               F32, 2,  4098, True,  2),
    ("MountainCarContinuous-v0", F32, 3,  1003, True,  None),
]

KERNEL_ENV = {"CartPole-v1": "CartPole", "Pendulum-v1": "Pendulum", "MountainCar-v0": "MountainCar", "Acrobot-v1": "Acrobot",
              "MountainCarContinuous-v0": "MountainCarContinuous"}
OBS_DIM = {"CartPole-v1": 4, "Pendulum-v1": 3, "MountainCar-v0": 2, "Acrobot-v1": 6, "MountainCarContinuous-v0": 2}
# Pendulum has no terminal state: its rows carry a time limit (and with it the bookkeeping kernel variant) so that lanes are re-drawn
TIME_LIMIT = {"Pendulum-v1": 5}


def case_id(case):
    env, dtype, G, nl, overlap, force = case
    return f"{KERNEL_ENV[env]}{'64' if dtype is F64 else ''}-{G}x{nl}-{'overlap' if overlap else 'serial'}" + (f"-vec{force}" if force else "")


def wide_form(env, dtype):
    """lanes per thread of the env's wide form: two for Acrobot and float64 CartPole, else four (capi.hip apply_policy)"""
    return 2 if (env == "Acrobot-v1" or dtype is F64) else 4


def rows_allow(env, dtype, G, nl, lanes):
    """Whether every member's rows allow `lanes` lanes per thread: each row of each member starts on a (lanes * 4)-byte line
    (a float64 pair of lanes is one 16-byte access) — worked out from the layout alone, replica + (m * D + k) * n_local elements
    with the replica itself 256-byte aligned."""
    esz = 8 if dtype is F64 else 4
    line = 16 if dtype is F64 else 4 * lanes
    D = OBS_DIM[env]
    return all(((m * D + k) * nl * esz) % line == 0 for m in range(G) for k in range(D))


def expected_vec(case):
    """Lanes per thread every member must resolve to: the forced form, else default_policy()'s choice at these sizes (all far below
    the 2^19 lanes where float32 members switch to dwordx4): float64 members take the pair form wherever their rows allow it."""
    env, dtype, G, nl, overlap, force = case
    if force:
        return force
    return 2 if (dtype is F64 and rows_allow(env, dtype, G, nl, 2)) else 1
