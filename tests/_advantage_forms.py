"""Every kernel gfx950 compiles from gym.net_amd/csrc/advantage.hip, and the gymnet_gae_device arguments that reach it: V = 4 needs
count >= NARROW_BELOW, count % 4 == 0, stride % 4 == 0, every float pointer 16-byte and the done pointer 4-byte aligned (advantage.hpp,
pick_advantage_form); values / boot say whether d_value / d_boot is given.  tests/test_advantage_forms.py holds the table to the compiled
set; tests/test_gpu_advantage.py launches every row."""

U = {4: 4, 1: 8}              # rows in flight per V (advantage.hip, Tuning<V>::U): the GPU test sizes T around both
NARROW_BELOW = 4 * 64 * 1024  # advantage.hpp kAdvantageNarrowBelow: fewer lanes run V = 1


def _name(vec, values, boot):
    return f"advantage_kernel<{vec},{'true' if values else 'false'},{'true' if boot else 'false'}>"


FORMS = [
    {"kernel": _name(vec, values, boot), "vec": vec, "values": values, "boot": boot,
     # count, stride - count, base pointer offset in elements: arguments that reach the row (V = 4: the smallest count that does, plus 4 —
     # a last block that holds one thread)
     "reach": {"count": NARROW_BELOW + 4, "pad": 12, "offset": 0} if vec == 4 else {"count": 1030, "pad": 1, "offset": 0}}
    for vec in (1, 4) for values in (False, True) for boot in (False, True)
]


def kernel_for(count, stride, aligned16, values, boot):
    """the table's restatement of the picker, for the GPU test to name the row a launch reaches"""
    vec = 4 if count >= NARROW_BELOW and count % 4 == 0 and stride % 4 == 0 and aligned16 else 1
    return _name(vec, values, boot)
