"""The Box actor's policies (include/gymnet_amd.h, gymnet_vecenv_actor_box_set_policy) in NumPy float64, lane by lane (helper module, not
a conftest): the tanh head, Gaussian exploration noise, and the error bounds the float32 kernels of actor_box_policy.hip are held to.

Exact parts: `raw` comes from tests/_actor_twin.py's fmaf chain (the caller passes it in), the explore mask is the integer compare of word
B with coin_threshold(epsilon), and the three words of a lane come from the NumPy Philox twin (oracle/numpy_ref.py): A and B through
action_words, the noise word N = word (L & 3) of Philox(key = seed ^ NOISE_STREAM, counter = (L >> 2, tick)), picked the way action_words
picks A and B.  Everything after the words — greedy, z, the action — is float64 in closed form, not the kernel's operation order.

Bounds (absolute, against the float64 value):
  z         Z_BOUND = _space_sampling_ref.UNBOUNDED_BOUND = 1e-5: that derivation covers exactly these operations — logf of u1, sqrtf, the
            float32 angle 2pi_f32 * u2 and its cosine at 4 ulp of a value <= 1, two products — and r = sqrt(-2 ln u1) <= sqrt(48 ln 2) =
            5.77 bounds |z| as well.  (The kernel's cosine is the envs' own sincos_f32; restated in NumPy over all 2^24 values of u2 it is
            within 9.3e-8 of the cosine of the float32 angle: inside the 4 ulp = 2.4e-7 the derivation grants the library's.)
  clamp     0: the clamp of a float32 is that float32.
  tanh      tanh_bound(low, high): the math library's tanhf is within 5 ulp (OpenCL's limit, which the device library is built to) of a
            value of magnitude at most 1, so within 5 * 2^-24 (an ulp of a float32 in [0.5, 1) is 2^-24, smaller below); times half.  The
            product half * tanh and the sum mid + product round once each, half a spacing of float32(max(|low|, |high|)) at the most
            apiece (|product| <= half <= max, |sum| <= max): together one spacing.
  gaussian  bound(greedy) + sigma * Z_BOUND + spacing(float32(|greedy| + sigma * |z|)): greedy's own error, z's scaled by sigma, and the
            product sigma * z and the sum greedy + product rounded once each, neither larger than |greedy| + sigma * |z| (half a spacing
            of it apiece).  The clamp to [low, high] is 1-Lipschitz, so the bound survives it.
  sample    0: low + (high - low) * u01_24(A) in float32, operation by operation (tests/_actor_box_forms.py sample)."""
import numpy as np

import _actor_box_forms as box
import _space_sampling_ref as ref
from oracle import numpy_ref

F32 = np.float32
NOISE_STREAM = 0xA0761D6478BD642F
HEADS = {"clamp": 0, "tanh": 1}
EXPLORES = {"sample": 0, "gaussian": 1}
Z_BOUND = ref.UNBOUNDED_BOUND
TWO24 = 16777216.0


def lanes_of(lane0, n):
    return np.uint64(int(lane0)) + np.arange(n, dtype=np.uint64)


def words(seed, lane0, tick, n):
    """(A, B, N) uint32 [n] of global lanes lane0 .. lane0 + n - 1 at (seed, tick)"""
    lanes = lanes_of(lane0, n)
    a, b = numpy_ref.action_words(int(seed), lanes, int(tick))
    pick = (lanes & np.uint64(3)).astype(np.intp)
    noise = numpy_ref.reset_words(int(seed) ^ NOISE_STREAM, lanes >> np.uint64(2), int(tick))[pick, np.arange(n)]
    return a, b, noise


def explore_mask(words_b, eps):
    return np.asarray(words_b, np.uint32) <= np.uint32(box.coin_threshold(eps))


def z64(words_a, words_n):
    """z = sqrt(-2 ln u1) * cos(2 pi u2), u1 = ((A >> 8) + 1) / 2^24 in (0, 1], u2 = (N >> 8) / 2^24 in [0, 1)"""
    u1 = ((np.asarray(words_a, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) / TWO24
    u2 = (np.asarray(words_n, np.uint32) >> np.uint32(8)).astype(np.float64) / TWO24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def tanh_bound(low, high):
    half = 0.5 * (float(F32(high)) - float(F32(low)))
    return half * 5.0 * 2.0 ** -24 + float(np.spacing(F32(max(abs(float(low)), abs(float(high))))))


def greedy64(raw, low, high, head):
    """(greedy float64, bound) of the float32 outputs `raw`"""
    raw = np.asarray(raw, F32)
    if head == "clamp":
        return box.clamp(raw, low, high).astype(np.float64), np.zeros(len(raw))
    assert head == "tanh"
    low, high = float(F32(low)), float(F32(high))
    return 0.5 * (low + high) + 0.5 * (high - low) * np.tanh(raw.astype(np.float64)), np.full(len(raw), tanh_bound(low, high))


def act64(raw, words_a, words_b, words_n, eps, low, high, head, explore, sigma):
    """(action float64, bound, explore mask) of one act call under the policy (head, explore, sigma)"""
    g, gb = greedy64(raw, low, high, head)
    mask = explore_mask(words_b, eps)
    if explore == "sample":
        drawn, db = box.sample(words_a, low, high).astype(np.float64), np.zeros(len(g))
    else:
        assert explore == "gaussian"
        z = z64(words_a, words_n)
        sigma = float(F32(sigma))
        drawn = np.clip(g + sigma * z, float(F32(low)), float(F32(high)))
        db = gb + sigma * Z_BOUND + np.spacing((np.abs(g) + sigma * np.abs(z)).astype(F32)).astype(np.float64)
    return np.where(mask, drawn, g), np.where(mask, db, gb), mask
