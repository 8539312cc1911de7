"""GPU tests of the hand-written gather's push kernel (kernels.hip push_obs_kernel / launch_push_obs) through
gymnet_push_obs_device, against a plain copy: dst[p][off : off + count] = src[:count] in NumPy, compared word for word
through uint32 / uint64 views (NaN payloads, infinities and signed zeros count), everything outside the range still poison.

What each test reaches (counts are 4-byte words; the peers are separate allocations on device 0):

  - test_small_counts_at_every_alignment: counts 0..8 and 1023..1025 at all 16 (source, destination) misalignments of
    0..3 words — the destination's mixed inside ONE call (four peers offset 0, 1, 2, 3), since `vec_ok` is decided per
    blockIdx.y.  Only (0, 0) takes the dwordx4 branch and its tail loop (k = (nvec << 2) + i); the other 15 take the scalar
    branch.  count < 4 is a launch whose vector loop has no trip at all.
  - test_grid_stride_trips: launch_push_obs caps the grid at 256 workgroups of 256 threads per peer, so 4 * 256 * 256 words is
    the last size one trip of the dwordx4 loop covers (and already four trips of the scalar loop); + 1 and + 3 add the tail
    behind a full grid, + 7 is the first size at which a thread takes a second dwordx4 trip, and 3 * 2^18 + 2 runs three
    dwordx4 trips / thirteen scalar trips — every one at all four source misalignments and four destination misalignments.
  - test_peer_counts: npeers 0, 1, 2, 7 and 15 (kMaxPeers), the peers' misalignments mixed, a poison-filled bystander that is
    not in the list; npeers = 0 also with a null list.
  - test_float64_rows_as_two_words_per_element: a float64 array counted the way allgather() and ShardedVectorEnv._push count
    it (two words per element), source and destinations 8 bytes off a 16-byte line.
  - test_refusals_leave_every_destination_untouched: npeers 16 and -1, count -1, a null source, a null list with npeers > 0
    and a null entry inside the list are GYMNET_ERR_INVALID_ARG, and nothing was launched.

Every destination range is fenced by GUARD poison words on both sides; each case runs well under a second.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 8                       # poison words before and after every destination range (a multiple of 4: the range's alignment is its offset's)
POISON = 0xDEADBEEF
SPECIALS = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x7FFFFFFF], np.uint32)
SMALL_COUNTS = [0, 1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025]
FULL_GRID = 4 * 256 * 256       # words one trip of the dwordx4 loop covers at the capped grid
BIG_COUNTS = [FULL_GRID, FULL_GRID + 1, FULL_GRID + 3, FULL_GRID + 7, 3 * FULL_GRID + 2]


def _payload(rng, nwords):
    """random bit patterns with quiet / signalling NaNs, both infinities, -0.0, a denormal — first and last word included"""
    w = rng.integers(0, 1 << 32, nwords, dtype=np.uint64).astype(np.uint32)
    if nwords:
        at = rng.integers(0, nwords, max(1, nwords // 16))
        w[at] = SPECIALS[rng.integers(0, len(SPECIALS), at.shape[0])]
        w[0], w[-1] = SPECIALS[0], SPECIALS[5]
    w[w == POISON] ^= 1
    return w


def _device_words(torch, words):
    t = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()
    assert t.data_ptr() % 16 == 0                     # the misalignments below are measured from a 16-byte line
    return t


def _poisoned(torch, nwords):
    return _device_words(torch, np.full(nwords, POISON, np.uint32))


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _call(pkg, src_ptr, dst_ptrs, npeers, count):
    lib = pkg.load_library()
    arr = None if dst_ptrs is None else (C.c_void_p * max(1, len(dst_ptrs)))(*dst_ptrs)
    return lib.gymnet_push_obs_device(0, None, None if src_ptr is None else C.c_void_p(src_ptr), arr, npeers, count)


def _push_and_check(pkg, torch, src, src_off, peers, dst_offs, count, bystander=None, null_list=False):
    """One call: src[src_off : src_off + count] into peers[p][GUARD + dst_offs[p] :][:count]; every peer (and the bystander)
    is re-poisoned first and compared as a whole afterwards."""
    for t in peers + ([bystander] if bystander is not None else []):
        t.fill_(int(np.uint32(POISON).view(np.int32)))
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() + 4 * (GUARD + o) for t, o in zip(peers, dst_offs)]
    st = _call(pkg, src.data_ptr() + 4 * src_off, None if null_list else ptrs, len(peers), count)
    assert st == pkg._capi.OK, (st, pkg._capi.last_error())
    torch.cuda.synchronize()
    want_src = _words(src)[src_off:src_off + count]
    for p, (t, o) in enumerate(zip(peers, dst_offs)):
        want = np.full(t.numel(), POISON, np.uint32)
        want[GUARD + o:GUARD + o + count] = want_src              # the plain copy
        got = _words(t)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"count {count}, source +{src_off} words, peer {p} of {len(peers)} +{o} words: {bad.size} words differ, "
                               f"first at {bad[:4] - GUARD - o} of the range")
    if bystander is not None:
        assert (_words(bystander) == POISON).all()


@pytest.mark.parametrize("count", SMALL_COUNTS)
def test_small_counts_at_every_alignment(gpu_pkg, count):
    import torch
    rng = np.random.default_rng(1000 + count)
    src = _device_words(torch, _payload(rng, count + 3))
    peers = [_poisoned(torch, GUARD + 3 + count + GUARD) for _ in range(4)]
    bystander = _poisoned(torch, GUARD + 3 + count + GUARD)
    for src_off in range(4):
        _push_and_check(gpu_pkg, torch, src, src_off, peers, [0, 1, 2, 3], count, bystander)
    _push_and_check(gpu_pkg, torch, src, 0, peers, [0, 0, 0, 0], count, bystander)       # every block row on the dwordx4 branch
    _push_and_check(gpu_pkg, torch, src, 0, peers, [3, 2, 1, 0], count, bystander)       # the aligned peer last


@pytest.mark.parametrize("count", BIG_COUNTS)
def test_grid_stride_trips(gpu_pkg, count):
    import torch
    rng = np.random.default_rng(count)
    src = _device_words(torch, _payload(rng, count + 3))
    peers = [_poisoned(torch, GUARD + 3 + count + GUARD) for _ in range(4)]
    for src_off in range(4):
        _push_and_check(gpu_pkg, torch, src, src_off, peers, [(src_off + p) % 4 for p in range(4)], count)


@pytest.mark.parametrize("npeers", [0, 1, 2, 7, 15])
def test_peer_counts(gpu_pkg, npeers):
    import torch
    count = 4 * 257 + 1                       # two workgroups per peer, a one-word tail
    rng = np.random.default_rng(npeers)
    src = _device_words(torch, _payload(rng, count + 3))
    peers = [_poisoned(torch, GUARD + 3 + count + GUARD) for _ in range(npeers)]
    bystander = _poisoned(torch, GUARD + 3 + count + GUARD)
    for src_off in (0, 1):
        _push_and_check(gpu_pkg, torch, src, src_off, peers, [(3 * p) % 4 for p in range(npeers)], count, bystander)
    _push_and_check(gpu_pkg, torch, src, 0, peers, [0] * npeers, count, bystander)
    if npeers == 0:
        _push_and_check(gpu_pkg, torch, src, 0, [], [], count, bystander, null_list=True)


def test_float64_rows_as_two_words_per_element(gpu_pkg):
    """A float64 slice [D = 4][n = 1001] moves as 2 * D * n words; element offsets of 0 and 1 put the source and the
    destinations on and 8 bytes off a 16-byte line (what rank 1 of a two-rank float64 gather with odd D * n sees)."""
    import torch
    rng = np.random.default_rng(64)
    elems = 4 * 1001
    bits = rng.integers(0, 1 << 63, elems + 1, dtype=np.uint64) | (rng.integers(0, 2, elems + 1, dtype=np.uint64) << np.uint64(63))
    bits[[0, 5, elems - 1, elems]] = np.array([0x7FF8000000000001, 0xFFF0000000000000, 0x8000000000000000, 0x7FF0000000000001], np.uint64)
    poison64 = np.uint64(POISON << 32 | POISON)
    bits[bits == poison64] ^= np.uint64(1)
    src = torch.from_numpy(bits.view(np.float64)).cuda()
    guard = GUARD // 2                        # in elements
    poison = np.full(guard + 1 + elems + guard, poison64, np.uint64).view(np.float64)
    for src_off in (0, 1):
        peers = [torch.from_numpy(poison.copy()).cuda() for _ in range(3)]
        offs = [0, 1, 1 - src_off]
        torch.cuda.synchronize()
        assert src.data_ptr() % 16 == 0 and all(t.data_ptr() % 16 == 0 for t in peers)
        ptrs = [t.data_ptr() + 8 * (guard + o) for t, o in zip(peers, offs)]
        st = _call(gpu_pkg, src.data_ptr() + 8 * src_off, ptrs, 3, elems * (src.element_size() // 4))
        assert st == gpu_pkg._capi.OK, gpu_pkg._capi.last_error()
        torch.cuda.synchronize()
        for t, o in zip(peers, offs):
            want = poison.view(np.uint64).copy()
            want[guard + o:guard + o + elems] = bits[src_off:src_off + elems]
            assert np.array_equal(t.cpu().numpy().view(np.uint64), want), (src_off, o)


def test_refusals_leave_every_destination_untouched(gpu_pkg):
    import torch
    capi = gpu_pkg._capi
    count = 1025
    src = _device_words(torch, _payload(np.random.default_rng(3), count))
    peers = [_poisoned(torch, GUARD + count + GUARD) for _ in range(16)]
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() + 4 * GUARD for t in peers]
    holed = list(ptrs[:4])
    holed[2] = None
    refused = {
        "npeers = 16": (src.data_ptr(), ptrs, 16, count),
        "npeers = -1": (src.data_ptr(), ptrs, -1, count),
        "count = -1": (src.data_ptr(), ptrs[:4], 4, -1),
        "null source": (None, ptrs[:4], 4, count),
        "null list": (src.data_ptr(), None, 4, count),
        "null entry": (src.data_ptr(), holed, 4, count),
    }
    for what, args in refused.items():
        assert _call(gpu_pkg, *args) == capi.ERR_INVALID_ARG, what
        torch.cuda.synchronize()
        for p, t in enumerate(peers):
            assert (_words(t) == POISON).all(), (what, p)
    with pytest.raises(ValueError):
        capi.check(_call(gpu_pkg, src.data_ptr(), ptrs, 16, count))
    assert _call(gpu_pkg, src.data_ptr(), ptrs[:15], 15, count) == capi.OK            # the same list, one shorter, is served
    torch.cuda.synchronize()
    assert all(np.array_equal(_words(t)[GUARD:GUARD + count], _words(src)) for t in peers[:15]) and (_words(peers[15]) == POISON).all()
