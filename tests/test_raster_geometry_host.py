"""CPU checks of the frame kernels' case table (tests/_raster_geometry_cases.py), which tests/test_gpu_raster_geometry.py holds the
kernels to: the table is the one agreed on, every case keeps the twin's ambiguous pixels under the cap (a condition of the table, so a
new state that breaks it is the thing to change), and every case would notice each of five deliberate mistakes in the rasteriser's
arithmetic — or says in the table why it cannot."""
import numpy as np
import pytest

import _raster_geometry_cases as cases
import _render_twin as twin

DTYPES = [np.float32, np.float64]


def test_the_table_and_the_state_set():
    assert twin.EPS == 1e-3 and cases.AMBIGUOUS_CAP == 0.002
    assert len(cases.NAMES) == 13
    assert [cases.crop_size(k) for k in cases.NAMES] == [
        ((0, 0, 600, 400), (1, 1)), ((0, 0, 600, 400), (5, 3)), ((0, 0, 600, 400), (1, 37)), ((0, 0, 600, 400), (17, 61)),
        ((200, 150, 200, 150), (84, 84)), ((270, 240, 64, 80), (256, 320)), ((299, 294, 2, 2), (64, 64)), ((0, 299, 600, 2), (16384, 1)),
        ((299, 0, 2, 400), (1, 16384)), ((0, 0, 50, 50), (10, 10)), ((550, 290, 50, 20), (25, 10)), ((37, 101, 501, 263), (97, 53)),
        ((0, 0, 600, 400), (160, 210))]
    assert [k for k in cases.NAMES if k not in cases.SMALL] == ["up4"]
    assert (cases.pixels("17x61"), cases.waves("17x61"), cases.pixels("17x61") - 1024) == (1037, 2, 13)
    for k in cases.NAMES:                                  # an exemption names a mistake and gives a reason
        assert set(cases.CASES[k][3]) <= set(cases.MISTAKES) and all(len(why) > 20 for why in cases.CASES[k][3].values())
        (_, _, cw, ch), (w, h) = cases.crop_size(k)
        assert (cases.SWAP in cases.CASES[k][3]) == (cw * h == ch * w or k == "background"), k
    assert [k for k in cases.NAMES if len(cases.CASES[k][3]) == len(cases.MISTAKES)] == ["background"]
    f32max = np.finfo(np.float32).max
    for dtype in DTYPES:
        s = cases.states(dtype)
        rows = set(zip(s[0].tolist(), s[2].tolist()))
        assert s.dtype == dtype and s.shape == (4, 56 + 40 + 6 + 3 + (dtype == np.float64))
        finite, rest = cases.edge_rows()
        assert len(finite) + len(rest) == 56
        for x, t in finite + [(0.3, 7.0e4), (-0.3, -1.0e4), (1e30, 0.1), (f32max, 0.1)]:
            assert (dtype(x).item(), dtype(t).item()) in rows, (x, t)
        assert ((s[0] == 0) & np.signbit(s[0]) & (s[2] == 0) & np.signbit(s[2])).any()                        # (-0.0, -0.0)
        tiny = (s[0] > 0) & (s[0] < np.finfo(np.float32).tiny)
        assert tiny.any() and (s[0, tiny] == dtype(1e-40)).all() and (s[2, tiny] == dtype(1e-40)).all()
        assert ((s[0].astype(np.float64) == 1e300) & (s[2].astype(np.float64) == 1e300)).any() == (dtype == np.float64)
        assert (~np.isfinite(s[0]) | ~np.isfinite(s[2])).sum() == 7
        sub = cases.states(dtype, "up4")
        assert sub.shape == (4, cases.SUBSET) and sub.tobytes() == np.ascontiguousarray(s[:, :cases.SUBSET]).tobytes()
        assert (~np.isfinite(sub[0]) | ~np.isfinite(sub[2])).sum() == 7                                       # the subset keeps them
        rnd = s[:, -40:]
        assert (np.abs(rnd[0]) < 2.6).all() and (np.abs(rnd[2]) < np.pi).all() and np.abs(rnd[2]).max() > 2.5


def test_frames_of_is_twin_render():
    s = cases.states(np.float64)
    for name in ("1x1", "5x3", "edge", "17x61"):
        crop, size = cases.crop_size(name)
        rgb, gray, amb = cases.frames_of(s[0], s[2], crop, size)
        for fmt, got in ((twin.RGB8, rgb), (twin.GRAY8, gray)):
            want, want_amb = twin.render(s[0], s[2], fmt, crop, size)
            assert np.array_equal(got, want) and np.array_equal(amb, want_amb) and got.dtype == want.dtype
        again = cases.mistaken_gray(s[0], s[2], crop, size, None)                 # the local painter without a mistake paints the same
        assert np.array_equal(again, gray)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", cases.NAMES)
def test_ambiguous_share_stays_under_the_cap(name, dtype):
    """Over all lanes and pixels of the case.  Measured: 0.00062 at 160x210, 0.00038 at up4, 0.00025 at wide, 0.00015 at edge, at or
    below 0.00009 everywhere else."""
    amb = cases.truth(name, dtype)["amb"]
    share = float((amb > 0).mean())
    print(f"{name}: {amb.shape[0]} lanes, ambiguous share {share:.5f}")
    assert share <= cases.AMBIGUOUS_CAP


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_notices_each_mistake(name):
    """The twin's painter restated with one mistake (cases.mistaken_gray) must fail twin.compare against the correct twin frame on at
    least one lane of the case's float32 state set — unless the table exempts the mistake for this case, and then it must indeed not
    show (an exemption that has become untrue is removed, not kept)."""
    crop, size = cases.crop_size(name)
    s = cases.states(np.float32, name)
    t = cases.truth(name, np.float32)
    exempt = cases.CASES[name][3]
    step = max(1, (1 << 21) // (16 * cases.pixels(name)))
    for mistake in cases.MISTAKES:
        noticed = False
        for b in range(0, s.shape[1], step):
            got = cases.mistaken_gray(s[0, b:b + step], s[2, b:b + step], crop, size, mistake)
            try:
                twin.compare(got, t[twin.GRAY8][b:b + step], t["amb"][b:b + step])
            except AssertionError:
                noticed = True
                break
        assert noticed == (mistake not in exempt), (name, mistake, exempt.get(mistake))
