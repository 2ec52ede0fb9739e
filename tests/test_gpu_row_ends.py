"""The end of a steer pass of the four-episode RRT kernels on its own, through the auvp_row_ends_dev probe -- the text
rrt_rows_body.h runs: rows_idle_zero for the lanes past the pass's n sub-arcs, rows_theta_chain_dpp, the increments' LDS rows,
rows_sums_chain, rows_pass_ends_dpp (auv_sim_amd/csrc/rrt_rows_kernel.h).  The kernels take a row's x, y, t, length and theta after
the pass from where the five chains END (lanes 0 .. 3's sums after fifteen additions, lane 14's angle after fifteen steps, handed
to the row by 64-bit DPP moves), not from the prefix values of sub-arc n - 1.  That is the same number only if everything past n
adds nothing, for every value the sums can have: lanes from n on add -0.0 (x + -0.0 == x for every x; +0.0 would turn a sum of
-0.0 into +0.0), and entry 15 of an LDS row, which nobody sets, is never added (the probe puts a NaN there).  A row that is not
`on` keeps its state bit for bit: its four sums are not run, and its angle gets fifteen times -0.0.
Reference: numpy float64, left to right, stopped at n -- acc = start; acc = acc + inc_j, j = 0 .. n - 1 -- compared bit for bit,
the sign of a zero included, in all 16 lanes of every row.  What the lanes from n on hold in the input is noise the probe must not
look at.  n = 1 (the last sub-arc on lane 0), 2 and 15 (on lane 14: a full pass), mixed over the rows of a wavefront together with
rows that are off.  Where a sum is a NaN (inf + -inf) only the NaN pattern is compared, not the payload."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W = 64  # wavefronts per case


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _rows(rnd):
    """n and on for the four rows of every wavefront: each n in every row position, rows that are off beside rows that are on"""
    n = rnd.choice([1, 2, 15], (W, 4))
    on = (rnd.random((W, 4)) < 0.75).astype(np.float64)
    for k, v in enumerate([1, 2, 15]):      # (whatever the draw gave: wavefronts of one n only, and one with every row off)
        n[k] = v
        on[k] = 1.0
    on[3] = 0.0
    return n, on


def _reference(n, on, start, incs):
    lanes = incs.reshape(W, 5, 4, 16)
    acc = np.transpose(start, (0, 2, 1)).copy()          # [W, 5, 4]
    nn = np.where(on != 0.0, n, 0)[:, None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(15):
            acc = np.where(j < nn, acc + lanes[:, :, :, j], acc)
    return np.repeat(acc[:, :, :, None], 16, axis=3).reshape(W, 5, 64)


def _check(ctx, rnd, start, incs, n=None, on=None):
    if n is None:
        n, on = _rows(rnd)
    start, incs = np.ascontiguousarray(start, dtype=np.float64), np.ascontiguousarray(incs, dtype=np.float64)
    assert start.shape == (W, 4, 5) and incs.shape == (W, 5, 64)
    got, ref = ctx.row_ends(n, on, start, incs), _reference(n, on, start, incs)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    same = got.view(np.uint64) == ref.view(np.uint64)
    bad = np.argwhere(~(same | nan))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], ref[tuple(bad[0])], n[bad[0][0]], on[bad[0][0]])
    # a row that is off has the state it came with, payloads and all
    off = np.repeat((on == 0.0)[:, None, :, None], 16, axis=3).repeat(5, axis=1).reshape(W, 5, 64)
    assert np.array_equal(got.view(np.uint64)[off], np.repeat(np.transpose(start, (0, 2, 1))[:, :, :, None], 16, axis=3)
                          .reshape(W, 5, 64).view(np.uint64)[off])
    return n, on, ref


def _magnitudes(rnd, shape, center, spread):
    e = np.clip(center + spread * rnd.standard_normal(shape), -300.0, 299.5)
    return rnd.choice([-1.0, 1.0], shape) * (rnd.uniform(1.0, 10.0, shape) * 10.0 ** np.floor(e))     # 1e-300 <= |.| < 1e300


def test_random_magnitudes_1e_minus_300_to_1e300_mixed_signs(ctx):
    """a row's exponents scatter round a centre of its own by 0, 3, 20 or 300 decades: sums that cancel, addends that are absorbed,
    and everything between"""
    rnd = np.random.default_rng(20261021)
    center = rnd.uniform(-300.0, 300.0, (W, 5, 4, 1))
    spread = rnd.choice([0.0, 3.0, 20.0, 300.0], (W, 5, 4, 1))
    incs = _magnitudes(rnd, (W, 5, 4, 16), center, spread).reshape(W, 5, 64)
    start = np.transpose(_magnitudes(rnd, (W, 5, 4), center[..., 0], spread[..., 0]), (0, 2, 1))
    assert 1e-300 <= np.abs(incs).min() < 1e-200 and 1e200 < np.abs(incs).max() <= 1e300
    n, on, ref = _check(ctx, rnd, start, incs)
    # the sums are not the start values (the chains ran) and differ between the rows of a wavefront
    moved = ref.reshape(W, 5, 4, 16)[:, :, :, 0] != np.transpose(start, (0, 2, 1))
    assert moved[np.repeat((on != 0.0)[:, None, :], 5, axis=1)].mean() > 0.5


@pytest.mark.parametrize("start_zero", [0.0, -0.0])
def test_zeros_of_either_sign(ctx, start_zero):
    """-0 + -0 = -0, every other sum of zeros +0: a row whose start and first n addends are all -0.0 must END at -0.0 -- with +0.0
    from the idle lanes (or from entry 15) it would not"""
    rnd = np.random.default_rng(7)
    incs = np.where(rnd.random((W, 5, 64)) < 0.5, 0.0, -0.0)
    incs[0:3] = -0.0      # (n = 1, 2, 15 in all rows, every row on: _rows)
    incs[4] = 0.0
    start = np.full((W, 4, 5), start_zero)
    start[W // 2:, 1::2] = -start_zero
    n, on, ref = _check(ctx, rnd, start, incs)
    assert np.signbit(ref).any() and (~np.signbit(ref)).any()
    if np.signbit(start_zero):
        assert np.signbit(ref[0:3]).all()       # the case the idle lanes' -0.0 is there for


def test_noise_past_n_and_in_rows_that_are_off_is_never_added(ctx):
    """the lanes from n on hold NaNs, infinities and 1e300 in the input; a row that is off holds them everywhere"""
    rnd = np.random.default_rng(9)
    n, on = _rows(rnd)
    incs = rnd.uniform(-3.0, 3.0, (W, 5, 4, 16))
    noise = rnd.choice([np.nan, np.inf, -np.inf, 1e300, -1e300], (W, 5, 4, 16))
    dead = (np.arange(16)[None, None, None, :] >= n[:, None, :, None]) | (on == 0.0)[:, None, :, None]
    incs = np.where(dead, noise, incs).reshape(W, 5, 64)
    start = rnd.uniform(-100.0, 100.0, (W, 4, 5))
    _, _, ref = _check(ctx, rnd, start, incs, n, on)
    assert np.isfinite(ref).all()


def test_subnormal_addends_and_start(ctx):
    """sums that stay below 2^-1022, and sums that cross into the normal range and back"""
    rnd = np.random.default_rng(11)
    tiny = np.float64(5e-324)
    incs = rnd.choice([-1.0, 1.0], (W, 5, 64)) * rnd.integers(1, 1 << 52, (W, 5, 64)).astype(np.float64) * tiny
    big = rnd.random((W, 5, 64)) < 0.1
    incs[big] = rnd.choice([-1.0, 1.0], big.sum()) * rnd.uniform(1.0, 4.0, big.sum()) * 2.0 ** -1022
    start = rnd.choice([-1.0, 1.0], (W, 4, 5)) * rnd.integers(0, 1 << 52, (W, 4, 5)).astype(np.float64) * tiny
    _, _, ref = _check(ctx, rnd, start, incs)
    sub = (np.abs(ref) < 2.0 ** -1022) & (ref != 0.0)
    assert sub.mean() > 0.3 and (~sub).mean() > 0.05


def test_round_to_even_ties(ctx):
    """above 2^53 an odd addend lies exactly between two doubles, and the sum goes to the even one"""
    rnd = np.random.default_rng(13)
    start = rnd.choice([-1.0, 1.0], (W, 4, 5)) * (2.0 ** 53 + 2.0 * rnd.integers(0, 1 << 20, (W, 4, 5)).astype(np.float64))
    start[:, 0, :] = np.where(rnd.random((W, 5)) < 0.5, 1e16, -1e16)
    incs = rnd.choice([-3.0, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0], (W, 5, 64))
    incs[:, :, :16] = rnd.choice([-1.0, 1.0], (W, 5, 16))
    n, on, ref = _check(ctx, rnd, start, incs)
    # 1e16 +- 1.0 lies between 1e16 and its neighbour (the spacing is 2.0 on both sides); 1e16's significand is even: row 0 of the
    # wavefront with n = 1 in every row ends where it started
    assert (ref.reshape(W, 5, 4, 16)[0, :, 0, 0] == start[0, 0, :]).all()


def test_an_infinity_below_n(ctx):
    """an infinite addend below n makes the sum infinite, a second one of the other sign a NaN (pattern compared); at n or
    beyond it reaches nobody"""
    rnd = np.random.default_rng(17)
    incs = rnd.uniform(-3.0, 3.0, (W, 5, 64))
    lane = rnd.integers(0, 64, (W, 5))
    sign = rnd.choice([-1.0, 1.0], (W, 5))
    wi, qi = np.meshgrid(np.arange(W), np.arange(5), indexing="ij")
    incs[wi, qi, lane] = sign * np.inf
    second = (wi % 3 == 0) & (lane % 16 < 15)
    lane2 = np.minimum(lane + 1, 63)
    incs[wi[second], qi[second], lane2[second]] = -sign[second] * np.inf
    start = rnd.uniform(-3.2, 3.2, (W, 4, 5))
    _, _, ref = _check(ctx, rnd, start, incs)
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).mean() > 0.3
