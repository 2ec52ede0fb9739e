"""rows_theta_chain_dpp (auv_sim_amd/csrc/rrt_rows_kernel.h) on its own, through the auvp_theta_chain_dev probe: the ordered sum
theta += phi of a steer pass, for the four 16-lane rows of a wavefront at once, one v_fmac_f64_dpp (row_newbcast) per step with a
multiplier of 1.0.  Lane rl of a row must end with (((theta0 + phi_0) + phi_1) + ... + phi_rl) of ITS row, bit for bit what a plain
left-to-right float64 sum gives: fma(phi, 1.0, th) rounds th + phi once.  A pass has fifteen sub-arcs, the chain fifteen steps
(phi_0 .. phi_14): lane 15, which carries the pass-entry angle in the kernels, ends with lane 14's sum and its own phi is never
added -- the reference below says so too, so a sixteenth step or a phi_15 that leaked into another lane shows.  The four rows of
every wavefront carry different data, so a broadcast that crossed a row boundary, a step under the wrong mask or a lane that took
another lane's start angle shows.
Where a sum is a NaN (inf + -inf) only the NaN pattern is compared, not the payload."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W = 2048  # wavefronts per case


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _reference(theta0, phi):
    """theta0 [W, 4], phi [W, 64] -> [W, 64]: per row, acc = theta0; acc = acc + phi_j, j = 0 .. 14, every prefix kept; lane 15
    has the last one"""
    rows = phi.reshape(-1, 4, 16)
    out = np.empty_like(rows)
    acc = theta0.astype(np.float64).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(15):
            acc = acc + rows[:, :, j]
            out[:, :, j] = acc
    out[:, :, 15] = acc
    return out.reshape(-1, 64)


def _check(ctx, theta0, phi):
    theta0, phi = np.ascontiguousarray(theta0, dtype=np.float64), np.ascontiguousarray(phi, dtype=np.float64)
    assert theta0.shape == (W, 4) and phi.shape == (W, 64)
    # the rows of a wavefront differ (what makes a crossed row boundary visible)
    r = phi.reshape(W, 4, 16).view(np.uint64)
    assert all((r[:, a] != r[:, b]).any(axis=1).mean() > 0.9 for a in range(4) for b in range(a))
    got, ref = ctx.theta_chain(theta0, phi), _reference(theta0, phi)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(np.isinf(got), np.isinf(ref))
    same = got.view(np.uint64) == ref.view(np.uint64)
    bad = np.argwhere(~(same | nan))
    assert len(bad) == 0, (len(bad), bad[:4], got[tuple(bad[0])], ref[tuple(bad[0])])
    return ref


def _magnitudes(rnd, shape, center, spread):
    e = np.clip(center + spread * rnd.standard_normal(shape), -300.0, 299.5)
    return rnd.choice([-1.0, 1.0], shape) * (rnd.uniform(1.0, 10.0, shape) * 10.0 ** np.floor(e))     # 1e-300 <= |.| < 1e300


def test_random_magnitudes_1e_minus_300_to_1e300_mixed_signs(ctx):
    """a row's exponents scatter round a centre of its own by 0, 3, 20 or 300 decades: sums of like magnitudes that cancel, addends
    far below the running sum that are absorbed, and everything between; a quarter of the lanes negate their left neighbour"""
    rnd = np.random.default_rng(20261020)
    center = rnd.uniform(-300.0, 300.0, (W, 4, 1))
    spread = rnd.choice([0.0, 3.0, 20.0, 300.0], (W, 4, 1))
    phi = _magnitudes(rnd, (W, 4, 16), center, spread)
    neg = rnd.random((W, 4, 16)) < 0.25
    neg[:, :, 0] = False
    for j in range(1, 16):
        phi[:, :, j] = np.where(neg[:, :, j], -phi[:, :, j - 1], phi[:, :, j])
    theta0 = _magnitudes(rnd, (W, 4), center[:, :, 0], spread[:, :, 0])
    assert 1e-300 <= np.abs(phi).min() < 1e-250 and 1e250 < np.abs(phi).max() <= 1e300
    ref = _check(ctx, theta0, phi.reshape(W, 64))
    rows = ref.reshape(W, 4, 16)
    absorbed = (rows[:, :, 1:] == rows[:, :, :-1]).mean()        # an addend that changed nothing
    cancelled = (np.abs(rows[:, :, 1:]) < 1e-3 * np.abs(rows[:, :, :-1])).mean()
    assert absorbed > 0.05 and cancelled > 0.02, (absorbed, cancelled)


@pytest.mark.parametrize("start", [0.0, -0.0])
def test_zero_phis_of_either_sign(ctx, start):
    """-0 + -0 = -0, every other sum of zeros +0: the sign of the zero is part of the angle's bits"""
    rnd = np.random.default_rng(7)
    phi = np.where(rnd.random((W, 64)) < 0.5, 0.0, -0.0)
    phi[0] = -0.0       # one wavefront of -0 only, one of +0 only
    phi[1] = 0.0
    theta0 = np.full((W, 4), start)
    theta0[W // 2:, 1::2] = -start    # (half of the wavefronts: rows of either start)
    got = ctx.theta_chain(theta0, phi)
    ref = _reference(theta0, phi)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    assert np.signbit(ref).any() and (~np.signbit(ref)).any()
    if np.signbit(start):
        assert np.signbit(got[0]).all()


def test_subnormal_phis_and_start(ctx):
    """sums that stay below 2^-1022, and sums that cross into the normal range and back"""
    rnd = np.random.default_rng(11)
    tiny = np.float64(5e-324)
    phi = rnd.choice([-1.0, 1.0], (W, 64)) * rnd.integers(1, 1 << 52, (W, 64)).astype(np.float64) * tiny
    big = rnd.random((W, 64)) < 0.1
    phi[big] = rnd.choice([-1.0, 1.0], big.sum()) * rnd.uniform(1.0, 4.0, big.sum()) * 2.0 ** -1022
    theta0 = rnd.choice([-1.0, 1.0], (W, 4)) * rnd.integers(0, 1 << 52, (W, 4)).astype(np.float64) * tiny
    ref = _check(ctx, theta0, phi)
    sub = (np.abs(ref) < 2.0 ** -1022) & (ref != 0.0)
    assert sub.mean() > 0.3 and (~sub).mean() > 0.1


def test_round_to_even_ties(ctx):
    """1e16 + 1.0 and its kin: above 2^53 an odd addend lies exactly between two doubles, and the sum goes to the even one"""
    rnd = np.random.default_rng(13)
    theta0 = rnd.choice([-1.0, 1.0], (W, 4)) * (2.0 ** 53 + 2.0 * rnd.integers(0, 1 << 20, (W, 4)).astype(np.float64))
    theta0[:, 0] = np.where(rnd.random(W) < 0.5, 1e16, -1e16)
    phi = rnd.choice([-3.0, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0, 3.0, 5.0], (W, 64))
    phi[:, :16] = rnd.choice([-1.0, 1.0], (W, 16))
    ref = _check(ctx, theta0, phi)
    # 1e16 +- 1.0 lies between 1e16 and its neighbour (the spacing is 2.0 on both sides); 1e16's significand is even
    assert (ref.reshape(W, 4, 16)[:, 0, 0] == theta0[:, 0]).all()


def test_an_infinity_in_one_lane(ctx):
    """every lane from the infinite one on is infinite, the lanes before it are not; a second infinity of the other sign later in
    the row makes NaNs from there on (pattern compared, not payload)"""
    rnd = np.random.default_rng(17)
    phi = rnd.uniform(-3.0, 3.0, (W, 64))
    lane = rnd.integers(0, 64, W)     # (lane 15 of a row among them: its infinity must reach nobody)
    sign = rnd.choice([-1.0, 1.0], W)
    phi[np.arange(W), lane] = sign * np.inf
    second = (np.arange(W) % 3 == 0) & (lane % 16 < 15)
    lane2 = lane + rnd.integers(1, np.maximum(16 - lane % 16, 2))     # a later lane of the same row
    phi[np.arange(W)[second], lane2[second]] = -sign[second] * np.inf
    theta0 = rnd.uniform(-3.2, 3.2, (W, 4))
    ref = _check(ctx, theta0, phi)
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).mean() > 0.5
    rows, k = ref.reshape(W, 4, 16), np.arange(W)
    assert np.isfinite(rows[k, lane // 16, :][np.arange(16)[None, :] < (lane % 16)[:, None]]).all()
