"""The LDS plan of rrt_rows_stream_kernel's two ring forms and the host's choice between them (no GPU: the plan and the rule
are host code, auvp_rrt_rows_stream_shape).

masked    256 doubles per episode, every read forms (position + j) & 255;
mirrored  256 + 48: the first 48 entries a second time behind the ring, reads at one address per lane plus an immediate.
The mirrored form costs 384 B per episode.  A wavefront fewer per workgroup costs 8.7 % (profiles/r6_rows_waves.md), so the
host takes the mirror only where its plan fits at the wave count the masked plan allows."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LDS_LIMIT = 160 * 1024
OBST_TILE = 256 * (8 + 8 + 4)          # RW_MAX_OBST slots of x, y (f64) and the cull radius (f32)
SCRATCH = 4 * 18 * 8                   # the running sums


def _bins(K):
    return ((K + 2) * 2 + 15) & ~15


def _expected(K, tables, waves, mirror):
    per_ep = (256 + (48 if mirror else 0)) * 8 + SCRATCH + _bins(K)
    return ((tables + 15) & ~15) + waves * 4 * per_ep + OBST_TILE


def _tables(H, V, T):
    from auv_sim_amd import _lib
    # (the table bytes of a world: what an empty plan of one wave holds beside its four episodes and the tile)
    w, m, lds = _lib.rows_stream_shape(0, H, V, T, waves_wanted=1, force=0)
    return lds - _expected(0, 0, 1, False)


def test_mirrored_plan_of_the_headline_fits_twelve_waves():
    from auv_sim_amd import _lib
    from bench_sides.common import RRT_KW, bench_world
    world = bench_world(256, 200)
    H, V, T = len(world["habitats"]), len(world["polygon"]), len(world["bins"])
    K = int(round(RRT_KW.get("max_traj_time", 500.0) / RRT_KW.get("bin_interval", 5)))
    assert K == 100
    waves, mirror, lds = _lib.rows_stream_shape(K, H, V, T, waves_wanted=12)
    assert (waves, mirror) == (12, True)
    assert lds == _expected(K, _tables(H, V, T), 12, True)
    assert lds <= 163840
    # per episode: 2 832 B masked, 3 216 B mirrored
    masked = _lib.rows_stream_shape(K, H, V, T, waves_wanted=12, force=0)
    assert masked[:2] == (12, False) and lds - masked[2] == 48 * (3216 - 2832)
    # 64 mirrored entries would not have fitted
    assert lds + 48 * 16 * 8 > 163840


def test_the_rule_never_gives_up_a_wavefront_for_the_mirror():
    from auv_sim_amd import _lib
    n_mirror = n_masked = 0
    for K in list(range(1, 140, 3)) + list(range(140, 700, 37)):
        for H, V, T in ((0, 0, 0), (10, 4, 10), (40, 12, 10), (64, 64, 40), (200, 100, 100)):
            tables = _tables(H, V, T)
            for want in (1, 2, 7, 11, 12):
                unmirrored = _lib.rows_stream_shape(K, H, V, T, waves_wanted=want, force=0)
                auto = _lib.rows_stream_shape(K, H, V, T, waves_wanted=want)
                forced = _lib.rows_stream_shape(K, H, V, T, waves_wanted=want, force=1)
                assert not unmirrored[1] and forced[1]
                assert auto[0] == unmirrored[0], (K, H, V, T, want, auto, unmirrored)
                assert auto[2] == _expected(K, tables, auto[0], auto[1])
                assert auto[2] <= LDS_LIMIT or auto[0] == 1
                # the mirror exactly where it fits at that count
                assert auto[1] == (_expected(K, tables, unmirrored[0], True) <= LDS_LIMIT), (K, H, V, T, want)
                assert forced[0] <= unmirrored[0] and (forced[2] <= LDS_LIMIT or forced[0] == 1)
                n_mirror += auto[1]
                n_masked += not auto[1]
    assert n_mirror > 100 and n_masked > 100, (n_mirror, n_masked)


def test_where_the_classic_kernel_fits_the_mirror_fits():
    """the host runs the four-episode kernels only where rrt_rows_kernel's own twelve-wave plan (2 496 B of generator state per
    episode) fits; the mirrored ring (2 432 B) is smaller than that state, so on every such world the rule's answer is the mirror
    and the masked form is reached through option ROWS_STREAM_MIRROR = 0 alone"""
    from auv_sim_amd import _lib
    for K in range(1, 400, 7):
        for H, V, T in ((0, 0, 0), (10, 4, 10), (64, 64, 40)):
            tables = _tables(H, V, T)
            classic = ((tables + 15) & ~15) + 48 * (624 * 4 + SCRATCH + _bins(K)) + OBST_TILE
            if classic <= LDS_LIMIT:
                assert _lib.rows_stream_shape(K, H, V, T, waves_wanted=12)[:2] == (12, True), (K, H, V, T)
