"""RRT.replanning_session and set_shark_grids(first_bin=...) without a GPU: every argument error is raised before anything
reaches the device.  The planner object is made without its constructor (which needs a GPU) and its context is a stand-in that
fails the test if it is called."""
import numpy as np
import pytest

from auv_sim_amd.rrt_dubins import RRT, ReplanSession, put_shark_tables


class _NoDevice:
    """a context that must not be reached"""
    device = 0
    session = None

    def __getattr__(self, name):
        raise AssertionError("the device context was reached: %s" % name)


class _S:
    def __init__(self, x=0.0, y=0.0, size=0.0):
        self.x, self.y, self.theta, self.size = x, y, 0.0, size
        self.traj_time_stamp = self.plan_time_stamp = self.length = 0.0


T, CELLS = 4, [(0.0, 0.0, 10.0, 10.0), (10.0, 0.0, 20.0, 10.0), (0.0, 10.0, 10.0, 20.0)]


def _planner(n_sets=2):
    rrt = RRT.__new__(RRT)
    rrt.sharkGrid = {(50 * t, 50 * t + 50): {c: 0.1 for c in CELLS} for t in range(T)}
    rrt._bins = np.array([k for k in rrt.sharkGrid], dtype=np.float64)
    rrt._cells = np.array(CELLS, dtype=np.float64)
    rrt._set_prob = np.zeros((n_sets, T, len(CELLS))) if n_sets else None
    rrt._session, rrt._batch, rrt._ctx = None, None, _NoDevice()
    rrt.freq, rrt.dist_to_end, rrt.diff_max = 30, 2, 0.5
    return rrt


N = 4
ARGS = ([_S() for _ in range(N)], [_S(5.0, 5.0, 2.0)], 2.0, 150.0, 48.0, [-3, -3, -4])
OK = dict(max_iter=50, seeds=[1, 2, 3, 4])


@pytest.mark.parametrize("bad", [
    dict(shark_of=[0, 1, 0]),                       # a wrong length
    dict(shark_of=[0, 1, 2, 0]),                    # a table that is not there
    dict(shark_of=[0, 1, 0.5, 0]),
    dict(teams=[0, 0, 1]),
    dict(teams=[0, 0, True, 1]),
    dict(team_pick="claims"),                       # needs teams
    dict(teams=[0, 0, 1, 1], team_pick="other"),
    dict(trees_per_auv=0),
    dict(team_separation=5.0),                      # needs teams
    dict(teams=[0, 0, 1, 1], team_separation=-1.0),
    dict(teams=[0, 0, 1, 1], team_separation=5.0, separation_tick=0.0),
    dict(teams=[0, 0, 1, 1], team_separation=5.0, separation_ticks=2000),
    dict(teams=[0, 0, 1, 1], team_separation=5.0, separation_tick=1e-8),  # the horizon's end is tick 2**31 or later
    dict(seeds=None),
    dict(seeds=[1, 2, 3]),
    dict(seeds=[1, None, 3, 4]),
])
def test_replanning_session_refuses_before_any_launch(bad):
    rrt = _planner()
    with pytest.raises(ValueError):
        rrt.replanning_session(*ARGS, **dict(OK, **bad))
    assert rrt._session is None


def test_shark_of_without_tables_is_refused():
    with pytest.raises(ValueError):
        _planner(n_sets=0).replanning_session(*ARGS, shark_of=[0, 0, 0, 0], **OK)


def test_the_same_errors_as_replanning_batch():
    """one check function serves both: the first error of a call with several is the same one"""
    rrt = _planner()
    kw = dict(OK, teams=[0, 0, 1], team_pick="other", trees_per_auv=0)
    with pytest.raises(ValueError) as a:
        rrt.replanning_session(*ARGS, **kw)
    with pytest.raises(ValueError) as b:
        rrt.replanning_batch(*ARGS, commit="device", **kw)
    assert str(a.value) == str(b.value)


def test_a_second_session_and_everything_else_is_refused_while_one_is_open():
    rrt = _planner()
    open_one = ReplanSession.__new__(ReplanSession)
    open_one.inside, open_one.closed, open_one.rrt = False, False, rrt
    rrt._session = open_one
    for call in (lambda: rrt.replanning_session(*ARGS, **OK), lambda: rrt.replanning_batch(*ARGS, **OK),
                 lambda: rrt.replanning_batch(*ARGS, commit="device", **OK), lambda: rrt.set_shark_grids(None),
                 lambda: rrt.exploring_batch(ARGS[0], ARGS[1], 0.5, 5, 2, 50.0, seeds=OK["seeds"]),
                 lambda: rrt.exploring_best_of(ARGS[0], ARGS[1], 0.5, 5, 2, 50.0, seeds=[[1]] * N),
                 lambda: rrt.exploring(ARGS[0][0], ARGS[1], 0.5, 5, 2, 50.0, seed=1), lambda: rrt.rerank(None)):
        with pytest.raises(RuntimeError):
            call()
    assert rrt._session is open_one and not open_one.closed
    open_one.close()
    assert rrt._session is None and open_one.closed
    for call in (open_one.round, open_one.finish, lambda: open_one.set_shark_grids(None)):
        with pytest.raises(RuntimeError):
            call()


class _Forecast:
    def __init__(self, F, R1, cells=CELLS):
        self.prob = np.arange(F * R1 * len(cells), dtype=np.float64).reshape(F, R1, len(cells))
        self.cell_bounds = list(cells)
        self.ctx = None


@pytest.mark.parametrize("first_bin", [-1, T, T + 5, 1.0, 0.5, True, "0"])
def test_first_bin_outside_the_bins_is_refused(first_bin):
    rrt = _planner()
    with pytest.raises(ValueError):
        rrt.set_shark_grids(_Forecast(2, T), first_bin=first_bin)
    with pytest.raises(ValueError):
        rrt.set_shark_grids(_Forecast(2, 2), first_bin=first_bin)
    assert rrt._set_prob.shape == (2, T, len(CELLS))  # (refused calls change nothing)


def test_other_refusals_of_set_shark_grids():
    rrt = _planner()
    with pytest.raises(ValueError):  # without first_bin the forecast must have the planner's bin count, as before
        rrt.set_shark_grids(_Forecast(2, T - 1))
    with pytest.raises(ValueError):  # another cell list
        rrt.set_shark_grids(_Forecast(2, T, CELLS[::-1]), first_bin=1)
    with pytest.raises(ValueError):  # first_bin speaks about a forecast's rounds: dict tables have the planner's bins already
        rrt.set_shark_grids([rrt.sharkGrid], first_bin=1)


def test_host_path_places_the_rounds():
    """a forecast without a device copy goes through the host path: what reaches set_prob_sets is the placed table"""
    got = []

    class _Ctx:
        device = 0

        def set_prob_sets(self, prob=None, **kw):
            got.append(np.array(prob))

    fc = _Forecast(2, 2)
    bins, cells = np.array([(50 * t, 50 * t + 50) for t in range(T)], dtype=np.float64), np.array(CELLS)
    out = put_shark_tables(_Ctx(), bins, cells, fc, first_bin=1)
    assert len(got) == 1 and np.array_equal(got[0], out) and out.shape == (2, T, len(CELLS))
    assert np.array_equal(out, fc.prob[:, [0, 0, 1, 1], :])
    out = put_shark_tables(_Ctx(), bins, cells, _Forecast(2, T), first_bin=0)  # the identity: the forecast as it lies
    assert np.array_equal(got[1], _Forecast(2, T).prob) and np.array_equal(out, got[1])
