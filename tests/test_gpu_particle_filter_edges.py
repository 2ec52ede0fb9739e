"""pf_step_kernel (csrc/pf_kernel.h) where the G10 goldens and seeded uniform measurements never take it: the two per-filter
error statuses and the sticky status word, the 899/900-level limit of the wrap loops, a failing filter among healthy ones,
object sharing far beyond what resampling produces, the rejection sampler at acceptance ~0.5, update and draw counts that
end exactly on a state block's last word, and the particle counts at which the kernel's structure changes.

The reference is the CPU checker, oracle.orc_pf.run(..., kind="portable").  Wherever it returns status 0 the bar is
test_gpu_particle_filter.py's: array_equal on updated, choice, list_len, mean, range_error, the final particles, the object
ids, the 624 state words, mt_pos and n_draw32.  No tolerance appears in this file.  After an error status only the status
itself (and what the failing step produced before the error) is specified: the device goes on through the launch's remaining
steps, the checker stops at the end of the failing step."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TWO_PI = 2 * np.pi
PF_ERR_ANGLE, PF_ERR_EMPTY = 1, 2
# "flat weights": every particle on FLAT_ROW and one measurement FLAT_MEAS put every normalised weight in (0.8, 1], so
# `correct` makes five copies of each particle: list length exactly 5 N
FLAT_ROW = [10, 20, 1, 0.2, 0.001]
FLAT_MEAS = [600, -400, 0.1, 50, 1]


@pytest.fixture(scope="module")
def ctx():
    from auv_sim_amd import _lib
    return _lib.Context(0)


def _seed_states(seeds):
    from auv_sim_amd import _pf_lib
    return np.stack([_pf_lib.np_seed_state(int(s))[0] for s in seeds])


def _particles(rng, F, N):
    """[F,N,5] rows like Particle.__init__ makes around the origin"""
    p = np.zeros((F, N, 5))
    p[..., 0:2] = rng.uniform(-150, 150, size=(F, N, 2))
    p[..., 2] = rng.uniform(0, 5, size=(F, N))
    p[..., 3] = rng.uniform(-np.pi, np.pi, size=(F, N))
    p[..., 4] = 1.0 / 1000
    return p


def _meas(rng, S, F, A, centre=None):
    """[S,F,A,5] measurement rows and [S,F,2] shark positions like test_batches_match_checker's"""
    centre = np.zeros((F, 2)) if centre is None else np.asarray(centre, dtype=np.float64)
    m = np.zeros((S, F, A, 5))
    m[..., 0:2] = centre[None, :, None, :] + rng.uniform(-200, 200, size=(S, F, A, 2))
    m[..., 2] = rng.uniform(-np.pi, np.pi, size=(S, F, A))
    m[..., 3] = rng.uniform(0, 300, size=(S, F, A))
    m[..., 4] = rng.uniform(-np.pi, np.pi, size=(S, F, A))
    return m, centre[None] + rng.uniform(-30, 30, size=(S, F, 2))


class _Out:
    """everything a batch reports after a logged run"""

    def __init__(self, b):
        self.upd, self.cho = b.step_log()
        self.mean, self.err, self.ll = b.estimates()
        self.final, self.obj = b.particles()
        self.st, self.nd = b.status()
        self.mt, self.pos = b.rng_state()


def _assert_steps(o, f, ref, n, ref0=0, what=""):
    """steps [0, n) of the launch == steps [ref0, ref0 + n) of the checker's run"""
    r = slice(ref0, ref0 + n)
    assert np.array_equal(o.upd[:n, f], ref["updated"][r]), (what, f, "updated")
    assert np.array_equal(o.cho[:n, f], ref["choice"][r]), (what, f, "choice")
    assert np.array_equal(o.ll[:n, f], ref["list_len"][r]), (what, f, "list_len")
    assert np.array_equal(o.mean[:n, f], ref["mean"][r]), (what, f, "mean")
    assert np.array_equal(o.err[:n, f], ref["range_error"][r]), (what, f, "range_error")


def _assert_rng(o, f, ref, what=""):
    assert np.array_equal(o.mt[f], ref["mt"]), (what, f, "mt")
    assert (int(o.pos[f]), int(o.nd[f])) == (ref["mt_pos"], ref["n_draw32"]), (what, f, "mt_pos, n_draw32")


def _assert_end(o, f, ref, what=""):
    assert o.st[f] == 0, (what, f, "status")
    assert np.array_equal(o.final[f], ref["resampled"][-1]), (what, f, "final particles")
    assert np.array_equal(o.obj[f], ref["choice"][-1]), (what, f, "object ids")
    _assert_rng(o, f, ref, what)


def _assert_all(o, f, ref, what=""):
    """the latest launch of a healthy filter == the last steps of the checker's whole run, and the same state after it"""
    assert ref["status"] == 0, (what, f, "checker status")
    n = len(o.ll)
    _assert_steps(o, f, ref, n, len(ref["list_len"]) - n, what)
    _assert_end(o, f, ref, what)


def _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark, obj=None, list_len=None):
    """set_particles + one logged launch; the checker's runs from the same lists"""
    from auv_sim_amd import _pf_lib
    F, N = parts.shape[:2]
    b = _pf_lib.FilterBatch(ctx, F, N).set_particles(parts, mts, pos, obj=obj, list_len=list_len)
    b.run(meas=meas, shark_xy=shark, log=True)
    refs = [orc_pf.run(N, meas[:, f], shark[:, f], (0.0, 0.0), mts[f], int(pos[f]), init=parts[f],
                       init_obj=None if obj is None else obj[f], kind="portable") for f in range(F)]
    return b, _Out(b), refs


# ---- A1: the 899/900-level limit of angle_wrap and the 900 subtractions of velocity_wrap

def test_theta_wrap_limit(ctx, orc):
    """a particle 899 turns away is wrapped (899 adds: the deepest chain the checker's 900-level loop accepts), 900 turns away
    (and 1e4 rad) is PF_ERR_ANGLE"""
    from oracle import orc_pf
    thetas = [899 * TWO_PI, -899 * TWO_PI, 900 * TWO_PI, -900 * TWO_PI, 1e4]
    F, N, A, S = len(thetas), 100, 2, 2
    rng = np.random.default_rng(11)
    parts = _particles(rng, F, N)
    for f, th in enumerate(thetas):
        parts[f, 7 + 13 * f, 3] = th
    meas, shark = _meas(rng, S, F, A)
    mts, pos = _seed_states(range(20, 20 + F)), rng.integers(0, 625, size=F).astype(np.int32)
    _, o, refs = _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark)
    for f in (0, 1):
        _assert_all(o, f, refs[f], thetas[f])
    for f in (2, 3, 4):
        assert refs[f]["status"] != 0, thetas[f]
        assert o.st[f] == PF_ERR_ANGLE, thetas[f]


def test_measurement_wrap_limit(ctx, orc):
    """the same limit at update_weights' second angle_wrap (particle alpha - measurement[3]), and a nan heading at the first.
    The first error of a launch stays: a nan heading also makes every weight nan and the new list empty, and filter 3 meets
    an empty list one step after its angle error -- both are PF_ERR_ANGLE, not PF_ERR_EMPTY"""
    from oracle import orc_pf
    F, N, A, S = 4, 100, 3, 2   # three measurements: one pair and one single trip of the AUV loop
    rng = np.random.default_rng(12)
    parts = _particles(rng, F, N)
    meas, shark = _meas(rng, S, F, A)
    meas[:, 0, :, 3] = 899 * TWO_PI
    meas[:, 1, :, 3] = 900 * TWO_PI
    meas[:, 2, :, 2] = np.nan
    meas[0, 3, :, 3] = 900 * TWO_PI
    meas[1, 3, :, 4] = np.nan
    mts, pos = _seed_states(range(30, 30 + F)), rng.integers(0, 625, size=F).astype(np.int32)
    _, o, refs = _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark)
    _assert_all(o, 0, refs[0], "899 turns")
    for f in (1, 2, 3):
        assert refs[f]["status"] != 0, f
        assert o.st[f] == PF_ERR_ANGLE, f
        assert np.array_equal(o.upd[0, f], refs[f]["updated"][0]), f   # create_and_update came before the error


def test_velocity_wrap_limit(ctx, orc):
    """velocity_wrap stops after 900 subtractions without an error: v + U(0, 5) from 4497 needs 899 or 900 of them, from
    4503 900 or 901, and from 4510 the result still exceeds 5"""
    from oracle import orc_pf
    F, N, A, S = 1, 100, 1, 2
    rng = np.random.default_rng(13)
    parts = _particles(rng, F, N)
    parts[0, 0:30, 2] = np.repeat([4497.0, 4503.0, 4510.0], 10)
    meas, shark = _meas(rng, S, F, A)
    mts, pos = _seed_states([40]), np.array([300], dtype=np.int32)
    _, o, refs = _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark)
    v = refs[0]["updated"][0][:30, 2]
    assert (v[:10] <= 5).all() and (v[10:20] > 5).any() and (v[20:] > 5).all()   # the cases have their point
    _assert_all(o, 0, refs[0])


# ---- A2: an empty list_of_new_particles

def test_empty_list_status(ctx, orc):
    """a nan range makes every weight nan, no weight class matches, list_of_new_particles is empty: PF_ERR_EMPTY, both sides
    stop after that step's update draws, the later steps' outputs stay the host's zeros"""
    from oracle import orc_pf
    F, N, A, S = 2, 100, 2, 3
    rng = np.random.default_rng(14)
    parts = _particles(rng, F, N)
    meas, shark = _meas(rng, S, F, A)
    meas[1, :, :, 4] = np.nan
    mts, pos = _seed_states([50, 51]), np.array([0, 411], dtype=np.int32)
    _, o, refs = _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark)
    for f in range(F):
        ref = refs[f]
        assert ref["status"] != 0 and ref["list_len"][0] > 0 and ref["list_len"][1] == 0
        assert o.st[f] == PF_ERR_EMPTY
        assert np.array_equal(o.upd[:2, f], ref["updated"][:2])
        assert np.array_equal(o.cho[0, f], ref["choice"][0])
        assert np.array_equal(o.ll[:2, f], ref["list_len"][:2])
        assert np.array_equal(o.mean[:2, f], ref["mean"][:2]) and np.array_equal(o.err[:2, f], ref["range_error"][:2])
        _assert_rng(o, f, ref)
        assert not o.mean[1:, f].any() and not o.err[1:, f].any() and o.ll[2, f] == 0


# ---- A3: failing filters in a batch, the sticky status word

def test_failing_filters_among_healthy_ones(ctx, orc):
    from auv_sim_amd import _pf_lib
    from oracle import orc_pf
    F, N, A, S = 6, 300, 2, 3
    ANGLE, EMPTY = 1, 4
    healthy = [f for f in range(F) if f not in (ANGLE, EMPTY)]
    rng = np.random.default_rng(15)
    shark0 = rng.uniform(-500, 500, size=(F, 2))
    meas, shark = _meas(rng, 2 * S, F, A, shark0)
    clean = meas.copy()
    meas[1, ANGLE, :, 3] = 900 * TWO_PI
    meas[1, EMPTY, :, 4] = np.nan
    mts, pos = _seed_states(range(60, 60 + F)), rng.integers(0, 625, size=F).astype(np.int32)

    def ref_of(f, m):
        return orc_pf.run(N, m[:, f], shark[:len(m), f], shark0[f], mts[f], int(pos[f]), kind="portable")

    b = _pf_lib.FilterBatch(ctx, F, N).create(shark0, mts, pos)
    b.run(meas=meas[:S], shark_xy=shark[:S], log=True)
    o = _Out(b)
    for f in healthy:
        _assert_all(o, f, ref_of(f, meas[:S]), "first launch")
    for f, code in ((ANGLE, PF_ERR_ANGLE), (EMPTY, PF_ERR_EMPTY)):
        ref = ref_of(f, meas[:S])
        assert ref["status"] != 0
        _assert_steps(o, f, ref, 1, what="before the failing step")
        assert np.array_equal(o.upd[1, f], ref["updated"][1])
        assert o.st[f] == code
    # a second launch with clean measurements: the statuses stay, the healthy filters go on as if alone
    b.run(meas=meas[S:], shark_xy=shark[S:], log=True)
    o = _Out(b)
    assert (o.st[ANGLE], o.st[EMPTY]) == (PF_ERR_ANGLE, PF_ERR_EMPTY)
    for f in healthy:
        _assert_all(o, f, ref_of(f, meas), "second launch")
    # new lists on the same handle: every status cleared
    parts = _particles(rng, F, N)
    b.set_particles(parts, mts, pos)
    assert not b.status()[0].any()
    b.run(meas=clean[:S], shark_xy=shark[:S], log=True)
    o = _Out(b)
    for f in range(F):
        _assert_all(o, f, orc_pf.run(N, clean[:S, f], shark[:S, f], (0.0, 0.0), mts[f], int(pos[f]), init=parts[f],
                                     kind="portable"), "after set_particles")
    b.create(shark0, mts, pos)   # and create clears it too
    b.run(meas=meas[:2], shark_xy=shark[:2])
    st = b.status()[0]
    assert st[ANGLE] == PF_ERR_ANGLE and st[EMPTY] == PF_ERR_EMPTY and not st[healthy].any()
    b.create(shark0, mts, pos)
    assert not b.status()[0].any()


# ---- A4: the drop-in class turns the statuses into the reference's exceptions

@pytest.mark.parametrize("column,value,exc", [(3, 900 * TWO_PI, RecursionError), (4, float("nan"), ValueError)],
                         ids=["angle", "empty"])
def test_dropin_exceptions(orc, column, value, exc):
    """update_weights raises what the reference's run ends with, and numpy's global stream sits where the checker's does.
    After an angle error both sides finish the failing step, the checker with the particles' previous weights (all equal
    after create: a list of 5 N).  The row lies > 500 from every particle, which keeps the device's weights flat as well
    (both Gaussians < 1e-5 of the 0.001 floors): both lists have 5 N entries and the N index draws use the same words."""
    from auv_sim_amd.particleFilter import ParticleFilter
    from oracle import orc_pf
    N, seed = 300, 21
    row = [600.0, -400.0, 0.1, 50.0, 1.0, 1]
    row[column] = value
    np.random.seed(seed)
    pf = ParticleFilter(10.0, 20.0, [], number_of_particles=N)
    particles = pf.create_and_update(pf.create())
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(exc):
            pf.update_weights(particles, [row])
    mt, pos = orc_pf.np_seed_state(seed)
    ref = orc_pf.run(N, np.array([[row[:5]]]), [[10.0, 20.0]], (10.0, 20.0), mt, pos, kind="portable")
    assert ref["status"] != 0 and ref["list_len"][0] == (5 * N if exc is RecursionError else 0)
    st = np.random.get_state()
    assert np.array_equal(st[1], ref["mt"]) and st[2] == ref["mt_pos"]


# ---- A5: object sharing beyond what resampling produces

def _shared_rows(rng, N, obj):
    """[1,N,5] particles in which positions with one object id carry one row"""
    per_id = _particles(rng, 1, 5 * N)[0]
    return per_id[obj][None]


def _sharing_case(name):
    rng = np.random.default_rng(16)
    if name == "all_on_one":      # N rounds of the atomicMin loop, kb down to (4096 - N + 1) << 12
        N, A, S = 2048, 2, 2
        obj, ll = np.zeros(N, dtype=np.int32), None
    elif name == "top_of_table":  # ids at the top of 0 .. 5N-1 with list_len = 5N: the whole L.slot table
        N, A, S = 257, 1, 3
        obj = rng.choice(np.arange(1, 5 * N - 2), size=N, replace=False).astype(np.int32)   # singletons ...
        obj[rng.permutation(N)[:90]] = np.repeat([5 * N - 1, 5 * N - 2, 0], 30)              # ... and three big objects
        ll = [5 * N]
    else:                         # ten_by_hundred: 10 objects of multiplicity 100
        N, A, S = 1000, 3, 2
        obj, ll = rng.permutation(np.repeat(rng.choice(5 * N, size=10, replace=False), 100)).astype(np.int32), None
    return N, A, S, obj[None], ll


@pytest.mark.parametrize("name", ["all_on_one", "top_of_table", "ten_by_hundred"])
def test_sharing_extremes(ctx, orc, name):
    from oracle import orc_pf
    N, A, S, obj, ll = _sharing_case(name)
    rng = np.random.default_rng(17)
    parts = _shared_rows(rng, N, obj[0])
    meas, shark = _meas(rng, S, 1, A)
    mts, pos = _seed_states([70]), np.array([123], dtype=np.int32)
    _, o, refs = _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark, obj=obj, list_len=ll)
    _assert_all(o, 0, refs[0], name)
    if name == "all_on_one":   # one object, moved N times: every position shows the same row
        assert (o.upd[0, 0] == o.upd[0, 0, 0]).all()
        assert not np.array_equal(o.upd[0, 0, 0, :4], parts[0, 0, :4])


# ---- B: positions that share an object id must carry one row

def test_contradictory_aliases_are_refused(ctx):
    from auv_sim_amd import _lib, _pf_lib
    N = 20
    rng = np.random.default_rng(18)
    obj = np.arange(N, dtype=np.int32)[None].repeat(2, axis=0)
    obj[1, 9] = obj[1, 3] = 57
    parts = _particles(rng, 2, N)
    mts, pos = _seed_states([80, 81]), 624
    with pytest.raises(_lib.AuvpError, match="filter 1: positions 3 and 9") as e:
        _pf_lib.FilterBatch(ctx, 2, N).set_particles(parts, mts, pos, obj=obj)
    assert e.value.code == -1   # AUVP_ERR_ARG
    parts[1, 9] = parts[1, 3]
    parts[1, 9, 1] = np.nextafter(parts[1, 3, 1], np.inf)   # one bit of one column
    with pytest.raises(_lib.AuvpError, match="positions 3 and 9"):
        _pf_lib.FilterBatch(ctx, 2, N).set_particles(parts, mts, pos, obj=obj)


def test_identical_aliases_are_accepted(ctx):
    from auv_sim_amd import _pf_lib
    N = 20
    rng = np.random.default_rng(18)
    obj = np.arange(N, dtype=np.int32)[None].repeat(2, axis=0)
    obj[1, 9] = obj[1, 3] = 57
    parts = _particles(rng, 2, N)
    parts[1, 9] = parts[1, 3]
    parts[1, 9, 2] = parts[1, 3, 2] = np.nan   # bitwise: a nan equals itself
    b = _pf_lib.FilterBatch(ctx, 2, N).set_particles(parts, _seed_states([80, 81]), 624, obj=obj)
    got, got_obj = b.particles()
    assert np.array_equal(got, parts, equal_nan=True) and np.array_equal(got_obj, obj)
    assert not b.status()[0].any()


# ---- A6: the sampler at acceptance ~0.5, and counts that end on a state block's last word

@pytest.mark.parametrize("n_particles", [205, 410])
def test_flat_weights_worst_acceptance(ctx, orc, n_particles):
    """list length 5 N = 2^k + 1 or 2^k + 2: the masked rejection accepts half of the words"""
    from oracle import orc_pf
    F, N, S = 4, n_particles, 4
    rng = np.random.default_rng(N)
    parts = np.tile(np.array(FLAT_ROW, dtype=np.float64), (F, N, 1))
    meas = np.tile(np.array(FLAT_MEAS, dtype=np.float64), (S, F, 1, 1))
    shark = rng.uniform(-30, 30, size=(S, F, 2))
    mts, pos = _seed_states(range(90, 90 + F)), rng.integers(0, 625, size=F).astype(np.int32)
    _, o, refs = _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark)
    for f in range(F):
        assert (refs[f]["list_len"] == 5 * N).all() and 5 * N - (1 << (5 * N - 1).bit_length() - 1) <= 2
        _assert_all(o, f, refs[f])


@pytest.mark.parametrize("n_particles,start", [(156, 0), (156, 624), (312, 0)])
def test_update_words_end_on_a_block_edge(ctx, orc, n_particles, start):
    """create_and_update takes 4 N words: one or two whole state blocks, ending exactly on word 623"""
    from oracle import orc_pf
    F, N, A, S = 2, n_particles, 2, 3
    assert (start + 4 * N) % 624 == 0
    rng = np.random.default_rng(N + start)
    parts = _particles(rng, F, N)
    meas, shark = _meas(rng, S, F, A)
    mts, pos = _seed_states([100, 101]), np.full(F, start, dtype=np.int32)
    _, o, refs = _uploaded(ctx, orc_pf, parts, mts, pos, meas, shark)
    for f in range(F):
        _assert_all(o, f, refs[f])


def _edge_inputs(N):
    rng = np.random.default_rng(1000 + N)
    parts = _particles(rng, 1, N)
    meas, shark = _meas(rng, 2, 1, 2)
    return parts, meas, shark


# (N, seed, start position, exit position of the first step): found with the checker for _edge_inputs(N) by scanning seeds
# 1..3 x positions 0..624.  624: the N-th accepted word is word 623 of a state block; 1: it is word 0 of the next one
EDGE_CASES = [(64, 1, 296, 624), (156, 2, 342, 624), (64, 1, 297, 1), (156, 3, 349, 1)]


@pytest.mark.parametrize("n_particles,seed,start,exit_pos", EDGE_CASES)
def test_last_draw_on_a_block_edge(ctx, orc, n_particles, seed, start, exit_pos):
    """two launches of one step each; the first leaves the stream exactly at a block edge, the second starts there"""
    from auv_sim_amd import _pf_lib
    from oracle import orc_pf
    N = n_particles
    parts, meas, shark = _edge_inputs(N)
    mts, pos = _seed_states([seed]), np.array([start], dtype=np.int32)
    ref1 = orc_pf.run(N, meas[:1, 0], shark[:1, 0], (0.0, 0.0), mts[0], start, init=parts[0], kind="portable")
    ref2 = orc_pf.run(N, meas[:, 0], shark[:, 0], (0.0, 0.0), mts[0], start, init=parts[0], kind="portable")
    assert ref1["mt_pos"] == exit_pos and ref1["status"] == 0
    b = _pf_lib.FilterBatch(ctx, 1, N).set_particles(parts, mts, pos)
    b.run(meas=meas[:1], shark_xy=shark[:1], log=True)
    _assert_all(_Out(b), 0, ref1, "first launch")
    b.run(meas=meas[1:], shark_xy=shark[1:], log=True)
    _assert_all(_Out(b), 0, ref2, "second launch")


# ---- A7: particle counts at the kernel's structural edges

COUNTS = [1, 2, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 2047, 2048]


@pytest.mark.parametrize("n_particles,n_auv", [(n, (1, 4, 7)[i % 3]) for i, n in enumerate(COUNTS)])
def test_particle_counts(ctx, orc, n_particles, n_auv):
    """1: alone; 512/513: a second position per thread; 1024/1025: pf_step_kernel<512,2> -> <512,4>; 15..17: the mean's
    16-wide blocks; odd counts: the rounding of the LDS carve"""
    from auv_sim_amd import _pf_lib
    from oracle import orc_pf
    F, N, A, S = 3, n_particles, n_auv, 3
    rng = np.random.default_rng(5000 + N)
    shark0 = rng.uniform(-500, 500, size=(F, 2))
    meas, shark = _meas(rng, S, F, A, shark0)
    mts, pos = _seed_states(rng.integers(0, 2 ** 32, size=F)), rng.integers(1, 624, size=F).astype(np.int32)
    b = _pf_lib.FilterBatch(ctx, F, N).create(shark0, mts, pos)
    created, obj = b.particles()
    b.run(meas=meas, shark_xy=shark, log=True)
    o = _Out(b)
    for f in range(F):
        ref = orc_pf.run(N, meas[:, f], shark[:, f], shark0[f], mts[f], int(pos[f]), kind="portable")
        assert np.array_equal(created[f], ref["created"]) and np.array_equal(obj[f], np.arange(N))
        _assert_all(o, f, ref)
