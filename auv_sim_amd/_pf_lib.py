"""ctypes binding of the particle-filter entry points of libauvplan.so (auvp_pf_*, include/auvplan.h)."""
import ctypes as C

import numpy as np

from . import _lib

UPDATE, WEIGHTS, MEAN = 1, 2, 4


def _bind():
    return _lib.load()


def np_seed_state(seed):
    """MT19937 key + position right after np.random.seed(seed) (numpy legacy seeding = init_genrand)"""
    mt = np.zeros(624, dtype=np.uint32)
    s = int(seed) & 0xffffffff
    for i in range(624):
        mt[i] = s
        s = (1812433253 * (s ^ (s >> 30)) + i + 1) & 0xffffffff
    return mt, 624


class FilterBatch:
    """F particle filters x N particles resident on one GPU (one per Context: the handle keeps one batch)."""

    def __init__(self, ctx, n_filters, n_particles=1000):
        self.ctx, self.F, self.N = ctx, int(n_filters), int(n_particles)
        self.L = _bind()
        self.S = 0

    def _rng_args(self, mt, pos):
        mt = _lib._arr(mt, np.uint32, (self.F, 624))
        pos = np.ascontiguousarray(np.broadcast_to(np.asarray(pos, dtype=np.int32), (self.F,)))
        return mt, pos

    def create(self, shark_xy0, mt, pos=624):
        xy = _lib._f64(shark_xy0, (self.F, 2))
        mt, pos = self._rng_args(mt, pos)
        self.ctx._chk(self.L.auvp_pf_create_batch(self.ctx.h, self.F, self.N, _lib._p(xy), _lib._p(mt),
                                                  _lib._p(pos)))
        return self

    def set_particles(self, particles, mt, pos, obj=None, list_len=None):
        pa = _lib._f64(particles, (self.F, self.N, 5))
        mt, pos = self._rng_args(mt, pos)
        ob = _lib._arr(obj, np.int32, (self.F, self.N)) if obj is not None else None
        ll = _lib._arr(list_len, np.int32, (self.F,)) if list_len is not None else None
        self.ctx._chk(self.L.auvp_pf_set_particles(self.ctx.h, self.F, self.N, _lib._p(pa),
                                                   _lib._p(ob) if ob is not None else None,
                                                   _lib._p(ll) if ll is not None else None,
                                                   _lib._p(mt), _lib._p(pos)))
        return self

    def set_rng(self, mt, pos):
        mt, pos = self._rng_args(mt, pos)
        self.ctx._chk(self.L.auvp_pf_set_rng(self.ctx.h, _lib._p(mt), _lib._p(pos)))

    def run(self, meas=None, shark_xy=None, phases=UPDATE | WEIGHTS | MEAN, n_steps=None, log=False):
        """meas [S,F,A,5], shark_xy [S,F,2]; one launch for all S steps."""
        m = sx = None
        A = 0
        if meas is not None:
            m = _lib._arr(meas, np.float64)
            if m.ndim != 4 or m.shape[1] != self.F or m.shape[3] != 5:
                raise ValueError("meas must be [S, F, A, 5]")
            n_steps, A = m.shape[0], m.shape[2]
        if shark_xy is not None:
            sx = _lib._arr(shark_xy, np.float64, (-1, self.F, 2))
            n_steps = len(sx) if n_steps is None else n_steps
            if len(sx) != n_steps:
                raise ValueError("shark_xy must be [S, F, 2]")
        self.S = int(n_steps or 1)
        self.ctx._chk(self.L.auvp_pf_run(self.ctx.h, self.S, A, int(phases), _lib._p(m) if m is not None else None,
                                         _lib._p(sx) if sx is not None else None, 1 if log else 0))
        return self

    def run_dev_meas(self, meas_dev, n_auv, shark_xy, phases=UPDATE | WEIGHTS | MEAN, n_steps=1, log=False):
        """run with meas [S, F, A, 5] already in HBM on this context's device (auvp_pf_run_dev_meas): meas_dev a device pointer
        whose producer has synchronised its stream (Context.replan_measure), n_auv = A; shark_xy [S, F, 2] from the host"""
        S = int(n_steps)
        sx = _lib._arr(shark_xy, np.float64, (-1, self.F, 2))
        if len(sx) != S:
            raise ValueError("shark_xy must be [S, F, 2]")
        if not meas_dev or int(n_auv) < 1:
            raise ValueError("need a device pointer and n_auv >= 1")
        self.S = S
        self.ctx._chk(self.L.auvp_pf_run_dev_meas(self.ctx.h, S, int(n_auv), int(phases), C.c_void_p(meas_dev), _lib._p(sx), 1 if log else 0))
        return self

    def particles(self):
        out = np.zeros((self.F, self.N, 5))
        obj = np.zeros((self.F, self.N), dtype=np.int32)
        self.ctx._chk(self.L.auvp_pf_particles(self.ctx.h, _lib._p(out), _lib._p(obj)))
        return out, obj

    def estimates(self):
        mean, err = np.zeros((self.S, self.F, 2)), np.zeros((self.S, self.F))
        ll = np.zeros((self.S, self.F), dtype=np.int32)
        self.ctx._chk(self.L.auvp_pf_estimates(self.ctx.h, _lib._p(mean), _lib._p(err), _lib._p(ll)))
        return mean, err, ll

    def status(self):
        st = np.zeros(self.F, dtype=np.int32)
        nd = np.zeros(self.F, dtype=np.uint64)
        self.ctx._chk(self.L.auvp_pf_status(self.ctx.h, _lib._p(st), _lib._p(nd)))
        return st, nd

    def rng_state(self):
        mt = np.zeros((self.F, 624), dtype=np.uint32)
        pos = np.zeros(self.F, dtype=np.int32)
        self.ctx._chk(self.L.auvp_pf_rng_state(self.ctx.h, _lib._p(mt), _lib._p(pos)))
        return mt, pos

    def step_log(self):
        upd = np.zeros((self.S, self.F, self.N, 5))
        cho = np.zeros((self.S, self.F, self.N), dtype=np.int32)
        self.ctx._chk(self.L.auvp_pf_step_log(self.ctx.h, _lib._p(upd), _lib._p(cho)))
        return upd, cho
