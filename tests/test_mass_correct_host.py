# -*- coding: utf-8 -*-
'''
flow_mass_correct without a GPU: the refusals of the entry point through the
loaded library (every check precedes the first launch, so pointers that are
never dereferenced do), the bindings, and which settings of
solver_parameters['correction'] send the velocity correction down which route.
'''
import ctypes
import os
import re

import pytest

from flow_amd import _hip
from flow_amd.navier_stokes import pressure_correction as pc
from flow_amd.navier_stokes import start_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# addresses that are only ever compared (16-byte aligned, all different)
ADDR = [0x10000 + 0x1000 * k for k in range(32)]


def _fake_mass(kind=4, n=100):
    A = _hip.Operator()
    A.kind, A.n, A.nnz, A.nblocks = kind, n, 7 * n, 3
    A.rowptr, A.cols, A.rowblocks = ADDR[0], ADDR[1], ADDR[2]
    A.vals[0] = ADDR[3]
    A.rowmask = ADDR[4] if kind == 4 else None
    M = _hip.MassS()
    M.A = ctypes.pointer(A)
    M.dinv = ADDR[5]
    M.nblocks16 = 2
    M.rowblocks16 = ADDR[6]
    M.vals16 = ADDR[7]
    M.lam_min, M.lam_max = 0.4, 2.1
    M.steps = 6
    M.contraction = 0.1
    M.work16 = ADDR[8]
    M._keep = A
    return M


def _call(M, g=ADDR[10], ui=ADDR[11], xbc=ADDR[12], delta0=ADDR[13], nbc=5,
          bc_dofs=ADDR[14], x_out=ADDR[15], inc_out=ADDR[16], rtol=1e-10,
          atol=0.0, maxit=10, first_check=0, work=ADDR[17], work_len=None,
          n=100):
    lib = _hip.load_library()
    if work_len is None:
        work_len = _hip.REDUCE_WORK + 2 * 2 + 2 + 2 * n
    its = ctypes.c_int(0)
    res = ctypes.c_double(0.0)
    return lib.flow_mass_correct(
        ctypes.byref(M) if M is not None else None, g, ui, xbc, delta0, nbc,
        bc_dofs, x_out, inc_out, rtol, atol, maxit, first_check, work, work_len,
        ctypes.byref(its), ctypes.byref(res), None)


def _refused(rc, what):
    assert rc == 2, rc
    msg = _hip.load_library().flow_last_error().decode()
    assert what in msg, msg
    with pytest.raises(ValueError):
        _hip.check(rc)


def test_symbol_is_declared_bound_and_exported():
    assert 'flow_mass_correct' in _hip.SYMBOLS
    assert len(_hip.SYMBOLS['flow_mass_correct']) == 18
    lib = _hip.load_library()
    assert lib.flow_mass_correct.argtypes == _hip.SYMBOLS['flow_mass_correct']
    with open(os.path.join(ROOT, 'include', 'flow_hip.h')) as f:
        header = f.read()
    m = re.search(r'int flow_mass_correct\(([^;]*)\);', header)
    assert m is not None
    assert len(m.group(1).split(',')) == 18
    # the old entries stay
    for name in ('flow_mass_solve', 'flow_mass_solve_increment'):
        assert name in _hip.SYMBOLS and getattr(lib, name) is not None


def test_refusals():
    _refused(_call(None), 'flow_mass is NULL')
    # a scalar operator: the entry is the velocity correction's (kind 4)
    _refused(_call(_fake_mass(kind=0)), 'operator kind 4')
    M = _fake_mass()
    _refused(_call(M, g=None), 'solver pointers')
    _refused(_call(M, ui=None), 'solver pointers')
    _refused(_call(M, x_out=None), 'solver pointers')
    _refused(_call(M, work=None), 'solver pointers')
    # identity rows need their indices and their values
    _refused(_call(M, bc_dofs=None), 'bc_dofs and xbc')
    _refused(_call(M, xbc=None), 'bc_dofs and xbc')
    _refused(_call(M, nbc=-1), 'bc_dofs and xbc')
    # the outputs are vectors of their own
    _refused(_call(M, x_out=ADDR[11]), 'x_out is a vector of its own')
    _refused(_call(M, x_out=ADDR[13]), 'x_out is a vector of its own')
    _refused(_call(M, x_out=ADDR[16]), 'x_out is a vector of its own')
    _refused(_call(M, inc_out=ADDR[11]), 'inc_out is a vector of its own')
    _refused(_call(M, inc_out=ADDR[13]), 'inc_out is a vector of its own')
    _refused(_call(M, rtol=-1.0), 'solver tolerances')
    _refused(_call(M, maxit=0), 'solver tolerances')
    _refused(_call(M, first_check=-1), 'solver tolerances')
    # the solver's increment lives in the workspace
    _refused(_call(M, work_len=_hip.REDUCE_WORK + 4), 'workspace too small')
    _refused(_call(M, work_len=_hip.REDUCE_WORK + 4 + 2 * 100 - 1),
             'workspace too small')
    # ... and a broken solver description is refused before anything else
    M = _fake_mass()
    M.steps = 2
    _refused(_call(M), 'Chebyshev steps')


ROUTES = [
    # (settings, sharded, graphs) -> route
    ({}, False, False, 'around_caller'),
    ({'around_caller': True}, False, False, 'around_caller'),
    ({'around_caller': False}, False, False, 'increment'),
    ({}, True, False, 'increment'),
    ({}, False, True, 'increment'),
    ({'increment': False}, False, False, 'solve'),
    ({'increment': False}, True, False, 'solve'),
    ({'extrapolate': True}, False, False, 'solve'),
    ({'method': 'cg'}, False, False, 'cg'),
    ({'method': 'cg'}, True, False, 'cg'),
    ({'method': 'cg', 'around_caller': True}, False, False, 'cg'),
    ({'increment_start': 'zero'}, False, False, 'around_caller'),
    ]


@pytest.mark.parametrize('settings,sharded,graphs,route', ROUTES)
def test_routing(settings, sharded, graphs, route):
    par = dict(pc.solver_parameters['correction'])
    par.update(settings)
    assert pc._correction_route(par, sharded, graphs) == route


def test_default_settings_take_the_new_route():
    par = pc.solver_parameters['correction']
    assert par['around_caller'] is True
    assert pc._correction_route(par, False, False) == 'around_caller'
    # mode 'fast' extrapolates the start itself: the right-hand side is then
    # not the defect of ui, no increment form at all
    fast = dict(par)
    fast.update(pc._MODES['fast']['correction'])
    assert pc._correction_route(fast, False, False) == 'solve'


class _Lay(object):
    def __init__(self):
        self._dev = {}


class _Vec(object):
    '''Stands in for a device vector: the history only asks for its length.'''
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def _trajectory(lay, level):
    st = start_vectors._state(lay)
    tr = start_vectors.Trajectory()
    tr.level = level
    st.trajectories.append(tr)
    st.current = tr
    st.unresolved = False
    return tr


def test_history_slots_follow_remember_increment(monkeypatch):
    '''increment_slot / file_increment leave the history as remember_increment
    does: newest first, KEEP_POINTS + 1 entries at the most, the oldest one's
    vector re-used, a repeated step replacing its own entry -- and the vector
    handed out is never one extrapolated_increment may read.'''
    from flow_amd import device
    made = []

    def empty(n):
        made.append(_Vec(n))
        return made[-1]
    monkeypatch.setattr(device, 'empty', empty)
    lay = _Lay()
    key = 'correction_increments'
    assert start_vectors.increment_slot(lay, 10, key=key) is None
    tr = _trajectory(lay, 0)
    keep = start_vectors.KEEP_POINTS
    for level in range(1, keep + 4):
        tr.level = level
        before = list(tr.entries(key))
        slot = start_vectors.increment_slot(lay, 10, key=key)
        # none of the entries the extrapolation may read
        assert all(slot is not h[0] for h in tr.entries(key)[:keep])
        if len(before) >= keep + 1:
            assert slot is before[-1][0]
        start_vectors.file_increment(lay, 0.5 * level, slot, key=key)
        hist = tr.entries(key)
        assert hist[0] == (slot, 0.5 * level, level)
        assert [h[2] for h in hist] == list(range(level, max(0, level - keep - 1),
                                                  -1))
        assert len(hist) <= keep + 1
    assert len(made) == keep + 1
    # the same time level again: its own entry, in place
    tr.redo = True
    again = start_vectors.increment_slot(lay, 10, key=key)
    assert again is tr.entries(key)[0][0]
    n = len(tr.entries(key))
    start_vectors.file_increment(lay, 9.0, again, key=key)
    assert len(tr.entries(key)) == n
    assert tr.entries(key)[0] == (again, 9.0, tr.level)
    # vectors of another length are dropped like remember_increment drops them
    tr.level += 1
    other = start_vectors.increment_slot(lay, 12, key=key)
    assert other.numel() == 12 and tr.entries(key) == []
