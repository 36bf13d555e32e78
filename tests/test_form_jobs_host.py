# -*- coding: utf-8 -*-
'''
The jobs of form assembly on the host (ops.newton_jobs, the Job record, the
scratch rule of the block launches) and the three opt-in switches of
forms.py.  The cases are those of tests/form_assembly_cases.py on
UnitSquareMesh(4, 3), P1 and P2; the expectations below were recorded from
the two planners this one replaced (the gate's `plan` mode), field by field:
(kind, sign of the matrix part, sign of the vector part, nout of the program,
degree, scheme, index of the ds part among its form's parts or None, tag,
call).  No GPU.
'''
import collections
import itertools
import os

import pytest

from flow_amd import fem
from flow_amd.fem import forms, ops

import form_assembly_cases as gate_cases


@pytest.fixture(scope='module')
def gate():
    saved = [s.enabled for s in _SWITCHES]
    gate_cases.switches()
    yield gate_cases
    for s, on in zip(_SWITCHES, saved):
        s.enabled = on


_SWITCHES = (forms.vector_arguments, forms.vector_derivatives,
             forms.facet_arguments)

EXPECTED = {
    'P1 fused pair': [
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 0, (0, 0)),
        ('vector', 0.0, -1.0, 3, 3, 'default', None, 0, (None, 1)),
        ],
    'P1 fuse=False': [
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 0, (0, None)),
        ('vector', 0.0, 1.0, 3, 2, 'default', None, 0, (None, 0)),
        ('vector', 0.0, -1.0, 3, 3, 'default', None, 0, (None, 1)),
        ],
    'P1 other degree': [
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 0, (0, None)),
        ('vector', 0.0, 1.0, 3, 3, 'default', None, 0, (None, 0)),
        ],
    'P1 two programs': [
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 0, (0, None)),
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 0, (1, 1)),
        ('vector', 0.0, 1.0, 3, 2, 'default', None, 0, (None, 0)),
        ],
    'P1 ds in J and F': [
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 0, (0, 0)),
        ('facet_matrix', 1.0, 0.0, 9, 3, 'default', 1, 0, (1, None)),
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 0, (2, 3)),
        ('facet_vector', 0.0, 1.0, 3, 3, 'default', 1, 0, (None, 1)),
        ('facet_vector', 0.0, -1.0, 3, 3, 'default', 2, 0, (None, 2)),
        ],
    'P1 first sign -1': [
        ('newton', -1.0, -1.0, 12, 4, 'default', None, 0, (0, 0)),
        ('newton', 1.0, 1.0, 12, 0, 'default', None, 0, (1, 1)),
        ],
    'P2 fused pair': [
        ('newton', 1.0, 1.0, 12, 6, 'default', None, 0, (0, 0)),
        ('vector', 0.0, -1.0, 3, 4, 'default', None, 0, (None, 1)),
        ],
    'P2 fuse=False': [
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 0, (0, None)),
        ('vector', 0.0, 1.0, 3, 6, 'default', None, 0, (None, 0)),
        ('vector', 0.0, -1.0, 3, 4, 'default', None, 0, (None, 1)),
        ],
    'P2 other degree': [
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 0, (0, None)),
        ('vector', 0.0, 1.0, 3, 3, 'default', None, 0, (None, 0)),
        ],
    'P2 two programs': [
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 0, (0, None)),
        ('newton', 1.0, 1.0, 12, 4, 'default', None, 0, (1, 1)),
        ('vector', 0.0, 1.0, 3, 6, 'default', None, 0, (None, 0)),
        ],
    'P2 ds in J and F': [
        ('newton', 1.0, 1.0, 12, 6, 'default', None, 0, (0, 0)),
        ('facet_matrix', 1.0, 0.0, 9, 6, 'default', 1, 0, (1, None)),
        ('newton', 1.0, 1.0, 12, 4, 'default', None, 0, (2, 3)),
        ('facet_vector', 0.0, 1.0, 3, 6, 'default', 1, 0, (None, 1)),
        ('facet_vector', 0.0, -1.0, 3, 4, 'default', 2, 0, (None, 2)),
        ],
    'P2 first sign -1': [
        ('newton', -1.0, -1.0, 12, 8, 'default', None, 0, (0, 0)),
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 0, (1, 1)),
        ],
    'P1 burgers': [
        ('newton', 1.0, 1.0, 12, 3, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 3, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 3, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 3, 'default', None, 2, (0, 0)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (1, 1)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (1, 1)),
        ],
    'P1 forchheimer': [
        ('newton', 1.0, 1.0, 12, 6, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 6, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 2, (0, 0)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (1, 1)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (1, 1)),
        ],
    'P1 kirchhoff': [
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 1, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 1, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 2, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 2, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 3, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 3, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 3, (0, None)),
        ('matrix', 1.0, 0.0, 9, 0, 'default', None, 3, (0, None)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (1, 1)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (1, 1)),
        ('vector', 0.0, 1.0, 3, 0, 'default', None, 0, (None, 0)),
        ('vector', 0.0, 1.0, 3, 0, 'default', None, 0, (None, 0)),
        ('vector', 0.0, 1.0, 3, 0, 'default', None, 1, (None, 0)),
        ('vector', 0.0, 1.0, 3, 0, 'default', None, 1, (None, 0)),
        ],
    'P1 traction robin': [
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 2, (0, 0)),
        ('facet_matrix', 1.0, 0.0, 9, 2, 'default', 1, 0, (1, None)),
        ('facet_matrix', 1.0, 0.0, 9, 2, 'default', 1, 3, (1, None)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (2, 3)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (2, 3)),
        ('facet_vector', 0.0, -1.0, 3, 3, 'default', 1, 0, (None, 1)),
        ('facet_vector', 0.0, -1.0, 3, 3, 'default', 1, 1, (None, 1)),
        ('facet_vector', 0.0, 1.0, 3, 2, 'default', 2, 0, (None, 2)),
        ('facet_vector', 0.0, 1.0, 3, 2, 'default', 2, 1, (None, 2)),
        ],
    'P1 burgers, source apart': [
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 2, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 2, (0, 0)),
        ('vector', 0.0, -1.0, 3, 3, 'default', None, 0, (None, 1)),
        ('vector', 0.0, -1.0, 3, 3, 'default', None, 1, (None, 1)),
        ],
    'P1 burgers, fuse=False': [
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 1, (0, None)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 2, (0, None)),
        ('matrix', 1.0, 0.0, 9, 2, 'default', None, 3, (0, None)),
        ('vector', 0.0, 1.0, 3, 2, 'default', None, 0, (None, 0)),
        ('vector', 0.0, 1.0, 3, 2, 'default', None, 1, (None, 0)),
        ('vector', 0.0, -1.0, 3, 3, 'default', None, 0, (None, 1)),
        ('vector', 0.0, -1.0, 3, 3, 'default', None, 1, (None, 1)),
        ],
    'P2 burgers': [
        ('newton', 1.0, 1.0, 12, 5, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 5, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 2, (0, 0)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (1, 1)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (1, 1)),
        ],
    'P2 forchheimer': [
        ('newton', 1.0, 1.0, 12, 10, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 10, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 10, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 10, 'default', None, 2, (0, 0)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (1, 1)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (1, 1)),
        ],
    'P2 kirchhoff': [
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 1, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 1, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 2, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 2, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 3, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 3, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 3, (0, None)),
        ('matrix', 1.0, 0.0, 9, 4, 'default', None, 3, (0, None)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (1, 1)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (1, 1)),
        ('vector', 0.0, 1.0, 3, 4, 'default', None, 0, (None, 0)),
        ('vector', 0.0, 1.0, 3, 4, 'default', None, 0, (None, 0)),
        ('vector', 0.0, 1.0, 3, 4, 'default', None, 1, (None, 0)),
        ('vector', 0.0, 1.0, 3, 4, 'default', None, 1, (None, 0)),
        ],
    'P2 traction robin': [
        ('newton', 1.0, 1.0, 12, 6, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 6, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 6, 'default', None, 2, (0, 0)),
        ('facet_matrix', 1.0, 0.0, 9, 4, 'default', 1, 0, (1, None)),
        ('facet_matrix', 1.0, 0.0, 9, 4, 'default', 1, 3, (1, None)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 0, (2, 3)),
        ('newton', 1.0, 1.0, 12, 1, 'default', None, 3, (2, 3)),
        ('facet_vector', 0.0, -1.0, 3, 4, 'default', 1, 0, (None, 1)),
        ('facet_vector', 0.0, -1.0, 3, 4, 'default', 1, 1, (None, 1)),
        ('facet_vector', 0.0, 1.0, 3, 4, 'default', 2, 0, (None, 2)),
        ('facet_vector', 0.0, 1.0, 3, 4, 'default', 2, 1, (None, 2)),
        ],
    'P2 burgers, source apart': [
        ('newton', 1.0, 1.0, 12, 5, 'default', None, 0, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 1, (0, 0)),
        ('newton', 1.0, 1.0, 12, 5, 'default', None, 3, (0, 0)),
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 2, (0, 0)),
        ('vector', 0.0, -1.0, 3, 4, 'default', None, 0, (None, 1)),
        ('vector', 0.0, -1.0, 3, 4, 'default', None, 1, (None, 1)),
        ],
    'P2 burgers, fuse=False': [
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 0, (0, None)),
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 1, (0, None)),
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 2, (0, None)),
        ('matrix', 1.0, 0.0, 9, 5, 'default', None, 3, (0, None)),
        ('vector', 0.0, 1.0, 3, 5, 'default', None, 0, (None, 0)),
        ('vector', 0.0, 1.0, 3, 5, 'default', None, 1, (None, 0)),
        ('vector', 0.0, -1.0, 3, 4, 'default', None, 0, (None, 1)),
        ('vector', 0.0, -1.0, 3, 4, 'default', None, 1, (None, 1)),
        ],
    }


def _fields(job, J, F):
    where = None
    if job.part is not None:
        parts = [p for _, p in (J if job.kind == 'facet_matrix' else F).terms()]
        where = [i for i, p in enumerate(parts) if p is job.part][0]
    return (job.kind, job.msign, job.vsign, job.program.nout, job.degree,
            job.scheme, where, job.tag, job.call)


def test_job_lists_field_by_field(gate):
    mesh = fem.UnitSquareMesh(4, 3)
    cases = gate.all_cases(mesh)
    assert sorted(c.name for c in cases) == sorted(EXPECTED)
    for case in cases:
        jobs = ops.newton_jobs(case.J, case.F, fuse=case.fuse)
        assert all(isinstance(j, ops.Job) and len(j) == 9 for j in jobs)
        got = [_fields(j, case.J, case.F) for j in jobs]
        assert got == EXPECTED[case.name], case.name
        # positions and names read the same record
        for j in jobs:
            assert (j[0], j[3], j[6], j[7], j[8]) == (
                j.kind, j.program, j.part, j.tag, j.call)
            assert (j.part is not None) == j.kind.startswith('facet')
    by_name = dict((c.name, c) for c in cases)
    # the two rules of `fused`, side by side: a scalar list is fused without a
    # 'matrix' job; a block list keeps the 'matrix' jobs of a fused row
    kinds = dict((n, [j[0] for j in EXPECTED[n]]) for n in EXPECTED)
    for name, want in (('P2 fused pair', True), ('P2 fuse=False', False),
                       ('P2 other degree', False), ('P2 two programs', False),
                       ('P2 ds in J and F', True), ('P2 first sign -1', True)):
        c = by_name[name]
        assert ops._scalar_jobs_fused(
            ops.newton_jobs(c.J, c.F, fuse=c.fuse)) is want, name
        assert ('matrix' not in kinds[name]) is want
    for name, want in (('P2 burgers', True), ('P2 kirchhoff', False),
                       ('P2 traction robin', True),
                       ('P2 burgers, source apart', False),
                       ('P2 burgers, fuse=False', False)):
        c = by_name[name]
        assert ops.block_jobs_fused(
            ops.newton_jobs(c.J, c.F, fuse=c.fuse)) is want, name
    assert 'matrix' in kinds['P2 burgers']


def test_one_scratch_rule_for_the_block_launches(gate):
    '''_block_newton_scratch on the 'matrix' jobs or the 'vector' jobs of one
    call is (blocks present + 1 where a block has several programs) *
    nloc**rank * nc, the size the one-shot path used to compute for
    flow_form_block_matrix / flow_form_block_vector: for every dx call of
    every job list of the gate.'''
    mesh = fem.UnitSquareMesh(4, 3)
    nc = mesh.num_cells()
    lists = []
    for case in gate.all_cases(mesh):
        if case.V.dim == 2:
            lists.append((case.V, ops.newton_jobs(case.J, case.F)))
            lists.append((case.V, ops.newton_jobs(case.J, case.F, fuse=False)))
    # (the dx parts of the one-shot forms, as _block_part tags them)
    Part = collections.namedtuple('Part', 'kind tag call')
    for _, form, _ in gate.one_shot_forms(mesh):
        V = form.arguments()[0]
        if V.dim == 2:
            lists.append((V, [
                Part('matrix' if form.rank == 2 else 'vector', p, i)
                for i, (_, part) in enumerate(form.terms())
                if part.integral_type == 'cell'
                for p, block in forms.block_items(
                    part.argument_table()[1], form.rank)
                for _ in forms.argument_programs(block, form.rank)]))
    checked = several = 0
    for V, jobs in lists:
        nl = V.layout.nloc
        for call, group in itertools.groupby(jobs, key=lambda j: j.call):
            group = list(group)
            kinds = [j.kind for j in group]
            if kinds[0].startswith('facet'):
                continue
            if 'newton' in kinds:               # (a fused call: not this rule)
                continue
            assert len(set(kinds)) == 1 and kinds[0] in ('matrix', 'vector')
            rank = 2 if kinds[0] == 'matrix' else 1
            tags = [j.tag for j in group]
            present = len(set(tags))
            extra = len(tags) > present
            assert ops._block_newton_scratch(kinds, tags, nl, nc) == \
                (present + extra) * nl**rank * nc
            checked += 1
            several += extra
    # (not vacuous: dozens of launches, several with a block of many programs)
    assert checked >= 50 and several >= 10, (checked, several)


def test_switches():
    '''Each switch: off by default, on at construction, .previous, restored
    on context exit, nesting, and no effect on the other two.'''
    for sw in _SWITCHES:
        others = [s for s in _SWITCHES if s is not sw]
        before = [s.enabled for s in _SWITCHES]
        sw.enabled = False
        for s in others:
            s.enabled = False
        try:
            assert sw.__doc__ and sw.__name__ in sw.__doc__
            assert 'enabled' in vars(sw)            # its own, not the base's
            on = sw(True)
            assert sw.enabled is True and on.previous is False
            assert [s.enabled for s in others] == [False, False]
            off = sw(False)
            assert sw.enabled is False and off.previous is True
            with sw(True) as outer:
                assert sw.enabled is True and outer.previous is False
                with sw(False) as inner:
                    assert sw.enabled is False and inner.previous is True
                    with sw():                      # (on is the default)
                        assert sw.enabled is True
                    assert sw.enabled is False
                assert sw.enabled is True
                assert [s.enabled for s in others] == [False, False]
            assert sw.enabled is False
            # the others switched on stay on while this one goes off again
            for s in others:
                s(True)
            with sw(True):
                pass
            assert sw.enabled is False
            assert [s.enabled for s in others] == [True, True]
            assert forms._Switch.enabled is False
        finally:
            for s, on in zip(_SWITCHES, before):
                s.enabled = on


def test_switches_are_off_in_a_fresh_process():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.check_output(
        [sys.executable, '-c',
         'from flow_amd.fem import forms; print(forms.vector_arguments.enabled'
         ', forms.vector_derivatives.enabled, forms.facet_arguments.enabled)'],
        cwd=root)
    assert out.decode().split() == ['False', 'False', 'False']
