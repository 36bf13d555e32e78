# -*- coding: utf-8 -*-
'''
Digests of the register programs that the cases of
tests/form_assembly_cases.py compile to: {case name: sha256 of the code of
every program of the case, in order}.  tests/golden/form_program_digests.json
holds them as they were before interior facets existed; a program without a
restriction and without FacetArea must stay byte for byte what it was
(tests/test_interior_facets_host.py).  Run as a script it prints the JSON.
'''
import hashlib
import json
import struct

from flow_amd import fem
from flow_amd.fem import forms, ops

import form_assembly_cases as gate_cases


def _digest(programs):
    h = hashlib.sha256()
    for prog in programs:
        for ins in prog.code:
            h.update(struct.pack('<4i', *[int(x) for x in ins]))
        h.update(b'|')
    return h.hexdigest()


def _one_shot_programs(form):
    progs = []
    for _, part in form.terms():
        rank, table = part.argument_table()
        facet = part.integral_type == 'exterior_facet'
        if isinstance(table, forms.BlockTable):
            for _, block in forms.block_items(table, rank):
                progs += forms.argument_programs(block, rank, facet)
        else:
            progs += forms.argument_programs(table, rank, facet)
    return progs


def digests():
    previous = (forms.vector_arguments.enabled,
                forms.vector_derivatives.enabled,
                forms.facet_arguments.enabled)
    gate_cases.switches()
    try:
        mesh = fem.UnitSquareMesh(3, 3)
        out = {}
        for case in gate_cases.all_cases(mesh):
            jobs = ops.newton_jobs(case.J, case.F, fuse=case.fuse)
            out['newton: ' + case.name] = _digest([j.program for j in jobs])
        for name, form, _ in gate_cases.one_shot_forms(mesh):
            out['one shot: ' + name] = _digest(_one_shot_programs(form))
        X = fem.SpatialCoordinate(mesh)
        n = fem.FacetNormal(mesh)
        u = fem.Function(fem.FunctionSpace(mesh, 'CG', 2))
        h = fem.CellDiameter(mesh)
        rank0 = [('dx', fem.sin(X[0]) * u**2 + fem.grad(u)[1], False),
                 ('ds', fem.dot(fem.grad(u), n) * h + X[1], True),
                 ('conditional', fem.conditional(fem.gt(u, 0.5), u, h), False)]
        for name, f, facet in rank0:
            out['functional: ' + name] = _digest(
                [forms.compile_trees([f.comps], facet=facet)])
        return out
    finally:
        forms.vector_arguments.enabled, forms.vector_derivatives.enabled, \
            forms.facet_arguments.enabled = previous


if __name__ == '__main__':
    print(json.dumps(digests(), indent=1, sort_keys=True))
