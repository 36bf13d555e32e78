# -*- coding: utf-8 -*-
'''
numpy restatement of fem.Supermesh (flow_amd/fem/supermesh.py, csrc/
projection_kernels.hip: flow_supermesh_norms) on the supermesh of tests/
projection_reference.py, which is imported and left as it is: ALL nc_b x
nc_a pairs, the target triangle clipped against the source's half-planes,
the polygon fanned from its centroid, the 7-point rule from its closed form.
Its own here: the derivatives of the P1 / P2 bases with respect to the
barycentric coordinates, the gradients of the barycentric coordinates from
the inverse of the cells' (1, x, y) matrices, and the sums per target cell.

V_a / u are the "from" side of that file (the source), V_b / w its "to"
side (the target: the results live on its cells).

sum_in_device_order restates the order in which the device sums a plane of
per-cell values (include/flow_hip.h: flow_supermesh_norms).
'''
import numpy

import projection_reference as pref
from projection_reference import meshes, pair, PAIRS, COVERED      # noqa: F401

KBLOCK, KRED = 256, 1024


def dbasis(degree, L):
    '''d phi_i / d lambda_k (..., nloc, 3) at barycentric L (..., 3), the
    three coordinates taken as independent.'''
    z = numpy.zeros_like(L[..., 0])
    if degree == 1:
        out = numpy.zeros(L.shape[:-1] + (3, 3))
        out[..., numpy.arange(3), numpy.arange(3)] = 1.0
        return out
    L0, L1, L2 = L[..., 0], L[..., 1], L[..., 2]
    rows = [[4 * L0 - 1, z, z], [z, 4 * L1 - 1, z], [z, z, 4 * L2 - 1],
            [z, 4 * L2, 4 * L1], [4 * L2, z, 4 * L0], [4 * L1, 4 * L0, z]]
    return numpy.stack([numpy.stack(r, axis=-1) for r in rows], axis=-2)


def bary_gradients(v):
    '''grad lambda_k (n, 3, 2) of the triangles v (n, 3, 2): lambda_k(x) =
    c_k + g_k . x with [1 x_j y_j] (c_k, g_k) = delta_jk.'''
    A = numpy.concatenate([numpy.ones(v.shape[:2] + (1,)), v], axis=2)
    M = numpy.linalg.inv(A)                       # columns (c_k, g_k)
    return numpy.transpose(M[:, 1:, :], (0, 2, 1))


def _field(V, mesh, cells, L, values):
    '''(val (dim, np, 7), grad (dim, np, 7, 2)) of the nodal values at the
    barycentric points L (np, 7, 3) of the cells `cells` (np,).'''
    phi = pref.basis(V.degree, L)                               # (np, 7, nl)
    dphi = dbasis(V.degree, L)                                  # (np, 7, nl, 3)
    g = bary_gradients(mesh.points[mesh.cell_vertices])[cells]  # (np, 3, 2)
    gphi = numpy.einsum('pqlk,pkd->pqld', dphi, g)
    cd = V.layout.cell_dofs[cells]                              # (np, nl)
    U = numpy.asarray(values).reshape(V.dim, V.N)[:, cd]        # (dim, np, nl)
    return (numpy.einsum('pql,apl->apq', phi, U),
            numpy.einsum('pqld,apl->apqd', gphi, U))


def norms(name, V_a, V_b, u, w):
    '''Of the named mesh pair, for nodal values u (dim * N_a,) of V_a and w
    (dim * N_b,) of V_b, per cell of V_b's mesh: 'l2', 'h10' (squared
    errors), 'uw', 'gugw' (products), 'coverage'; and 'area', the covered
    area.'''
    mesh_a, mesh_b, sm = pair(name)
    assert V_a.mesh() is mesh_a and V_b.mesh() is mesh_b
    nc = mesh_b.num_cells()
    uv, ug = _field(V_a, mesh_a, sm.src, sm.L_from, u)
    wv, wg = _field(V_b, mesh_b, sm.tgt, sm.L_to, w)
    wq = pref.RULE_W[None, :] * sm.area[:, None]                # (np, 7)

    def per_cell(f):
        return numpy.bincount(sm.tgt, weights=(wq * f).sum(axis=1), minlength=nc)

    return {
        'l2': per_cell(((uv - wv)**2).sum(axis=0)),
        'h10': per_cell(((ug - wg)**2).sum(axis=(0, 3))),
        'uw': per_cell((uv * wv).sum(axis=0)),
        'gugw': per_cell((ug * wg).sum(axis=(0, 3))),
        'coverage': sm.coverage,
        'area': float(sm.area.sum()),
        }


def _block_sum(v):
    '''256 lanes as the device sums them: a shuffle tree per wave of 64
    (lane l takes lane l + 32, + 16, ... in turn), then the four waves in
    turn.'''
    v = numpy.asarray(v, dtype=numpy.float64).reshape(4, 64)
    for half in (32, 16, 8, 4, 2, 1):
        v = v[:, :half] + v[:, half:2 * half]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def _strided_block_sums(x, nblocks):
    '''Block b, lane t: x[b * 256 + t] + x[b * 256 + t + 256 * nblocks] + ...
    in turn, from 0; then the block's sum.'''
    n = len(x)
    rounds = -(-n // (KBLOCK * nblocks))
    padded = numpy.zeros(rounds * nblocks * KBLOCK)
    padded[:n] = x
    lanes = numpy.zeros((nblocks, KBLOCK))
    for r in padded.reshape(rounds, nblocks, KBLOCK):
        lanes = lanes + r
    return numpy.array([_block_sum(lanes[b]) for b in range(nblocks)])


def sum_in_device_order(x):
    '''The sum of the per-cell values x as flow_supermesh_norms forms it:
    G = min(ceil(n / 256), 1024) block partials, then one block over them.'''
    x = numpy.asarray(x, dtype=numpy.float64)
    nparts = min(max(-(-len(x) // KBLOCK), 1), KRED)
    return float(_strided_block_sums(_strided_block_sums(x, nparts), 1)[0])
