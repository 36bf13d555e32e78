# -*- coding: utf-8 -*-
'''
Connected components of level sets ("Regions"): what
fem.Regions costs on the bench mesh, and which CHECK_EVERY to keep.

On the mesh of KarmanProblem(nx, ny) (default 2182 x 509: 1.1 M vertices), P1
and P2, a synthetic street -- rows of Gaussian vortices of alternating sign
behind the obstacle, as nodal values (tools/isolines_lab.py's) -- labelled at
{w >= 0.3 max w}:

  label ms     Regions.label between two events on the package's stream (the
               read-backs of the flag and of the count sit inside), for
               CHECK_EVERY = 4, 8 and 32; 2 warm-up calls, median of 7 with
               min - max; the sweeps it ran;
  sweep us     one sweep of flow_region_sweeps: 32 sweeps in one call from the
               initial labels, divided by 32 -- for the street (a lane of an
               outside dof returns at once) and with every dof inside; next
               to it one sweep of flow_distance_sweeps on the same space (32
               from Distance's start values), the kernel with the same row
               walk;
  integrate ms Components.integrate of the field itself (one moments launch
               and one segment sum; no read-back).

    python tools/regions_lab.py [--mesh NX NY] [--every 4 8 32]
                                [--degrees 1 2] [--repeat 7]
'''
import argparse
import ctypes
import importlib
import os
import sys
import time

import numpy
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from flow_amd import _hip, fem, device           # noqa: E402
from flow_amd.fem import ops                      # noqa: E402
from isolines_lab import street, timed            # noqa: E402

freg = importlib.import_module('flow_amd.fem.regions')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mesh', type=int, nargs=2, default=[2182, 509])
    ap.add_argument('--every', type=int, nargs='+', default=[4, 8, 32])
    ap.add_argument('--degrees', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--repeat', type=int, default=7)
    args = ap.parse_args()
    t0 = time.perf_counter()
    mesh = fem.karman_channel(args.mesh[0], args.mesh[1], fitted=True)
    print('mesh %d x %d: %d vertices, %d cells (%.1f s)'
          % (args.mesh[0], args.mesh[1], mesh.num_vertices(), mesh.num_cells(),
             time.perf_counter() - t0), flush=True)
    lib = _hip.lib()
    kept = freg.CHECK_EVERY
    for deg in args.degrees:
        V = fem.FunctionSpace(mesh, 'CG', deg)
        N = V.N
        values = street(V.layout.dof_coords)
        level = 0.3 * values.max()
        f = fem.Function(V)
        f.set_array(values)
        R = fem.Regions(V)
        print('P%d: %d dofs, level %.3f' % (deg, N, level), flush=True)
        for every in args.every:
            freg.CHECK_EVERY = every
            C = R.label(f, level)
            ms = timed(lambda: R.label(f, level), repeat=args.repeat)
            print('    CHECK_EVERY %3d: %d components, %4d sweeps, label %7.3f ms '
                  '(%.3f - %.3f)' % (every, C.count, C.sweeps, ms[0], ms[1], ms[2]),
                  flush=True)
        freg.CHECK_EVERY = kept
        C = R.label(f, level)
        it = timed(lambda: C.integrate(f), repeat=args.repeat)
        print('    integrate %7.3f ms (%.3f - %.3f); largest component %d dofs'
              % (it[0], it[1], it[2], int(device.to_host(C.size.max()))), flush=True)
        # one sweep of each kind
        mesh_s, space_s = ops.mesh_struct(mesh), ops.space_struct(V.layout)
        dev = device.get()
        start = torch.where(torch.from_numpy(values >= level).to(dev),
                            torch.arange(N, dtype=torch.int32, device=dev),
                            torch.full((N,), -1, dtype=torch.int32, device=dev))
        a, b = torch.empty_like(start), torch.empty_like(start)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)

        def region_sweeps():
            a.copy_(start)
            _hip.check(lib.flow_region_sweeps(
                ctypes.byref(mesh_s), ctypes.byref(space_s), 32, _hip.i32(a, N),
                _hip.i32(b, N), _hip.i32(flag, 1), _hip.stream()))

        D = fem.Distance(V)
        dstart, da, db, dflag = D._buffers()

        def distance_sweeps():
            da.copy_(dstart)
            _hip.check(lib.flow_distance_sweeps(
                ctypes.byref(mesh_s), ctypes.byref(space_s), 32, _hip.f64(da, N),
                _hip.f64(db, N), _hip.i32(dflag, 1), _hip.stream()))

        rs = timed(region_sweeps, repeat=args.repeat)
        # ... and with every dof inside: no lane returns early, as in the
        # distance sweep
        start = torch.arange(N, dtype=torch.int32, device=dev)
        ra = timed(region_sweeps, repeat=args.repeat)
        ds = timed(distance_sweeps, repeat=args.repeat)
        print('    one sweep: regions %7.2f us (%.1f %% of the dofs inside), %7.2f us '
              '(all inside), distance %7.2f us (32 in one call, the copy of the '
              'start values included in all)'
              % (1.0e3 * rs[0] / 32, 100.0 * (values >= level).mean(),
                 1.0e3 * ra[0] / 32, 1.0e3 * ds[0] / 32), flush=True)


if __name__ == '__main__':
    main()
