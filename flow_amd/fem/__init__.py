# -*- coding: utf-8 -*-
'''
Minimal finite-element front end: the vocabulary the reference's drivers import
from dolfin (tests/test_navier_stokes.py:10-14, tests/test_karman_vortex_street.py:7-11,
tests/test_boussinesq.py:14-18, tests/test_sealed_box.py:9-13), restricted to
what the Navier-Stokes / heat hot path needs.  dolfin is not available on the
GPU box, so the counterpart drivers import these names from here instead.
'''
from .mesh import (                                             # noqa: F401
    Mesh, Point, RectangleMesh, UnitSquareMesh, rectangle_with_hole,
    karman_channel, karman_channel_graded, heater_box, heater_box_coarse,
    MeshFunction, FacetFunction, CellFunction,
    )
from .space import (                                            # noqa: F401
    FunctionSpace, VectorFunctionSpace, FiniteElement, VectorElement,
    )
from .function import (                                         # noqa: F401
    Function, Constant, Expression, NodalExpression, Vector,
    as_cell_coefficient, cell_lattice_points, scalar_value,
    )
from .bcs import DirichletBC, SubDomain                         # noqa: F401
from .io import XDMFFile, mpi_comm_world, read_mesh             # noqa: F401
from .space import MixedFunctionSpace                           # noqa: F401
from .forms import (                                            # noqa: F401
    dx, ds, Measure, FacetNormal, SpatialCoordinate, as_vector, sqrt, exp,
    ln, sin, cos, dot, inner, grad, div, curl, TestFunction, TrialFunction,
    lhs, rhs, system, dS, derivative, action, adjoint,
    conditional, lt, le, gt, ge, eq, ne, And, Or, Not, max_value, min_value,
    sign, tanh, CellVolume, Circumradius, CellDiameter, facet_arguments,
    cell_subdomains,
    vector_arguments, vector_derivatives, sym, tr, transpose, Identity, outer,
    interior_facets, jump, avg, FacetArea,
    mixed_arguments, TestFunctions, TrialFunctions, split, mixed_gmres,
    mixed_derivatives,
    )
from .space import RectLayout, rect_layout                      # noqa: F401
from .mixed import MixedMatrix                                  # noqa: F401
from .points import Probes                                      # noqa: F401
from .tracers import Tracers                                    # noqa: F401
from .transfer import Transfer                                  # noqa: F401
from .projection import Projection, project_onto               # noqa: F401
from .supermesh import Supermesh, mesh_errornorm                # noqa: F401
from .adapt import (                                            # noqa: F401
    JumpIndicator, jump_indicator, mark, refine, refined_markers,
    )
from .recovery import (                                         # noqa: F401
    GradientRecovery, recover_gradient, zz_indicator,
    )
from .snapshots import Snapshots                                # noqa: F401
from .eigen import Eigenmodes, eigensolve, vector_eigenmodes    # noqa: F401
from .nullspace import (                                        # noqa: F401
    VectorSpaceBasis, constant_nullspace, rigid_body_modes,
    )
from .statistics import Statistics                              # noqa: F401
from .distance import Distance, wall_distance                   # noqa: F401
from .isolines import Isolines, isolines                        # noqa: F401
from .regions import Regions, regions                           # noqa: F401
from .profile import (                                          # noqa: F401
    BoundaryProfile, traction, wall_shear, pressure_coefficient, normal_flux,
    )
from ..message import begin, end, info                          # noqa: F401

DOLFIN_EPS = 3.0e-16
triangle = 'triangle'
pi = 3.141592653589793


def __getattr__(name):
    # the operations below run on the HIP path; import them lazily so that the
    # host-only parts (meshes, spaces, BC search) work without the library
    if name in ('project', 'interpolate', 'errornorm', 'norm', 'assemble_mass',
                'assemble_stiffness', 'integral', 'project_magnitude', 'ops',
                'assemble', 'assemble_system', 'solve',
                'interior_facet_integrals', 'cell_indicator'):
        import importlib
        ops = importlib.import_module('.ops', __name__)
        return ops if name == 'ops' else getattr(ops, name)
    raise AttributeError(name)
