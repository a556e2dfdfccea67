"""fenris_amd -- MI355X-native FEM assembly engine behind fenris's element-assembler interface.

Python host layer over the C ABI of libfenris_hip.so (include/fenris_hip.h).  Only the hot path of
fenris -- global stiffness / residual assembly -- lives here; see DESIGN.md.
"""
from . import _ffi, amg, assembly, boundary, contact, degree, dirichlet, dynamics, eigen, interpolate, io, mesh, multigrid, operators, quadrature, recovery, refinement, reorder
from ._ffi import (ASSEMBLE_OVERWRITE, ASSEMBLE_REPRODUCIBLE, HEX8, HEX27, LAPLACE, LINEAR_ELASTIC, NEO_HOOKEAN, QUAD4, SCATTER_ATOMIC,
                   SCATTER_COLORED, SCATTER_GATHER, STVK, STABLE_NEO_HOOKEAN, PRECOND_IDENTITY, PRECOND_JACOBI, PRECOND_MULTIGRID, PRECOND_AMG, AMG_CONSTANT, AMG_RIGID_BODY, AMG_USER, TET4, TRI3, TET10, QUAD9, TRI6, HEX20, TET20, MASS_SCALAR, MASS_VECTOR, FenrisError, SingularJacobianError)
from .assembly import (CsrAssembler, CsrMatrix, CsrParAssembler, DisjointSubsetsColors, ElementEllipticAssembler, ElementMassAssembler,
                       ElementEllipticAssemblerBuilder, ElementSourceAssembler, ElementSourceAssemblerBuilder, Engine,
                       MockElementAssembler, UniformQuadratureTable, CompactQuadratureTable, GeneralQuadratureTable,
                       compact_quadrature_table,
                       VectorAssembler, VectorParAssembler, apply_homogeneous_dirichlet_bc_csr,
                       apply_homogeneous_dirichlet_bc_rhs, apply_homogeneous_dirichlet_dofs_csr, apply_homogeneous_dirichlet_dofs_rhs, assemble_scalar, color_nodes, CgSolveError, ConjugateGradient,
                       IdentityOperator, JacobiPreconditioner, MatrixFreeMass, MatrixFreeNewton, NewtonSettings, NoLineSearch,
                       BacktrackingLineSearch, NewtonError, NewtonResult, MaximumIterationsReached, JacobianError, LineSearchError, MatrixFreeOperator, MatrixFreeShiftedTangent, MatrixFreeTangent, RelativeResidualCriterion, estimate_H1_seminorm_error,
                       estimate_H1_seminorm_error_squared, estimate_L2_error, estimate_L2_error_squared)
from .compose import (AggregateElementAssembler, MapElementNodes, TransformElementMatrix, TransformElementScalar,
                      TransformElementVector)
from .amg import SmoothedAggregationAMG
from .boundary import BoundaryFaces, SurfaceLoad, SurfaceMesh
from .degree import (coarsen_degree, coarsen_degree_with_transfer, degree_hierarchy, degree_hierarchy_from_linear, elevate_degree,
                     elevate_degree_with_transfer, matching_vertex_permutation)
from .interpolate import FixedInterpolator, SpatiallyIndexed, ValuesOrGradients
from .multigrid import GeometricMultigrid
from .dirichlet import DofSet, dof_masks
from .dynamics import (BackwardEuler, CentralDifference, DynamicsError, DynamicsRecord, FirstOrderIntegrator, FirstOrderRecord, ForwardEuler, Newmark,
                       RayleighDamping, RungeKuttaLegendre, ThetaMethod, TimeIntegrator)
from .contact import AugmentedLagrangian, AugmentedLagrangianError, AugmentedLagrangianResult, MultiplierUpdate
from .contact import Ball, Cavity, Contact, GridObstacle, HalfSpace, ObstaclePath, Obstacles, SdfGrid, sdf_box, sdf_circle, sdf_union
from .eigen import EigenResult, EigenSolveError, MatrixFreeEigensolver
from .recovery import Recovery
from .refinement import (Transfer, permute_transfer, refine_uniformly, refine_uniformly_repeat, refine_uniformly_repeat_with_transfers,
                         refine_uniformly_with_transfer)
from .mesh import Mesh, hex20_mesh_from_hex8, hex27_mesh_from_hex8, procedural, quad9_mesh_from_quad4, tet10_mesh_from_tet4, tet20_mesh_from_tet4, tri6_mesh_from_tri3
from .operators import (Density, GravitySource, SourceFunction, LameParameters, LaplaceOperator, LinearElasticMaterial, MaterialEllipticOperator,
                        NeoHookeanMaterial, StableNeoHookeanMaterial, StVKMaterial, TensorEllipticOperator, YoungPoisson)

__all__ = [n for n in dir() if not n.startswith("_")]
