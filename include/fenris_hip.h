/*
 * fenris_hip.h -- C ABI of the MI355X-native FEM assembly engine (libfenris_hip.so).
 *
 * This is the drop-in boundary for fenris's global stiffness / residual assembly path: every entry
 * point names the reference interface it replaces (paths relative to the fenris checkout).  The
 * reference's plugin point is the Element*Assembler trait family (src/assembly/local.rs:18-149)
 * consumed by CsrAssembler / CsrParAssembler / VectorAssembler (src/assembly/global.rs); arbitrary
 * Rust element assemblers cannot run on a GPU, so the engine implements the closed family the
 * reference ships -- ElementEllipticAssembler<Mesh<C>, Op, UniformQuadratureTable>
 * (src/assembly/local/elliptic.rs:152-340) -- selected through plain descriptors.
 *
 * Conventions
 *   - plain pointers and sizes only; `usize` of the reference is uint64_t; all reals are f64.
 *   - vertices are AoS [x,y(,z)] (Vec<OPoint<f64,D>>, src/mesh.rs:23-40); connectivity is E x n
 *     uint64_t (Vec<[usize; n]>, src/connectivity.rs:606-607) -- both are zero-copy views of the
 *     reference's own storage.
 *   - dof numbering: s*node + component (src/assembly/global.rs:163-164); CSR as in nalgebra-sparse
 *     (row_offsets[R+1], col_indices[nnz] ascending per row, values[nnz]).
 *   - pointers are HOST pointers unless the function name ends in _dev (then: device pointers valid on
 *     the context's device; the call is enqueued on the context's stream and returns after enqueueing
 *     unless it has a host out-parameter, in which case it synchronises the stream).
 *   - every function returns an int32 status; nothing aborts.  fh_last_error() gives the message.
 *   - a context is bound to one device and one host thread at a time (thread-compatible, like
 *     CsrAssembler which is !Sync, src/assembly/global.rs:27-31).
 */
#ifndef FENRIS_HIP_H
#define FENRIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FH_ABI_VERSION 1

/* Tuning and diagnostics: environment variables named FENRIS_HIP_* (the table fenris_amd/csrc/options.def declares every one, with its
 * reading, default and meaning; fh_option_name lists the names) are read ONCE, by fh_create, into the
 * context; no later call reads the environment.  They change which kernel variant runs or print diagnostics, never results
 * beyond rounding -- except FENRIS_HIP_ABLATE / FENRIS_HIP_TRACE, which select instrumented instantiations for profiling
 * (FENRIS_HIP_ABLATE switches work off and produces wrong values by design). */

/* status codes.  FH_SINGULAR_JACOBIAN is the reference's only runtime error on the path:
 * eyre!("Singular element Jacobian encountered"), src/assembly/local/elliptic.rs:401-404. */
enum {
    FH_OK = 0,
    FH_SINGULAR_JACOBIAN = 1,
    FH_BAD_ARGUMENT = 2,
    FH_HIP_ERROR = 3,         /* a HIP or RCCL call failed; fh_last_error has the text */
    FH_OUT_OF_MEMORY = 4,     /* a buffer the call needs does not fit: device memory, or a cap such as FENRIS_HIP_TWO_PASS_MAX_GB (round 6; the value was reserved) */
    FH_INVALID_STATE = 5,     /* e.g. assemble before pattern, operator/element dimension mismatch */
    FH_UNSUPPORTED = 6,
    /* SolveErrorKind of the conjugate-gradient solver (fenris-sparse/src/cg.rs:277-286) */
    FH_CG_MAX_ITERATIONS = 7,
    FH_CG_INDEFINITE_OPERATOR = 8,
    FH_CG_INDEFINITE_PRECONDITIONER = 9,
    /* NewtonError of Newton's method (fenris-optimize/src/newton.rs:25-34): MaximumIterationsReached, JacobianError (an error of the inner
     * PCG: fh_newton_solve's stats[3] holds its code), LineSearchError */
    FH_NEWTON_MAX_ITERATIONS = 10,
    FH_NEWTON_JACOBIAN_ERROR = 11,
    FH_NEWTON_LINE_SEARCH_FAILED = 12,
    /* the eigensolver (fh_eigs_lowest): max_iter exhausted before every pair met the criterion; a Cholesky factor or the dense
     * Rayleigh-Ritz problem met a pivot that is not positive (also fh_dense_generalized_eigh on its own) */
    FH_EIG_MAX_ITERATIONS = 13,
    FH_EIG_BREAKDOWN = 14,
    /* time integration (fh_dynamics_step): the kinetic or the stored energy of a recorded state is not finite */
    FH_DYNAMICS_NONFINITE = 15
};

/* element kinds: Quad4d2Element (src/element/quadrilateral.rs:70-142), Hex8Element
 * (src/element/hexahedron.rs:34-117), Tet4Element (src/element/tetrahedron.rs:543-608),
 * Hex27Element (hexahedron.rs:157-335), Tri3d2Element (src/element/triangle.rs:63-110) */
enum { FH_QUAD4 = 0, FH_HEX8 = 1, FH_TET4 = 2, FH_HEX27 = 3, FH_TRI3 = 4,
       /* quadratic elements, sub-parametric like Hex27 -- the geometry map is the embedded linear element's:
        * Tet10Element (src/element/tetrahedron.rs:92-246), Quad9d2Element (quadrilateral.rs:150-330),
        * Tri6d2Element (triangle.rs:130-260) */
       FH_TET10 = 5, FH_QUAD9 = 6, FH_TRI6 = 7,
       /* Hex20Element, 20-node serendipity (src/element/hexahedron.rs:357-563), geometry from the embedded Hex8 */
       FH_HEX20 = 8,
       /* Tet20Element, cubic (src/element/tetrahedron.rs:248-470), geometry from the embedded Tet4 */
       FH_TET20 = 9 };

/* operator kinds: LaplaceOperator (src/assembly/operators/laplace.rs), MaterialEllipticOperator over
 * LinearElasticMaterial / NeoHookeanMaterial / StVKMaterial (fenris-solid/src/lib.rs:412-508,
 * fenris-solid/src/materials.rs:83-123, 236-353, 392-469) */
enum { FH_LAPLACE = 0, FH_LINEAR_ELASTIC = 1, FH_NEO_HOOKEAN = 2, FH_STVK = 3,
       /* ElementMassAssembler::with_solution_dim(1 | D) (src/assembly/local/mass.rs:48-286): M_IJ = I_s sum_q w |det J|
        * rho phi_I phi_J; the per-point parameter pair carries Density(rho) in its first slot.  Matrix only. */
       FH_MASS_SCALAR = 4, FH_MASS_VECTOR = 5,
       /* An elliptic operator given as DATA instead of code (round 6): the contraction of an EllipticContraction (src/assembly/operators.rs:146-189)
        * whose coefficients do not depend on grad u,
        *     C(a, b)[i][k] = sum_{j, l} a[j] A[i][j][k][l] b[l],       s = d,
        * with one tensor A per quadrature point (fh_set_operator_tensor).  Covers every LINEAR elliptic operator -- anisotropic elasticity,
        * a linearisation frozen at some state, operators that are not symmetric -- without a closure crossing the boundary; a caller
        * with a nonlinear operator evaluates its tangent at the quadrature data it owns.  Stiffness matrix only (all scatter modes). */
       FH_TENSOR = 6,
       /* Stable Neo-Hookean (Smith, de Goes, Kim 2018), rest value subtracted and its alpha eliminated: finite for EVERY F, det F <= 0 included,
        * with no branch on det F.  With U = (grad u)^T, F = I + U, c = 2 tr U + U:U (= F:F - d), gamma = det F - 1 (expanded in U, never
        * det(F) - 1), k = mu d / (d + 1), cof F = dJ/dF and m = d + 1 + c (>= 1):
        *     psi     = mu/2 [c - log1p(c / (d + 1))] + lambda/2 gamma^2 - k gamma
        *     P       = mu (1 - 1/m) F + (lambda gamma - k) cof F
        *     C(a, b) = mu (1 - 1/m) (a.b) I + 2 mu/m^2 (F a)(F b)^T + lambda (cof F a)(cof F b)^T + (lambda gamma - k) G(a, b)
        *     G(a, b)[i][k] = sum_jl a[j] (d cof F[i][j] / d F[k][l]) b[l]:   d = 3: G v = v x w with w = F (a x b);
        *                                                                     d = 2: (a0 b1 - a1 b0) [[0, 1], [-1, 0]]
        * mu, lambda are the law's own pair per point; they linearise at F = I to the Lame pair mu_L = mu d/(d+1),
        * lambda_L = lambda + 2 mu/(d+1)^2 - mu d/(d+1) (fh_stable_neo_hookean_parameters converts).  lambda = 0 is allowed.  Everything the
        * other two nonlinear laws have: matrix, residual, energy, matrix-free tangent, solvers, recovery.  At inverted states K(u) is
        * indefinite (no per-element projection). */
       FH_STABLE_NEO_HOOKEAN = 7 };

/* how K_e contributions reach the CSR values (flags argument of fh_assemble_matrix*):
 *   FH_SCATTER_ATOMIC  : element-parallel, fp64 atomic adds (replaces the rayon colour loop)
 *   FH_SCATTER_COLORED : one launch per colour, plain read-modify-write -- CsrParAssembler semantics
 *                        (src/assembly/global.rs:314-376); needs fh_color() or fh_set_colors()
 *   FH_SCATTER_GATHER  : owner-computes: each CSR row block is produced by one workgroup from all
 *                        elements adjacent to its node and written once, coalesced; no atomics on HBM
 * OR-in FH_ASSEMBLE_OVERWRITE to store K instead of accumulating into the existing values
 * (= CsrAssembler::assemble, global.rs:124-131, without the explicit zero fill). */
enum { FH_SCATTER_ATOMIC = 0, FH_SCATTER_COLORED = 1, FH_SCATTER_GATHER = 2, FH_SCATTER_MASK = 0xff };
enum { FH_ASSEMBLE_OVERWRITE = 0x100 };
/* OR-in FH_ASSEMBLE_REPRODUCIBLE (with FH_SCATTER_GATHER) to get the same bits from run to run and from launch geometry to launch geometry, like the
 * reference's coloured loop (global.rs:322-373: every entry is a sum in a fixed order).  The row-owner kernels (affine and general Hex8 with the
 * eight-point rule, Tet4) and the two-pass form (Hex27, NeoHookean, StVK, Stable Neo-Hookean) already are; the configurations whose one-pass kernel accumulates with
 * LDS atomics in hardware order (Quad4 / Tri3, Hex8 with other rules or per-point parameters) take the two-pass form instead -- slower, and the
 * dense element matrices need E (s n)^2 doubles (9 E n (n + 1) / 2 for 3 x 3 blocks on the 3D elements: node-block triangles); FH_UNSUPPORTED under a row range.  FH_SCATTER_COLORED is reproducible as it is;
 * FH_SCATTER_ATOMIC never is (FH_BAD_ARGUMENT with this flag). */
enum { FH_ASSEMBLE_REPRODUCIBLE = 0x200 };

typedef struct fh_ctx fh_ctx;
typedef struct fh_mg fh_mg;
typedef struct fh_amg fh_amg;

/* ---- context ------------------------------------------------------------------------------- */
fh_ctx* fh_create(int device_id);               /* NULL if the device cannot be initialised */
void fh_destroy(fh_ctx*);
const char* fh_last_error(const fh_ctx*);
int fh_abi_version(void);
/* hipStream_t to launch on (NULL = default stream).  Not owned. */
int fh_set_stream(fh_ctx*, void* hip_stream);
int fh_synchronize(fh_ctx*);

/* ---- inputs -------------------------------------------------------------------------------- */
/* Mesh<f64, D, C>: replaces passing &Mesh to ElementEllipticAssemblerBuilder::with_finite_element_space
 * (src/assembly/local/elliptic.rs:86-97).  Data is copied to the device (connectivity narrowed to i32;
 * num_vertices must be < 2^31).  Invalidates pattern, colours and u.  The element records of the affine-element kernel (Hex8) are a
 * function of the context's copy of this data: fh_set_mesh*, fh_update_vertices and fh_set_affine_tolerance are the calls after which the
 * next assembly forms them again; assemblies in between reuse them, whatever the material, the operator's parameters or the flags. */
int fh_set_mesh(fh_ctx*, int elem_kind, const double* vertices, uint64_t num_vertices,
                const uint64_t* connectivity, uint64_t num_elements);
int fh_set_mesh_dev(fh_ctx*, int elem_kind, const double* vertices_dev, uint64_t num_vertices,
                    const uint64_t* connectivity_dev, uint64_t num_elements);
/* only the vertex coordinates change (e.g. moving mesh); pattern stays valid.  The affine flags of the elements and the element records
 * of the affine-element kernel follow the new coordinates (the records at the next assembly). */
int fh_update_vertices(fh_ctx*, const double* vertices);
/* Generic ElementConnectivityAssembler with ragged element node lists (src/assembly/local.rs:18-47),
 * e.g. the mock connectivities of tests/unit_tests/assembly/global.rs:70-142.  Only fh_pattern*,
 * fh_color work on such a context.  elem_offsets has num_elements+1 entries. */
int fh_set_connectivity_ragged(fh_ctx*, uint64_t solution_dim, uint64_t num_nodes, const uint64_t* elem_offsets,
                               const uint64_t* elem_nodes, uint64_t num_elements);
/* Restrict the NUMERIC assembly (matrix, vector, scalar) to the elements with mask[e] != 0 while the sparsity
 * pattern keeps coming from all elements.  No reference counterpart (fenris is single-process): this is how a
 * mesh partition assembles its own elements into rows that carry the global pattern (own + halo elements),
 * see fenris_amd/distributed.py.  mask has num_elements bytes; NULL removes the mask. */
int fh_set_active_elements(fh_ctx*, const uint8_t* mask);
/* Restrict FH_SCATTER_GATHER assembly to the rows of the nodes [node_begin, node_end): only those CSR rows are
 * produced (the others are left untouched).  Together with fh_assemble_matrix_rows_dev (below) one context assembles
 * the matrix in two launches over complementary ranges -- the multi-GPU path launches the rows of a partition interface
 * first and sends them while the rest is computed (fenris_amd/distributed.py).  (0, num_nodes) restores the default. */
int fh_set_row_range(fh_ctx*, uint64_t node_begin, uint64_t node_end);
/* Operator: replaces .with_operator(&op) (elliptic.rs:99-108).  Solution dim s = 1 for Laplace, D else. */
int fh_set_operator(fh_ctx*, int op_kind);
/* The coefficient tensors of FH_TENSOR: nq x d^4 doubles, index ((i d + j) d + k) d + l, nq = the points of the quadrature table in use (set the
 * table first; a later fh_set_quadrature_* with another point count invalidates them).  symmetric != 0: the caller asserts
 * A[i][j][k][l] == A[k][l][i][j], i.e. Symmetry::Symmetric -- only the blocks I <= J are formed and the rest mirrored exactly like for the
 * built-in operators (operators.rs:176-181, util.rs:38-51); 0: Symmetry::NonSymmetric -- every block of every row is formed (operators.rs:180),
 * nothing is mirrored, and the assembled matrix is not symmetric. */
int fh_set_operator_tensor(fh_ctx*, const double* tensors, uint32_t nq, int symmetric);
/* UniformQuadratureTable::from_points_and_weights(points, weights).with_data / with_uniform_data
 * (src/assembly/local/quadrature_table.rs:213-298).  params: nq x 2 doubles (LameParameters{mu,lambda}
 * per point, fenris-solid/src/materials.rs:8-12) or NULL for operators without parameters. */
int fh_set_quadrature_uniform(fh_ctx*, const double* weights, const double* points, uint32_t nq,
                              const double* params);
/* The same table with the per-point data where and how the caller keeps it (`data: Vec<Parameters>` of
 * UniformQuadratureTable, quadrature_table.rs:213-298): `stride` bytes from one point's record to the next (a multiple of
 * 8), `kind` says what a record starts with -- FH_DATA_LAME: LameParameters {mu, lambda} (fenris-solid/src/materials.rs:8-12),
 * FH_DATA_DENSITY: Density(rho) of the mass / gravity assemblers (fenris-solid/src/gravity_source.rs), FH_DATA_NONE: `()`. */
enum { FH_DATA_NONE = 0, FH_DATA_LAME = 1, FH_DATA_DENSITY = 2 };
int fh_set_quadrature_uniform_data(fh_ctx*, const double* weights, const double* points, uint32_t nq, const void* data,
                                   uint32_t stride, int kind);
/* CompactQuadratureTable::from_quadrature_rules_and_map (src/assembly/local/quadrature_table.rs:300-439) for rules
 * that share points and weights and differ in their per-point data -- piecewise material parameters: element e
 * uses rule_params[elem_to_rule[e]] (num_rules x nq x 2, same pair layout as the uniform table).  A rule index out
 * of bounds is FH_BAD_ARGUMENT (the reference panics).  Rules with different point sets: fh_set_quadrature_rules below.
 * Rules whose data are the same at every point (one
 * LameParameters pair per element: the multi-material case) keep the fastest LinearElastic stiffness kernel, which then
 * reads the pair per element; rules that vary over their points take the per-point-coefficient kernels. */
int fh_set_quadrature_compact(fh_ctx*, const double* weights, const double* points, uint32_t nq, uint64_t num_rules,
                              const double* rule_params, const uint64_t* elem_to_rule);
/* Rule-set tables: GeneralQuadratureTable (one rule per element, src/assembly/local/quadrature_table.rs:57-210) and
 * CompactQuadratureTable::from_quadrature_rules_and_map with rules of DIFFERENT point sets (:300-439).  Rule r holds the
 * points [rule_offsets[r], rule_offsets[r + 1]) of `weights` (total), `points` (total x d) and `params` (total x 2, the pair
 * layout of the uniform table, or NULL for operators without parameters); element e uses rule elem_to_rule[e]
 * (NULL: rule e, then num_rules must equal the number of elements).  A rule index out of bounds or an empty rule is
 * FH_BAD_ARGUMENT (the reference panics: check_rules_consistency, quadrature_table.rs:366-372).
 * The engine groups the rules by (points, weights): a group runs as one uniform / compact device table over its elements,
 * and fh_assemble_matrix*, fh_assemble_vector*, fh_assemble_scalar and fh_assemble_element_matrices* walk the groups
 * inside the library, accumulating -- a table whose rules share their points costs one pass, E different point sets cost
 * E passes.  The source-vector, physical-point and error-estimate entry points answer FH_UNSUPPORTED while such a table
 * is set.  Replaced by the next fh_set_quadrature_* call; dropped by fh_set_mesh*. */
int fh_set_quadrature_rules(fh_ctx*, uint64_t num_rules, const uint64_t* rule_offsets, const double* weights,
                            const double* points, const double* params, const uint64_t* elem_to_rule);
/* number of (points, weights) groups of the rule-set table in use (0: none set) = passes per assembly */
int fh_quadrature_rule_groups(const fh_ctx*, uint64_t* num_groups);
/* Affine-element fast path of FH_SCATTER_GATHER (Hex8; Laplace / LinearElastic with uniform parameters).  On an element
 * whose geometry map is affine the Jacobian of elliptic.rs:399 is the same at every quadrature point, so
 * K_ab = |det J| C(J^-T Ghat_ab J^-1) with Ghat_ab = sum_q w_q ghat_a ghat_b^T depending on the rule only -- the engine
 * detects such elements from the vertex coordinates and runs the node blocks whose elements all qualify on a kernel
 * without a quadrature loop; every other block keeps the general kernels.  An element qualifies when the four mixed
 * coefficients of its trilinear map are at most rel_tol times its shortest edge-direction coefficient.  Results change
 * by O(rel_tol) relative at most (exactly affine elements -- every generated box mesh -- agree to rounding).
 * Default 2^-46 (1.4e-14); 0 switches the path off.  No reference counterpart (the reference has one code path).
 * Only the stiffness fast path follows a loosened tolerance: the residual / energy kernels take the all-affine shortcut of a mesh
 * only at the default tolerance (or tighter) and use the exact geometry otherwise.  A changed tolerance classifies the elements again
 * and, like new vertices, makes the next assembly form the element records again. */
int fh_set_affine_tolerance(fh_ctx*, double rel_tol);
/* how the last FH_SCATTER_GATHER assembly was split: elements found affine, node blocks on the affine kernel, node blocks on
 * the general kernels (any pointer may be NULL; zeros before the first assembly) */
int fh_affine_stats(const fh_ctx*, uint64_t* affine_elements, uint64_t* affine_blocks, uint64_t* general_blocks);
/* The element tiles of the mesh in use (Hex8, Tet4, Quad4, Tri3: what the residual, energy, source and matrix-free passes walk): the number of
 * tiles of 256 elements, the number of partial node sums (the distinct nodes of a tile, summed over the tiles), the largest number of
 * distinct nodes of one tile, and the longest list of partials of one node (0 for a node without elements).  Any pointer may be NULL.
 * Read-only for the passes: the tables are built here if the topology has none yet, and the two maxima are reduced from them on the device
 * at every call (nothing is kept for it; the call waits for the stream).  FH_UNSUPPORTED where the mesh has no tiles: another element kind,
 * a ragged connectivity, FENRIS_HIP_NO_VECTOR_TILES, or tables that could not be built. */
int fh_vector_tiles_stats(fh_ctx*, uint64_t* tiles, uint64_t* partials, uint64_t* max_tile_nodes, uint64_t* max_node_partials);
/* The affine kernel of the last FH_SCATTER_GATHER assembly: whether its loader took the element records from the table of DISTINCT records
 * (elements whose records agree bit for bit share one entry; structured, graded and extruded meshes have a few hundred) and the slots of a
 * node block from the table of distinct slot lists, how many entries the two tables have (0 when it did not), and -- when it did not -- why (a string owned by
 * the library, "" when shared).  Contexts with an element mask or a row range, more than 4096 distinct records or 8192 distinct lists
 * (FENRIS_HIP_AFFINE_SHARED_MAX_RECORDS / _MAX_LISTS), FENRIS_HIP_AFFINE_SHARED=0 and -- unless FENRIS_HIP_AFFINE_SHARED=1 asks for it, it is
 * slower there -- the Laplace and scalar mass operators keep the per-element loader; the values are the same
 * bits either way.  The tables follow the vertices, the connectivity and the tolerance; building them costs tens of assemblies, so the
 * first FENRIS_HIP_AFFINE_SHARED_AFTER (default 2) assemblies of a mesh generation keep the per-element loader, twice as many after every
 * build in a row that ended over a limit, and fh_time_assembly_dev builds them in its untimed first assembly.  THE ASSEMBLY THAT BUILDS
 * THEM BLOCKS: fh_assemble_matrix_async_dev, otherwise an enqueue, waits for the stream three times in that one call (record hashes to the host;
 * the result of the record check with the list hashes; the result of the list check) and returns only after 28 - 39 ms on the 216^3 headline mesh (a few ms where
 * the build ends over a limit); work the caller meant to overlap with that call waits with it.  A caller that cannot afford the stall at
 * that place sets FENRIS_HIP_AFFINE_SHARED_AFTER=0 to have it in the first assembly of the generation, or FENRIS_HIP_AFFINE_SHARED=0. */
int fh_affine_shared_stats(const fh_ctx*, int* shared, uint64_t* num_records, uint64_t* num_lists, const char** reason);
/* INTERNAL, not a supported part of the interface: a view of the partition for the project's own tests and tools, which restate the shared
 * tables from it; the layout it exposes may change with any release.  The node blocks of the affine kernel as the last FH_SCATTER_GATHER
 * assembly's partition holds them: slots per block, number of blocks, and (elements_out, blocks x slots_per_block int32 on the host, may
 * be NULL) the element of every slot, -1 for an empty one. */
int fh_affine_slot_elements(fh_ctx*, int* slots_per_block, uint64_t* blocks, int32_t* elements_out);
/* .with_u(&u) (elliptic.rs:123-137); u has s*N entries; NULL = zeros */
int fh_set_u(fh_ctx*, const double* u);
int fh_set_u_dev(fh_ctx*, const double* u_dev);

/* ---- queries (ElementConnectivityAssembler, src/assembly/local.rs:18-27) ---------------------- */
uint64_t fh_solution_dim(const fh_ctx*);
uint64_t fh_num_elements(const fh_ctx*);
uint64_t fh_num_nodes(const fh_ctx*);
uint64_t fh_num_rows(const fh_ctx*);   /* s*N */
uint64_t fh_nnz(const fh_ctx*);        /* 0 before fh_pattern */

/* ---- sparsity pattern: CsrAssembler::assemble_pattern / CsrParAssembler::assemble_pattern
 *      (src/assembly/global.rs:65-120, 206-297); bit-identical output ---------------------------- */
/* builds the pattern on the device; row_offsets (R+1 entries) may be NULL; nnz_out may be NULL */
int fh_pattern(fh_ctx*, uint64_t* row_offsets, uint64_t* nnz_out);
int fh_pattern_cols(fh_ctx*, uint64_t* col_indices /* nnz */);
/* device outputs; either may be NULL.  Requires a prior fh_pattern(). */
int fh_pattern_dev(fh_ctx*, uint64_t* row_offsets_dev, uint64_t* col_indices_dev);

/* ---- colouring: color_nodes + sequential_greedy_coloring (src/assembly/global.rs:540-551,
 *      fenris-paradis/src/coloring.rs:6-70); reference-identical ----------------------------------- */
/* color_offsets: capacity num_elements+2 (or NULL); labels: num_elements entries (or NULL):
 * elements of colour c are labels[color_offsets[c] .. color_offsets[c+1]) in ascending order */
int fh_color(fh_ctx*, uint64_t* num_colors, uint64_t* color_offsets, uint64_t* labels);
/* the same outputs, computed ON the device: Luby-style rounds (propose the smallest colour no finished neighbour holds, keep it unless
 * a neighbour of smaller hashed priority proposed the same), deterministic.  A valid colouring -- no two elements of a colour share a
 * node, which is all CsrParAssembler / DisjointSubsets require -- but generally not the sequential greedy one of fh_color (more colours
 * are possible).  Fixed-size connectivity only. */
int fh_color_parallel(fh_ctx*, uint64_t* num_colors, uint64_t* color_offsets, uint64_t* labels);
/* reuse a colouring computed elsewhere (colours are serialisable in the reference, paradis lib.rs:170) */
int fh_set_colors(fh_ctx*, uint64_t num_colors, const uint64_t* color_offsets, const uint64_t* labels);

/* ---- numeric assembly ------------------------------------------------------------------------ */
/* CsrAssembler::assemble_into_csr / CsrParAssembler::assemble_into_csr (global.rs:133-182, 314-376):
 * values (nnz doubles, layout of the fh_pattern CSR) are ACCUMULATED into unless FH_ASSEMBLE_OVERWRITE.
 * On FH_SINGULAR_JACOBIAN *failed_element is the lowest failing element index (may be NULL) and the
 * values are unspecified (the reference aborts at the first failing element). */
int fh_assemble_matrix(fh_ctx*, double* values, int flags, uint64_t* failed_element);
int fh_assemble_matrix_dev(fh_ctx*, double* values_dev, int flags, uint64_t* failed_element);
/* same, but only enqueues; check the status later with fh_poll_status (no host sync; for timing loops).  The FIRST calls after a change of
 * the mesh, the pattern, the mask or the operator do block the host: the first builds the owner-computes tables (tens of milliseconds), and
 * on general Hex8 meshes the second runs the lane tuner of k_hex8_rows in front of its launch (a device synchronisation and ~20 ms of host
 * work, once; FENRIS_HIP_TUNE_AFTER moves it, FENRIS_HIP_NO_LANE_TUNING removes it).  fh_time_assembly_dev and fh_tune_placement_dev run both
 * before their timed assemblies. */
int fh_assemble_matrix_async_dev(fh_ctx*, double* values_dev, int flags);
int fh_poll_status(fh_ctx*, uint64_t* failed_element);
/* Placement of the streamed buffers.  On MI355X the time of the owner-computes kernels follows how the large buffers they stream
 * through happen to be backed by device memory: the same context and arguments run at one of several levels up to 10 % apart, for
 * the life of an allocation, and no HIP call chooses the backing.  fh_time_assembly_dev times `reps` assemblies (after one untimed)
 * with events on the context's stream; a caller uses it to keep the better of several allocations of its `values`.
 * fh_tune_placement_dev does the same for the library's own large buffer (the element records of the affine-element kernel): up to
 * `tries` re-allocations, each timed with three assemblies (behind an untimed one that fills the candidate with the records), the fastest
 * kept.  BOTH need FH_ASSEMBLE_OVERWRITE (the timed / trial
 * assemblies are real ones and write `values`; FH_BAD_ARGUMENT otherwise).  No reference counterpart. */
/* A tuning switch of this context (a FENRIS_HIP_* name as fh_create reads them from the environment): set, or removed with value ==
 * NULL.  Launch-variant switches act at the next call.  For comparing variants inside ONE context on the same buffers.  A name that
 * fenris_amd/csrc/options.def does not declare is FH_BAD_ARGUMENT (fh_last_error names it), and so is FENRIS_HIP_RCCL_LIB, which is read
 * from the environment of the process and not per context. */
int fh_set_option(fh_ctx*, const char* name, const char* value);
/* The full name ("FENRIS_HIP_...") of the index-th declared switch, NULL past the end of the table.  Needs neither a context nor a GPU. */
const char* fh_option_name(int index);
/* Device memory through the virtual-memory API with an explicit physical chunk size (hipMemAddressReserve / hipMemCreate / hipMemMap): `bytes`
 * on `device` from chunks of `chunk_bytes` (rounded up to the allocation granularity, reported in *granularity_out; 0 = one chunk).  For
 * experiments on how a large `values` array is backed (profiles/r05_vmm_experiment.txt); free with fh_vmm_free.  No reference counterpart. */
int fh_vmm_alloc(int device, uint64_t bytes, uint64_t chunk_bytes, void** out, uint64_t* granularity_out);
int fh_vmm_free(void* ptr);
/* Host staging memory of the set-up stages comes from a process-wide pool that is never returned to the operating system while in use (unmapping
 * memory a device copy has touched suspends the process's GPU queues for tens of milliseconds, profiles/r05_setup.txt): at most 1 GiB is retained.
 * fh_host_pool_trim frees what the pool holds (call it when no latency-critical launch is near); returns the bytes freed. */
uint64_t fh_host_pool_trim(void);
int fh_time_assembly_dev(fh_ctx*, double* values_dev, int flags, int reps, double* ms_per_assembly);
int fh_tune_placement_dev(fh_ctx*, double* values_dev, int flags, int tries, double* ms_before, double* ms_after);
/* The CSR rows of the nodes [node_begin, node_end) only (FH_SCATTER_GATHER), whatever the context's own row range is: the
 * context keeps a second set of owner-computes tables for this range next to its own (mesh, pattern, quadrature and operator
 * are shared, nothing is duplicated), built on first use and rebuilt when the range or the context's configuration changes.
 * A context with fh_set_row_range(split, N) plus this call on [0, split) produces the matrix in two launches.  Not with
 * rule-set tables (fh_set_quadrature_rules).  The _async form only enqueues; fh_poll_status reports its errors too. */
int fh_assemble_matrix_rows_dev(fh_ctx*, double* values_dev, int flags, uint64_t node_begin, uint64_t node_end,
                                uint64_t* failed_element);
int fh_assemble_matrix_rows_async_dev(fh_ctx*, double* values_dev, int flags, uint64_t node_begin, uint64_t node_end);
/* VectorAssembler::assemble_vector_into / VectorParAssembler (global.rs:582-608, 643-685) with
 * assemble_element_elliptic_vector (elliptic.rs:457-531): out (s*N) is accumulated into. */
int fh_assemble_vector(fh_ctx*, double* out, uint64_t* failed_element);
int fh_assemble_vector_dev(fh_ctx*, double* out_dev, uint64_t* failed_element);
/* the same, only enqueued on the context's stream: a singular element is reported by the next fh_poll_status (like
 * fh_assemble_matrix_async_dev) -- also over a rule-set table (one launch per rule group; the status is reset once in front of them).
 * The FIRST assembly of a context still builds the pattern and the adjacency, which synchronises; later calls only enqueue. */
int fh_assemble_vector_async_dev(fh_ctx*, double* out_dev);
/* assemble_scalar (global.rs:697-711) with compute_element_elliptic_energy (elliptic.rs:551-605) */
int fh_assemble_scalar(fh_ctx*, double* out, uint64_t* failed_element);
/* ElementSourceAssembler through VectorAssembler (src/assembly/local/source.rs:159-278, global.rs:582-608):
 *   out[s node + c] += sum_e sum_q w |det J| f_c(e, q) phi_node(xi_q)
 * independent of fh_set_operator; solution_dim is 1 or the geometry dimension.  The reference's SourceFunction is
 * arbitrary code; the closed family behind this ABI:
 *   values == NULL: f(e, q) = density_q * g   -- GravitySource (fenris-solid/src/gravity_source.rs:57-65); density_q
 *                   is the first parameter of the quadrature table (Density<T>), g has solution_dim entries (host)
 *   values != NULL: f(e, q) = values[(e nq + q) solution_dim ..] -- any source, sampled by the caller at the physical
 *                   points returned by fh_physical_quadrature_points (x = map_reference_coords(xi_q), source.rs:263)
 * Only |det J| enters (source.rs:276): no singular-Jacobian error on this path. */
int fh_assemble_source_vector(fh_ctx*, uint32_t solution_dim, const double* g, const double* values, double* out);
int fh_assemble_source_vector_dev(fh_ctx*, uint32_t solution_dim, const double* g /* host */, const double* values_dev,
                                  double* out_dev);
int fh_physical_quadrature_points(fh_ctx*, double* x /* E x nq x d */);
int fh_physical_quadrature_points_dev(fh_ctx*, double* x_dev);
/* ---- boundary of the mesh: Mesh::find_boundary_faces / find_boundary_vertices / find_boundary_cells (src/mesh.rs:154-216), on the
 *      device; bit-identical index arrays ------------------------------------------------------------------------------------------
 * Every cell emits its faces in local order with the node lists of get_face_connectivity (src/connectivity.rs: Quad4 / Tri3 ->
 * Segment2, Quad9 / Tri6 -> Segment3, Tet4 -> Tri3, Tet10 -> Tri6, Hex8 -> Quad4, Hex20 -> Quad8, Hex27 -> Quad9, Tet20 -> no faces:
 * an empty result); faces point outward.  Two faces are the same face iff their sorted full node tuples are equal; a boundary face
 * is one whose tuple occurs exactly once; the output is in ascending lexicographic order of the sorted tuples (the BTreeMap iteration,
 * mesh.rs:187-202).  fh_find_boundary_faces runs the search and keeps the result on the context: fh_set_mesh* and
 * fh_set_connectivity_ragged drop it, fh_update_vertices keeps it; the queries below run it when it is missing.  Before a mesh is
 * set: FH_INVALID_STATE; on a ragged generic connectivity: FH_UNSUPPORTED.  Scratch, released when the
 * search returns: 24 bytes per (cell, local face) for keys and face ids plus the radix sort's own temporary, 36 bytes in all
 * (fh_boundary_search_scratch_bytes: the figure of the search that produced the cached result). */
int fh_find_boundary_faces(fh_ctx*, uint64_t* num_faces, uint32_t* nodes_per_face);
/* face_nodes: F x nodes_per_face in the cell's orientation; cells: F; local_faces: F.  Any pointer may be NULL. */
int fh_boundary_faces(fh_ctx*, uint64_t* face_nodes, uint64_t* cells, uint32_t* local_faces);
int fh_boundary_faces_dev(fh_ctx*, uint64_t* face_nodes_dev, uint64_t* cells_dev, uint32_t* local_faces_dev);
/* sorted and unique (mesh.rs:208-216 / 154-163); two-phase like fh_pattern: a NULL array gives *count only.  The vertex list can be
 * passed to fh_apply_dirichlet_* and fh_set_operator_dirichlet_nodes as it is. */
int fh_boundary_vertices(fh_ctx*, uint64_t* count, uint64_t* nodes);
int fh_boundary_cells(fh_ctx*, uint64_t* count, uint64_t* cells);
int fh_boundary_search_scratch_bytes(const fh_ctx*, uint64_t* bytes);
/* ---- surface load vector on a list of (cell, local face) pairs -- any subset of the faces in any order, e.g. part of the boundary.
 * No reference counterpart (the reference has no Neumann assembler); solution_dim s is 1 or the geometry dimension d:
 *   FH_LOAD_TRACTION: out[s I + c] += sum_faces sum_q  w_q N_I(x_q) t_c(face, q) |a_q|
 *   FH_LOAD_PRESSURE: out[d I + c] += sum_faces sum_q -w_q N_I(x_q) p(face, q)   a_q[c]          (s == d)
 * a_q = det(J) J^-T n_ref times the reference face measure is the outward area vector (Nanson), with the CELL's Jacobian at the
 * face point mapped into the cell (the sub-parametric corner geometry of the high-order kinds, hexahedron.rs:324-330); in 2D the
 * face is an edge and a_q the tangent turned clockwise.  N_I is the cell's basis; only the face's own nodes are touched.  The face
 * rule (weights, points: nq x (d - 1), host) lives on the face's reference domain: [-1, 1] for a segment, [-1, 1]^2 for a
 * quadrilateral, the triangle (-1, -1), (1, -1), (-1, 1).  data holds t (s per item) or p (1 per item); data_count picks the shape:
 * 1: one item for all faces, num_faces: one per face, num_faces * nq: one per face and point.  out (s N) is ACCUMULATED into, per
 * node in ascending (position in the list, q) order without atomics: two calls agree bit for bit.  Only |a_q| enters a traction: a
 * degenerate face is not an error.  The node adjacency of the list is cached on the context, keyed on the list's contents.
 * Independent of operator and quadrature table.  A cell or local face out of range: FH_BAD_ARGUMENT. */
enum { FH_LOAD_TRACTION = 0, FH_LOAD_PRESSURE = 1 };
int fh_assemble_surface_load(fh_ctx*, int load_kind, uint32_t solution_dim, const uint64_t* cells, const uint32_t* local_faces,
                             uint64_t num_faces, const double* weights, const double* points, uint32_t nq, const double* data,
                             uint64_t data_count, double* out);
int fh_assemble_surface_load_dev(fh_ctx*, int load_kind, uint32_t solution_dim, const uint64_t* cells_dev, const uint32_t* local_faces_dev,
                                 uint64_t num_faces, const double* weights /* host */, const double* points /* host */, uint32_t nq,
                                 const double* data_dev, uint64_t data_count, double* out_dev);
/* x_q of every face and point (num_faces x nq x d), where the caller samples t(x) or p(x) -- as fh_physical_quadrature_points for volumes */
int fh_physical_face_quadrature_points(fh_ctx*, const uint64_t* cells, const uint32_t* local_faces, uint64_t num_faces,
                                       const double* points, uint32_t nq, double* x);
int fh_physical_face_quadrature_points_dev(fh_ctx*, const uint64_t* cells_dev, const uint32_t* local_faces_dev, uint64_t num_faces,
                                           const double* points /* host */, uint32_t nq, double* x_dev);
/* single element matrix, (s n)^2 column-major: ElementMatrixAssembler::assemble_element_matrix_into
 * (src/assembly/local.rs:78, elliptic.rs:299-340) -- for unit tests of the element kernels */
int fh_assemble_element_matrices(fh_ctx*, uint64_t first_element, uint64_t count, double* ke_out);
int fh_assemble_element_matrices_dev(fh_ctx*, uint64_t first_element, uint64_t count, double* ke_out_dev);

/* ---- post-assembly helpers (callers of the path) ------------------------------------------------ */
/* apply_homogeneous_dirichlet_bc_csr / _rhs (global.rs:379-451, 479-495) on device-resident CSR */
int fh_apply_dirichlet_csr_dev(fh_ctx*, double* values_dev, const uint64_t* nodes, uint64_t num_nodes);
int fh_apply_dirichlet_rhs_dev(fh_ctx*, double* rhs_dev, const uint64_t* nodes, uint64_t num_nodes);
/* ... of single components (nodes[k] with components[k] as for fh_set_operator_dirichlet_dofs; a node listed twice: the masks are OR-ed): the
 * rows and columns of the listed dofs, inside their node blocks, as apply_homogeneous_dirichlet_bc_csr treats the rows and columns of a node;
 * the same scale (|first nonzero diagonal entry| in row order, or 1).  A mask of 0, a component >= the solution dim, a node out of range:
 * FH_BAD_ARGUMENT.  The rhs call zeroes the listed dofs. */
int fh_apply_dirichlet_dofs_csr_dev(fh_ctx*, double* values_dev, const uint64_t* nodes, const uint8_t* components, uint64_t num_nodes);
int fh_apply_dirichlet_dofs_rhs_dev(fh_ctx*, double* rhs_dev, const uint64_t* nodes, const uint8_t* components, uint64_t num_nodes);

/* ---- host-side input generators (no device needed) -------------------------------------------- */
/* fenris-quadrature/src/univariate.rs:66-118, tensor.rs:13-55 */
int fh_gauss(uint32_t n, double* weights, double* points);
int fh_quadrilateral_gauss(uint32_t n, double* weights, double* points);
int fh_hexahedron_gauss(uint32_t n, double* weights, double* points);
/* polyquad tables (fenris-quadrature/rules/polyquad/expanded/{tet,tri}); returns FH_UNSUPPORTED for
 * strengths that are not tabulated here; *num_points receives the rule size */
int fh_tetrahedron_rule(uint32_t strength, double* weights, double* points, uint32_t* num_points);
int fh_triangle_rule(uint32_t strength, double* weights, double* points, uint32_t* num_points);
/* src/mesh/procedural.rs:46-93, 216-277, 286-403.  Sizes first (vertices/cells may be NULL). */
int fh_quad_mesh_2d(double unit_length, uint64_t units_x, uint64_t units_y, uint64_t cells_per_unit,
                    const double top_left[2], double* vertices, uint64_t* connectivity,
                    uint64_t* num_vertices, uint64_t* num_cells);
int fh_hex_mesh(double unit_length, uint64_t units_x, uint64_t units_y, uint64_t units_z, uint64_t cells_per_unit,
                double* vertices, uint64_t* connectivity, uint64_t* num_vertices, uint64_t* num_cells);
int fh_tet_mesh(double unit_length, uint64_t units_x, uint64_t units_y, uint64_t units_z, uint64_t cells_per_unit,
                double* vertices, uint64_t* connectivity, uint64_t* num_vertices, uint64_t* num_cells);
/* Hex27Mesh::from(&hex8_mesh) (src/mesh_convert.rs:85-166, 227-330).  out_vertices capacity
 * 27*num_cells*3 doubles, out_connectivity 27*num_cells. */
int fh_hex8_to_hex27(const double* vertices, uint64_t num_vertices, const uint64_t* hex8, uint64_t num_cells,
                     double* out_vertices, uint64_t* out_num_vertices, uint64_t* out_connectivity);
/* p-refinement of the linear meshes (src/mesh_convert.rs): Tet10Mesh::from(&tet4) (:42-83, 444-452: vertex nodes then
 * the edge nodes (0,1) (1,2) (0,2) (0,3) (2,3) (1,3), labels in order of first occurrence), Tri6 from Tri3 (:332-383)
 * and Quad9 from Quad4 (:385-442): the old vertices keep their indices, edge midpoints are appended in order of first
 * occurrence, Quad9 also appends the cell midpoint.  from_kind is FH_TET4 / FH_TRI3 / FH_QUAD4, FH_HEX8 for
 * Hex20Mesh::from(&hex8) (:168-217: the 8 vertex nodes and the 12 edge nodes of Hex27, same labelling); out_vertices capacity
 * (nodes per refined element) * num_cells * d doubles. */
/* Tet20Mesh::from(&tet4) (src/mesh_convert.rs:658-775): new vertices = the sorted, deduplicated 4-tuples [idx,0,0,0]
 * (vertex), [min,max,local,1] (two nodes per edge, local counted from min), [a,b,c,2] (face centroid); the label of a
 * vertex is its rank in that order.  out_vertices capacity 20 * num_cells * 3 doubles. */
int fh_tet4_to_tet20(const double* vertices, uint64_t num_vertices, const uint64_t* tet4, uint64_t num_cells,
                     double* out_vertices, uint64_t* out_num_vertices, uint64_t* out_connectivity);
int fh_refine_to_quadratic(int from_kind, const double* vertices, uint64_t num_vertices, const uint64_t* connectivity,
                           uint64_t num_cells, double* out_vertices, uint64_t* out_num_vertices, uint64_t* out_connectivity);
/* load_msh_from_bytes (src/io/msh.rs:47-111), Gmsh MSH 4.1 ASCII: vertices of all node blocks in file order (x, y for the
 * 2-D kinds), the elements of every block whose (Gmsh element type, entity dimension) matches elem_kind, node tags
 * minus one, no reordering.  Two-phase: call with vertices = connectivity = NULL for the sizes.  Blocks with
 * non-consecutive tags are refused like in the reference; binary files are not supported (FH_BAD_ARGUMENT, message
 * from fh_msh_last_error, thread-local). */
int fh_load_msh(const char* bytes, uint64_t len, int elem_kind, double* vertices, uint64_t* num_vertices,
                uint64_t* connectivity, uint64_t* num_elements);
const char* fh_msh_last_error(void);
/* Uniform refinement of a Hex8 mesh: every hexahedron splits into 8 children in the Hex8 node order, with the parent's orientation.
 * Fine vertices: the coarse vertices first under their own indices, then one per unique edge, face and cell in order of first
 * appearance (cells in order; within a cell the points of its 3x3x3 reference lattice, x fastest).  The transfer, CSR by fine node:
 * fine i = sum_k w_k coarse j_k, parents in ascending index, weights 1 (vertex), 1/2 (edge), 1/4 (face), 1/8 (cell) -- the trilinear
 * interpolation, also the placement of the new vertices.  Two calls: with out_connectivity NULL only *out_num_vertices and *out_nnz
 * are written; then out_vertices (3 per vertex), out_connectivity (64 per coarse cell), transfer_offsets (num_vertices + 1),
 * transfer_indices and transfer_weights (nnz each). */
int fh_refine_hex8_uniform(const double* vertices, uint64_t num_vertices, const uint64_t* hex8, uint64_t num_cells, double* out_vertices,
                           uint64_t* out_num_vertices, uint64_t* out_connectivity, uint64_t* transfer_offsets, uint64_t* transfer_indices,
                           double* transfer_weights, uint64_t* out_nnz);
/* ---- uniform refinement of the context's mesh on the device: Tet4 (8 children), Tri3 (4: refine_uniformly, src/mesh/refinement.rs),
 *      Quad4 (4) and Hex8 (8); any other kind and a ragged connectivity: FH_UNSUPPORTED ------------------------------------------------
 * The numbering is fh_refine_hex8_uniform's for every kind: coarse vertices keep their indices; the new vertices follow in order of
 * first appearance while sweeping the cells in order and, within a cell, the kind's list of new points in order; a new point is
 * identified by the sorted tuple of its parent coarse vertices, lies at (sum of the parents in ascending index) * (1 / count), and its
 * transfer row lists the parents in ascending index with weight 1 / count.  The result -- index arrays, vertices and weights -- is
 * bit-identical to that sequential sweep; for Hex8, to fh_refine_hex8_uniform.  New points (parents as local nodes; local index
 * n + p names point p) and children:
 *   Tet4   4=(0,1) 5=(1,2) 6=(0,2) 7=(0,3) 8=(2,3) 9=(1,3)
 *          [0,4,6,7] [4,1,5,9] [6,5,2,8] [7,9,8,3] [4,6,7,9] [4,9,5,6] [6,7,9,8] [6,8,9,5]      (Bey; every child has the parent's
 *          orientation and 1/8 of its volume; 3 congruence classes under repeated refinement)
 *   Tri3   3=(0,1) 4=(1,2) 5=(2,0)                     [0,3,5] [3,1,4] [5,4,2] [3,4,5]
 *   Quad4  4=(0,1) 5=(1,2) 6=(2,3) 7=(3,0) 8=(0,1,2,3) [0,4,8,7] [4,1,5,8] [8,5,2,6] [7,8,6,3]
 *   Hex8   the 3x3x3 lattice, x fastest, and child (cx, cy, cz), exactly as fh_refine_hex8_uniform
 * The children of cell e are cells C e .. C e + C - 1.  fh_refine_uniform keeps the result on the context, on the device, until the next
 * fh_refine_uniform, fh_set_mesh* or fh_set_connectivity_ragged (fh_update_vertices keeps it, with the positions it was formed from);
 * without a held result the three functions below return FH_INVALID_STATE.  num_elements * new points per cell (6, 3, 5, 19) must be
 * < 2^31, else FH_UNSUPPORTED.  Scratch, released on return: 24 bytes per (cell, new point) plus the radix sort's own temporary. */
int fh_refine_uniform(fh_ctx*, uint64_t* out_num_vertices, uint64_t* out_num_cells, uint64_t* out_nnz);
/* copies of the held result; any pointer may be NULL.  vertices: d per vertex; connectivity: n per cell; transfer_offsets:
 * num_vertices + 1; transfer_indices, transfer_weights: nnz each (the layout fh_mg_create reads) */
int fh_refinement_mesh(fh_ctx*, double* vertices, uint64_t* connectivity);
int fh_refinement_transfer(fh_ctx*, uint64_t* transfer_offsets, uint64_t* transfer_indices, double* transfer_weights);
/* fh_set_mesh on `fine` with the refinement that `coarse` holds, device to device (fine == coarse is allowed: the context then holds
 * no refinement afterwards).  Contexts on different devices: FH_BAD_ARGUMENT. */
int fh_set_mesh_from_refinement(fh_ctx* fine, fh_ctx* coarse);
/* ---- degree coarsening of the context's mesh on the device: Tet10 -> Tet4, Tri6 -> Tri3, Quad9 -> Quad4, Hex20 -> Hex8, Hex27 -> Hex8;
 *      a linear kind, Tet20 and a ragged connectivity: FH_UNSUPPORTED --------------------------------------------------------------------
 * The linear mesh on the vertex nodes of the mesh, and the transfer that interpolates linear nodal values to all of its nodes: the
 * p-coarsening step of a multigrid hierarchy (fh_mg_create takes the transfer as it is).
 *   vertex nodes   the nodes in a vertex slot of a cell: its first 3 (Tri6), 4 (Tet10, Quad9) or 8 (Hex20, Hex27) local nodes.  The
 *                  coarse index of a vertex node is its rank among the vertex nodes in ascending fine index; vertex_nodes[j] is the
 *                  fine index of coarse vertex j, and coarse vertex j has that node's position, bit for bit.
 *   coarse cells   coarse cell e is the vertex slots of fine cell e in their order, renamed to coarse indices: cell order and node order
 *                  are the fine mesh's.
 *   transfer       CSR by fine node.  A vertex node's row is (its coarse index, 1.0).  Any other node lists the vertex nodes of its edge,
 *                  face or cell in ascending coarse index, each with weight 1 / count: 1/2 on an edge, 1/4 on a face, 1/8 in a cell --
 *                  the linear element's basis functions at the node's reference position.
 * Parents of the non-vertex local nodes, as local nodes (the node orders of the element kinds):
 *   Tet10          4=(0,1) 5=(1,2) 6=(0,2) 7=(0,3) 8=(2,3) 9=(1,3)
 *   Tri6           3=(0,1) 4=(1,2) 5=(0,2)
 *   Quad9          4=(0,1) 5=(1,2) 6=(2,3) 7=(0,3) 8=(0,1,2,3)
 *   Hex20, Hex27   8=(0,1) 9=(0,3) 10=(0,4) 11=(1,2) 12=(1,5) 13=(2,3) 14=(2,6) 15=(3,7) 16=(4,5) 17=(4,7) 18=(5,6) 19=(6,7)
 *   Hex27          20=(0,1,2,3) 21=(0,1,4,5) 22=(0,3,4,7) 23=(1,2,5,6) 24=(2,3,6,7) 25=(4,5,6,7) 26=(0,..,7)
 * The pass validates the mesh and returns FH_BAD_ARGUMENT, with a message naming the smallest such node, when a node belongs to no
 * cell, when a node is in a vertex slot of one cell and in another slot of another, or when the sorted parents of a non-vertex node
 * differ between two cells that share it; the context stays usable.  num_elements * nodes per cell and num_vertices * most parents
 * of a node (2, 2, 4, 2, 8) must be < 2^31, else FH_UNSUPPORTED.  The output is the same on every call.
 * fh_coarsen_degree keeps the result on the context, on the device, until the next fh_coarsen_degree, fh_set_mesh* or
 * fh_set_connectivity_ragged (fh_update_vertices keeps it, with the positions it was formed from); without a held result the three
 * functions below return FH_INVALID_STATE.  A held refinement (fh_refine_uniform) and a held degree coarsening do not touch each other.
 * Scratch, released on return: 28 bytes per node plus the scan's own temporary. */
int fh_coarsen_degree(fh_ctx*, uint64_t* out_num_vertices, uint64_t* out_nnz);
/* copies of the held result; any pointer may be NULL.  vertices: d per coarse vertex; connectivity: 3, 4 or 8 per cell; vertex_nodes:
 * one per coarse vertex; transfer_offsets: (nodes of the fine mesh) + 1; transfer_indices, transfer_weights: nnz each */
int fh_degree_coarsening_mesh(fh_ctx*, double* vertices, uint64_t* connectivity, uint64_t* vertex_nodes);
int fh_degree_coarsening_transfer(fh_ctx*, uint64_t* transfer_offsets, uint64_t* transfer_indices, double* transfer_weights);
/* fh_set_mesh on `linear` with the degree coarsening that `high` holds, device to device (linear == high is allowed: the context then
 * holds no coarsening afterwards).  Contexts on different devices: FH_BAD_ARGUMENT. */
int fh_set_mesh_from_degree_coarsening(fh_ctx* linear, fh_ctx* high);
/* ---- degree elevation of the context's mesh on the device: Tet4 -> Tet10, Tri3 -> Tri6, Quad4 -> Quad9, Hex8 -> Hex20, Hex8 -> Hex27;
 *      any other to_kind for a linear context: FH_BAD_ARGUMENT; a quadratic or cubic context and a ragged connectivity: FH_UNSUPPORTED ---
 * The straight-sided quadratic mesh over the linear one, and the transfer that interpolates linear nodal values to all of its nodes (the
 * p-step of a multigrid hierarchy; fh_mg_create takes the transfer as it is).  Index arrays and vertex coordinates are bit-identical to
 * fh_refine_to_quadratic and, for Hex27, fh_hex8_to_hex27; the parents of the non-vertex local nodes are those listed above.
 *   Tet10, Hex20,  sweep the cells in order and, within a cell, its local nodes 0 .. n - 1 in order; a node is identified by the sorted
 *   Hex27          tuple of its parent linear vertices (1, 2, 4 or 8); its label is its rank in order of first occurrence.  Old vertex
 *                  indices are not kept, and a vertex of no cell disappears.
 *   Tri6, Quad9    the old vertices keep their indices (those of no cell too); the midpoints of the edges (m, m + 1 mod n0) follow in
 *                  order of first occurrence, for Quad9 the cell's centre right after the cell's edges.
 *   position       computed by the (cell, slot) of the node's first occurrence in that cell's local node order: X[a] for a vertex;
 *                  0.5 X[b] + 0.5 X[a] on an edge of Tet10, Hex20 and Hex27, (X[a] + X[b]) / 2 of Tri6 and Quad9; on a Hex27 face and in
 *                  its centre the 8-term trilinear sum over the local nodes in order (weights 1/4 on the face, 1/8 in the centre, 0
 *                  elsewhere); sum_k 0.25 X[k], k ascending, in a Quad9's centre.
 *   transfer       CSR by high node over the context's vertices.  A vertex node's row is (its linear index, 1.0).  Any other node lists
 *                  its parents in ascending linear index, each with weight 1 / count: the convention of fh_coarsen_degree.
 * num_elements * nodes per high cell must be < 2^31, else FH_UNSUPPORTED.  The output does not depend on the launch geometry and is the
 * same on every call.  fh_elevate_degree keeps the result on the context, on the device, until the next fh_elevate_degree, fh_set_mesh*
 * or fh_set_connectivity_ragged (fh_update_vertices keeps it, with the positions it was formed from); without a held result the three
 * functions below return FH_INVALID_STATE.  A held elevation, a held refinement and a held degree coarsening do not touch each other.
 * Scratch, released on return: 24 bytes per labelled (cell, slot) -- every slot of Tet10, Hex20 and Hex27, the non-vertex slots of Tri6
 * and Quad9 -- plus the radix sort's own temporary. */
int fh_elevate_degree(fh_ctx*, int to_kind, uint64_t* out_num_vertices, uint64_t* out_nnz);
/* copies of the held result; any pointer may be NULL.  vertices: d per high node; connectivity: n per cell; transfer_offsets:
 * num_vertices + 1; transfer_indices, transfer_weights: nnz each (the layout fh_mg_create reads) */
int fh_degree_elevation_mesh(fh_ctx*, double* vertices, uint64_t* connectivity);
int fh_degree_elevation_transfer(fh_ctx*, uint64_t* transfer_offsets, uint64_t* transfer_indices, double* transfer_weights);
/* fh_set_mesh on `high` with the degree elevation that `linear` holds, device to device (high == linear is allowed: the context then
 * holds no elevation afterwards).  Contexts on different devices: FH_BAD_ARGUMENT. */
int fh_set_mesh_from_degree_elevation(fh_ctx* high, fh_ctx* linear);
/* ---- point location and interpolation at arbitrary points on the device (SpatiallyIndexed, FixedInterpolator of src/space) ---
 * Tri3, Tri6, Tet4, Tet10 and Tet20 meshes; quadrilateral and hexahedral kinds and a ragged connectivity: FH_UNSUPPORTED (the
 * reference has no closest_point for them).  The kinds are sub-parametric: location uses the vertex nodes (the Tri3 / Tet4
 * geometry), basis values and gradients the element's own kind.
 * Every element e reports closest_point(e, p) as the reference's element code does (triangle.rs:440-527, tetrahedron.rs:616-672):
 * InElement or ClosestPoint, reference coordinates xi_e, and d2_e = |x_e(xi_e) - p|^2.  The answer for p is the InElement report
 * with the LOWEST element index when there is one, else the report with the smallest d2_e, the lower index on a tie: one of the
 * answers the reference may give (it takes the first InElement in R-tree order), made independent of any traversal order.  The
 * index prunes only what cannot change that answer.  No floating-point atomics: every call repeats bit for bit.
 * The index (element boxes scaled by 1.01 about their centres, a uniform cell grid, per-cell element lists in ascending order) is
 * held on the context; fh_set_mesh*, fh_set_mesh_from_*, fh_set_connectivity_ragged and fh_update_vertices drop it, and the calls
 * below build it when it is missing. */
int fh_point_index_build(fh_ctx*);
/* points: m x d.  element: m (UINT64_MAX: no element, a mesh without elements or, _dev only, a non-finite coordinate); xi: m x d
 * reference coordinates; in_element (may be NULL): m flags, 1 for InElement.  The host entry point returns FH_BAD_ARGUMENT for a
 * non-finite coordinate; the _dev one (all pointers on the device, enqueued on the context's stream) gives such a point
 * UINT64_MAX and xi = 0. */
int fh_locate_points(fh_ctx*, const double* points, uint64_t m, uint64_t* element, double* xi, uint8_t* in_element);
int fh_locate_points_dev(fh_ctx*, const double* points_dev, uint64_t m, uint64_t* element_dev, double* xi_dev, uint8_t* in_element_dev);
/* A fixed interpolator: for each of m points the n nodes of its element in element order, their basis values and / or their
 * physical gradients J^-T grad phi (d per node) -- a CSR by point with offsets n i.  It owns its device arrays and outlives changes
 * of the context's mesh; it works on the device and stream the context had when it was created.  A point without an element
 * (see above) has index 0 and zero weights; gradients on an element without volume are NaN. */
typedef struct fh_interpolator fh_interpolator;
#define FH_INTERP_BOTH 0
#define FH_INTERP_VALUES 1
#define FH_INTERP_GRADIENTS 2
int fh_interpolator_create(fh_ctx*, const double* points, uint64_t m, int what, fh_interpolator** out);
int fh_interpolator_create_dev(fh_ctx*, const double* points_dev, uint64_t m, int what, fh_interpolator** out);
/* FixedInterpolator::from_compressed_values with its assertions as FH_BAD_ARGUMENT (the message: fh_last_error of the context):
 * offsets (m + 1) within num_indices and not decreasing -- rows may differ in length or be empty --, num_values == num_indices
 * when values are given, num_gradients == d * num_indices when gradients are given (d = 1, 2 or 3).  Either may be NULL. */
int fh_interpolator_from_compressed(fh_ctx*, uint32_t d, uint64_t m, const uint64_t* offsets, const uint64_t* indices, uint64_t num_indices,
                                    const double* values, uint64_t num_values, const double* gradients, uint64_t num_gradients,
                                    fh_interpolator** out);
void fh_interpolator_destroy(fh_interpolator*);
const char* fh_interpolator_last_error(const fh_interpolator*);
/* any pointer may be NULL.  offsets: num_points + 1; indices, values: num_indices; gradients: d * num_indices, d per index */
int fh_interpolator_sizes(const fh_interpolator*, uint64_t* num_points, uint64_t* num_indices, uint32_t* geometry_dim, int* has_values,
                          int* has_gradients);
int fh_interpolator_data(fh_interpolator*, uint64_t* offsets, uint64_t* indices, double* values, double* gradients);
/* out[p sdim + j] = sum over the entries k of point p, in stored order, of value_k u[sdim node_k + j]  (m x sdim);
 * gradients: out[p d sdim + j d + i] = sum of gradient_k[i] u[sdim node_k + j]  (per point d x sdim, column-major).
 * u_len: the doubles u holds; sdim * (largest node index + 1) > u_len: FH_BAD_ARGUMENT (an interpolator created from a mesh counts
 * the mesh's last node).  Applying what was not computed: FH_INVALID_STATE.  m == 0 is valid.  sdim: 1 .. 64. */
int fh_interpolator_apply(fh_interpolator*, uint32_t sdim, const double* u, uint64_t u_len, double* out);
int fh_interpolator_apply_dev(fh_interpolator*, uint32_t sdim, const double* u_dev, uint64_t u_len, double* out_dev);
int fh_interpolator_apply_gradients(fh_interpolator*, uint32_t sdim, const double* u, uint64_t u_len, double* out);
int fh_interpolator_apply_gradients_dev(fh_interpolator*, uint32_t sdim, const double* u_dev, uint64_t u_len, double* out_dev);
/* cuthill_mckee on a square sparsity pattern (src/mesh/reorder.rs:171-233): perm_out[target] = source.  The
 * reference orders equal-degree neighbours with an unstable sort (unspecified); ties are broken by ascending index. */
int fh_cuthill_mckee(uint64_t num_rows, const uint64_t* row_offsets, const uint64_t* col_indices, uint64_t* perm_out);
/* reorder_mesh_par (src/mesh/reorder.rs:54-95): reverse Cuthill-McKee vertex permutation + elements sorted by their
 * smallest new vertex index.  vertex_perm[new] = old, connectivity_perm[new] = old; MeshPermutation::apply
 * (reorder.rs:29-52) relabels the vertex indices inside the elements with the inverse vertex permutation. */
int fh_reorder_mesh(uint64_t num_vertices, uint64_t nodes_per_element, const uint64_t* connectivity, uint64_t num_elements,
                    uint64_t* vertex_perm, uint64_t* connectivity_perm);
/* LameParameters::from(YoungPoisson) (fenris-solid/src/materials.rs:31-43) */
int fh_lame_from_young_poisson(double young, double poisson, double* mu, double* lambda);
/* The (mu, lambda) of FH_STABLE_NEO_HOOKEAN whose linearisation at F = I has the Lame parameters (mu_lame, lambda_lame) in dimension dim:
 * mu = (d + 1)/d mu_lame, lambda = lambda_lame + mu_lame - 2 mu_lame / (d (d + 1))  (d = 3: 4/3 mu_lame and lambda_lame + 5/6 mu_lame).
 * FH_BAD_ARGUMENT for a dim other than 2 or 3 or a null pointer. */
int fh_stable_neo_hookean_parameters(uint32_t dim, double mu_lame, double lambda_lame, double* mu, double* lambda);

/* ---- introspection for benchmarks --------------------------------------------------------------- */
/* name of the device kernel the last fh_assemble_matrix* call launched (for rocprof matching) */
const char* fh_last_kernel_name(const fh_ctx*);

/* ---- solve + error estimation on the device-resident system (what every caller does next) ------------ */
/* y = K x on the CSR of the context's pattern: LinearOperator for CsrMatrix (fenris-sparse/src/cg.rs:44-52) */
int fh_spmv_dev(fh_ctx*, const double* values_dev, const double* x_dev, double* y_dev);
/* ConjugateGradient::solve_with_guess (fenris-sparse/src/cg.rs:366-478) with RelativeResidualCriterion(rel_tol)
 * (:86-124, the solver's own residual, ||r|| <= tol ||b||) and, for FH_PRECOND_JACOBI, the inverse diagonal as
 * the preconditioner -- exactly how solve_linear_system drives it (tests/convergence_tests/
 * poisson_mms_common.rs:142-163: max_iter 10000, tol 1e-9).  x holds the initial guess on entry and the solution on
 * return (the iterate reached so far on failure); max_iter == 0 means no limit; *num_iterations counts the updates
 * of x.  Errors: FH_CG_MAX_ITERATIONS, FH_CG_INDEFINITE_OPERATOR (p.Ap <= 0), FH_CG_INDEFINITE_PRECONDITIONER
 * (z.r <= 0).  Reductions are ordered (no floating-point atomics): runs are bitwise reproducible. */
enum { FH_PRECOND_IDENTITY = 0, FH_PRECOND_JACOBI = 1, FH_PRECOND_MULTIGRID = 2 };
int fh_cg_solve(fh_ctx*, const double* values, const double* b, double* x, int preconditioner, double rel_tol,
                uint64_t max_iter, uint64_t* num_iterations);
int fh_cg_solve_dev(fh_ctx*, const double* values_dev, const double* b_dev, double* x_dev, int preconditioner, double rel_tol,
                    uint64_t max_iter, uint64_t* num_iterations);
/* ---- matrix-free operator: LinearOperator (fenris-sparse/src/cg.rs:16-51) for FH_LAPLACE and FH_LINEAR_ELASTIC without a pattern
 * or values.  The element vector of these operators is linear in u, so the residual's element pass fed x gives  A x = K x;  it honours
 * the context's operator, quadrature table (uniform, per-point, compact, rule sets), element mask (fh_set_active_elements) and every
 * element kind.  Other operators: FH_UNSUPPORTED.  Missing mesh, operator or quadrature table: FH_INVALID_STATE.
 *
 * fh_set_operator_dirichlet_nodes: homogeneous Dirichlet nodes of the operator (membership flags on the device; NULL / 0 clears them, and
 * so does fh_set_mesh*).  With them, A is the matrix fh_apply_dirichlet_csr_dev leaves of the assembled K (global.rs:379-451): the rows and
 * columns of the constrained dofs are zero and their diagonal is scale = |first nonzero diagonal entry| in row order, or 1. */
int fh_set_operator_dirichlet_nodes(fh_ctx*, const uint64_t* nodes, uint64_t num_nodes);
/* Single displacement components (rollers, symmetry planes): nodes[k] with components[k], bit j set = component j of that node is constrained
 * (j < solution dim).  Replaces whatever fh_set_operator_dirichlet_nodes / _dofs set before; NULL / 0 clears; fh_set_mesh* clears.  A node
 * listed twice: the masks are OR-ed.  A mask of 0: FH_BAD_ARGUMENT.  A node >= num_vertices: FH_BAD_ARGUMENT.  fh_set_operator_dirichlet_nodes
 * is this call with every component of each node, bit for bit.  Every route that honours the node set honours the dofs with the same meaning
 * per dof: the operator, tangent and shifted tangent and their solvers, Newton, multigrid, fh_eigs_lowest, the time integrators (prescribed
 * boundary motion moves the constrained components alone) and the contact term, whose force and tangent block act on the free components of a
 * partly constrained node.  A mask, other than all ones, that names a component >= the solution dim of the operator in use is refused with
 * FH_BAD_ARGUMENT and the node's name when a route uses the set (the operator may be set after the dofs). */
int fh_set_operator_dirichlet_dofs(fh_ctx*, const uint64_t* nodes, const uint8_t* components, uint64_t num_nodes);
/* y = A x, both s N doubles on the device.  y is OVERWRITTEN (LinearOperator::apply, cg.rs:16-18); x may hold anything on the constrained
 * dofs; the context's u (fh_set_u*) is neither read nor changed.  FH_SINGULAR_JACOBIAN as the residual reports it.  Deterministic
 * on every element kind (no floating-point atomics: element vectors summed per node in a fixed order).  With Dirichlet nodes set, the
 * scale comes from the diagonal, formed again only after the mesh, vertices, operator, table or element mask have changed. */
int fh_apply_operator_dev(fh_ctx*, const double* x_dev, double* y_dev);
/* the diagonal of A (s N doubles on the device), after the Dirichlet modification when nodes are set, without forming A: per point
 * w |det J| |g_a|^2 (Laplace) or w |det J| (mu (|g_a|^2 + g_a,i^2) + lambda g_a,i^2) (LinearElastic) for dof (a, i), g_a the physical
 * gradient of basis function a, summed in a fixed order like the residual. */
int fh_operator_diagonal_dev(fh_ctx*, double* diag_dev);
/* fh_cg_solve(_dev) with A the matrix-free operator: the same contract (RelativeResidualCriterion, error codes, the iterate handed back
 * on failure, ordered reductions, bitwise reproducible); FH_PRECOND_JACOBI takes the inverse of fh_operator_diagonal_dev.  On the element
 * kinds of the tiles (Hex8, Tet4, Quad4, Tri3) it allocates no pattern and no values. */
int fh_cg_solve_matrix_free(fh_ctx*, const double* b, double* x, int preconditioner, double rel_tol, uint64_t max_iter,
                            uint64_t* num_iterations);
int fh_cg_solve_matrix_free_dev(fh_ctx*, const double* b_dev, double* x_dev, int preconditioner, double rel_tol, uint64_t max_iter,
                                uint64_t* num_iterations);
/* ---- matrix-free tangent: T(u) = dr/du at the context's u (fh_set_u*; zeros when none is set), r the residual of fh_assemble_vector
 * (elliptic.rs:457-605).  T(u) is the matrix fh_assemble_matrix assembles for the same context, K_IJ = sum_q w |det J| C(F_q; g_I, g_J) with C
 * the stress contraction (fenris-solid/src/materials.rs); for FH_LAPLACE and FH_LINEAR_ELASTIC it is the operator above, bit for bit (the
 * same kernels and the same Dirichlet scale).  Per point the element vector of x is  y_a += w |det J| dP(F)[H] g_a,  F = I + grad u^T,
 * H = grad x^T:
 *   Laplace h;  LinearElastic mu (H + H^T) + lambda tr(H) I;
 *   NeoHookean mu H + lambda tr(F^-1 H) F^-T + (mu - lambda ln J) F^-T H^T F^-T;
 *   StVK H S + F (lambda tr(dE) I + 2 mu dE), S = lambda tr(E) I + 2 mu E, dE = sym(F^T H).
 * x enters linearly.  A point of an active element with J <= 0 puts NaN into that element's rows (like the assembled K(u)); masked elements
 * add zero.  It honours the quadrature table (uniform, per-point, compact, rule sets), the element mask and every element kind.  Errors:
 * FH_UNSUPPORTED for the mass operators and FH_TENSOR; FH_INVALID_STATE for a missing mesh, operator or table; FH_SINGULAR_JACOBIAN as the
 * residual reports it.  Dirichlet nodes: those of fh_set_operator_dirichlet_nodes, with the same meaning as for fh_apply_operator_dev (the
 * matrix fh_apply_dirichlet_csr_dev leaves of the assembled K(u); scale = |first nonzero diagonal entry| of K(u) in row order, or 1).  The scale
 * is the operator's cache, formed again after the mesh, vertices, operator, table or element mask have changed, and for FH_NEO_HOOKEAN,
 * FH_STVK and FH_STABLE_NEO_HOOKEAN also after u has changed.
 *
 * y = T(u) x, both s N doubles on the device; y is OVERWRITTEN, u is read and not changed.  Deterministic on every element kind (no
 * floating-point atomics). */
int fh_apply_tangent_dev(fh_ctx*, const double* x_dev, double* y_dev);
/* the diagonal of T(u) (s N doubles on the device), after the Dirichlet modification when nodes are set, formed per element without forming
 * T: entry (a, i) = sum_q w |det J| (dP(F)[e_i g_a^T] g_a)_i, e.g. NeoHookean sum w |det J| ((lambda - alpha) (F^-T g_a)_i^2 + mu |g_a|^2),
 * alpha = -mu + lambda ln J. */
int fh_tangent_diagonal_dev(fh_ctx*, double* diag_dev);
/* fh_cg_solve_matrix_free(_dev) with A = T(u): the same contract and error codes, the iterate handed back on failure, bitwise reproducible;
 * FH_PRECOND_JACOBI takes the inverse of fh_tangent_diagonal_dev. */
int fh_cg_solve_tangent(fh_ctx*, const double* b, double* x, int preconditioner, double rel_tol, uint64_t max_iter, uint64_t* num_iterations);
int fh_cg_solve_tangent_dev(fh_ctx*, const double* b_dev, double* x_dev, int preconditioner, double rel_tol, uint64_t max_iter,
                            uint64_t* num_iterations);
/* ---- matrix-free shifted tangent for implicit time stepping: (alpha M + beta T(u)) Delta = b, e.g. backward Euler alpha = 1, beta = dt^2.
 * M is the mass matrix the assembled FH_MASS_SCALAR / FH_MASS_VECTOR form on the same mesh and quadrature table, M_IJ = I_s sum_q w |det J|
 * rho phi_I phi_J with s the context operator's solution dim (Laplace: the scalar mass, the materials: the vector mass), rho the density of
 * fh_set_mass_density; T(u) is fh_apply_tangent_dev's map.  Operators: FH_LAPLACE, FH_LINEAR_ELASTIC, FH_NEO_HOOKEAN, FH_STVK, FH_STABLE_NEO_HOOKEAN (mass operators
 * and FH_TENSOR: FH_UNSUPPORTED).  alpha != 0 without a density: FH_INVALID_STATE; alpha and beta not finite: FH_BAD_ARGUMENT.  alpha == 0
 * runs the tangent's kernels alone (alpha == 0, beta == 1: exactly fh_apply_tangent_dev); beta == 0 runs no stiffness work and does not read
 * u.  It honours every element kind, every table form, the element mask and the Dirichlet nodes of fh_set_operator_dirichlet_nodes, with the
 * same meaning as for the tangent: the matrix fh_apply_dirichlet_csr_dev leaves of the assembled alpha M + beta K(u), scale = |first nonzero
 * diagonal entry of alpha M + beta K(u)| in row order, or 1.  The scale shares the tangent's one-entry cache, keyed also on alpha, beta and
 * the density: calls that alternate between the shifted map and the plain one (or between two pairs of coefficients) form it again each
 * time.  Deterministic (no floating-point atomics).
 *
 * fh_set_mass_density: count == 1, one density for the whole mesh; count == E, one per element (by element id).  Other counts or a null
 * pointer: FH_BAD_ARGUMENT.  fh_set_mesh* drops the density. */
int fh_set_mass_density(fh_ctx*, const double* rho, uint64_t count);
/* y = (alpha M + beta T(u)) x, both s N doubles on the device; y is OVERWRITTEN. */
int fh_apply_shifted_tangent_dev(fh_ctx*, double alpha, double beta, const double* x_dev, double* y_dev);
/* its diagonal alpha sum_q w |det J| rho phi_a^2 + beta diag T(u), after the Dirichlet modification when nodes are set. */
int fh_shifted_tangent_diagonal_dev(fh_ctx*, double alpha, double beta, double* diag_dev);
/* ---- per-element expansion: thermal strain, swelling, growth, shrink fits.  theta_e > 0 is the isotropic stress-free stretch of element e
 * (1: none; thermal expansion: theta_e = 1 + alpha_e (T_e - T_ref)).  With d the dimension and gu = grad u at a quadrature point,
 *   FH_LINEAR_ELASTIC, additive small strain:     gu_e = gu - (theta - 1) I,  P = P_0(gu_e),  psi = psi_0(gu_e),  the tangent unchanged
 *                                                 (so A x, the assembled stiffness and fh_apply_tangent* do not change; r(0) = -f_th);
 *   FH_NEO_HOOKEAN, FH_STVK, FH_STABLE_NEO_HOOKEAN, multiplicative split F = F_e theta:
 *                                                 gu_e = (gu - (theta - 1) I) / theta,  psi = theta^d psi_0(gu_e),  P = theta^(d-1) P_0(gu_e),
 *                                                 dP[H] = theta^(d-2) dP_0(gu_e)[H]   (linearised about theta = 1: the additive law).
 * While a field is set, every element-to-node route of these four operators honours it: fh_assemble_vector(_dev, _async_dev),
 * fh_assemble_scalar, fh_apply_tangent_dev and fh_tangent_diagonal_dev, the shifted tangent and its diagonal, their CG solves,
 * fh_newton_solve(_dev), the second- and first-order time integrators (they see a frozen field), fh_dynamics_stable_dt, fh_eigs_lowest and
 * fh_recover* (the stresses and the energy density come from the elastic part -- the Cauchy and von Mises stress of F_e, the first
 * Piola-Kirchhoff stress and the energy density per reference volume; strain and grad u stay the total ones).  Element masks and compact
 * tables work; contact, friction and the Dirichlet handling are node-level and untouched; the mass operators ignore the field.  While no
 * field is set every route runs the kernels it ran before and gives the same bits; a field whose stretches are all exactly 1 runs those
 * kernels too (it is no expansion), while the refusals below and fh_element_expansion treat it as the field it is.
 * FH_UNSUPPORTED, with a message that names the expansion, while a field is set: FH_LAPLACE and FH_TENSOR on the routes above; the assembled
 * stiffness (fh_assemble_matrix*, fh_assemble_element_matrices*, and so FH_PRECOND_AMG) of the three hyperelastic operators (the matrix of
 * FH_LINEAR_ELASTIC is unaffected and allowed); FH_PRECOND_MULTIGRID with a hyperelastic operator (linear elasticity is allowed); rule-set
 * tables (fh_set_quadrature_rules); ragged connectivity (at the setters).
 *
 * fh_set_element_expansion(_dev): count == 1, one stretch for the mesh; count == E, one per element (by element id, as fh_set_mass_density);
 * a null pointer or count == 0 clears the field.  A value that is not finite or not positive: FH_BAD_ARGUMENT, the message names the lowest
 * such element; any other count: FH_BAD_ARGUMENT; the standing field is kept then.  fh_set_mesh* drops the field.  Setting or clearing it
 * invalidates what the context cached for the old one (the tangent's Dirichlet scale, the integrators' accelerations).
 * fh_set_thermal_expansion(_dev): theta_e = 1 + alpha_e (mean of the element's nodal temperatures - T_ref) formed on the device, the
 * temperatures (N doubles) summed in local node order; alpha_count is 1 or E.  The same validity check on the result.
 * fh_element_expansion: the E stretches in force (a uniform field E times); FH_INVALID_STATE when none is set. */
int fh_set_element_expansion(fh_ctx*, const double* theta, uint64_t count);
int fh_set_element_expansion_dev(fh_ctx*, const double* theta_dev, uint64_t count);
int fh_set_thermal_expansion(fh_ctx*, const double* T_nodes, const double* alpha, uint64_t alpha_count, double T_ref);
int fh_set_thermal_expansion_dev(fh_ctx*, const double* T_nodes_dev, const double* alpha_dev, uint64_t alpha_count, double T_ref);
int fh_element_expansion(fh_ctx*, double* theta_out);
/* the thermal load f_th = -r(0) of FH_LINEAR_ELASTIC under the field in force (s N doubles, OVERWRITTEN): K u = f + f_th is the linear
 * problem.  The context's u is neither read nor changed.  Any other operator: FH_UNSUPPORTED (the hyperelastic residual is not affine in
 * u); no field set: FH_INVALID_STATE. */
int fh_thermal_load(fh_ctx*, double* out);
int fh_thermal_load_dev(fh_ctx*, double* out_dev);
/* fh_cg_solve_tangent(_dev) with A = alpha M + beta T(u): the same contract and error codes, the iterate handed back on failure, bitwise
 * reproducible; FH_PRECOND_JACOBI takes the inverse of fh_shifted_tangent_diagonal_dev. */
int fh_cg_solve_shifted_tangent(fh_ctx*, double alpha, double beta, const double* b, double* x, int preconditioner, double rel_tol,
                                uint64_t max_iter, uint64_t* num_iterations);
int fh_cg_solve_shifted_tangent_dev(fh_ctx*, double alpha, double beta, const double* b_dev, double* x_dev, int preconditioner, double rel_tol,
                                    uint64_t max_iter, uint64_t* num_iterations);
/* ---- Newton's method for F(u) = 0 with F(u) = alpha M (u - u_ref) + beta (r(u) - f) and the Jacobian J(u) = alpha M + beta T(u), the map of
 * fh_apply_shifted_tangent_dev: alpha = 0, beta = 1 is static equilibrium r(u) = f; alpha = 1, beta = dt^2 a backward-Euler step on positions
 * (u_ref = u_n + dt v_n).  newton_line_search (fenris-optimize/src/newton.rs:77-130) step for step:
 *   - converged when ||F||_2 <= tolerance (absolute), tested before every iteration: a guess that satisfies it returns after 0 iterations;
 *   - MaximumIterationsReached when the iteration count has reached max_iterations (0: no limit) before convergence (newton.rs:99-106);
 *   - the Newton step: J (-dx) = F by fh_cg_solve_shifted_tangent_dev's Jacobi-PCG (preconditioner, RelativeResidualCriterion(linear_rel_tol),
 *     linear_max_iter; 0: no limit) from a zero guess, p = -(-dx) (newton.rs:108-117); any error of that solve (the FH_CG_* codes, or what
 *     the map reports, e.g. FH_SINGULAR_JACOBIAN) gives FH_NEWTON_JACOBIAN_ERROR with the inner code in stats[3];
 *   - FH_NEWTON_NO_LINE_SEARCH: u += p (NoLineSearch, newton.rs:140-163);
 *   - FH_NEWTON_BACKTRACKING: BacktrackingLineSearch (newton.rs:165-249), c = 1e-4, alpha_min = 1e-6: trial step lengths a = 1, 0.75, 0.5,
 *     0.25, 0.0625, ... (0.25 each time), u += (a - a_prev) p, accepted when g <= (1 - c a) g_0 with g = ||F||^2 / 2; after a trial with
 *     a < alpha_min that is not accepted: FH_NEWTON_LINE_SEARCH_FAILED.  A trial state whose residual is NaN (NeoHookean with det F <= 0 at
 *     a quadrature point) compares false and the search backtracks past it.
 * One deliberate deviation: newton.rs:98 leaves its loop on a NaN norm and reports success; here a non-finite ||F|| of an ACCEPTED state (the
 * guess, or any state under FH_NEWTON_NO_LINE_SEARCH) ends the solve with FH_NEWTON_LINE_SEARCH_FAILED.
 * Dirichlet dofs: the nodes of fh_set_operator_dirichlet_nodes, held at the values u has on entry (inhomogeneous values allowed): F is zero on
 * their rows and so is the step, so those entries of u come back bit for bit.  f_dev (the load) and u_ref_dev: S N doubles, or null for zero.
 * u_dev: the guess on entry (with the Dirichlet values); on return the iterate the reference leaves in x -- the solution, or on failure the
 * last iterate (for FH_NEWTON_LINE_SEARCH_FAILED from the search: the last trial).  The context's u (fh_set_u*) holds the same on return and
 * u_gen has moved.  Operators: FH_LAPLACE, FH_LINEAR_ELASTIC, FH_NEO_HOOKEAN, FH_STVK, FH_STABLE_NEO_HOOKEAN (mass operators, FH_TENSOR: FH_UNSUPPORTED); alpha != 0
 * without fh_set_mass_density: FH_INVALID_STATE; alpha, beta or tolerance not finite, a null u, an unknown line search or preconditioner:
 * FH_BAD_ARGUMENT.  It honours the element kinds, table forms and element masks of the residual.  The residual and its norm come from one node
 * pass over the tile partials on Hex8, Tet4, Quad4 and Tri3 (no rule-set table); elsewhere from element vectors summed per node in a fixed
 * order and the mass term, composed.  No floating-point atomics on either route: a solve repeats bit for bit on every element kind.
 * stats (may be null): [0] Newton iterations, [1] residual evaluations, [2] PCG iterations summed, [3] status of the last PCG;
 * norms (may be null): [0] ||F(u_0)||, [1] ||F|| at return, [2] the last accepted step length (0: none). */
enum { FH_NEWTON_NO_LINE_SEARCH = 0, FH_NEWTON_BACKTRACKING = 1 };
int fh_newton_solve_dev(fh_ctx*, double alpha, double beta, const double* f_dev, const double* u_ref_dev, double* u_dev, double tolerance,
                        uint64_t max_iterations, int line_search, int preconditioner, double linear_rel_tol, uint64_t linear_max_iter,
                        uint64_t* stats, double* norms);
/* the same with host arrays */
int fh_newton_solve(fh_ctx*, double alpha, double beta, const double* f, const double* u_ref, double* u, double tolerance, uint64_t max_iterations,
                    int line_search, int preconditioner, double linear_rel_tol, uint64_t linear_max_iter, uint64_t* stats, double* norms);
/* ---- the lowest eigenpairs of  T(u) phi = lambda M phi  (natural frequencies and mode shapes; the stiffness of a prestressed state; the
 * smallest eigenvalue of a Newton iterate's tangent), matrix-free: T(u) is fh_apply_tangent_dev's map at the context's u (Laplace,
 * LinearElastic: K), M the mass of fh_set_mass_density.  The problem is restricted to the dofs that are not Dirichlet
 * (fh_set_operator_dirichlet_nodes): iterates, residuals and results are zero on the constrained dofs, so the pair scale_K / scale_M of
 * the modified matrices does not appear.
 *
 * Block vectors are column-major: column j is a contiguous n-vector at base + j ld, ld >= n, n = s N < 2^31.  Two kernels of the block
 * layer are reachable on their own:
 *   fh_block_gram_dev     G = S^T T, S n x p and T n x q on the device, 1 <= p, q <= 96, G p x q row-major on the host.  At most 1024
 *                         workgroups own one contiguous row range each and leave a partial tile; the partials are summed in workgroup order
 *                         (no floating-point atomics): the result repeats bit for bit and does not depend on the rows between n and ld.
 *   fh_block_combine_dev  Y = S C (accumulate != 0: Y += S C), C p x q row-major on the host, Y n x q on the device; Y may not overlap S;
 *                         rows >= n of Y are not touched.
 * Both: FH_BAD_ARGUMENT for a null pointer, p or q of 0 or above 96, ld < n, n >= 2^31; n == 0 is FH_OK (G zero).
 *
 * fh_dense_generalized_eigh: A c = w B c for symmetric A and symmetric positive definite B (p x p row-major, 1 <= p <= 96) on the host, by
 * Cholesky of B and cyclic Jacobi on L^-1 A L^-T: w ascending, the columns of C the vectors with C^T B C = I.  Needs no context and no
 * GPU.  FH_BAD_ARGUMENT: null pointer, p of 0 or above 96; FH_EIG_BREAKDOWN: a pivot of B is not positive, or an entry is not finite.
 *
 * fh_eigs_lowest(_dev): Knyazev's LOBPCG on the basis [X W P] for the lowest m pairs, 1 <= m <= FH_EIG_MAX_BLOCK.
 *   - W = B R on the columns that have not converged, R = K X - theta M X, B the preconditioner of shift M + T(u): FH_PRECOND_IDENTITY,
 *     FH_PRECOND_JACOBI (the inverse of fh_shifted_tangent_diagonal_dev(shift, 1)) or FH_PRECOND_MULTIGRID (one V-cycle of the attached
 *     hierarchy per column).  W is M-orthogonalised against X, then W and P are M-orthonormalised by Cholesky of their Gram matrices.
 *   - K X, M X, K P, M P follow by recombination; only W goes through the maps (two applications per active column and iteration).
 *   - Rayleigh-Ritz on [X W P] with both Gram matrices formed in full (fh_dense_generalized_eigh); the new X and the new P come from one
 *     read of the basis.
 *   - criterion per column: ||r_i||_2 <= tol (|theta_i| + shift) ||M x_i||_2.  A column that meets it leaves the active set (soft locking:
 *     no W or P for it, but it stays in X for the Rayleigh-Ritz step).  On a free body pass shift > 0 of the order of the first elastic
 *     eigenvalue: the rigid modes (theta ~ 0) are then a reachable target and the preconditioner's matrix is definite.
 *   - a Cholesky or Rayleigh-Ritz breakdown restarts the iteration once without P; a second one returns FH_EIG_BREAKDOWN.
 *   - once every column meets the criterion, K X and M X are applied afresh and one Rayleigh-Ritz step on X alone makes X M-orthonormal and
 *     theta ascending; the criterion is tested again on these residuals (and the iteration goes on if a column misses it).  The same step
 *     opens the solve, so a guess that already meets the criterion returns after 0 iterations.
 * use_guess == 0: X is filled by the library, X(dof, j) = (splitmix64((j << 32) | dof) >> 11) 2^-52 - 1 in [-1, 1) with
 *   splitmix64(z): z += 0x9e3779b97f4a7c15; z = (z ^ z >> 30) 0xbf58476d1ce4e5b9; z = (z ^ z >> 27) 0x94d049bb133111eb; z ^ z >> 31,
 * so a solve needs no input and repeats.  use_guess != 0: the m columns in X are the start block (their Dirichlet entries are zeroed).
 * X: n x m, ld = n (device for _dev); theta: m on the host; residual_norms (host, m, may be null): ||r_i||_2 of the returned pairs;
 * stats (may be null): [0] iterations, [1] map applications, [2] preconditioner applications, [3] restarts.
 * Errors: FH_EIG_MAX_ITERATIONS when max_iter (0: no limit) is exhausted and FH_EIG_BREAKDOWN -- in both cases the pairs reached so far are
 * handed back (X M-orthonormal, theta its Rayleigh quotients); FH_INVALID_STATE without a density or for FH_PRECOND_MULTIGRID without a
 * hierarchy; FH_UNSUPPORTED for the mass operators and FH_TENSOR; FH_BAD_ARGUMENT for a null X or theta, m of 0, above FH_EIG_MAX_BLOCK or
 * above a third of the free dofs, shift < 0 or not finite, tol not finite, an unknown preconditioner; FH_SINGULAR_JACOBIAN from the maps.
 * No floating-point atomics anywhere: a solve repeats bit for bit, and the host and device entry points return the same bits.  The host
 * waits for the device once per Gram matrix (the small dense problem lives on the host).  Device memory: 17 n m doubles.
 * With FENRIS_HIP_EIGS_PROFILE set when the context was created, the solver waits for the device after every phase and fh_eigs_profile
 * returns the seconds of the last solve: [0] map applications, [1] preconditioning, [2] Gram matrices, [3] recombinations, [4] residuals,
 * [5] dense host work, [6] other, [7] the whole solve (without the variable only [7] is filled). */
enum { FH_EIG_MAX_BLOCK = 32 };
int fh_block_gram_dev(fh_ctx*, uint64_t n, uint32_t p, const double* S_dev, uint64_t lds, uint32_t q, const double* T_dev, uint64_t ldt,
                      double* G);
int fh_block_combine_dev(fh_ctx*, uint64_t n, uint32_t p, const double* S_dev, uint64_t lds, uint32_t q, const double* C, double* Y_dev,
                         uint64_t ldy, int accumulate);
int fh_dense_generalized_eigh(uint32_t p, const double* A, const double* B, double* w, double* C);
int fh_eigs_lowest_dev(fh_ctx*, uint32_t m, double shift, int preconditioner, double tol, uint64_t max_iter, int use_guess, double* X_dev,
                       double* theta, double* residual_norms, uint64_t* stats);
int fh_eigs_lowest(fh_ctx*, uint32_t m, double shift, int preconditioner, double tol, uint64_t max_iter, int use_guess, double* X, double* theta,
                   double* residual_norms, uint64_t* stats);
int fh_eigs_profile(fh_ctx*, double* seconds);
/* ---- time integration on the device:  M a + r(u) = lf_n f  with r the context's residual (FH_LAPLACE, FH_LINEAR_ELASTIC, FH_NEO_HOOKEAN,
 * FH_STVK, FH_STABLE_NEO_HOOKEAN; mass operators and FH_TENSOR: FH_UNSUPPORTED), M the mass of fh_set_mass_density (none: FH_INVALID_STATE) and
 * lf_n = load_factor[min(n, count - 1)] (null: 1), n the global index of the step being computed (the state of fh_dynamics_set_state is
 * step 0).  The Dirichlet nodes of fh_set_operator_dirichlet_nodes are held at the u of fh_dynamics_set_state with v = a = 0; those entries
 * of u come back bit for bit.  The handle uses the context's u as u_n: fh_set_u* holds the last state afterwards, as after fh_newton_solve.
 *
 * FH_DYN_CENTRAL_DIFFERENCE, in velocity-Verlet form with the row-sum lumped mass m = M 1 (no Dirichlet rows take part in forming it):
 *     a_0 = (lf_0 f - r(u_0)) / m;   v_h = v_n + dt/2 a_n;   u_{n+1} = u_n + dt v_h;   a_{n+1} = (lf_{n+1} f - r(u_{n+1})) / m;
 *     v_{n+1} = v_h + dt/2 a_{n+1}.
 *   An entry of m on a free dof that is not positive (decided from its value: the vertex rows of Tet10 and Tri6, for example) gives
 *   FH_UNSUPPORTED from fh_dynamics_step and fh_dynamics_stable_dt; the message names the dof.  On Hex8, Tet4, Quad4 and Tri3 without a
 *   rule-set table a step is the residual's element pass over the tiles and ONE node pass that sums the node's partials and does the whole
 *   state update -- acceleration, second kick, and either the stores of a record or the next step's first kick and drift into the context's
 *   u; lf is read from a device array indexed by the step.  Between records the loop only enqueues kernels: the kernels' status word and
 *   the kinetic energy are read at records and at the end of the call, where FH_SINGULAR_JACOBIAN is reported.  A step that is recorded
 *   stores v, a and the energy partials and the following step opens with a kick-and-drift launch of its own (the record reads u_{n+1});
 *   kick, drift and acceleration are one device function each with explicit fma, so a run gives the same bits however it is cut into calls
 *   and records.  On every other route (Hex27, Quad9, the quadratic simplices, rule-set tables) the residual is summed first (element
 *   vectors, ordered node sums; the host waits once per step there) and k_dynamics_update does the same arithmetic.
 * FH_DYN_NEWMARK(newmark_beta, newmark_gamma) and FH_DYN_BACKWARD_EULER: each step is one Newton solve as fh_newton_solve_dev runs it, with
 *     alpha = 1, beta = newmark_beta dt^2 (backward Euler: dt^2), the load lf_{n+1} f,
 *     u_ref = u_n + dt v_n + dt^2 (1/2 - newmark_beta) a_n (backward Euler: u_n + dt v_n), the guess u_ref with the Dirichlet entries of u_n;
 *     Newmark: a_{n+1} = (u_{n+1} - u_ref) / (newmark_beta dt^2), v_{n+1} = v_n + dt ((1 - gamma) a_n + gamma a_{n+1});
 *     backward Euler: v_{n+1} = (u_{n+1} - u_n) / dt (a_{n+1} = (v_{n+1} - v_n) / dt is kept for fh_dynamics_state only).
 *   Newmark's a_0 solves M a_0 = lf_0 f - r(u_0) on the free dofs by fh_cg_solve_shifted_tangent_dev(1, 0, ...) at linear_rel_tol (Jacobi
 *   where the settings ask for the hierarchy).  A Newton failure ends the call with that Newton code (FH_NEWTON_*); *steps_done counts the
 *   steps completed before it and the state is that of the last completed step.
 * fh_dynamics_create: FH_BAD_ARGUMENT for an unknown scheme, dt <= 0, newmark_beta <= 0, settings that are not finite, an unknown line
 *   search or preconditioner; the context must have its mesh, operator, table and density.  fh_set_mesh* on the context invalidates the
 *   handle (every later call: FH_INVALID_STATE); destroy the handle before the context.  Vertices, operator data, table, element mask,
 *   density and Dirichlet nodes may change between calls: m, a_n and the caches are formed again, keyed on the context's generation counters
 *   (so is a_n after fh_set_u* or fh_dynamics_set_load).
 * fh_dynamics_set_state: u and v (S N doubles each, null: zero); the step counter and the time return to 0.
 * fh_dynamics_set_load: f (S N doubles, null: no load) and load_factor (host, count >= 1 entries, null: 1).
 * fh_dynamics_step: num_steps steps.  A record is taken after every record_every steps of the call and after its last step (record_every
 *   == 0: the last step only); records (host, may be null) receives one row of 4 per record: [0] the kinetic energy 1/2 v^T M v (lumped m
 *   for central differences, the consistent M for the implicit schemes), [1] the stored energy (fh_assemble_scalar at u), [2] lf f . u,
 *   [3] the time.  Every sum is ordered: no floating-point atomics, a run repeats bit for bit.  A kinetic or stored energy that is not
 *   finite (a NeoHookean point with det F <= 0 makes it so) returns FH_DYNAMICS_NONFINITE; for central differences *steps_done is then the
 *   last clean record of the call (as for FH_SINGULAR_JACOBIAN) and the state is not to be used.  A state whose residual is not finite when
 *   a_n has to be formed (the first call after fh_dynamics_set_state) returns the same code with *steps_done == 0, under every scheme.
 *   stats (may be null): [0] steps done in this call, [1] residual evaluations, [2] Newton iterations summed, [3] PCG iterations summed,
 *   [4] records written.
 * fh_dynamics_state: u, v, a (S N each, any may be null), the time and the step count; a is a_n of the state as it stands (a_0 before the
 *   first step: it is formed here when asked for, with the errors of fh_dynamics_step).  The _dev forms take device arrays for u, v, a, f.
 * fh_dynamics_stable_dt: `iterations` steps of the power iteration x <- m^-1 T(u) x on the free dofs from column 0 of fh_eigs_lowest's
 *   fill (X(dof, 0)), the iterates normalised in the m-norm; omega_max^2 is the last Rayleigh quotient, dt_crit = 2 / omega_max.  A Rayleigh
 *   quotient never exceeds the largest eigenvalue, so dt_crit errs on the LARGE side: apply a safety factor (0.9 or less) before stepping. */
typedef struct fh_dynamics fh_dynamics;
enum { FH_DYN_CENTRAL_DIFFERENCE = 0, FH_DYN_BACKWARD_EULER = 1, FH_DYN_NEWMARK = 2 };
typedef struct {
    int scheme;
    double dt;
    double newmark_beta, newmark_gamma;   /* FH_DYN_NEWMARK only */
    /* the implicit schemes: fh_newton_solve's arguments */
    double newton_tolerance;
    uint64_t newton_max_iterations;
    int line_search;
    int preconditioner;
    double linear_rel_tol;
    uint64_t linear_max_iter;
} fh_dynamics_settings;
int fh_dynamics_create(fh_ctx*, const fh_dynamics_settings* settings, fh_dynamics** out);
void fh_dynamics_destroy(fh_dynamics*);
int fh_dynamics_set_state(fh_dynamics*, const double* u, const double* v);
int fh_dynamics_set_state_dev(fh_dynamics*, const double* u_dev, const double* v_dev);
int fh_dynamics_set_load(fh_dynamics*, const double* f, const double* load_factor, uint64_t count);
int fh_dynamics_set_load_dev(fh_dynamics*, const double* f_dev, const double* load_factor, uint64_t count);
int fh_dynamics_step(fh_dynamics*, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* steps_done, uint64_t* stats);
int fh_dynamics_state(fh_dynamics*, double* u, double* v, double* a, double* time, uint64_t* step);
int fh_dynamics_state_dev(fh_dynamics*, double* u_dev, double* v_dev, double* a_dev, double* time, uint64_t* step);
int fh_dynamics_stable_dt(fh_dynamics*, uint32_t iterations, double* omega_max, double* dt_crit);
/* ---- Rayleigh damping of the second-order problem:  M a + C(u) v + r(u) = lf_n f  with  C(u) = eta_mass M + eta_stiffness T(u),  T(u) the
 * element tangent of the context's operator at the current state (FH_LAPLACE, FH_LINEAR_ELASTIC: the constant operator A).  The obstacle
 * term of fh_set_obstacles stays out of C; the contact force joins r as without damping.  The default is (0, 0), and with (0, 0), set or
 * not, every launch and every bit is that of the undamped step.
 *
 * FH_DYN_CENTRAL_DIFFERENCE, with F(u, w) = lf f - r(u) - eta_stiffness T(u) w and the lumped mass m:
 *     a_0 = F(u_0, v_0) / m - eta_mass v_0;   v_h = v_n + dt/2 a_n;   u_{n+1} = u_n + dt v_h;
 *     a_{n+1} = (F(u_{n+1}, v_h) / m - eta_mass v_h) / (1 + eta_mass dt/2);   v_{n+1} = v_h + dt/2 a_{n+1}.
 *   The stiffness part takes the half-step velocity, which keeps the step explicit; the mass part is implicit in v_{n+1}.  On the tiles a
 *   step with eta_stiffness > 0 is ONE element pass that gathers v beside u and leaves the partials of r(u) + eta_stiffness T(u) v_h
 *   (k_damped_pass_tiled: for the linear operators the residual's body on u + eta_stiffness v_h) and the same one node pass; with
 *   eta_stiffness == 0 the residual's element pass runs unchanged and only the node arithmetic differs.  On every other route
 *   eta_stiffness T(u) v_h, summed like the residual, is added to it before k_dynamics_update.
 *   fh_dynamics_stable_dt then returns dt_crit = (2 / omega_max)(sqrt(1 + xi^2) - xi), xi = eta_stiffness omega_max / 2 (the limit
 *   (omega dt)^2 + 2 eta_stiffness omega^2 dt <= 4 of the highest mode; eta_mass does not enter); omega_max as without damping.
 * FH_DYN_NEWMARK and FH_DYN_BACKWARD_EULER: C is frozen at the start of the step and folded into the Newton solve's four arguments.  With
 *   b = newmark_beta dt^2, g = newmark_gamma (backward Euler: b = dt^2, g = 1), v_p = v_n + dt (1 - g) a_n (backward Euler: v_n):
 *     alpha = 1 + eta_mass g dt;   u_ref* = u_ref - eta_mass b v_p / alpha;   beta' = b + eta_stiffness g dt;
 *     f' = (b lf_{n+1} f - eta_stiffness A (b v_p - g dt u_ref)) / beta'
 *   (for backward Euler these are u_ref* = (u_ref + eta_mass dt u_n) / alpha and f' = (dt^2 lf f + eta_stiffness dt A u_n) / beta'): one
 *   application of A per step, and only when eta_stiffness > 0.  a_{n+1} and v_{n+1} are recovered from the unmodified u_ref, and Newmark's
 *   a_0 solves M a_0 = lf_0 f - r(u_0) - C v_0.
 *   OUT OF SCOPE: eta_stiffness > 0 under these two schemes with FH_NEO_HOOKEAN, FH_STVK or FH_STABLE_NEO_HOOKEAN (the frozen T(u_n) differs
 *   from T(u): a second tangent state would have to enter the Newton residual and every CG product), and with obstacles set (the folded
 *   beta' would scale the contact force too): fh_dynamics_step and fh_dynamics_state (when a is asked for) return FH_UNSUPPORTED and leave
 *   the state as it is.  eta_mass works with every operator under every scheme.  The records keep their four columns (no dissipated work).
 * fh_dynamics_set_damping: FH_BAD_ARGUMENT for a coefficient that is negative or not finite, and for a handle of fh_first_order_create (a
 *   first-order problem has no velocity).  Changing the coefficients invalidates a_n, as fh_dynamics_set_load does.
 * fh_dynamics_damping: the coefficients in use (either pointer may be null). */
int fh_dynamics_set_damping(fh_dynamics*, double eta_mass, double eta_stiffness);
int fh_dynamics_damping(fh_dynamics*, double* eta_mass, double* eta_stiffness);
/* ---- the first-order problem on the same handle:  M du/dt + r(u) = lf_n f  (the heat equation for FH_LAPLACE; the gradient flow of the
 * stored energy for the elastic operators), Dirichlet nodes held.  fh_first_order_create makes an fh_dynamics handle on which every
 * fh_dynamics_* call works as described above, with these differences.  The state is u alone (the context's u) and the step counter:
 * fh_dynamics_set_state with a non-null v is FH_BAD_ARGUMENT.
 *
 * FH_FO_RKL(stages = s): a Runge-Kutta-Legendre super-step of s stages with the row-sum lumped mass m = M 1, formed and checked as for
 * central differences (FH_UNSUPPORTED names the dof).  With L(y) = (lf_n f - r(y)) / m, w1 = 2 / (s^2 + s), mu_j = (2j - 1) / j and
 * nu_j = (1 - j) / j (formed on the host in double; every stage of step n uses lf_n, the factor at the step's start):
 *     Y_0 = u_n;   Y_1 = fma(w1 dt, L(Y_0), Y_0);   Y_j = mu_j Y_{j-1} + nu_j Y_{j-2} + mu_j w1 dt L(Y_{j-1}), j = 2..s;   u_{n+1} = Y_s.
 *   Per free dof one device function does a stage (Dirichlet dofs are not touched):
 *     w = fma(lf, f, -r) / m;   y = fma(mu_j w1 dt, w, fma(mu_j, u, nu_j * prev))   (stage 1: y = fma(w1 dt, w, u));   prev = u;   u = y
 *   so s = 1 is forward Euler to the bit.  On an eigenmode of (K, diag m) with eigenvalue lambda a step multiplies by the Legendre
 *   polynomial P_s(1 - 2 lambda dt / (s^2 + s)): stable for dt <= (s^2 + s) / lambda_max, at the cost of s residual passes.  On Hex8, Tet4,
 *   Quad4 and Tri3 without a rule-set table a stage is the residual's element pass over the tiles and ONE node pass
 *   (k_first_order_from_partials); the last stage of a recorded step leaves the partials of the record in the same launch.  The loop only
 *   enqueues between records; the kernels' status word is read at records and at the end of the call.  Every other route sums the residual
 *   first and k_first_order_update does the same arithmetic.
 * FH_FO_THETA(theta), 0.5 <= theta <= 1 (1/2: Crank-Nicolson; 1: implicit Euler), with the consistent mass: each step is one Newton solve as
 *   fh_newton_solve_dev runs it, with alpha = 1, beta = theta dt, u_ref = u_n, the guess u_n and the load
 *     g = (lf_{n+1} + c lf_n) f - c r(u_n),  c = (1 - theta) / theta   (theta = 1 evaluates no r(u_n)),
 *   which is M (u_{n+1} - u_n) + dt [theta (r(u_{n+1}) - lf_{n+1} f) + (1 - theta) (r(u_n) - lf_n f)] = 0.  A Newton failure restores u_n and
 *   returns the Newton code, as backward Euler does.
 * fh_first_order_create: FH_BAD_ARGUMENT for an unknown scheme, dt <= 0, stages == 0 (FH_FO_RKL), theta outside [0.5, 1] (FH_FO_THETA),
 *   settings that are not finite, and for FH_FO_THETA an unknown line search or preconditioner; everything else as fh_dynamics_create.
 * fh_dynamics_step: records keep their layout and cadence; [0] is 1/2 u^T B u over all dofs, B = diag m for FH_FO_RKL and the consistent M
 *   for FH_FO_THETA, [1] the stored energy, [2] lf f . u, [3] the time.  [0] or [1] not finite: FH_DYNAMICS_NONFINITE (FH_FO_RKL:
 *   *steps_done is the last clean record).  The first call after fh_dynamics_set_state forms lf_0 f - r(u_0) once; if that is not finite
 *   the call returns FH_DYNAMICS_NONFINITE with *steps_done == 0.  stats: residual evaluations are s per FH_FO_RKL step plus that one per
 *   state; for FH_FO_THETA Newton's, plus one per step when theta < 1, plus that one per state.
 * fh_dynamics_state: v receives the rate du/dt of the state as it stands -- FH_FO_RKL: L(u_n); FH_FO_THETA: M w = lf_n f - r(u_n) on the
 *   free dofs, by the CG that forms Newmark's a_0 -- formed when asked for and kept until the state, the load or the context changes; zero
 *   on the Dirichlet dofs.  a receives zeros.
 * fh_dynamics_stable_dt: the same power iteration and omega_max; dt_crit = (s^2 + s) / omega_max^2 for FH_FO_RKL, which errs on the LARGE
 *   side as above (apply a safety factor), and HUGE_VAL for FH_FO_THETA (unconditionally stable for theta >= 1/2). */
enum { FH_FO_RKL = 0, FH_FO_THETA = 1 };
typedef struct {
    int scheme;
    double dt;
    uint32_t stages;        /* FH_FO_RKL: s >= 1 (1 is forward Euler) */
    double theta;           /* FH_FO_THETA: 0.5 <= theta <= 1 */
    /* FH_FO_THETA: fh_newton_solve's arguments, as in fh_dynamics_settings */
    double newton_tolerance;
    uint64_t newton_max_iterations;
    int line_search;
    int preconditioner;
    double linear_rel_tol;
    uint64_t linear_max_iter;
} fh_first_order_settings;
int fh_first_order_create(fh_ctx*, const fh_first_order_settings* settings, fh_dynamics** out);

/* ---- penalty contact with rigid obstacles (engine_contact.hip; the arithmetic: contact_kernels.hpp); fixed unless given a path below --
 * Obstacle o has a signed distance phi_o(x), positive where the body may be, and a stiffness k_o > 0.  With x_i = X_i + u_i the current
 * position of node i, w_i >= 0 a node weight (default 1) and p = min(0, phi_o(x_i)):
 *   energy   E_c(u) = sum_o sum_i (k_o w_i / 2) p^2
 *   force    g_i    = sum_o k_o w_i p grad phi_o(x_i)                                        (added to the residual r(u))
 *   tangent  B_i    = sum_o k_o w_i ([phi_o < 0] n n^T + c (I - n n^T)),  n = grad phi_o     (a block on the diagonal, per node)
 * FH_OBSTACLE_HALF_SPACE: phi = (x - point) . normal (normalised here), c = 0.  FH_OBSTACLE_BALL (the body stays outside): phi = |y| - radius,
 * y = x - point, n = y / |y|, c = 0: the curvature term p Hess phi is negative semi-definite and is dropped, so B_i is a Gauss-Newton
 * tangent there.  FH_OBSTACLE_CAVITY (the body stays inside): phi = radius - |y|, n = -y / |y|, c = -p / |y| >= 0: B_i is the exact
 * derivative of g_i.  B_i is symmetric positive semi-definite for every kind.  A node with phi == 0 is inactive (the test is phi < 0); a
 * node at y == 0 of a ball or a cavity gets no force and no block from it but counts in E_c.
 * fh_set_obstacles: count == 0 (or a null list) clears them; node_weights: num_nodes doubles or NULL.  FH_BAD_ARGUMENT: count above
 *   FH_MAX_OBSTACLES, an unknown kind, a value that is not finite, a zero normal, stiffness <= 0, radius <= 0 (ball, cavity), a negative
 *   weight; FH_INVALID_STATE: no mesh.  fh_set_mesh* clears the obstacles.
 * While obstacles are set, the term is part of: fh_apply_tangent_dev, fh_tangent_diagonal_dev, fh_cg_solve_tangent(_dev) and the shifted
 *   family (alpha M + beta (T(u) + B(u)), the scale of the Dirichlet rows from the diagonal with B), fh_newton_solve(_dev)
 *   (F = alpha M (u - u_ref) + beta (r + g - f)), every scheme of fh_dynamics_* and fh_first_order_* (E_c is added to the stored-energy
 *   column of the records), fh_dynamics_stable_dt and fh_eigs_lowest(_dev).  These need the solution dim to equal the geometric dim:
 *   FH_LAPLACE answers FH_UNSUPPORTED.  FH_PRECOND_MULTIGRID and fh_mg_apply_dev with obstacles set: FH_UNSUPPORTED (the coarse levels
 *   would not see the term).
 *   Not part of: fh_apply_operator_dev, fh_operator_diagonal_dev, fh_cg_solve_matrix_free, every fh_assemble_*, fh_recover*.
 *   Without obstacles all of them compute what they computed before, bit for bit.
 * The stand-alone terms at the context's u (none set: u = 0), over every node (Dirichlet nodes included), for users of the assembled path:
 *   fh_contact_energy; fh_contact_force_dev ADDS g into out_dev (S N doubles); fh_contact_gap_dev writes min_o phi_o(x_i) per node (N
 *   doubles; without obstacles +infinity); fh_add_contact_tangent_csr_dev ADDS B_i into the diagonal node blocks of the fh_pattern CSR
 *   values (FH_INVALID_STATE without a pattern).
 * FH_OBSTACLE_GRID: a rigid obstacle of any shape, as a signed distance sampled on a regular grid (fh_sdf_grid_create below) and
 *   interpolated on the device.  `grid` is the id of a live grid whose dim is the mesh's geometric dim (else FH_BAD_ARGUMENT), `point` the
 *   position of sample (0, 0, 0) -- one grid may stand in several places, and a path moves it like any obstacle --, `stiffness` as ever;
 *   `normal` and `radius` are not read.  With h the spacings, cnt the sample counts and t_a = (x_a - point_a) / h_a, a node is INSIDE the
 *   box iff 0 <= t_a <= cnt_a - 1 on every axis (a NaN is outside); i_a = min(floor(t_a), cnt_a - 2), f_a = t_a - i_a; phi is the bi- /
 *   trilinear interpolant of the 4 / 8 corner samples of cell i at f and m = grad phi (1 / h_a per axis included, NOT a unit vector).  With
 *   gn = |m|:  E = (k w / 2) p^2,  g = k w p m,  B = k w [phi < 0] m m^T  (Gauss-Newton: p Hess phi has a zero diagonal, is indefinite and
 *   is dropped, c = 0),  and in friction nbar = m / gn, lam = k w max(0, -phi) gn at the lag position, so |q| <= mu times the actual normal
 *   force.  A flat spot (gn == 0) counts in E_c and gives nothing else.  OUTSIDE the box the obstacle does not exist for that node: no
 *   energy, no force, no block, no friction, and fh_contact_gap_dev takes +infinity from it.  THE BOX MUST COVER EVERY PLACE A NODE CAN BE
 *   WHILE phi < 0: a node that leaves the box while in contact loses the term abruptly.  The gradient is continuous inside a cell and has a
 *   kink across cell faces. */
enum { FH_OBSTACLE_HALF_SPACE = 0, FH_OBSTACLE_BALL = 1, FH_OBSTACLE_CAVITY = 2, FH_OBSTACLE_GRID = 3 };
#define FH_MAX_OBSTACLES 16
typedef struct {
    int kind;
    int grid;               /* FH_OBSTACLE_GRID: the id fh_sdf_grid_create gave; not read for the other kinds (the four bytes were padding) */
    double stiffness;
    double point[3];        /* a point of the plane, the centre, or the position of sample (0, 0, 0); 2-D: the first two entries */
    double normal[3];       /* FH_OBSTACLE_HALF_SPACE: points into the admissible side, any length > 0 */
    double radius;          /* FH_OBSTACLE_BALL, FH_OBSTACLE_CAVITY */
} fh_obstacle;
int fh_set_obstacles(fh_ctx*, const fh_obstacle* obstacles, uint64_t count, const double* node_weights);
int fh_contact_energy(fh_ctx*, double* energy);
int fh_contact_force_dev(fh_ctx*, double* out_dev);
int fh_contact_gap_dev(fh_ctx*, double* gap_dev);
int fh_add_contact_tangent_csr_dev(fh_ctx*, double* values_dev);
/* ---- sampled signed-distance grids: resources of the context, referred to by FH_OBSTACLE_GRID obstacles ----------------------------------
 * fh_sdf_grid_create: dim 2 or 3; n: the sample counts per axis (2-D: n[2] must be 1, spacing[2] is not read); values: host memory, x
 *   fastest -- sample (ix, iy, iz) at values[(iz n[1] + iy) n[0] + ix] --, copied to the device once.  *id is a slot number in
 *   [0, FH_MAX_SDF_GRIDS); a destroyed slot is reused.  FH_BAD_ARGUMENT: another dim, n[a] < 2 on an axis with extent, 2^31 samples or more,
 *   a spacing that is not finite and positive, a sample that is not finite, a null pointer; FH_UNSUPPORTED: every slot is taken.
 * Grids belong to the context: fh_set_mesh* and fh_set_obstacles leave them alone, fh_destroy frees them.  fh_sdf_grid_destroy:
 *   FH_BAD_ARGUMENT for an id that is not live, FH_INVALID_STATE while an obstacle that stands refers to the grid.
 * fh_sdf_grid_info: dim, n and spacing as given (any may be NULL).
 * fh_sdf_grid_sample_dev: the interpolant alone (k_sdf_grid_sample), with sample (0, 0, 0) at `origin` (dim entries read), at m points
 *   (points_dev: m x dim doubles) into phi_dev (m) and grad_dev (m x dim, may be NULL); a point outside gets +infinity and a zero gradient. */
#define FH_MAX_SDF_GRIDS 16
int fh_sdf_grid_create(fh_ctx*, uint32_t dim, const uint32_t n[3], const double spacing[3], const double* values, uint32_t* id);
int fh_sdf_grid_destroy(fh_ctx*, uint32_t id);
int fh_sdf_grid_info(fh_ctx*, uint32_t id, uint32_t* dim, uint32_t n[3], double spacing[3]);
int fh_sdf_grid_sample_dev(fh_ctx*, uint32_t id, const double origin[3], const double* points_dev, uint64_t m, double* phi_dev,
                           double* grad_dev);
/* ---- Coulomb friction on the obstacles, lagged and smoothed (Li et al., "Incremental Potential Contact", 2020, section 5) -------------
 * Obstacle o has a coefficient mu_o >= 0 (default 0); the context has a slip length eps > 0 and a lag displacement ubar (S N doubles on the
 * device, owned by the context; u = 0 until fh_set_friction_reference is called).  With xbar_i = X_i + ubar_i, constants of u:
 *   nbar = grad phi_o(xbar_i),   P = I - nbar nbar^T,   lam = k_o w_i max(0, -phi_o(xbar_i))
 * and with the slip s = P (u_i - ubar_i), y = |s|:
 *   potential  D(u) = sum_o sum_i mu_o lam f0(y),      f0 = -y^3 / (3 eps^2) + y^2 / eps + eps / 3  (y < eps),  y  otherwise
 *   force      q_i  = sum_o mu_o lam c1 s,             c1 = 2 / eps - y / eps^2  (y < eps),  1 / y  otherwise        (added to r(u) beside g)
 *   tangent    H_i  = sum_o mu_o lam (c1 P - c2 s s^T), c2 = 1 / (eps^2 y)  (0 < y < eps),  0  (y == 0),  1 / y^3  otherwise
 * q is the gradient of the convex D and H_i, a block on the diagonal per node beside B_i, its exact symmetric positive semi-definite
 * Hessian with ubar frozen; |q_i| <= mu_o lam, with equality for y >= eps.  A node out of contact at xbar, or at the centre of a ball or
 * cavity there, gets nothing from that obstacle.  2-D and 3-D, the elastic operators, as for the normal term.
 * fh_set_friction: one mu per obstacle set; count == 0 or a null list turns friction off.  FH_BAD_ARGUMENT: a mu that is negative or not
 *   finite, slip_length <= 0 or not finite, count != the number of obstacles; FH_INVALID_STATE: no obstacles.  fh_set_obstacles and
 *   fh_set_mesh* clear it.  With friction never set, or with every mu_o == 0, every route computes the bits it computed before.
 * fh_set_friction_reference(_dev): ubar (S N doubles; NULL: the context's current u).  FH_INVALID_STATE before fh_set_friction.
 * fh_friction_potential: D at the context's u; fh_friction_force_dev ADDS q into out_dev (S N doubles); fh_add_contact_tangent_csr_dev adds
 *   B_i + H_i while friction is set.
 * While friction is set the term travels with the normal term, in the same launches: fh_apply_tangent_dev, fh_tangent_diagonal_dev,
 *   fh_cg_solve_tangent(_dev) and the shifted family apply T(u) + B(u) + H(u); fh_newton_solve(_dev) solves
 *   F = alpha M (u - u_ref) + beta (r + g + q - f) with the context's ubar and eps as the caller set them (a quasi-static user moves ubar
 *   to the converged u between load steps).
 * FH_DYN_NEWMARK, FH_DYN_BACKWARD_EULER: at the start of step n the handle sets ubar = u_n (a device copy enqueued with the step) and
 *   eps = eps_v dt (fh_dynamics_set_slip_velocity; without one the context's slip length stays), then runs its one Newton solve; a_0 is
 *   formed with ubar = u_0, that is without friction force.  The context's ubar and eps are left as the last step set them.
 * FH_DYN_CENTRAL_DIFFERENCE: the term is evaluated with the current position as the lag state and the slip of the half-step velocity,
 *   s = P (dt v_h), eps = eps_v dt (a_0: v_0); no lag array is read or written, and q joins r before the acceleration is formed, as the
 *   stiffness damping does.  On a node of lumped mass m with friction rate c = 2 mu lam / (eps_v m) the step needs
 *   (omega dt)^2 + 2 c dt <= 4; fh_dynamics_stable_dt stays the frictionless figure.
 * Left out: fh_eigs_lowest(_dev), fh_dynamics_stable_dt and the operator's entry points (fh_apply_operator_dev, ...) leave the term out;
 *   fh_first_order_* handles answer FH_UNSUPPORTED from fh_dynamics_step and fh_dynamics_state while any mu_o > 0 (a gradient flow has no
 *   slip velocity); FH_PRECOND_MULTIGRID stays FH_UNSUPPORTED with obstacles.  The records keep four columns: the dissipated work is not
 *   recorded.
 * fh_dynamics_set_slip_velocity: eps_v > 0 and finite, else FH_BAD_ARGUMENT; FH_BAD_ARGUMENT on a handle of fh_first_order_create. */
int fh_set_friction(fh_ctx*, const double* mu, uint64_t count, double slip_length);
int fh_set_friction_reference(fh_ctx*, const double* ubar);
int fh_set_friction_reference_dev(fh_ctx*, const double* ubar_dev);
int fh_friction_potential(fh_ctx*, double* potential);
int fh_friction_force_dev(fh_ctx*, double* out_dev);
int fh_dynamics_set_slip_velocity(fh_dynamics*, double eps_v);
/* ---- moving obstacles: translation along piecewise-linear paths, and the force resultants per obstacle ---------------------------------
 * fh_set_obstacle_paths: obstacle o owns the knots knot_begin[o] .. knot_begin[o + 1] (knot_begin: count + 1 entries, non-decreasing from
 *   0; knot_time: one per knot, strictly increasing within an obstacle; knot_offset: 3 per knot, 2-D uses the first two).  Its offset d_o(t)
 *   is piecewise linear through them -- in a segment, with w = (t - t_k) / (t_{k+1} - t_k), d = fma(w, d_{k+1} - d_k, d_k) per component --
 *   constant before the first knot and after the last; an obstacle with no knots never moves.  The obstacle's point is point_o + d_o(t):
 *   translation only, a half-space keeps its normal.  d_o is evaluated on the host in double.  Three NULL arrays clear the paths.
 *   FH_BAD_ARGUMENT: knot times not strictly increasing, a value that is not finite, knot_begin not non-decreasing from 0;
 *   FH_INVALID_STATE: no obstacles.  fh_set_obstacles and fh_set_mesh* clear the paths and return the clock to (0, 0).
 * fh_set_obstacle_time: the contact clock.  The context keeps two offsets per obstacle, the current one d_o(t) and the lag one d_o(t_lag)
 *   (fh_obstacle_offsets reads them: count x 3 doubles each, either may be NULL; fh_obstacle_count gives the count of the obstacles that
 *   stand, 0 without any); both times are 0 until the first call.  FH_BAD_ARGUMENT:
 *   a time that is not finite; FH_INVALID_STATE: no obstacles.  The caches keyed on the obstacles are invalidated only when an offset
 *   changes bitwise.
 * The normal term (energy, force, tangent block, gap, diagonal, CSR blocks) is evaluated against the obstacle at its CURRENT position on
 *   every route: the same bits as obstacles placed at point_o + d_o(t) by fh_set_obstacles.
 * Friction, with c_o = d_o(t) - d_o(t_lag) the obstacle's own displacement over the lag interval: the solvers and the implicit integrators
 *   evaluate nbar, P and lam at xbar_i against the obstacle at its LAG position and take the slip relative to the obstacle,
 *   s = P (u_i - ubar_i - c_o); central differences keep the current configuration as the lag one and take s = P (dt v_i - c_o).  f0, c1, c2
 *   are unchanged and H_i stays the exact symmetric positive semi-definite Hessian of D with ubar and both offsets frozen.  A node that moves
 *   with the obstacle feels no friction force.  A quasi-static user of fh_newton_solve calls, between load steps,
 *   fh_set_friction_reference(NULL), then fh_set_obstacle_time(t_next, t_now), then solves.
 * fh_dynamics_create handles drive the clock themselves: every launch or solve that forms a residual for step n + 1 first sets the clock to
 *   (t_{n+1}, t_n) with t_n = (double)n dt as in the records' time column; a_0 uses (t_0, t_0); fh_dynamics_set_state returns the clock to
 *   (0, 0).  A central-difference launch carries its own offsets in its kernel arguments: nothing is waited for, no time lives on the device,
 *   no launch is added, and a run repeats bit for bit however it is cut into calls.  The context is left at the clock of the last step.
 *   fh_dynamics_stable_dt and fh_eigs_lowest take the obstacles where they stand.  fh_first_order_create handles answer FH_UNSUPPORTED from
 *   fh_dynamics_step and fh_dynamics_state while any obstacle has knots (the stage times of a super-step are not defined here).
 *   With no knots set every route computes the bits it computed before.
 * fh_contact_resultants: R_o = sum_i k_o w_i p n, obstacle o's share of g and with it the force the body exerts on the obstacle, into
 *   normal (count x 3 doubles), and Q_o = sum_i mu_o lam c1 s, its share of q, into friction (count x 3, may be NULL; zeros without
 *   friction); both at the context's u over every node, Dirichlet nodes included; the third components are 0 in 2-D.  One launch of
 *   k_contact_resultants (a fixed reduction tree per workgroup, one partial row each) and the ordered sum of the rows: no atomics, two calls
 *   return the same bits. */
int fh_set_obstacle_paths(fh_ctx*, const uint64_t* knot_begin, const double* knot_time, const double* knot_offset);
int fh_set_obstacle_time(fh_ctx*, double t, double t_lag);
int fh_obstacle_count(fh_ctx*, uint64_t* count);
int fh_obstacle_offsets(fh_ctx*, double* current, double* lag);
int fh_contact_resultants(fh_ctx*, double* normal, double* friction);
/* ---- augmented-Lagrangian contact: a multiplier per obstacle and node, updated between solves (Uzawa) --------------------------------------
 * The penalty term alone leaves a node pressed with force F a depth F / (k w) inside the obstacle.  A multiplier removes that error at a
 * fixed, moderate k.  It is kept as a LENGTH s_oi >= 0 per obstacle o and node i, standing for the force lam_oi = k_o w_i s_oi (no division
 * on the device; w_i = 0 is harmless); layout [o][i], count x N doubles, owned by the context.  With
 *   phi_eff = phi_o(x_i) - s_oi,  p = min(0, phi_eff)
 * every route that carries the term forms it from phi_eff where it formed it from phi:
 *   E_c = sum (k w / 2) (p^2 - s^2)     (active: k w / 2 phi^2 - lam phi; otherwise -lam^2 / (2 k w))
 *   g_i = sum k w p n,   B_i = sum k w ([phi_eff < 0] n n^T + c (I - n n^T)),  c = -p / |y| for the cavity; a grid: m m^T, c = 0
 *   friction: a node is in contact at xbar iff phi_eff(xbar) < 0, lam = k w max(0, -phi_eff(xbar)) (a grid: times gn), with the s_oi that
 *   stands NOW;  fh_contact_resultants: R_o and Q_o from the same p and lam.
 * g is the exact gradient of E_c with s frozen; B keeps its exact / Gauss-Newton status per kind and stays symmetric positive
 * semi-definite.  fh_contact_gap_dev keeps reporting the geometric min_o phi_o, not phi_eff.  With every s = 0 each expression is the one
 * without multipliers, bit for bit (phi - 0.0, e - 0.0); with none set the kernels are the ones without the shift.
 * fh_set_contact_multipliers(_dev): count x N doubles are copied into the context; NULL clears them.  FH_BAD_ARGUMENT: a negative or
 *   non-finite entry (host form only; the device form is not read here); FH_INVALID_STATE: no obstacles, no mesh.
 * fh_contact_multipliers(_dev): reads them back (count x N doubles), zeros while none are set.  FH_INVALID_STATE: no obstacles.
 * fh_contact_multiplier_forces_dev: lam_oi = k_o w_i s_oi into lam_dev (count x N doubles), for a grid times gn = |grad phi| at the node's
 *   current position (0 outside its box); zeros while none are set.
 * fh_contact_multiplier_update: s_oi <- max(0, s_oi - phi_o(x_i)) at the context's u and the contact clock's current time; phi = +infinity
 *   (outside a grid's box) gives 0; a node at the centre of a ball or cavity is updated like any other.  The first call starts from zeros.
 *   skip_nodes (skip_count host indices, may be NULL with 0: the fully held nodes) keep s = 0 and stay out of the statistics;
 *   FH_BAD_ARGUMENT: an index >= N.  stats (may be NULL), over the counted (node, obstacle) pairs: max_change = max |s_new - s_old| (|phi|
 *   where the pair is active afterwards, the released multiplier otherwise: the convergence measure), max_penetration = max max(0, -phi),
 *   active = the number with s_new > 0, max_force = max lam after the update.  One launch of k_contact_multiplier_update (one thread per
 *   node, a fixed reduction tree per workgroup, one partial row each) and the combination of the rows in index order: no atomics, two
 *   calls on equal input return equal bits.  Waits for the device.
 * Setting, clearing or updating invalidates every cache keyed on the obstacles.  fh_set_obstacles and fh_set_mesh* clear the multipliers;
 *   fh_set_obstacle_time, fh_set_obstacle_paths and fh_set_friction* leave them (a quasi-static indentation warm-starts from the last load
 *   step).  fh_newton_solve, the integrators, fh_dynamics_stable_dt and fh_eigs_lowest see them as a frozen field: no route updates them. */
typedef struct {
    double max_change;
    double max_penetration;
    double max_force;
    uint64_t active;
} fh_multiplier_update;
int fh_set_contact_multipliers(fh_ctx*, const double* s);
int fh_set_contact_multipliers_dev(fh_ctx*, const double* s_dev);
int fh_contact_multipliers(fh_ctx*, double* s);
int fh_contact_multipliers_dev(fh_ctx*, double* s_dev);
int fh_contact_multiplier_forces_dev(fh_ctx*, double* lam_dev);
int fh_contact_multiplier_update(fh_ctx*, const uint64_t* skip_nodes, uint64_t skip_count, fh_multiplier_update* stats);
/* ---- prescribed motion of the Dirichlet nodes during time integration (second-order handles) -------------------------------------------
 * fh_dynamics_set_boundary_motion(_dev): direction (S N doubles, read on the Dirichlet dofs only; NULL clears the motion) and a factor
 *   table of count >= 1 finite entries (host memory in both forms; else FH_BAD_ARGUMENT).  With g_n = factor[min(n, count - 1)], a Dirichlet
 *   dof holds u_n = fma(g_n - g_0, direction, u_0), u_0 the value fh_dynamics_set_state gave (the handle keeps a device copy from the first
 *   motion on, taken from the u that stands when no fh_dynamics_set_state follows; a motion set after another was cleared is measured
 *   from that same u_0, not from where the first one left the dofs).  g_n - g_0 is formed on the host: the entries are a pure
 *   function of n and come back bit for bit however a run is cut into calls.  Setting or clearing a motion invalidates a_n, as
 *   fh_dynamics_set_load does.  While a motion is set, v on the Dirichlet dofs is the handle's own and is no longer zeroed: at step 0 it is
 *   what fh_dynamics_set_state gave, and the CALLER matches it to the slope of the factor table, v_0 = ((g_1 - g_0) / dt) direction there.
 * FH_DYN_CENTRAL_DIFFERENCE: the drift from step n to n + 1 writes u_{n+1} as above and v = ((g_{n+1} - g_n) / dt) direction, the half-step
 *   velocity of the boundary, so stiffness damping and the friction slip see it move; a stored state keeps that v and has a = 0 there; the
 *   kinetic-energy column still counts the free dofs only.  No launch is added: the fused node pass and the stand-alone update share it.
 * FH_DYN_BACKWARD_EULER: a moved Dirichlet dof has the kinematics of a free one, u_ref = u_n + dt v_n, v_{n+1} = (u_{n+1} - u_n) / dt,
 *   a_{n+1} = (v_{n+1} - v_n) / dt; the prescribed u_{n+1} enters the Newton guess and Newton holds it; the consistent kinetic energy
 *   includes those dofs; a failed Newton solve restores u_n on them too.
 * FH_UNSUPPORTED from fh_dynamics_step and fh_dynamics_state: a motion under FH_DYN_NEWMARK (its kinematics on a prescribed displacement
 *   oscillate unless v_0 and a_0 match the path), under backward Euler together with Rayleigh damping, or on a first-order handle. */
int fh_dynamics_set_boundary_motion(fh_dynamics*, const double* direction, const double* factor, uint64_t count);
int fh_dynamics_set_boundary_motion_dev(fh_dynamics*, const double* direction_dev, const double* factor, uint64_t count);
/* Geometric multigrid for the matrix-free solvers (FH_PRECOND_MULTIGRID of fh_cg_solve_matrix_free, fh_cg_solve_tangent,
 * fh_cg_solve_shifted_tangent and fh_newton_solve; fh_cg_solve on assembled values takes identity, Jacobi or FH_PRECOND_AMG).  Every level is an
 * ordinary context with its own mesh, operator (Laplace, LinearElastic, NeoHookean or StVK), quadrature, data, density and
 * fh_set_operator_dirichlet_nodes, on the fine context's device; the hierarchy uses each level's matrix-free map and diagonal as they are.
 * coarse: num_coarse contexts, coarsest first.  Pair k maps coarse[k] to coarse[k + 1] (the fine context for the last pair):
 * transfer_offsets[k] (fine nodes + 1), transfer_indices[k], transfer_weights[k] are its CSR by fine node, 1 to 8 parents per row
 * (fh_refine_hex8_uniform writes it).  A row with one parent of weight 1 injects that coarse node: every coarse node needs exactly one,
 * and a coarse node is Dirichlet exactly when its injected fine node is; else FH_BAD_ARGUMENT.  A coarsest level of more than 4096 dofs
 * is FH_UNSUPPORTED.  The Dirichlet sets are read at creation.  The contexts must outlive the hierarchy's use; destroying the fine
 * context while the hierarchy is attached (or attaching another one) orphans it, and fh_mg_destroy then only frees it.
 * Each solve (and fh_mg_apply_dev) first injects the fine u into every NeoHookean / StVK level (a coarse LinearElastic context with the
 * same Lame data is the linearized coarse operator), then forms per level what changed since the last solve: the diagonal of
 * alpha M + beta T(u), lambda_max of D^-1 A (a fixed number of Jacobi-PCG / Lanczos steps from a fixed start vector), and on the
 * coarsest level the dense matrix of its map, probed through the map and factored on the host (not SPD: FH_CG_INDEFINITE_PRECONDITIONER).
 * The V-cycle: Chebyshev-Jacobi smoothing of degree m before and after the coarse correction, restriction P^T of the residual (fine
 * Dirichlet dofs excluded, coarse Dirichlet rows zero), the correction prolongated by P (fine Dirichlet dofs untouched), the dense
 * inverse on the coarsest level, and the Dirichlet rows of the result = r / scale.  Smoother, with lambda_hi = 1.1 lambda_max,
 * lambda_lo = lambda_max / range, theta = (hi + lo)/2, delta = (hi - lo)/2, r = b - A x, d = D^-1 r / theta, rho = delta / theta, for
 * k = 1..m:  x += d;  if k < m:  r -= A d,  rho' = 1 / (2 theta / delta - rho),  d = rho' rho d + (2 rho' / delta) D^-1 r,  rho = rho'.
 * Pre-smoothing starts from x = 0.  Every call runs on the fine context's stream (the coarse contexts' streams are pointed at it for the
 * duration of the call); no host synchronisation inside a V-cycle, no floating-point atomics: every solve repeats bit for bit.
 *
 * LIFETIME OF A HIERARCHY OR HANDLE MADE FOR A CONTEXT (fh_mg, fh_amg, fh_dynamics): it is sized for the mesh the context
 * held at its creation and is invalidated by fh_set_mesh*, fh_set_mesh_from_* and fh_set_connectivity_ragged on that context -- for an
 * fh_mg on ANY of its levels' contexts -- and by an operator of another solution dim.  An fh_amg also holds the context's pattern arrays:
 * the fh_pattern that builds a pattern again (after a new mesh; a repeated fh_pattern on an unchanged context builds nothing and keeps
 * the hierarchy valid) invalidates it.  Every entry that uses an invalidated hierarchy or handle -- the FH_PRECOND_MULTIGRID solves,
 * fh_newton_solve, the integrators and fh_eigs_lowest with it, fh_mg_apply_dev; fh_cg_solve* with FH_PRECOND_AMG, fh_amg_apply_dev,
 * fh_amg_update_values, fh_amg_set_smoother, fh_amg_level_matrix of level 0 -- returns FH_INVALID_STATE with a message that names the
 * creating call (and, for fh_mg, the level) and touches no device memory.  The only valid uses left are fh_*_destroy and detaching
 * (fh_set_multigrid / fh_set_amg with NULL or another hierarchy); make a new one for the new mesh.  The same holds for the FH_TENSOR
 * coefficients of fh_set_operator_tensor: they go with the mesh, and every assembler answers FH_INVALID_STATE until they are sent again. */
int fh_mg_create(fh_ctx* fine, uint64_t num_coarse, fh_ctx* const* coarse, const uint64_t* const* transfer_offsets,
                 const uint64_t* const* transfer_indices, const double* const* transfer_weights, fh_mg** out);
void fh_mg_destroy(fh_mg*);
/* attach (or with NULL detach) the hierarchy the fine context's FH_PRECOND_MULTIGRID solves use */
int fh_set_multigrid(fh_ctx* fine, fh_mg* mg);
/* degree m (default 3), range (default 15) and Lanczos steps of the eigenvalue estimate (default 10) */
int fh_mg_set_smoother(fh_mg*, uint32_t degree, double range, uint32_t eig_steps);
/* level 0 is the coarsest, num_coarse the fine one: lambda_max of its last setup (0 before one, and on the coarsest) and its dofs */
int fh_mg_level_info(fh_mg*, uint32_t level, double* lambda_max, uint64_t* num_dofs);
/* one V-cycle z = B r on alpha M + beta T(u) (the plain map: alpha = 0, beta = 1) after the setup of a solve; r, z on the device */
int fh_mg_apply_dev(fh_mg*, double alpha, double beta, const double* r_dev, double* z_dev);
/* Smoothed-aggregation algebraic multigrid for PCG on the assembled matrix (FH_PRECOND_AMG of fh_cg_solve and fh_cg_solve_dev only; the
 * matrix-free solves and fh_newton_solve reject it).  AMG-PCG assumes an SPD matrix (no FH_TENSOR operators).  The hierarchy is built from
 * the context's pattern and values_dev, its node-block CSR values (after fh_apply_dirichlet_csr_dev or not), on the context's stream:
 *   strength: i != j strong when ||A_ij||_F >= theta sqrt(||A_ii||_F ||A_jj||_F) and A_ij != 0 (theta = 0: the pattern's node graph); a node
 *     without a nonzero off-diagonal block is isolated: no aggregate, a zero row of P, and z_i = A_ii^-1 r_i in the V-cycle (Cholesky of
 *     the block; a pivot at most 1e-14 of its diagonal leaves that dof out);
 *   aggregates: roots form a distance-2 maximal independent set of the strength graph, built in synchronous rounds with the priority
 *     ((h(i) & 0x7fffffff) << 32) | i, with the 32-bit hash h(x): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15,
 *     x *= 0x846ca68b, x ^= x >> 16 (unsigned arithmetic); every node next to a root joins the adjacent root of highest
 *     priority, then each node still left joins the aggregate of its aggregated strong neighbour of highest priority.  The aggregates
 *     depend on the matrix alone;
 *   near-nullspace B (s N x nb, row-major): FH_AMG_CONSTANT (nb = s unit translations), FH_AMG_RIGID_BODY (s = d: translations and rotations
 *     about the centroid of the context's vertices, nb = 3 in 2D, 6 in 3D) or FH_AMG_USER (B, nb columns, 1 <= nb <= 6);
 *   T: per aggregate, modified Gram-Schmidt of its rows of B, columns in order; a column whose norm after orthogonalisation is at most
 *     1e-10 of its norm before is zero in Q and its row of R is zero.  Q's rows form T, R the aggregate's rows of the coarse B;
 *   P = (I - omega D^-1 A) T, omega = 4 / (3 lambda), D the point diagonal, lambda the Lanczos estimate of lambda_max(D^-1 A) (as fh_mg_*);
 *   A_c = P^T (A P) with P^T stored explicitly; block (J, I) of A_c is the transpose of block (I, J) bit for bit.  Coarse dofs with a zero
 *     diagonal have D^-1 = 0 and no correction.
 * Levels are coarsened until one has at most 4096 dofs or max_levels levels exist (0: 10); a coarsest level above 4096 dofs, or a step that
 * keeps more than 90 % of the dofs, is FH_UNSUPPORTED.  The coarsest level is inverted densely (Cholesky on the host; a pivot at most 1e-12 of its diagonal leaves that dof out, so a
 * free-floating body's semidefinite coarsest level is accepted).  The V-cycle is the
 * one of fh_mg_* (Chebyshev-Jacobi of degree m before and after, restriction by P^T, prolongation by P) with no floating-point atomics and
 * no host synchronisation; setup sums every entry in a fixed order, so a create, a refresh and a solve repeat bit for bit.
 * Errors: no pattern: FH_INVALID_STATE; nb of 0 or above 6, a null B for FH_AMG_USER, FH_AMG_RIGID_BODY with s != d, theta < 0:
 * FH_BAD_ARGUMENT; a row of A P or P^T (A P) with more than 512 blocks: FH_UNSUPPORTED.  values_dev must stay allocated while the hierarchy
 * is used (level 0 reads it).  The values passed to an FH_PRECOND_AMG solve must be those the hierarchy was built from or last refreshed with.
 * The hierarchy refers to the context's pattern: destroying the context while it is attached (or attaching another one) orphans it,
 * and every later call on it but fh_amg_destroy returns FH_BAD_ARGUMENT; fh_amg_destroy then only frees it.  A pattern built again
 * on the context, or another solution dim, invalidates it: FH_INVALID_STATE (the lifetime rule above fh_mg_create). */
enum { FH_PRECOND_AMG = 3 };
enum { FH_AMG_CONSTANT = 0, FH_AMG_RIGID_BODY = 1, FH_AMG_USER = 2 };
int fh_amg_create(fh_ctx*, const double* values_dev, int nullspace, const double* B, uint32_t nb, double theta, uint32_t max_levels,
                  fh_amg** out);
/* numeric refresh for new values on the same pattern (K(u) of a Newton or time-stepping loop): the aggregates, T and every pattern are
 * kept; lambda, the values of P and A_c and the coarse factor are formed again, the same bits as a create with the same aggregates */
int fh_amg_update_values(fh_amg*, const double* values_dev);
void fh_amg_destroy(fh_amg*);
/* attach (or with NULL detach) the hierarchy the context's FH_PRECOND_AMG solves use; FH_PRECOND_AMG without one: FH_INVALID_STATE */
int fh_set_amg(fh_ctx*, fh_amg*);
/* degree m (default 3), range (default 15) and Lanczos steps of the eigenvalue estimate (default 10); forms lambda, P and A_c again */
int fh_amg_set_smoother(fh_amg*, uint32_t degree, double range, uint32_t eig_steps);
/* one V-cycle z = B r; r, z on the device */
int fh_amg_apply_dev(fh_amg*, const double* r_dev, double* z_dev);
/* level 0 is the fine one: its dofs, nonzero blocks, block size and lambda_max (0 on the coarsest); level >= number of levels:
 * FH_BAD_ARGUMENT */
int fh_amg_level_info(fh_amg*, uint32_t level, uint64_t* num_dofs, uint64_t* nnz_blocks, uint32_t* block_size, double* lambda_max);
/* the aggregate of every node of a level that has a coarser one (UINT64_MAX: isolated) */
int fh_amg_aggregates(fh_amg*, uint32_t level, uint64_t* agg_of_node);
/* A (which = 0), P (1), the tentative prolongator T (2) or the level's near-nullspace B (3; rows: the level's dofs, nb columns) of a level
 * as scalar CSR, two-phase like fh_pattern: null arrays give *nnz only; row_offsets has rows + 1 entries, cols and vals *nnz.  P and T
 * exist on every level but the coarsest. */
int fh_amg_level_matrix(fh_amg*, uint32_t level, int which, uint64_t* row_offsets, uint64_t* cols, double* vals, uint64_t* nnz);
/* estimate_L2_error_squared / estimate_H1_seminorm_error_squared (src/error.rs:287-372):
 *   sum_e sum_q w |det J| |u_h(x_q) - u(x_q)|^2      resp.   |grad u_h(x_q) - grad u(x_q)|_F^2
 * with the quadrature table of the context.  The reference solution is arbitrary code in the reference; here the
 * caller samples it at the physical points of fh_physical_quadrature_points: u_exact is (E, nq, s); grad_exact is
 * (E, nq, d, s) with grad[i][k] = d u_k / d x_i.  The H1 form inverts J: FH_SINGULAR_JACOBIAN if det J == 0. */
int fh_estimate_L2_error_squared(fh_ctx*, uint32_t solution_dim, const double* u_h, const double* u_exact, double* out);
int fh_estimate_L2_error_squared_dev(fh_ctx*, uint32_t solution_dim, const double* u_h_dev, const double* u_exact_dev, double* out);
int fh_estimate_H1_seminorm_error_squared(fh_ctx*, uint32_t solution_dim, const double* u_h, const double* grad_exact, double* out);
int fh_estimate_H1_seminorm_error_squared_dev(fh_ctx*, uint32_t solution_dim, const double* u_h_dev, const double* grad_exact_dev,
                                              double* out);

/* ---- recovery: what a user reads off a solved field.  For the context's mesh, operator, quadrature table and u (fh_set_u*; zeros when
 * none is set), with s the operator's solution dimension and d the geometry dimension; every array is row-major doubles.
 *   FH_RECOVER_GRAD_U          d x s   g[i][k] = d u_k / d x_i (the convention of fh_estimate_H1_seminorm_error_squared)
 *   FH_RECOVER_STRAIN          d x d   FH_LINEAR_ELASTIC: sym(grad u); FH_NEO_HOOKEAN, FH_STVK, FH_STABLE_NEO_HOOKEAN: Green-Lagrange (F^T F - I) / 2 with
 *                                      F = I + (grad u)^T (fenris-solid/src/lib.rs:20-29); the full symmetric matrix
 *   FH_RECOVER_STRESS_PK1      s x d   the operator's stress P (fenris-solid/src/materials.rs), the flux grad u for FH_LAPLACE;
 *                                      NeoHookean with det F <= 0: NaN, as in the residual; Stable Neo-Hookean: finite for every F
 *   FH_RECOVER_STRESS_CAUCHY   d x d   P F^T / det F for NeoHookean, StVK and Stable Neo-Hookean (NaN when det F <= 0, for Stable
 *                                      Neo-Hookean too: its P is finite there, the push-forward is not defined), P for LinearElastic
 *   FH_RECOVER_VON_MISES       1       of the Cauchy stress: sqrt(3/2 dev : dev) in 3-D; in 2-D the IN-PLANE form
 *                                      sqrt(sxx^2 - sxx syy + syy^2 + 3 sxy^2) (no out-of-plane stress is assumed or added)
 *   FH_RECOVER_ENERGY_DENSITY  1       psi; NeoHookean: +inf when det F <= 0; Stable Neo-Hookean: finite for every F
 *   FH_RECOVER_VOLUME          1       sum_q w_q |det J_q|; FH_AT_ELEMENTS only
 * FH_LAPLACE has no strain, Cauchy or von Mises stress: FH_UNSUPPORTED, as are the mass operators and FH_TENSOR.
 * Locations:
 *   FH_AT_POINTS    (E nq) x ncomp, one row per (element, quadrature point) in the order of fh_physical_quadrature_points; Lame
 *                   parameters from wherever the residual takes them (uniform, per-point or compact table)
 *   FH_AT_ELEMENTS  E x ncomp, the measure-weighted mean  sum_q w |det J| v_q / sum_q w |det J|  in point order (a von Mises mean is the
 *                   mean of the pointwise values); FH_RECOVER_VOLUME is the denominator
 *   FH_AT_NODES     N x ncomp, the volume-weighted patch average  sum_e V_e mean_e / sum_e V_e  over the active elements of the node in
 *                   ascending element order (no atomics: two calls agree bit for bit); a node without an active element gets zeros.
 *                   Deliberately not an L2 projection: vertex basis functions of Tet10 and Hex20 have non-positive integrals.
 * Elements masked by fh_set_active_elements give zeros at points and elements and take no part at the nodes.  Rule-set tables
 * (fh_set_quadrature_rules): FH_UNSUPPORTED, like fh_physical_quadrature_points.  det J == 0 in an active element:
 * FH_SINGULAR_JACOBIAN, read once at the end of the call like the residual reads it.  An unknown quantity or location, or
 * FH_RECOVER_VOLUME anywhere but FH_AT_ELEMENTS: FH_BAD_ARGUMENT.  The launches go to the context's stream; `out` is OVERWRITTEN. */
enum { FH_RECOVER_GRAD_U = 0, FH_RECOVER_STRAIN = 1, FH_RECOVER_STRESS_PK1 = 2, FH_RECOVER_STRESS_CAUCHY = 3, FH_RECOVER_VON_MISES = 4,
       FH_RECOVER_ENERGY_DENSITY = 5, FH_RECOVER_VOLUME = 6 };
enum { FH_AT_POINTS = 0, FH_AT_ELEMENTS = 1, FH_AT_NODES = 2 };
/* components per row of a quantity for the context's operator and mesh; also validates quantity x operator */
int fh_recover_components(fh_ctx*, int quantity, uint32_t* ncomp);
/* rows of a location: E nq, E or N */
int fh_recover_rows(fh_ctx*, int where, uint64_t* rows);
int fh_recover_dev(fh_ctx*, int quantity, int where, double* out_dev);
int fh_recover(fh_ctx*, int quantity, int where, double* out);

/* ---- composition of element assemblers: AggregateElementAssembler, MapElementNodes and TransformElementMatrix / Vector with
 * a scale factor (src/assembly/local.rs:152-340; tests/unit_tests/assembly/local.rs:189-336).  Every body keeps its own
 * context -- mesh, operator, table, element kind, fastest kernels -- and what it assembled in ITS node numbering is added,
 * scaled, into a matrix / vector over the aggregate's node index space:
 *     dst(map[i] s + r, map[j] s + c) += scale * src(i s + r, j s + c)        dst(map[i] s + r) += scale * src(i s + r)
 * node_map_dev: num_nodes(ctx) u64 on the device, or NULL for the identity (an aggregate over one shared node space).
 * The destination pattern (scalar CSR, u64, on the device; e.g. fh_pattern of a context that holds the aggregate's ragged
 * connectivity, fh_set_connectivity_ragged) must hold every mapped entry: a node out of range or a missing column is
 * FH_BAD_ARGUMENT (the reference panics, global.rs:531-533).  src/dst values on the device, same solution dimension. */
int fh_add_mapped_matrix_dev(fh_ctx* ctx, const double* src_values_dev, const uint64_t* node_map_dev, double scale,
                             uint64_t dst_num_nodes, const uint64_t* dst_row_offsets_dev, const uint64_t* dst_col_indices_dev,
                             double* dst_values_dev);
int fh_add_mapped_vector_dev(fh_ctx* ctx, const double* src_dev, const uint64_t* node_map_dev, double scale,
                             uint64_t dst_num_nodes, double* dst_dev);
/* The same with the solution dimension given by the caller (> 0): for the vector of an ElementSourceAssembler body, whose
 * context holds a mesh and a quadrature table but no operator (local/source.rs:159-278; the dimension is the source's). */
int fh_add_mapped_vector_sdim_dev(fh_ctx* ctx, const double* src_dev, const uint64_t* node_map_dev, double scale, int solution_dim,
                                  uint64_t dst_num_nodes, double* dst_dev);

/* ---- multi-GPU: one process or thread per GPU, each with its own fh_ctx holding one partition (its own
 * elements plus the halo layers whose nodes it shares, so that interface rows have the global pattern and the same layout
 * on both sides; numerics over the own elements: fh_set_active_elements).  The only data that crosses a partition boundary
 * are the partial rows of interface nodes: the non-owner sends its contiguous segment of `values` to the owner, which adds
 * it -- RCCL point-to-point (ncclSend / ncclRecv) on a side stream, each interface on its own xGMI link, beside the
 * assembly launches; never a collective over the matrix.  Replaces, across partitions, what the shared address space does
 * for CsrParAssembler::assemble_into_csr (src/assembly/global.rs:314-376).
 * Bootstrap like NCCL: rank 0 draws an id, the host distributes its bytes to every rank by whatever means it has. */
typedef struct fh_group fh_group;
#define FH_GROUP_ID_BYTES 128
int fh_group_unique_id(uint8_t id[FH_GROUP_ID_BYTES]);
/* collective over all `world` ranks; `ctx` gives the device and the stream the exchange is ordered against */
int fh_group_create(fh_ctx* ctx, const uint8_t id[FH_GROUP_ID_BYTES], int rank, int world, fh_group** out);
/* A group refers to its context: destroy every group of a context BEFORE fh_destroy(ctx). */
void fh_group_destroy(fh_group*);
/* number of ranks of the communicator as RCCL reports it (ncclCommCount) */
int fh_group_size(const fh_group*, int* ranks);
/* What this rank moves in one exchange: values[send_first .. send_first + send_count) go to rank send_peer (-1: nothing);
 * recv_count values arrive from rank recv_peer (-1: nothing) and are ADDED to values[recv_first ..).  For z-slabs:
 * send = rows of the bottom ghost plane to rank - 1, receive = rows of the owned top plane from rank + 1. */
int fh_group_set_exchange(fh_group*, int send_peer, uint64_t send_first, uint64_t send_count, int recv_peer,
                          uint64_t recv_first, uint64_t recv_count);
/* start: call after enqueueing the launch that produces the rows to send (fh_assemble_matrix_rows_async_dev for the
 * interface rows); the transfers run on the group's stream while the caller enqueues the rest of the assembly.
 * finish: the context's stream waits for the transfers and adds the received rows.  Errors: fh_last_error(ctx). */
int fh_group_exchange_start(fh_group*, double* values_dev);
int fh_group_exchange_finish(fh_group*, double* values_dev);
/* Arbitrary partitions (an element partition elem_to_part[] of an unstructured mesh: no planes, any number of neighbours, interface
 * rows anywhere): per peer a list of LOCAL NODES whose rows (all S scalar rows of the node, as they lie in `values`) are packed and sent,
 * and a list of owned local nodes whose rows receive-and-add what the peer packed -- both sides list the shared nodes in the same
 * (ascending global) order, so no indices travel.  Offsets have peers + 1 entries.  The context's pattern must have been built.  All
 * transfers of one exchange are posted in one RCCL group; fh_group_exchange_start / _finish drive this mode once it is set.  A rank
 * may list itself as a peer (a device copy inside RCCL: the single-GPU test does).  The nodes of ONE peer's list must be distinct; a node
 * may appear in the lists of several peers (their rows are added peer by peer, in list order).
 * CONTRACT: the exchange ships the listed rows AS THEY STAND and the receiver ADDS them.  The rows a rank sends must therefore hold this
 * assembly's partial sums only -- assemble them with FH_ASSEMBLE_OVERWRITE (the reference's accumulate-into-the-output semantics,
 * global.rs:133-182, applies to the OWNED rows after the exchange, not to the rows in transit): earlier content of a sent row would be
 * counted once more on its owner for every rank that sends it, without any error. */
int fh_group_set_exchange_nodes(fh_group*, int num_send_peers, const int32_t* send_peers, const uint64_t* send_offsets,
                                const uint64_t* send_nodes, int num_recv_peers, const int32_t* recv_peers, const uint64_t* recv_offsets,
                                const uint64_t* recv_nodes);

/* Node VECTORS through the same lists (the residual / source vector of a partition: fh_assemble_vector_dev over the active elements
 * leaves partial sums at the nodes other ranks own): `components` values per node (the solution dim), packed, sent, received and added
 * exactly like the rows above.  Entries of nodes the rank does not own are scratch afterwards.
 * CONTRACT (as for the rows): `vec_dev` must hold THIS assembly's partial sums only -- assemble into a zeroed vector, exchange, then add the
 * owned entries to whatever they accumulate into (fenris_amd/partition.py: PartAssembly.assemble_vector does exactly that). */
int fh_group_exchange_vector_start(fh_group*, double* vec_dev, uint32_t components);
int fh_group_exchange_vector_finish(fh_group*, double* vec_dev, uint32_t components);

/* ---- element partitions of arbitrary meshes (host; SURVEY.md 8e "the engine takes elem_to_part[]").  What one rank needs to run
 * its share of CsrParAssembler::assemble_into_csr (global.rs:314-376): a node is owned by the LOWEST part that touches it; the
 * extended local mesh holds the rank's own elements plus every element touching a node they touch, numbered by ascending global id
 * (the rows of every node the rank contributes to then carry the GLOBAL pattern in the global column order); numerics over the own
 * elements (fh_set_active_elements); interface rows through fh_group_set_exchange_nodes.  fenris_amd/partition.py mirrors this. */
typedef struct fh_partition fh_partition;
/* default partitioner: Morton order of the element centroids cut into `world` equal runs */
int fh_morton_partition(uint32_t dim, const double* vertices, uint64_t num_vertices, uint64_t nodes_per_element,
                        const uint64_t* connectivity, uint64_t num_elements, uint32_t world, int32_t* elem_to_part);
/* NULL on a bad argument (a part outside [0, world), a node index >= num_nodes).  halo_mode != 0: the halo elements that touch an owned
 * node are active as well -- the owned rows are complete without any exchange (the lists stay empty). */
fh_partition* fh_partition_create(uint64_t num_nodes, uint64_t nodes_per_element, const uint64_t* connectivity, uint64_t num_elements,
                                  const int32_t* elem_to_part, int rank, int world, int halo_mode);
void fh_partition_destroy(fh_partition*);
/* sizes: local nodes, local elements, owned nodes, own elements, peers sent to, nodes sent, peers received from, nodes received */
int fh_partition_sizes(const fh_partition*, uint64_t sizes[8]);
/* global id of every local node / element, connectivity in local node ids, element mask, owned local nodes (NULL skips an array) */
int fh_partition_mesh(const fh_partition*, uint64_t* l2g, uint64_t* elem_l2g, uint64_t* local_connectivity, uint8_t* active,
                      uint64_t* owned_nodes);
/* the arguments of fh_group_set_exchange_nodes (NULL skips an array) */
int fh_partition_exchange(const fh_partition*, int32_t* send_peers, uint64_t* send_offsets, uint64_t* send_nodes, int32_t* recv_peers,
                          uint64_t* recv_offsets, uint64_t* recv_nodes);

#ifdef __cplusplus
}
#endif
#endif /* FENRIS_HIP_H */
