// Residual / source vectors through element TILES (vector_tiles.hip, round 4): interface of the translation unit.
// See that file for the design; engine.hip builds the tables once per mesh topology and launches the two passes.
#pragma once
#include <hip/hip_runtime.h>

#include "contact_kernels.hpp"
#include "device_common.hpp"
#include "dynamics_step.hpp"

namespace fenris_hip {


// device tables of one mesh (T tiles, P partial node sums, n nodes per element)
struct VecTiles {
    const int* elem;               // [T][256]        element of every tile thread, ascending inside a tile (-1: none)
    const int* tconn;              // [T][n][256]     node a of the thread's element (threads without one: the tile's first element)
    const unsigned* noff;          // [T + 1]         first partial of every tile
    const unsigned short* la_off;  // [P + T]         tile t: U + 1 starts into its entries, at noff[t] + t
    const unsigned short* la;      // [T][256 n]      entries (thread n + a) of the tile sorted by local node, then ascending
    const unsigned* np_off;        // [N + 1]         node -> its partials ...
    const unsigned* np_idx;        // [P]             ... ascending
    const unsigned* nodes;         // [P]             global node of every partial (a tile's distinct nodes, ascending)
    int ntiles, n;
    unsigned npartials;
    int ts;                        // elements per tile = threads per workgroup of the element pass
};

struct VecTilesStore {
    VecTiles v{};
    void* bufs[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    void release();
    ~VecTilesStore() { release(); }
};

// *bad (host) != 0: the tables cannot be built for this mesh (more than 2^32 partials ...): the caller keeps the two-pass kernels
hipError_t vector_tiles_build(hipStream_t stream, const int* conn, int n, long long E, const double* verts, int D, int num_nodes, VecTilesStore* out,
                              int* bad);

// what the tables look like (fh_vector_tiles_stats): the largest number of distinct nodes of a tile and the longest list of partials of a
// node, reduced from noff and np_off on the device when asked for (the stream is waited for)
hipError_t vector_tiles_stats(hipStream_t stream, const VecTiles& t, int num_nodes, unsigned* max_tile_nodes, unsigned* max_node_partials);

// element pass: every tile's elements in registers, their vectors summed per distinct node of the tile into partial[P][S].
// active (device, may be null): elements with active[e] == 0 contribute nothing.  Returns -1 when (elem_kind, op) is not covered.
int vector_tiles_element_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, double* partial);

// element pass of a central-difference step with Rayleigh stiffness damping: partial[P][S] of r(u) + eta_k T(u) v in one launch
// (k_damped_pass_tiled: the residual's body on u + eta_k v for the linear operators; the residual's and the tangent's body for the
// nonlinear ones), v S N doubles whose Dirichlet entries are zero.  Covers what vector_tiles_element_pass covers; -1 otherwise.
int vector_tiles_damped_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* v,
                             double eta_k, double* partial);

// energy over the tiles: one partial per workgroup into partial[] (the number of workgroups = partials comes back; -1: not covered);
// the caller sums them in index order (k_sum_partials)
int vector_tiles_energy_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, double* partial);
inline int vector_tiles_energy_partials(const VecTiles& t) { return 8 * ((t.ntiles + 7) / 8); }

// source vector (k_source_elements' arithmetic) over the tiles; g3: three doubles (host) or null; fact: scalar partials (GravitySource),
// the node pass multiplies by g.  Returns -1 when (D, n) is not covered.
int vector_tiles_source_pass(int D, int sdim, int n, bool fact, hipStream_t stream, const KArgs& a, const double* g3, const double* values,
                             const VecTiles& t, const unsigned char* active, double* partial);

// node pass: out[S node + c] += sum of the node's partials in ascending order (scaled_g != null: scalar partials, out += g[c] sum)
hipError_t vector_tiles_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* partial, double* out,
                                  const double* scaled_g = nullptr);

// diagonal of the matrix-free map (FH_LAPLACE, FH_LINEAR_ELASTIC: diagonal_element_body; FH_NEO_HOOKEAN, FH_STVK: tangent_diagonal_body at
// a.u; both element_pass.hpp, the material law material.hpp) over the tiles into partial[P][S]; the caller sums them with vector_tiles_node_pass.  Returns -1 when (elem_kind, op) is not covered.
int vector_tiles_diagonal_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, double* partial);

// tangent of the residual of FH_NEO_HOOKEAN and FH_STVK at a.u applied to x (k_tangent_tiled) over the tiles into partial[P][S] (the linear
// operators take vector_tiles_element_pass fed x); the caller sums them with vector_tiles_operator_node_pass (xbits null).  Returns -1 when
// (elem_kind, op) is not covered.
int vector_tiles_tangent_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* x,
                              double* partial);

// node pass of the matrix-free operator: y = the node sums of the partials, OVERWRITTEN; rows of the dofs dmask holds (the Dirichlet bytes, dof_fixed of
// device_common.hpp; dmask, scale: device, may be null / unused) are  *scale x; the other rows are multiplied by 2^e (xbits: mf_exponent, may be null).  dot_partial (may be null): one partial of x . y per workgroup
// (vector_tiles_operator_partials of them), to be summed in index order.  ct (count 0: off): contact_scale B x of the penalty contact term
// (contact_kernels.hpp; the unscaled x) joins the node's sum before the Dirichlet rows and the dot product.
inline int vector_tiles_operator_partials(int num_nodes) { return (num_nodes + 255) / 256; }
hipError_t vector_tiles_operator_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* partial, const double* x,
                                           const unsigned char* dmask, const double* scale, const unsigned long long* xbits, double* y,
                                           double* dot_partial, const ContactTable& ct, double contact_scale = 1.0);

// the mass term of the shifted map (engine_vector.hip) over the tiles into partial[P][S]: M x (x null: the diagonal of M), rho[rho_per_elem ? e : 0]
// the density, the entries of the dofs dmask holds read as zero (dmask may be null).  Returns -1 when (elem_kind, S) is not covered.
int vector_tiles_mass_pass(int elem_kind, int S, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* rho,
                           int rho_per_elem, const double* x, const unsigned char* dmask, double* partial);

// node pass of the shifted map: y = alpha (node sums of the mass partials) + beta tv, OVERWRITTEN (tv: may be y, or null = zero); the Dirichlet
// rows and dot_partial as vector_tiles_operator_node_pass
hipError_t vector_tiles_shift_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* partial, const double* x,
                                        const unsigned char* dmask, const double* scale, double alpha, double beta, const double* tv, double* y,
                                        double* dot_partial);

// node pass of the Newton residual: F = alpha (node sums of mpart) + beta (node sums of rpart - f), OVERWRITTEN, with rpart the residual's
// partials (vector_tiles_element_pass) and mpart the mass partials of d = u - u_ref (vector_tiles_mass_pass; null when alpha == 0), f null: zero;
// the rows of the dofs dmask holds are zero.  norm_partial: one partial of |F|^2 per workgroup (vector_tiles_operator_partials of
// them), to be summed in index order.  ct (count 0: off; here and in the two node passes below): the contact force g of the node
// (contact_kernels.hpp) joins its residual sum before anything else is formed from it.
hipError_t vector_tiles_newton_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* rpart, const double* mpart,
                                         const double* f, const unsigned char* dmask, double alpha, double beta, double* F, double* norm_partial,
                                         const ContactTable& ct);

// node pass of a central-difference step: the node sums of the residual's partials (vector_tiles_element_pass) and the integrator's state
// update of p.flags (DynStep, dynamics_kernels.hpp) in one visit; with DYN_STORE one partial of sum m v^2 per workgroup
// (vector_tiles_operator_partials of them) into p.ke_partial, to be summed in index order.
hipError_t vector_tiles_dynamics_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* rpart, const DynStep& p,
                                           const ContactTable& ct);

// node pass of one stage of a first-order Runge-Kutta-Legendre step, or of the rate alone (FoStage, dynamics_step.hpp): the node sums of the
// residual's partials and fo_dof in one visit; with FO_STORE one partial of sum m u^2 per workgroup (vector_tiles_operator_partials of them)
// into p.partial, to be summed in index order.
hipError_t vector_tiles_first_order_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* rpart, const FoStage& p,
                                              const ContactTable& ct);

// the shifted map fused on Hex8 with the monomial table (a.qmono; -1 otherwise): partial[P][S] of beta T(u) x + alpha M x in ONE element pass
// (k_shifted_pass_tiled for the linear operators, which read the operand from a.u; k_shifted_tangent_tiled for NeoHookean / StVK, operand x),
// or with mt.beta == 0 of alpha M x alone (k_mass_hex8_tiled, x read with the Dirichlet entries of dmask as zero; u not read).  The caller sums
// them with vector_tiles_operator_node_pass.
int vector_tiles_shifted_hex8_pass(int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* x,
                                   const unsigned char* dmask, const MassTerm& mt, double* partial);

}  // namespace fenris_hip
