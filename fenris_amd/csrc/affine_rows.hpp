// Affine-element owner-computes stiffness kernel, second form (k_affine_rows): interface of the translation unit
// affine_rows.hip.  See that file for the design; engine.hip only builds the tables and launches.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.hpp"

namespace fenris_hip {

// per-position tables (position = node block all of whose elements are affine, in CSR order)
struct AffineRowTables {
    const int4* hdr;      // [npos]       {r0: first node-level CSR entry, nrow: node-level entries of the block's rows,
                          //               flags (bit 0: every (node, column) block of the rows has an owner lane) | lane table << 8,
                          //               number of slots (bits 0-7) | id of the position's slot list << 8 once the shared tables were
                          //               built -- also after a build that ended in a mismatch: readers of the count mask with 0xff}
    const uint2* lanes;   // [ntab][256]  lane records, see affine_rows.hip; positions with identical records share a table
    // The shared form of the loader (affine_rows_launch: shared) reads slot_tab and rec_tab INSTEAD of elem and rec: they share the two places,
    // so that the argument block of the other instantiations -- and with it their instruction streams -- stays exactly what it was.
    union {
        const int* elem;                  // [npos][us]   element id per slot (-1: empty)
        const unsigned short* slot_tab;   // [nvec][us]   record class per slot (0xffff: empty); the list of a position: fourth word of its header >> 8
    };
    union {
        const double* rec;                // [E][GW]      element records (R or M) as affine_records_launch left them
        const double* rec_tab;            // [nrec][GW]   the distinct records among them (affine_shared_* below)
    };
    const double* ghat;   // [64][GW]     reference blocks Ghat_ab (all 64 (a, b); LinearElastic GW = 10, Laplace GW = 6)
    int us, npos, acc_max;  // slots per position, positions of this launch, largest S * S * nrow
    int pos0, npos_all;     // first position of this launch (launches may cover a part of the sweep), positions in the tables
    int incomplete;         // some position has a (node, column) block without an owner lane (element masks): staged rows are cleared behind the store
};

constexpr int AFFINE_ROWS_GW_LE = 10, AFFINE_ROWS_GW_LAP = 6;
constexpr int AFFINE_ROWS_NO_CLEAR = 0x40000;   // bits of the launcher's `ablate` argument kept from round 3's timing experiments (scripts/exp_slab_time3.py set them
constexpr int AFFINE_ROWS_NO_CARRY = 0x20000;   // through environment switches that are gone): never set by the library
constexpr int AFFINE_ROWS_PRIO_SHIFT = 24;        // bits 24-25 of the launcher's `ablate` argument: s_setprio level of the store wave, 26-27: of the loader wave
constexpr int AFFINE_ROWS_NT_STORES = 0x10000;  // bit of the launcher's `ablate` argument: non-temporal stores of the rows
constexpr int AFFINE_ROWS_THREADS = 384;  // four row waves + one loader wave + one store wave

size_t affine_rows_lds_bytes(int op, int us, int acc_max);

// lane records, headers and slot vertices of every position from the pipelined kernel's position records (p_rec, layout of
// k_build_pipe_tables) and its per-slot connectivity.  *status (device) is set to 1 when a block cannot be expressed
// (more than 8 terms per block, more than 256 lanes, offsets out of range).
hipError_t affine_rows_build(hipStream_t stream, const int* p_rec, int rw_old, int us, int ms, int nbs, int npos, int S,
                             const unsigned* ncols, const int* p_conn, int cs, const int* p_elem, int4* hdr, uint2* lanes,
                             int* status, unsigned long long* hash, int mirror = 0, unsigned long long* hash2 = nullptr, int max_row = 128);
// (max_row: the longest node row of the pattern -- the builder sizes its key space and its LDS by it; a row longer than 128 makes the position `bad`)
// lanes == nullptr: headers and hashes only (hash2: a second, independent 64-bit hash of the records) -- the records of the positions are
// never written in full; affine_rows_tables then forms the records of the FIRST position of every distinct table once more, straight into
// the compact tables, and puts the table ids into the headers (mismatch[1]: some position has a block without an owner lane)
hipError_t affine_rows_tables(hipStream_t stream, const int* p_rec, int rw_old, int us, int ms, int nbs, int npos, int S, const unsigned* ncols,
                              const int* p_conn, int cs, const int* p_elem, int mirror, const int* ids, const int* first_pos, int ntab,
                              uint2* lanes_tab, int4* hdr, int* mismatch, int max_row = 128);
// mirror != 0 (k_hex8_rows, hex8_rows.hip): a block whose two nodes are both owned by the position keeps the lanes of the smaller node's
// owner only (x bit 29: the lane also stores the transpose to the twin), and y = offset in doubles | node << 13 | twin offset << 16 |
// twin node << 29 (row strides from the position record)

// element records of the affine elements (elem_aff[e] != 0) among [e_first, e_end) from the current vertex coordinates, on the stream of
// affine_rows_launch in front of it.  They stay valid until the vertices, the connectivity or the flags change: the caller decides when to
// run this again (launch_affine).  A singular element (det J == 0 exactly) of the active set (active == NULL: all) is reported through
// `status`, and marked in `sing` whether active or not (affine_sing_words(E) words, zeroed by the caller: the number of marks, one bit per element).
hipError_t affine_records_launch(int op, hipStream_t stream, const double* verts, const int* conn, const unsigned char* elem_aff,
                                 const unsigned char* active, long long e_first, long long e_end, double* rec, DevStatus* status, unsigned* sing);
inline size_t affine_sing_words(unsigned long long E) { return 1 + (size_t)((E + 31) / 32); }
// what an assembly that does not run the records pass enqueues instead: the marked elements of [e_first, e_end) that are active now are
// reported through `status` exactly as the pass itself would have
hipError_t affine_replay_singular_launch(hipStream_t stream, const unsigned* sing, const unsigned char* active, long long e_first, long long e_end,
                                         DevStatus* status);

// Positions with identical lane records share one table: `lanes_full` [npos][256] as written by affine_rows_build, `ids` the
// table of every position, `first_pos` [ntab] a position that holds each table.  Writes the compact tables, puts the id into
// every header, and sets *mismatch if the records of a position differ from its table (callers fall back to ids = identity).
hipError_t affine_rows_compact(hipStream_t stream, const uint2* lanes_full, const int* ids, const int* first_pos, int npos, int ntab,
                               uint2* lanes_tab, int4* hdr, int* mismatch);

// op: FH_LAPLACE or FH_LINEAR_ELASTIC; depth (1 or 2): positions the loader wave's requests run ahead; ablate != 0 selects the instrumented
// instantiation (profiling only).  (Retired to scripts/attic/: the fused form whose seventh wavefront formed the element records, the chunked
// dealing of positions, a second store wave, and the ring form affine_ring.hip.)
// shared: T holds slot_tab / rec_tab (unmasked, not instrumented: anything else is an error)
hipError_t affine_rows_launch(int op, int depth, int grid, size_t lds_bytes, hipStream_t stream, const KArgs& a, const AffineRowTables& T, int ablate,
                              bool masked, bool shared = false);

// ---- shared records and slot lists (structured, graded, extruded meshes: most affine elements have bit-identical records).  The engine
// (launch_affine) merges on the host what these hash on the device, and uses the tables only after the two verify passes found every
// element's record and every position's list equal, bit for bit, to the table entry it was given.
// two 64-bit hashes of the record of every affine element of [e_first, e_end): hash[e - e_first] and hash[n + e - e_first], n = e_end - e_first;
// the second hash of an affine element is odd, an element that is not affine gets (0, 0)
hipError_t affine_shared_hash_records(int gw, hipStream_t stream, const double* rec, const unsigned char* elem_aff, long long e_first, long long e_end,
                                      unsigned long long* hash);
// rec_tab[c] = rec[first[c]]; then every affine element of [e_first, e_end) compares its record with rec_tab[cls[e]]: *mismatch = 1 on any difference
hipError_t affine_shared_record_table(int gw, hipStream_t stream, const double* rec, const unsigned char* elem_aff, const unsigned short* cls,
                                      const long long* first, int nrec, long long e_first, long long e_end, double* rec_tab, int* mismatch);
// two 64-bit hashes of every position's list {cls[elem[p][s]] or 0xffff}: hash[p] and hash[npos + p]
hipError_t affine_shared_hash_lists(hipStream_t stream, const int* elem, const unsigned short* cls, int npos, int us, unsigned long long* hash);
// slot_tab[v] = the list of position first_pos[v]; then every position compares its list with slot_tab[ids[p]] (*mismatch = 1 on any
// difference) and takes the id into the fourth word of its header: slot count | id << 8
hipError_t affine_shared_list_table(hipStream_t stream, const int* elem, const unsigned short* cls, const int* ids, const int* first_pos, int npos,
                                    int nvec, int us, unsigned short* slot_tab, int4* hdr, int* mismatch);

}  // namespace fenris_hip
