#pragma once
// Point location and interpolation at arbitrary points (engine_points.hip): the scaled element boxes and the cell
// grid over them, the closest point of a Tri3 / Tet4 geometry as the reference's element code forms it (src/element/triangle.rs:440-597,
// tetrahedron.rs:616-672, fenris-geometry line.rs:115-128), the locate kernel, the interpolator build and its two apply kernels.
// No floating-point atomics: every result is a function of its inputs alone.
#include <hip/hip_runtime.h>

namespace fenris_hip {

constexpr unsigned long long POINT_NO_ELEMENT = ~0ull;
constexpr double POINT_BOX_SCALE = 1.01;   // spatially_indexed.rs:99

// The uniform cell grid over the union of the scaled element boxes, by value in the kernel arguments.
struct PointGrid {
    double o[3], h[3], inv_h[3];   // origin, cell size and its inverse per axis (axes >= d: one cell)
    int n[3];                      // cells per axis
    double slack;                  // what the ring bound gives away for the rounding of the cell function
};

// the cell of a coordinate along one axis; monotone in x, so a box that lies beyond a block of cells lies beyond its far plane
__device__ __forceinline__ int point_cell(const PointGrid& g, int a, double x) {
    double f = floor((x - g.o[a]) * g.inv_h[a]);
    f = fmin(fmax(f, 0.0), (double)(g.n[a] - 1));
    return (int)f;
}

// ---- index build ---------------------------------------------------------------------------------------------------------------
// the box of an element's vertex nodes, scaled by 1.01 about its centre and padded by `pad` (a few ulps of the mesh: a box without
// extent along an axis still holds what rounds into it): min[D], max[D]
template <int D>
__global__ void k_point_boxes(const double* __restrict__ verts, const int* __restrict__ conn, int n, unsigned E, double pad,
                              double* __restrict__ box) {
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        const int* ec = conn + (size_t)e * n;
        double lo[D], hi[D];
#pragma unroll
        for (int a = 0; a < D; ++a) lo[a] = hi[a] = verts[(size_t)ec[0] * D + a];
#pragma unroll
        for (int v = 1; v <= D; ++v)
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const double x = verts[(size_t)ec[v] * D + a];
                lo[a] = fmin(lo[a], x);
                hi[a] = fmax(hi[a], x);
            }
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const double c = 0.5 * (lo[a] + hi[a]), half = 0.5 * (hi[a] - lo[a]) * POINT_BOX_SCALE + pad;
            box[(size_t)e * 2 * D + a] = c - half;
            box[(size_t)e * 2 * D + D + a] = c + half;
        }
    }
}

// min and max of the vertex coordinates the elements use (one workgroup; min and max do not depend on the order): out = min[D], max[D]
template <int D>
__global__ void k_point_mesh_box(const double* __restrict__ verts, const int* __restrict__ conn, int n, unsigned E, double* __restrict__ out) {
    __shared__ double s[2 * D][256];
    double lo[D], hi[D];
#pragma unroll
    for (int a = 0; a < D; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (unsigned e = threadIdx.x; e < E; e += blockDim.x)
#pragma unroll
        for (int v = 0; v <= D; ++v)
#pragma unroll
            for (int a = 0; a < D; ++a) {
                const double x = verts[(size_t)conn[(size_t)e * n + v] * D + a];
                lo[a] = fmin(lo[a], x);
                hi[a] = fmax(hi[a], x);
            }
#pragma unroll
    for (int a = 0; a < D; ++a) { s[a][threadIdx.x] = lo[a]; s[D + a][threadIdx.x] = hi[a]; }
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int a = 0; a < D; ++a) {
                s[a][threadIdx.x] = fmin(s[a][threadIdx.x], s[a][threadIdx.x + w]);
                s[D + a][threadIdx.x] = fmax(s[D + a][threadIdx.x], s[D + a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 2 * D) out[threadIdx.x] = s[threadIdx.x][0];
}

template <int D>
__device__ __forceinline__ void point_box_cells(const PointGrid& g, const double* __restrict__ b, int (&lo)[3], int (&hi)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        lo[a] = a < D ? point_cell(g, a, b[a]) : 0;
        hi[a] = a < D ? point_cell(g, a, b[D + a]) : 0;
    }
}

// the number of cells each element's box overlaps
template <int D>
__global__ void k_point_cell_counts(const double* __restrict__ box, unsigned E, PointGrid g, unsigned* __restrict__ count) {
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        int lo[3], hi[3];
        point_box_cells<D>(g, box + (size_t)e * 2 * D, lo, hi);
        const unsigned long long c = (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned)(hi[1] - lo[1] + 1) * (unsigned)(hi[2] - lo[2] + 1);
        count[e] = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)c;
    }
}

// (cell, element) keys of every overlap, at the element's place in the scan of the counts: sorted, they are the per-cell lists in
// ascending element order
template <int D>
__global__ void k_point_cell_keys(const double* __restrict__ box, unsigned E, PointGrid g, const unsigned* __restrict__ first,
                                  unsigned long long* __restrict__ keys) {
    for (unsigned e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        int lo[3], hi[3];
        point_box_cells<D>(g, box + (size_t)e * 2 * D, lo, hi);
        size_t k = first[e];
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) {
                    const unsigned long long cell = ((unsigned long long)z * g.n[1] + y) * g.n[0] + x;
                    keys[k++] = (cell << 32) | e;
                }
    }
}

// from the sorted keys: the first entry of every cell (thread ncell closes the offsets) and the element of every entry
__global__ void k_point_cell_lists(const unsigned long long* __restrict__ keys, unsigned total, unsigned ncell, unsigned* __restrict__ off,
                                   unsigned* __restrict__ list) {
    const unsigned stride = gridDim.x * blockDim.x, t0 = blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned c = t0; c <= ncell; c += stride) {
        unsigned lo = 0, hi = total;   // first key whose cell is >= c
        while (lo < hi) {
            const unsigned mid = lo + (hi - lo) / 2;
            if ((unsigned)(keys[mid] >> 32) < c) lo = mid + 1;
            else hi = mid;
        }
        off[c] = lo;
    }
    for (unsigned k = t0; k < total; k += stride) list[k] = (unsigned)(keys[k] & 0xFFFFFFFFull);
}

// ---- closest point, as the reference's element code --------------------------------------------------------------------------
// LineSegment::closest_point_parametric: the parameter in [0, 1] of the closest point of a + t (b - a); 0 for a segment without length
template <int D>
__device__ __forceinline__ double segment_parameter(const double (&a)[D], const double (&b)[D], const double (&p)[D]) {
    double d2 = 0.0, num = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const double dir = b[i] - a[i];
        d2 += dir * dir;
        num += (p[i] - a[i]) * dir;
    }
    const double t = d2 == 0.0 ? 0.0 : num / d2;
    return fmin(fmax(t, 0.0), 1.0);
}

// the closest point on the three edges (a, b), (b, c), (c, a) of a triangle in D dimensions, as 2-D reference coordinates; the first
// edge wins a tie (Iterator::min_by)
template <int D>
__device__ __forceinline__ void triangle_edges_closest(const double (&a)[D], const double (&b)[D], const double (&c)[D], const double (&p)[D],
                                                        double (&xi)[2], double& dist2) {
    const double RX[3] = {-1.0, 1.0, -1.0}, RY[3] = {-1.0, -1.0, 1.0};
    dist2 = INFINITY;
    xi[0] = xi[1] = -1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double(&x1)[D] = k == 0 ? a : k == 1 ? b : c;
        const double(&x2)[D] = k == 0 ? b : k == 1 ? c : a;
        const double t = segment_parameter<D>(x1, x2, p);
        double d2 = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double q = x1[i] + (x2[i] - x1[i]) * t;
            d2 += (p[i] - q) * (p[i] - q);
        }
        if (k == 0 || d2 < dist2) {
            dist2 = d2;
            const int k2 = (k + 1) % 3;
            xi[0] = RX[k] + (RX[k2] - RX[k]) * t;
            xi[1] = RY[k] + (RY[k2] - RY[k]) * t;
        }
    }
}

__device__ __forceinline__ bool likely_in_tri_ref_interior(const double (&xi)[2]) {
    const double eps = 4.0 * 2.220446049250313e-16;
    return xi[0] >= -1.0 - eps && xi[1] >= -1.0 - eps && xi[0] + xi[1] <= eps;
}

__device__ __forceinline__ bool likely_in_tet_ref_interior(const double (&xi)[3]) {
    const double eps = 4.0 * 2.220446049250313e-16;
    return xi[0] >= -1.0 - eps && xi[1] >= -1.0 - eps && xi[2] >= -1.0 - eps && xi[0] + xi[1] + xi[2] <= -1.0 + eps;
}

// x(xi) of a triangle in D dimensions and |x(xi) - p|^2
template <int D>
__device__ __forceinline__ double triangle_dist2(const double (&a)[D], const double (&b)[D], const double (&c)[D], const double (&xi)[2],
                                                 const double (&p)[D]) {
    const double n0 = -0.5 * xi[0] - 0.5 * xi[1], n1 = 0.5 * xi[0] + 0.5, n2 = 0.5 * xi[1] + 0.5;
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const double x = a[i] * n0 + b[i] * n1 + c[i] * n2;
        d2 += (p[i] - x) * (p[i] - x);
    }
    return d2;
}

// Tri3d2Element::closest_point: true for InElement
__device__ __forceinline__ bool tri3_closest_point(const double (&a)[2], const double (&b)[2], const double (&c)[2], const double (&p)[2],
                                                   double (&xi)[2]) {
    // A = X G^T: columns (b - a) / 2 and (c - a) / 2; p0 = x(0, 0) = (b + c) / 2
    const double a00 = 0.5 * (b[0] - a[0]), a10 = 0.5 * (b[1] - a[1]), a01 = 0.5 * (c[0] - a[0]), a11 = 0.5 * (c[1] - a[1]);
    const double det = a00 * a11 - a10 * a01;
    bool interior = false;
    double xin[2] = {0.0, 0.0};
    if (det != 0.0) {
        const double r0 = p[0] - (0.5 * b[0] + 0.5 * c[0]), r1 = p[1] - (0.5 * b[1] + 0.5 * c[1]);
        xin[0] = (a11 / det) * r0 + (-a01 / det) * r1;
        xin[1] = (-a10 / det) * r0 + (a00 / det) * r1;
        interior = likely_in_tri_ref_interior(xin);
    }
    double dist2_edge;
    triangle_edges_closest<2>(a, b, c, p, xi, dist2_edge);
    if (interior && triangle_dist2<2>(a, b, c, xin, p) < dist2_edge) {
        xi[0] = xin[0];
        xi[1] = xin[1];
        return true;
    }
    return false;
}

// Tri3d3Element::closest_point (always ClosestPoint): the projection into the plane when it falls into the triangle, else an edge
__device__ __forceinline__ void tri3d3_closest_point(const double (&a)[3], const double (&b)[3], const double (&c)[3], const double (&p)[3],
                                                     double (&xi)[2]) {
    double A0[3], A1[3], r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        A0[i] = 0.5 * (b[i] - a[i]);
        A1[i] = 0.5 * (c[i] - a[i]);
        r[i] = p[i] - (0.5 * b[i] + 0.5 * c[i]);
    }
    const double m00 = A0[0] * A0[0] + A0[1] * A0[1] + A0[2] * A0[2], m01 = A0[0] * A1[0] + A0[1] * A1[1] + A0[2] * A1[2],
                 m11 = A1[0] * A1[0] + A1[1] * A1[1] + A1[2] * A1[2];
    const double det = m00 * m11 - m01 * m01;
    bool interior = false;
    double xin[2] = {0.0, 0.0};
    if (det != 0.0) {
        const double t0 = A0[0] * r[0] + A0[1] * r[1] + A0[2] * r[2], t1 = A1[0] * r[0] + A1[1] * r[1] + A1[2] * r[2];
        xin[0] = (m11 / det) * t0 + (-m01 / det) * t1;
        xin[1] = (-m01 / det) * t0 + (m00 / det) * t1;
        interior = likely_in_tri_ref_interior(xin);
    }
    double dist2_edge;
    triangle_edges_closest<3>(a, b, c, p, xi, dist2_edge);
    if (interior && triangle_dist2<3>(a, b, c, xin, p) < dist2_edge) {
        xi[0] = xin[0];
        xi[1] = xin[1];
    }
}

// Tet4Element::closest_point: true for InElement.  v: the four vertices.
__device__ __forceinline__ bool tet4_closest_point(const double (&v)[4][3], const double (&p)[3], double (&xi)[3]) {
    // A = X G^T: columns (v_k - v_0) / 2; p0 = x(0, 0, 0) = -v0 / 2 + (v1 + v2 + v3) / 2
    double m[3][3], r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) m[i][k] = 0.5 * (v[k + 1][i] - v[0][i]);
        r[i] = p[i] - (v[0][i] * -0.5 + v[1][i] * 0.5 + v[2][i] * 0.5 + v[3][i] * 0.5);
    }
    const double minor_12_23 = m[1][1] * m[2][2] - m[2][1] * m[1][2], minor_11_23 = m[1][0] * m[2][2] - m[2][0] * m[1][2],
                 minor_11_22 = m[1][0] * m[2][1] - m[2][0] * m[1][1];
    const double det = m[0][0] * minor_12_23 - m[0][1] * minor_11_23 + m[0][2] * minor_11_22;
    bool interior = false;
    double xin[3] = {0.0, 0.0, 0.0};
    if (det != 0.0) {
        const double i00 = minor_12_23 / det, i01 = (m[0][2] * m[2][1] - m[2][2] * m[0][1]) / det, i02 = (m[0][1] * m[1][2] - m[1][1] * m[0][2]) / det;
        const double i10 = -minor_11_23 / det, i11 = (m[0][0] * m[2][2] - m[2][0] * m[0][2]) / det, i12 = (m[0][2] * m[1][0] - m[1][2] * m[0][0]) / det;
        const double i20 = minor_11_22 / det, i21 = (m[0][1] * m[2][0] - m[2][1] * m[0][0]) / det, i22 = (m[0][0] * m[1][1] - m[1][0] * m[0][1]) / det;
        xin[0] = i00 * r[0] + i01 * r[1] + i02 * r[2];
        xin[1] = i10 * r[0] + i11 * r[1] + i12 * r[2];
        xin[2] = i20 * r[0] + i21 * r[1] + i22 * r[2];
        interior = likely_in_tet_ref_interior(xin);
    }
    // the four faces (connectivity.rs:537-540); the first face wins a tie
    constexpr int F[4][3] = {{0, 2, 1}, {0, 1, 3}, {1, 2, 3}, {0, 3, 2}};
    const double RV[4][3] = {{-1.0, -1.0, -1.0}, {1.0, -1.0, -1.0}, {-1.0, 1.0, -1.0}, {-1.0, -1.0, 1.0}};
    double dist2_face = INFINITY;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        double xf[2];
        tri3d3_closest_point(v[F[f][0]], v[F[f][1]], v[F[f][2]], p, xf);
        const double d2 = triangle_dist2<3>(v[F[f][0]], v[F[f][1]], v[F[f][2]], xf, p);
        if (f == 0 || d2 < dist2_face) {
            dist2_face = d2;
            const double n0 = -0.5 * xf[0] - 0.5 * xf[1], n1 = 0.5 * xf[0] + 0.5, n2 = 0.5 * xf[1] + 0.5;
#pragma unroll
            for (int i = 0; i < 3; ++i) xi[i] = RV[F[f][0]][i] * n0 + RV[F[f][1]][i] * n1 + RV[F[f][2]][i] * n2;
        }
    }
    if (interior) {
        const double n0 = -0.5 * xin[0] - 0.5 * xin[1] - 0.5 * xin[2] - 0.5, n1 = 0.5 * xin[0] + 0.5, n2 = 0.5 * xin[1] + 0.5, n3 = 0.5 * xin[2] + 0.5;
        double d2 = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double x = v[0][i] * n0 + v[1][i] * n1 + v[2][i] * n2 + v[3][i] * n3;
            d2 += (p[i] - x) * (p[i] - x);
        }
        if (d2 < dist2_face) {
            xi[0] = xin[0];
            xi[1] = xin[1];
            xi[2] = xin[2];
            return true;
        }
    }
    return false;
}

// closest_point of element e and d2 = |x(xi) - p|^2
template <int D>
__device__ __forceinline__ bool element_closest_point(const double* __restrict__ verts, const int* __restrict__ ec, const double (&p)[D],
                                                      double (&xi)[D], double& d2) {
    double v[D + 1][D];
#pragma unroll
    for (int k = 0; k <= D; ++k)
#pragma unroll
        for (int a = 0; a < D; ++a) v[k][a] = verts[(size_t)ec[k] * D + a];
    bool in;
    double psi[D + 1];
    if constexpr (D == 2) {
        in = tri3_closest_point(v[0], v[1], v[2], p, xi);
        psi[0] = -0.5 * xi[0] - 0.5 * xi[1];
        psi[1] = 0.5 * xi[0] + 0.5;
        psi[2] = 0.5 * xi[1] + 0.5;
    } else {
        in = tet4_closest_point(v, p, xi);
        psi[0] = -0.5 * xi[0] - 0.5 * xi[1] - 0.5 * xi[2] - 0.5;
        psi[1] = 0.5 * xi[0] + 0.5;
        psi[2] = 0.5 * xi[1] + 0.5;
        psi[3] = 0.5 * xi[2] + 0.5;
    }
    d2 = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        double x = 0.0;
#pragma unroll
        for (int k = 0; k <= D; ++k) x += v[k][a] * psi[k];
        d2 += (x - p[a]) * (x - p[a]);
    }
    return in;
}

// ---- locate --------------------------------------------------------------------------------------------------------------------
// One lane per point.  The answer is that of the rule over ALL elements (the lowest InElement, else the smallest d2, the lower index on a
// tie): a listed element is passed over only when its box is strictly farther than the best d2, and the rings stop only when everything
// outside them is.  A point with a non-finite coordinate: POINT_NO_ELEMENT, xi = 0.
template <int D>
__global__ void __launch_bounds__(256) k_locate_points(const double* __restrict__ verts, const int* __restrict__ conn, int n,
                                                       const double* __restrict__ box, const unsigned* __restrict__ cell_off,
                                                       const unsigned* __restrict__ cell_list, PointGrid g,
                                                       const double* __restrict__ points, unsigned long long m,
                                                       unsigned long long* __restrict__ out_elem, double* __restrict__ out_xi,
                                                       unsigned char* __restrict__ out_in) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
        double p[D];
        bool finite = true;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            p[a] = points[i * D + a];
            finite = finite && isfinite(p[a]);
        }
        unsigned best_e = 0xFFFFFFFFu;
        bool best_in = false;
        double best_d2 = INFINITY, best_xi[D];
#pragma unroll
        for (int a = 0; a < D; ++a) best_xi[a] = 0.0;
        if (finite) {
            int c[3] = {0, 0, 0};
#pragma unroll
            for (int a = 0; a < D; ++a) c[a] = point_cell(g, a, p[a]);
            const int rmax = max(g.n[0], max(g.n[1], g.n[2]));
            for (int r = 0; r < rmax; ++r) {   // (r < rmax: the block covers the grid at the latest then)
                int lo[3], hi[3], ilo[3], ihi[3];   // the block of this ring and the block inside it
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    lo[a] = a < D ? max(c[a] - r, 0) : 0;
                    hi[a] = a < D ? min(c[a] + r, g.n[a] - 1) : 0;
                    ilo[a] = a < D ? max(c[a] - r + 1, 0) : 0;
                    ihi[a] = a < D ? min(c[a] + r - 1, g.n[a] - 1) : 0;
                }
                for (int z = lo[2]; z <= hi[2]; ++z)
                    for (int y = lo[1]; y <= hi[1]; ++y) {
                        // a row inside the ring's shell has two cells of the ring, its ends
                        const bool shell_row = (D == 3 && abs(z - c[2]) == r) || abs(y - c[1]) == r;
                        const int xstep = shell_row || r == 0 ? 1 : 2 * r;
                        for (int x = c[0] - r; x <= c[0] + r; x += xstep) {
                            if (x < lo[0] || x > hi[0]) continue;
                            const unsigned cell = ((unsigned)z * g.n[1] + y) * g.n[0] + x;
                            const unsigned k1 = cell_off[cell + 1];
                            for (unsigned k = cell_off[cell]; k < k1; ++k) {
                                const unsigned e = cell_list[k];
                                const double* b = box + (size_t)e * 2 * D;
                                double bl[D], bh[D], db2 = 0.0;
#pragma unroll
                                for (int a = 0; a < D; ++a) {
                                    bl[a] = b[a];
                                    bh[a] = b[D + a];
                                    const double dd = fmax(fmax(bl[a] - p[a], p[a] - bh[a]), 0.0);
                                    db2 += dd * dd;
                                }
                                if (db2 > best_d2) continue;
                                // an element is listed in several cells: it is taken in the lowest cell of its overlap with the block, and
                                // not at all when a smaller block met it
                                bool here = true, seen = r > 0;
                                const int cc[3] = {x, y, z};
#pragma unroll
                                for (int a = 0; a < D; ++a) {
                                    const int el = point_cell(g, a, bl[a]), eh = point_cell(g, a, bh[a]);
                                    here = here && max(el, lo[a]) == cc[a];
                                    seen = seen && el <= ihi[a] && eh >= ilo[a];
                                }
                                if (!here || seen) continue;
                                double xi[D], d2;
                                const bool in = element_closest_point<D>(verts, conn + (size_t)e * n, p, xi, d2);
                                const bool take = in ? (!best_in || e < best_e) : (!best_in && (d2 < best_d2 || (d2 == best_d2 && e < best_e)));
                                if (take) {
                                    best_e = e;
                                    best_d2 = in ? fmin(best_d2, d2) : d2;
                                    best_in = in;
#pragma unroll
                                    for (int a = 0; a < D; ++a) best_xi[a] = xi[a];
                                }
                                if (in && r == 0) break;   // the list ascends: the lowest InElement of the point's own cell
                            }
                        }
                    }
                if (best_in) break;
                // everything not met yet lies beyond a face of the block that is not a face of the grid
                double reach = INFINITY;
                bool whole = true;
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    if (lo[a] > 0) { reach = fmin(reach, p[a] - (g.o[a] + lo[a] * g.h[a])); whole = false; }
                    if (hi[a] < g.n[a] - 1) { reach = fmin(reach, (g.o[a] + (hi[a] + 1) * g.h[a]) - p[a]); whole = false; }
                }
                if (whole) break;
                reach = fmax(reach - g.slack, 0.0);
                if (reach * reach > best_d2) break;
            }
        }
        out_elem[i] = best_e == 0xFFFFFFFFu ? POINT_NO_ELEMENT : (unsigned long long)best_e;
#pragma unroll
        for (int a = 0; a < D; ++a) out_xi[i * D + a] = best_xi[a];
        out_in[i] = best_in ? 1 : 0;
    }
}

// ---- interpolator --------------------------------------------------------------------------------------------------------------
// Every basis of the supported kinds is a polynomial in the linear basis psi: its value, and its derivatives by psi (gradient = sum of
// dpsi[i] * grad psi_i).  Node order and formulas: triangle.rs:211-252, tetrahedron.rs:179-224, 346-466.
enum PointBasis { PB_LINEAR = 0, PB_TRI6 = 1, PB_TET10 = 2, PB_TET20 = 3 };

__device__ __forceinline__ double sel4(const double (&a)[4], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }
__device__ __forceinline__ void add4(double (&a)[4], int i, double x) {
    a[0] += i == 0 ? x : 0.0;
    a[1] += i == 1 ? x : 0.0;
    a[2] += i == 2 ? x : 0.0;
    a[3] += i == 3 ? x : 0.0;
}

__device__ __forceinline__ double point_basis(int basis, int k, const double (&psi)[4], double (&dpsi)[4]) {
    dpsi[0] = dpsi[1] = dpsi[2] = dpsi[3] = 0.0;
    if (basis == PB_LINEAR) {
        add4(dpsi, k, 1.0);
        return sel4(psi, k);
    }
    if (basis == PB_TRI6 || basis == PB_TET10) {
        const int nv = basis == PB_TRI6 ? 3 : 4;
        if (k < nv) {
            const double s = sel4(psi, k);
            add4(dpsi, k, 4.0 * s - 1.0);
            return s * (2.0 * s - 1.0);
        }
        // edge nodes: Tri6 (0,1) (1,2) (0,2); Tet10 (0,1) (1,2) (0,2) (0,3) (2,3) (1,3)
        const int m = k - nv;
        const int i = m == 1 ? 1 : m == 4 ? 2 : m == 5 ? 1 : 0;
        const int j = m == 0 ? 1 : m == 1 ? 2 : m == 2 ? 2 : 3;
        const double pi = sel4(psi, i), pj = sel4(psi, j);
        add4(dpsi, i, 4.0 * pj);
        add4(dpsi, j, 4.0 * pi);
        return 4.0 * pi * pj;
    }
    // Tet20: vertices, two nodes on each of the edges (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), one on each of the faces (0,1,2) (0,1,3) (0,2,3) (1,2,3)
    if (k < 4) {
        const double s = sel4(psi, k);
        add4(dpsi, k, 0.5 * (27.0 * s * s - 18.0 * s + 2.0));
        return 0.5 * s * (3.0 * s - 1.0) * (3.0 * s - 2.0);
    }
    if (k < 16) {
        const int m = (k - 4) >> 1, half = (k - 4) & 1;
        const int e0 = m < 3 ? 0 : m < 5 ? 1 : 2, e1 = m == 0 ? 1 : (m == 1 || m == 3) ? 2 : 3;
        const int cl = half ? e1 : e0, ot = half ? e0 : e1;
        const double pc = sel4(psi, cl), po = sel4(psi, ot);
        add4(dpsi, cl, (9.0 / 2.0) * (po * (6.0 * pc - 1.0)));
        add4(dpsi, ot, (9.0 / 2.0) * (pc * (3.0 * pc - 1.0)));
        return (9.0 / 2.0) * pc * po * (3.0 * pc - 1.0);
    }
    const int f = k - 16;
    const int a = f == 3 ? 1 : 0, b = f < 2 ? 1 : 2, c = f == 0 ? 2 : 3;
    const double pa = sel4(psi, a), pb = sel4(psi, b), pc = sel4(psi, c);
    add4(dpsi, a, 27.0 * pb * pc);
    add4(dpsi, b, 27.0 * pa * pc);
    add4(dpsi, c, 27.0 * pa * pb);
    return 27.0 * pa * pb * pc;
}

// From (element, xi) to the n entries of each point: the element's nodes in element order, the basis values and the physical gradients
// J^-T grad phi (d per node).  A point without an element: index 0 and zero weights.  An element without volume has no gradients: NaN.
template <int D>
__global__ void k_interpolator_build(const double* __restrict__ verts, const int* __restrict__ conn, int n, int basis,
                                     const unsigned long long* __restrict__ elem, const double* __restrict__ xi_all, unsigned long long m,
                                     unsigned long long* __restrict__ offsets, unsigned long long* __restrict__ indices,
                                     double* __restrict__ values, double* __restrict__ gradients) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += stride) {
        offsets[i] = i * (unsigned long long)n;
        if (i == m) break;
        const unsigned long long e = elem[i];
        const size_t base = (size_t)i * n;
        if (e == POINT_NO_ELEMENT) {
            for (int k = 0; k < n; ++k) {
                indices[base + k] = 0;
                if (values) values[base + k] = 0.0;
                if (gradients)
#pragma unroll
                    for (int a = 0; a < D; ++a) gradients[(base + k) * D + a] = 0.0;
            }
            continue;
        }
        const int* ec = conn + (size_t)e * n;
        double xi[3] = {0.0, 0.0, 0.0}, psi[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int a = 0; a < D; ++a) xi[a] = xi_all[i * D + a];
        if constexpr (D == 2) {
            psi[0] = -0.5 * xi[0] - 0.5 * xi[1];
            psi[1] = 0.5 * xi[0] + 0.5;
            psi[2] = 0.5 * xi[1] + 0.5;
        } else {
            psi[0] = -0.5 * xi[0] - 0.5 * xi[1] - 0.5 * xi[2] - 0.5;
            psi[1] = 0.5 * xi[0] + 0.5;
            psi[2] = 0.5 * xi[1] + 0.5;
            psi[3] = 0.5 * xi[2] + 0.5;
        }
        // physical gradients of the linear basis: psi_k = (1 + xi_{k-1}) / 2 has the gradient (row k-1 of J^-1) / 2, psi_0 minus their sum
        double gp[4][D];
        if (gradients) {
            double J[D][D];   // J[i][k] = (v_{k+1} - v_0)_i / 2
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int k = 0; k < D; ++k) J[a][k] = 0.5 * (verts[(size_t)ec[k + 1] * D + a] - verts[(size_t)ec[0] * D + a]);
            double inv[D][D], det;
            if constexpr (D == 2) {
                det = J[0][0] * J[1][1] - J[1][0] * J[0][1];
                inv[0][0] = J[1][1] / det; inv[0][1] = -J[0][1] / det;
                inv[1][0] = -J[1][0] / det; inv[1][1] = J[0][0] / det;
            } else {
                const double c00 = J[1][1] * J[2][2] - J[2][1] * J[1][2], c01 = J[1][0] * J[2][2] - J[2][0] * J[1][2],
                             c02 = J[1][0] * J[2][1] - J[2][0] * J[1][1];
                det = J[0][0] * c00 - J[0][1] * c01 + J[0][2] * c02;
                inv[0][0] = c00 / det; inv[0][1] = (J[0][2] * J[2][1] - J[2][2] * J[0][1]) / det; inv[0][2] = (J[0][1] * J[1][2] - J[1][1] * J[0][2]) / det;
                inv[1][0] = -c01 / det; inv[1][1] = (J[0][0] * J[2][2] - J[2][0] * J[0][2]) / det; inv[1][2] = (J[0][2] * J[1][0] - J[1][2] * J[0][0]) / det;
                inv[2][0] = c02 / det; inv[2][1] = (J[0][1] * J[2][0] - J[2][1] * J[0][0]) / det; inv[2][2] = (J[0][0] * J[1][1] - J[1][0] * J[0][1]) / det;
            }
            const double bad = det == 0.0 ? NAN : 0.0;
#pragma unroll
            for (int a = 0; a < D; ++a) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    gp[k + 1][a] = 0.5 * inv[k][a] + bad;
                    s += gp[k + 1][a];
                }
                gp[0][a] = -s;
            }
#pragma unroll
            for (int k = D + 1; k < 4; ++k)
#pragma unroll
                for (int a = 0; a < D; ++a) gp[k][a] = 0.0;
        }
        for (int k = 0; k < n; ++k) {
            double dpsi[4];
            const double val = point_basis(basis, k, psi, dpsi);
            indices[base + k] = (unsigned long long)ec[k];
            if (values) values[base + k] = val;
            if (gradients)
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    double s = 0.0;
#pragma unroll
                    for (int q = 0; q <= D; ++q) s += dpsi[q] * gp[q][a];
                    gradients[(base + k) * D + a] = s;
                }
        }
    }
}

// out[p s + j] = sum over the entries k of point p, in stored order, of v_k u[s node_k + j]: one lane per (point, component)
__global__ void k_interpolator_apply(const unsigned long long* __restrict__ off, const unsigned long long* __restrict__ idx,
                                     const double* __restrict__ val, unsigned long long m, int s, const double* __restrict__ u,
                                     double* __restrict__ out) {
    const unsigned long long total = m * (unsigned long long)s, stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const unsigned long long p = t / (unsigned)s;
        const int j = (int)(t - p * (unsigned)s);
        const unsigned long long k1 = off[p + 1];
        double acc = 0.0;
        for (unsigned long long k = off[p]; k < k1; ++k) acc += val[k] * u[idx[k] * (unsigned)s + j];
        out[t] = acc;
    }
}

// out[p d s + j d + i] = sum over the entries k of point p, in stored order, of g_k[i] u[s node_k + j]: one lane per (point, component)
template <int D>
__global__ void k_interpolator_apply_gradients(const unsigned long long* __restrict__ off, const unsigned long long* __restrict__ idx,
                                               const double* __restrict__ grad, unsigned long long m, int s, const double* __restrict__ u,
                                               double* __restrict__ out) {
    const unsigned long long total = m * (unsigned long long)s, stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const unsigned long long p = t / (unsigned)s;
        const int j = (int)(t - p * (unsigned)s);
        const unsigned long long k1 = off[p + 1];
        double acc[D];
#pragma unroll
        for (int a = 0; a < D; ++a) acc[a] = 0.0;
        for (unsigned long long k = off[p]; k < k1; ++k) {
            const double uk = u[idx[k] * (unsigned)s + j];
#pragma unroll
            for (int a = 0; a < D; ++a) acc[a] += grad[k * D + a] * uk;
        }
#pragma unroll
        for (int a = 0; a < D; ++a) out[t * D + a] = acc[a];
    }
}

}  // namespace fenris_hip
