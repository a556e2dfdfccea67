// Point location and interpolation at arbitrary points on the device (SpatiallyIndexed, FixedInterpolator of src/space): the cell-grid
// index over the scaled element boxes of the context's mesh, fh_locate_points, and the interpolator objects with their two apply kernels.
// Tri3, Tri6, Tet4, Tet10 and Tet20 meshes; location uses the vertex nodes (the kinds are sub-parametric).  DESIGN.md section 3.8.
#include "engine_internal.hpp"
#include "point_kernels.hpp"

#include <memory>

// the held index: boxes, grid and per-cell element lists (ascending), formed from the vertices as they were when it was built
struct PointIndex {
    int d = 0;
    unsigned E = 0, ncell = 0, total = 0;
    PointGrid g{};
    DevBuf<double> box;
    DevBuf<unsigned> cell_off, cell_list;
};

extern "C++" void point_index_drop(fh_ctx* c) {
    delete c->point_index;
    c->point_index = nullptr;
}

struct fh_interpolator {
    int device = 0;
    hipStream_t stream = nullptr;
    int d = 0;
    uint64_t m = 0, nnz = 0;
    bool has_values = false, has_gradients = false, has_max = false;
    uint64_t max_node = 0;
    DevBuf<unsigned long long> offsets, indices;
    DevBuf<double> values, gradients;
    std::string err;
    int fail(int code, const std::string& msg) { err = msg; return code; }
    int hip_fail(hipError_t e, const char* what) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return FH_HIP_ERROR;
    }
};

namespace {

struct WidenCount {
    __host__ __device__ unsigned long long operator()(unsigned x) const { return x; }
};

constexpr int POINT_GRID_CAP = 2048;   // workgroups of 256: enough to fill the device, the rest is walked with a grid stride

int point_grid_for(unsigned long long work) { return (int)std::max<unsigned long long>(1, std::min<unsigned long long>((work + 255) / 256, POINT_GRID_CAP)); }

int points_supported(fh_ctx* c, const char* who, int& basis) {
    if (c->ragged) return c->fail(FH_UNSUPPORTED, std::string(who) + ": ragged generic connectivity has no geometry to locate points in");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, std::string(who) + ": no mesh set");
    switch (c->elem_kind) {
        case FH_TRI3: case FH_TET4: basis = PB_LINEAR; return FH_OK;
        case FH_TRI6: basis = PB_TRI6; return FH_OK;
        case FH_TET10: basis = PB_TET10; return FH_OK;
        case FH_TET20: basis = PB_TET20; return FH_OK;
        default:
            return c->fail(FH_UNSUPPORTED, std::string(who) + ": point location is implemented for Tri3, Tri6, Tet4, Tet10 and Tet20 meshes "
                                                               "(the reference has no closest_point for quadrilaterals and hexahedra)");
    }
}

int build_index(fh_ctx* c) {
    hipStream_t st = c->stream;
    const int d = c->ei.d, n = c->ei.n;
    const unsigned E = (unsigned)c->E;
    auto r = std::make_unique<PointIndex>();
    r->d = d;
    r->E = E;
    PointGrid& g = r->g;
    for (int a = 0; a < 3; ++a) { g.o[a] = 0.0; g.h[a] = 1.0; g.inv_h[a] = 1.0; g.n[a] = 1; }
    g.slack = 0.0;
    if (E == 0) {
        r->ncell = 1;
        HIP_TRY(c, r->cell_off.alloc(2));
        HIP_TRY(c, hipMemsetAsync(r->cell_off.p, 0, 2 * sizeof(unsigned), st));
        HIP_TRY(c, r->cell_list.alloc(1));
        HIP_TRY(c, r->box.alloc(1));
        HIP_TRY(c, hipStreamSynchronize(st));
        point_index_drop(c);
        c->point_index = r.release();
        return FH_OK;
    }
    // the mesh's box, then the grid: cells of equal edge along the axes with extent, about one cell per two elements
    DevBuf<double> mb;
    HIP_TRY(c, mb.alloc(6));
    dispatch_or_last(int_list<2, 3>{}, d, [&](auto D) {
        hipLaunchKernelGGL(k_point_mesh_box<D()>, dim3(1), dim3(256), 0, st, c->verts.p, c->conn.p, n, E, mb.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    double hb[6];
    HIP_TRY(c, hipMemcpyAsync(hb, mb.p, sizeof(double) * 2 * d, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    double ext[3] = {0, 0, 0}, diam = 0.0, mag = 0.0;
    for (int a = 0; a < d; ++a) {
        if (!std::isfinite(hb[a]) || !std::isfinite(hb[d + a])) return c->fail(FH_BAD_ARGUMENT, "fh_point_index_build: the mesh has a non-finite vertex coordinate");
        ext[a] = hb[d + a] - hb[a];
        diam = std::max(diam, ext[a]);
        mag = std::max(mag, std::max(std::fabs(hb[a]), std::fabs(hb[d + a])));
    }
    const double pad = 0x1p-48 * std::max(diam, mag);   // a few thousand ulps of the coordinates
    int live = 0;
    double vol = 1.0;
    for (int a = 0; a < d; ++a)
        if (ext[a] > 0.0) { ++live; vol *= ext[a]; }
    const double target = std::max(1.0, 0.5 * (double)E);
    const double edge = live ? std::pow(vol / target, 1.0 / live) : 1.0;
    unsigned long long ncell = 1;
    for (int a = 0; a < d; ++a) {
        const double margin = 0.005 * ext[a] + 2.0 * pad;
        g.o[a] = hb[a] - margin;
        const double len = ext[a] + 2.0 * margin;
        double cells = (ext[a] > 0.0 && edge > 0.0) ? std::floor(ext[a] / edge + 0.5) : 1.0;
        cells = std::min(std::max(cells, 1.0), 1024.0);
        g.n[a] = (int)cells;
        g.h[a] = len > 0.0 ? len / cells : 1.0;
        g.inv_h[a] = 1.0 / g.h[a];
        ncell *= (unsigned long long)g.n[a];
    }
    g.slack = 0x1p-40 * std::max(diam, mag);
    r->ncell = (unsigned)ncell;   // <= 1024^3
    HIP_TRY(c, r->box.alloc((size_t)E * 2 * d));
    DevBuf<unsigned> count, first;
    HIP_TRY(c, count.alloc((size_t)E + 1));
    HIP_TRY(c, first.alloc((size_t)E + 1));
    const int eg = point_grid_for(E);
    HIP_TRY(c, hipMemsetAsync(count.p + E, 0, sizeof(unsigned), st));
    dispatch_or_last(int_list<2, 3>{}, d, [&](auto D) {
        hipLaunchKernelGGL(k_point_boxes<D()>, dim3(eg), dim3(256), 0, st, c->verts.p, c->conn.p, n, E, pad, r->box.p);
        hipLaunchKernelGGL(k_point_cell_counts<D()>, dim3(eg), dim3(256), 0, st, r->box.p, E, g, count.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    // the total in 64 bits, read back before anything is sized by it
    DevBuf<unsigned long long> wide;
    HIP_TRY(c, wide.alloc(1));
    size_t scan_bytes = 0, sum_bytes = 0, sort_bytes = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, count.p, first.p, (int)E + 1, st));
    HIP_TRY(c, hipcub::DeviceReduce::Sum(nullptr, sum_bytes, hipcub::TransformInputIterator<unsigned long long, WidenCount, unsigned*>(count.p, WidenCount{}),
                                         wide.p, (int)E, st));
    DevBuf<char> tmp;
    HIP_TRY(c, tmp.alloc(std::max(scan_bytes, sum_bytes)));
    HIP_TRY(c, hipcub::DeviceReduce::Sum(tmp.p, sum_bytes, hipcub::TransformInputIterator<unsigned long long, WidenCount, unsigned*>(count.p, WidenCount{}),
                                         wide.p, (int)E, st));
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, wide.p, sizeof total, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (total >= (1ull << 31))
        return c->fail(FH_UNSUPPORTED, "fh_point_index_build: the element boxes overlap 2^31 cells or more (elements that span the mesh?)");
    r->total = (unsigned)total;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, scan_bytes, count.p, first.p, (int)E + 1, st));
    DevBuf<unsigned long long> keys_in, keys;
    HIP_TRY(c, keys_in.alloc((size_t)total));
    HIP_TRY(c, keys.alloc((size_t)total));
    int bits = 1;
    while ((1ull << bits) < ncell) ++bits;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, keys_in.p, keys.p, (int)total, 0, 32 + bits, st));
    DevBuf<char> sort_tmp;
    HIP_TRY(c, sort_tmp.alloc(sort_bytes));
    dispatch_or_last(int_list<2, 3>{}, d, [&](auto D) {
        hipLaunchKernelGGL(k_point_cell_keys<D()>, dim3(eg), dim3(256), 0, st, r->box.p, E, g, first.p, keys_in.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceRadixSort::SortKeys(sort_tmp.p, sort_bytes, keys_in.p, keys.p, (int)total, 0, 32 + bits, st));
    HIP_TRY(c, r->cell_off.alloc((size_t)ncell + 1));
    HIP_TRY(c, r->cell_list.alloc((size_t)total));
    hipLaunchKernelGGL(k_point_cell_lists, dim3(point_grid_for(std::max<unsigned long long>(total, ncell + 1))), dim3(256), 0, st, keys.p,
                       (unsigned)total, (unsigned)ncell, r->cell_off.p, r->cell_list.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));   // the scratch is released on return
    point_index_drop(c);
    c->point_index = r.release();
    c->last_kernel = "k_point_mesh_box + k_point_boxes + k_point_cell_counts + scan + k_point_cell_keys + radix sort + k_point_cell_lists";
    return FH_OK;
}

int ensure_index(fh_ctx* c) { return c->point_index ? (int)FH_OK : build_index(c); }

// element, xi, in_element of m device points (all device pointers; in_element may not be null here)
int locate_dev(fh_ctx* c, const double* points, uint64_t m, unsigned long long* element, double* xi, unsigned char* in_element) {
    if (!m) return FH_OK;
    const PointIndex* r = c->point_index;
    dispatch_or_last(int_list<2, 3>{}, c->ei.d, [&](auto D) {
        hipLaunchKernelGGL(k_locate_points<D()>, dim3(point_grid_for(m)), dim3(256), 0, c->stream, c->verts.p, c->conn.p, c->ei.n, r->box.p,
                           r->cell_off.p, r->cell_list.p, r->g, points, (unsigned long long)m, element, xi, in_element);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_locate_points";
    return FH_OK;
}

int check_finite(fh_ctx* c, const char* who, const double* points, uint64_t count) {
    for (uint64_t k = 0; k < count; ++k)
        if (!std::isfinite(points[k])) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": non-finite point coordinate");
    return FH_OK;
}

int create_dev(fh_ctx* c, const char* who, const double* points_dev, uint64_t m, int what, fh_interpolator** out) {
    int basis = 0;
    int rc = points_supported(c, who, basis);
    if (rc) return rc;
    if (!out || (m && !points_dev)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null pointer");
    if (what != FH_INTERP_BOTH && what != FH_INTERP_VALUES && what != FH_INTERP_GRADIENTS)
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": what must be FH_INTERP_BOTH, FH_INTERP_VALUES or FH_INTERP_GRADIENTS");
    const int d = c->ei.d, n = c->ei.n;
    if (m >= (1ull << 40) / (uint64_t)n) return c->fail(FH_UNSUPPORTED, std::string(who) + ": too many points");
    rc = ensure_index(c);
    if (rc) return rc;
    auto ip = std::make_unique<fh_interpolator>();
    ip->device = c->device;
    ip->stream = c->stream;
    ip->d = d;
    ip->m = m;
    ip->nnz = m * (uint64_t)n;
    ip->has_values = what != FH_INTERP_GRADIENTS;
    ip->has_gradients = what != FH_INTERP_VALUES;
    ip->has_max = m > 0 && c->N > 0;
    ip->max_node = c->N ? c->N - 1 : 0;   // the mesh's last node: u holds the whole field
    HIP_TRY(c, ip->offsets.alloc((size_t)m + 1));
    HIP_TRY(c, ip->indices.alloc((size_t)ip->nnz));
    if (ip->has_values) HIP_TRY(c, ip->values.alloc((size_t)ip->nnz));
    if (ip->has_gradients) HIP_TRY(c, ip->gradients.alloc((size_t)ip->nnz * d));
    DevBuf<unsigned long long> elem;
    DevBuf<double> xi;
    DevBuf<unsigned char> in;
    HIP_TRY(c, elem.alloc((size_t)m));
    HIP_TRY(c, xi.alloc((size_t)m * d));
    HIP_TRY(c, in.alloc((size_t)m));
    rc = locate_dev(c, points_dev, m, elem.p, xi.p, in.p);
    if (rc) return rc;
    dispatch_or_last(int_list<2, 3>{}, d, [&](auto D) {
        hipLaunchKernelGGL(k_interpolator_build<D()>, dim3(point_grid_for(m + 1)), dim3(256), 0, c->stream, c->verts.p, c->conn.p, n, basis, elem.p,
                           xi.p, (unsigned long long)m, ip->offsets.p, ip->indices.p, ip->has_values ? ip->values.p : nullptr,
                           ip->has_gradients ? ip->gradients.p : nullptr);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // the located elements are released on return
    c->last_kernel = "k_locate_points + k_interpolator_build";
    *out = ip.release();
    return FH_OK;
}

int apply_checks(fh_interpolator* ip, const char* who, uint32_t sdim, const double* u, uint64_t u_len, const double* out, bool gradients) {
    if (gradients ? !ip->has_gradients : !ip->has_values)
        return ip->fail(FH_INVALID_STATE, std::string(who) + (gradients ? ": the interpolator holds no gradients" : ": the interpolator holds no values"));
    if (sdim == 0 || sdim > 64) return ip->fail(FH_BAD_ARGUMENT, std::string(who) + ": sdim must be in 1 .. 64");
    if (ip->has_max && (ip->max_node + 1) * (uint64_t)sdim > u_len)
        return ip->fail(FH_BAD_ARGUMENT, std::string(who) + ": u is shorter than sdim * (largest node index + 1)");
    if ((ip->m && !out) || (ip->has_max && !u)) return ip->fail(FH_BAD_ARGUMENT, std::string(who) + ": null pointer");
    return FH_OK;
}

int apply_dev(fh_interpolator* ip, uint32_t sdim, const double* u, double* out, bool gradients) {
    if (!ip->m) return FH_OK;
    const int grid = point_grid_for(ip->m * (uint64_t)sdim);
    if (!gradients)
        hipLaunchKernelGGL(k_interpolator_apply, dim3(grid), dim3(256), 0, ip->stream, ip->offsets.p, ip->indices.p, ip->values.p,
                           (unsigned long long)ip->m, (int)sdim, u, out);
    else
        dispatch_or_last(int_list<1, 2, 3>{}, ip->d, [&](auto D) {
            hipLaunchKernelGGL(k_interpolator_apply_gradients<D()>, dim3(grid), dim3(256), 0, ip->stream, ip->offsets.p, ip->indices.p,
                               ip->gradients.p, (unsigned long long)ip->m, (int)sdim, u, out);
            return 0;
        });
    HIP_TRY(ip, hipGetLastError());
    return FH_OK;
}

int apply_host(fh_interpolator* ip, const char* who, uint32_t sdim, const double* u, uint64_t u_len, double* out, bool gradients) {
    DevGuard dev_guard_(ip->device);
    int rc = apply_checks(ip, who, sdim, u, u_len, out, gradients);
    if (rc || !ip->m) return rc;
    const size_t out_len = (size_t)ip->m * sdim * (gradients ? ip->d : 1);
    DevBuf<double> du, dout;
    HIP_TRY(ip, du.alloc((size_t)u_len));
    HIP_TRY(ip, dout.alloc(out_len));
    if (u_len) HIP_TRY(ip, hipMemcpyAsync(du.p, u, sizeof(double) * u_len, hipMemcpyHostToDevice, ip->stream));
    rc = apply_dev(ip, sdim, du.p, dout.p, gradients);
    if (rc) return rc;
    HIP_TRY(ip, hipMemcpyAsync(out, dout.p, sizeof(double) * out_len, hipMemcpyDeviceToHost, ip->stream));
    HIP_TRY(ip, hipStreamSynchronize(ip->stream));
    return FH_OK;
}

}  // namespace

extern "C" {

int fh_point_index_build(fh_ctx* c) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int basis = 0;
    int rc = points_supported(c, "fh_point_index_build", basis);
    return rc ? rc : build_index(c);
}

int fh_locate_points_dev(fh_ctx* c, const double* points, uint64_t m, uint64_t* element, double* xi, uint8_t* in_element) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int basis = 0;
    int rc = points_supported(c, "fh_locate_points_dev", basis);
    if (rc) return rc;
    if (m && (!points || !element || !xi)) return c->fail(FH_BAD_ARGUMENT, "fh_locate_points_dev: null pointer");
    rc = ensure_index(c);
    if (rc || !m) return rc;
    DevBuf<unsigned char> in;
    if (!in_element) HIP_TRY(c, in.alloc((size_t)m));
    rc = locate_dev(c, points, m, reinterpret_cast<unsigned long long*>(element), xi, in_element ? in_element : in.p);
    if (rc) return rc;
    if (!in_element) HIP_TRY(c, hipStreamSynchronize(c->stream));   // (its scratch is released on return)
    return FH_OK;
}

int fh_locate_points(fh_ctx* c, const double* points, uint64_t m, uint64_t* element, double* xi, uint8_t* in_element) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int basis = 0;
    int rc = points_supported(c, "fh_locate_points", basis);
    if (rc) return rc;
    if (m && (!points || !element || !xi)) return c->fail(FH_BAD_ARGUMENT, "fh_locate_points: null pointer");
    const int d = c->ei.d;
    rc = check_finite(c, "fh_locate_points", points, m * d);
    if (rc) return rc;
    rc = ensure_index(c);
    if (rc || !m) return rc;
    DevBuf<double> dp, dxi;
    DevBuf<unsigned long long> de;
    DevBuf<unsigned char> din;
    HIP_TRY(c, dp.alloc((size_t)m * d));
    HIP_TRY(c, dxi.alloc((size_t)m * d));
    HIP_TRY(c, de.alloc((size_t)m));
    HIP_TRY(c, din.alloc((size_t)m));
    HIP_TRY(c, hipMemcpyAsync(dp.p, points, sizeof(double) * m * d, hipMemcpyHostToDevice, c->stream));
    rc = locate_dev(c, dp.p, m, de.p, dxi.p, din.p);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(element, de.p, sizeof(uint64_t) * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(xi, dxi.p, sizeof(double) * m * d, hipMemcpyDeviceToHost, c->stream));
    if (in_element) HIP_TRY(c, hipMemcpyAsync(in_element, din.p, m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_interpolator_create_dev(fh_ctx* c, const double* points, uint64_t m, int what, fh_interpolator** out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return create_dev(c, "fh_interpolator_create_dev", points, m, what, out);
}

int fh_interpolator_create(fh_ctx* c, const double* points, uint64_t m, int what, fh_interpolator** out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int basis = 0;
    int rc = points_supported(c, "fh_interpolator_create", basis);
    if (rc) return rc;
    if (m && !points) return c->fail(FH_BAD_ARGUMENT, "fh_interpolator_create: null pointer");
    const int d = c->ei.d;
    rc = check_finite(c, "fh_interpolator_create", points, m * d);
    if (rc) return rc;
    DevBuf<double> dp;
    HIP_TRY(c, dp.alloc((size_t)m * d));
    if (m) HIP_TRY(c, hipMemcpyAsync(dp.p, points, sizeof(double) * m * d, hipMemcpyHostToDevice, c->stream));
    return create_dev(c, "fh_interpolator_create", dp.p, m, what, out);
}

int fh_interpolator_from_compressed(fh_ctx* c, uint32_t d, uint64_t m, const uint64_t* offsets, const uint64_t* indices, uint64_t num_indices,
                                    const double* values, uint64_t num_values, const double* gradients, uint64_t num_gradients,
                                    fh_interpolator** out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_interpolator_from_compressed";
    if (!out || !offsets || (num_indices && !indices)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null pointer");
    if (d < 1 || d > 3) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the geometry dimension must be 1, 2 or 3");
    // the assertions of FixedInterpolator::from_compressed_values (fixed_interpolator.rs:207-230); rows may differ in length or be empty
    for (uint64_t i = 0; i <= m; ++i) {
        if (offsets[i] > num_indices)
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": supported node offsets must be in bounds with respect to supported nodes");
        if (i && offsets[i] < offsets[i - 1]) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": supported node offsets must not decrease");
    }
    if (values && num_values != num_indices)
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": number of node values and indices must be the same");
    if (gradients) {
        if (num_indices == 0 ? num_gradients != 0 : num_gradients % num_indices != 0)
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": number of gradient values must be compatible with number of indices");
        if (num_gradients != num_indices * d)
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the gradients hold d values per index");
    }
    auto ip = std::make_unique<fh_interpolator>();
    ip->device = c->device;
    ip->stream = c->stream;
    ip->d = (int)d;
    ip->m = m;
    ip->nnz = num_indices;
    ip->has_values = values != nullptr;
    ip->has_gradients = gradients != nullptr;
    ip->has_max = num_indices > 0;
    for (uint64_t k = 0; k < num_indices; ++k) ip->max_node = std::max(ip->max_node, indices[k]);
    HIP_TRY(c, ip->offsets.alloc((size_t)m + 1));
    HIP_TRY(c, ip->indices.alloc((size_t)num_indices));
    HIP_TRY(c, hipMemcpyAsync(ip->offsets.p, offsets, sizeof(uint64_t) * (m + 1), hipMemcpyHostToDevice, c->stream));
    if (num_indices) HIP_TRY(c, hipMemcpyAsync(ip->indices.p, indices, sizeof(uint64_t) * num_indices, hipMemcpyHostToDevice, c->stream));
    if (values) {
        HIP_TRY(c, ip->values.alloc((size_t)num_indices));
        if (num_indices) HIP_TRY(c, hipMemcpyAsync(ip->values.p, values, sizeof(double) * num_indices, hipMemcpyHostToDevice, c->stream));
    }
    if (gradients) {
        HIP_TRY(c, ip->gradients.alloc((size_t)num_gradients));
        if (num_gradients) HIP_TRY(c, hipMemcpyAsync(ip->gradients.p, gradients, sizeof(double) * num_gradients, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *out = ip.release();
    return FH_OK;
}

void fh_interpolator_destroy(fh_interpolator* ip) {
    if (!ip) return;
    DevGuard dev_guard_(ip->device);
    delete ip;
}

const char* fh_interpolator_last_error(const fh_interpolator* ip) { return ip ? ip->err.c_str() : "null interpolator"; }

int fh_interpolator_sizes(const fh_interpolator* ip, uint64_t* num_points, uint64_t* num_indices, uint32_t* geometry_dim, int* has_values,
                          int* has_gradients) {
    if (!ip) return FH_BAD_ARGUMENT;
    if (num_points) *num_points = ip->m;
    if (num_indices) *num_indices = ip->nnz;
    if (geometry_dim) *geometry_dim = (uint32_t)ip->d;
    if (has_values) *has_values = ip->has_values ? 1 : 0;
    if (has_gradients) *has_gradients = ip->has_gradients ? 1 : 0;
    return FH_OK;
}

int fh_interpolator_data(fh_interpolator* ip, uint64_t* offsets, uint64_t* indices, double* values, double* gradients) {
    if (!ip) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(ip->device);
    if ((values && !ip->has_values) || (gradients && !ip->has_gradients))
        return ip->fail(FH_INVALID_STATE, "fh_interpolator_data: the interpolator does not hold what was asked for");
    if (offsets) HIP_TRY(ip, hipMemcpyAsync(offsets, ip->offsets.p, sizeof(uint64_t) * (ip->m + 1), hipMemcpyDeviceToHost, ip->stream));
    if (indices && ip->nnz) HIP_TRY(ip, hipMemcpyAsync(indices, ip->indices.p, sizeof(uint64_t) * ip->nnz, hipMemcpyDeviceToHost, ip->stream));
    if (values && ip->nnz) HIP_TRY(ip, hipMemcpyAsync(values, ip->values.p, sizeof(double) * ip->nnz, hipMemcpyDeviceToHost, ip->stream));
    if (gradients && ip->nnz)
        HIP_TRY(ip, hipMemcpyAsync(gradients, ip->gradients.p, sizeof(double) * ip->nnz * ip->d, hipMemcpyDeviceToHost, ip->stream));
    HIP_TRY(ip, hipStreamSynchronize(ip->stream));
    return FH_OK;
}

int fh_interpolator_apply(fh_interpolator* ip, uint32_t sdim, const double* u, uint64_t u_len, double* out) {
    if (!ip) return FH_BAD_ARGUMENT;
    return apply_host(ip, "fh_interpolator_apply", sdim, u, u_len, out, false);
}

int fh_interpolator_apply_gradients(fh_interpolator* ip, uint32_t sdim, const double* u, uint64_t u_len, double* out) {
    if (!ip) return FH_BAD_ARGUMENT;
    return apply_host(ip, "fh_interpolator_apply_gradients", sdim, u, u_len, out, true);
}

int fh_interpolator_apply_dev(fh_interpolator* ip, uint32_t sdim, const double* u, uint64_t u_len, double* out) {
    if (!ip) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(ip->device);
    int rc = apply_checks(ip, "fh_interpolator_apply_dev", sdim, u, u_len, out, false);
    return rc ? rc : apply_dev(ip, sdim, u, out, false);
}

int fh_interpolator_apply_gradients_dev(fh_interpolator* ip, uint32_t sdim, const double* u, uint64_t u_len, double* out) {
    if (!ip) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(ip->device);
    int rc = apply_checks(ip, "fh_interpolator_apply_gradients_dev", sdim, u, u_len, out, true);
    return rc ? rc : apply_dev(ip, sdim, u, out, true);
}

}  // extern "C"
