// The regular lattice X(i, j, k) = ((origin + i du) + j dv) + k dw of shape (nu, nv, nw), k fastest, g = (i nv + j) nw + k, that
// field, mesh, parts, tsdf and closest work on: the one place its index, its point rule, the edges a point owns,
// the usable-point rule and the shape refusal are written; plain fp32 in the order written.  Internal.
#pragma once
#include "durf_common.h"

// passed to kernels by value
struct LatticeDims { int nu, nv, nw, n; };
struct LatticeFrame { float o[3], du[3], dv[3], dw[3]; };

inline LatticeFrame lattice_frame(const float* origin_host, const float* du_host, const float* dv_host, const float* dw_host) {
    LatticeFrame F;
    for (int c = 0; c < 3; c++) { F.o[c] = origin_host[c]; F.du[c] = du_host[c]; F.dv[c] = dv_host[c]; F.dw[c] = dw_host[c]; }
    return F;
}

__device__ __forceinline__ void lattice_ijk(const LatticeDims& D, int g, int& i, int& j, int& k) {
    const int r = g / D.nw;
    k = g % D.nw, j = r % D.nv, i = r / D.nv;
}
__device__ __forceinline__ int lattice_index(const LatticeDims& D, int i, int j, int k) { return (i * D.nv + j) * D.nw + k; }

// the point at the (fractional) lattice coordinates (fi, fj, fk)
__device__ __forceinline__ void lattice_point(const LatticeFrame& F, float fi, float fj, float fk, float* P) {
#pragma unroll
    for (int c = 0; c < 3; c++) P[c] = ((F.o[c] + fi * F.du[c]) + fj * F.dv[c]) + fk * F.dw[c];
}

// corner c = 4 di + 2 dj + dk of the cell at a point, and how far away in g it is; edge e = 0 .. 6 of the point (the Kuhn
// numbering of include/durf_mesh.h) ends at corner e + 1
__device__ __forceinline__ void lattice_corner(int c, int& di, int& dj, int& dk) { di = c >> 2, dj = c >> 1 & 1, dk = c & 1; }
__device__ __forceinline__ void lattice_edge(int e, int& di, int& dj, int& dk) { lattice_corner(e + 1, di, dj, dk); }
__device__ __forceinline__ int lattice_corner_offset(const LatticeDims& D, int c) { return lattice_index(D, c >> 2, c >> 1 & 1, c & 1); }
__device__ __forceinline__ int lattice_edge_offset(const LatticeDims& D, int e) { return lattice_corner_offset(D, e + 1); }

// a point takes part when its valid byte (if there is a map) is set and its density is a number; *d: the density
__device__ __forceinline__ bool lattice_usable(const float* __restrict__ density, const uint8_t* __restrict__ valid, int g, float* d) {
    const float x = density[g];
    *d = x;
    return (valid == nullptr || valid[g] != 0) && x == x;
}

// what mesh, parts and tsdf take: every dimension >= 2, fewer than max_points (2^27) points; check_: -> n, or -1 with the refusal set
inline bool lattice_cells(int nu, int nv, int nw) { return nu >= 2 && nv >= 2 && nw >= 2; }
inline bool lattice_shape_ok(int nu, int nv, int nw, int max_points) { return lattice_cells(nu, nv, nw) && (double)nu * nv * nw < (double)max_points; }
inline int check_lattice_shape(const char* who, int nu, int nv, int nw, int max_points) {
    if (lattice_shape_ok(nu, nv, nw, max_points)) return nu * nv * nw;
    if (!lattice_cells(nu, nv, nw)) durf_set_error("%s: requirement failed: nu, nv, nw >= 2, nu = %d, nv = %d, nw = %d", who, nu, nv, nw);
    else durf_set_error("%s: requirement failed: nu nv nw < 2^27 lattice points, %d x %d x %d", who, nu, nv, nw);
    return -1;
}
