/* C ABI of durf_amd/libdurf_mesh.so: the iso-surface of a density lattice as an indexed triangle mesh, on the device --
 * marching tetrahedra on the Kuhn (Freudenthal) subdivision of every cell, with welded vertices.  What durf_field_grid
 * (include/durf_field.h) leaves as a volume, this turns into the surface a simulator, a viewer or a collision checker takes.
 * A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs that
 * library for durf_last_error alone and takes plain arrays, so it meshes any volume a caller brings.  The house rules of
 * durf_hip.h hold: device pointers of caller-owned buffers unless marked HOST, asynchronous on `stream` (hipStream_t), 0 or
 * nonzero with the text in durf_last_error(), every argument checked before anything is launched, no stream synchronisation
 * and no device-to-host copy anywhere.  No atomics: the same inputs give the same bits.  All arithmetic is fp32, unfused, in
 * the order written here.
 *
 * Why tetrahedra and not the 256-case cube table: the six tetrahedra of a cell share its body diagonal and the face diagonals
 * of neighbouring cells coincide, so there is no ambiguous case -- the surface is a closed, consistently oriented 2-manifold
 * wherever the lattice is usable -- and the sixteen cases follow from the rule below (csrc/mesh.hip builds them at compile
 * time).  Every vertex lies on a lattice edge owned by exactly one lattice point; it is computed once and shared by index, so
 * watertightness does not depend on rounding.
 *
 * Lattice.  density [nu,nv,nw] float32, valid [nu,nv,nw] uint8 NULLABLE (NULL: all valid); point p = (i, j, k) has index
 *   g = (i nv + j) nw + k (durf_field_grid's order), n = nu nv nw.  p is USABLE when valid != 0 and its density is not NaN; a
 *   usable p is IN when density >= iso (an exact comparison).
 * Edges.  p owns seven edges e = 0 .. 6 towards p + o_e, (di, dj, dk) the bits of e + 1 = 4 di + 2 dj + dk: three axis edges,
 *   three face diagonals, the body diagonal.  An edge EXISTS when p + o_e is inside the lattice and is ACTIVE when both ends
 *   are usable and exactly one of them is in.
 * Vertex ids.  mask[g] holds the seven activity bits (bit e), voff[g] is the exclusive prefix sum of popcount(mask) in g order;
 *   the vertex of edge (g, e) has id voff[g] + popcount(mask[g] & ((1 << e) - 1)).
 * Vertex position.  a = p, b = p + o_e:  t = (iso - d_a) / (d_b - d_a), then fminf(fmaxf(t, 0), 1);
 *   q = ((float) i + t di, (float) j + t dj, (float) k + t dk);  X_c = ((origin_c + q_0 du_c) + q_1 dv_c) + q_2 dw_c
 *   (t = 0: durf_field_grid's own formula).
 * Normals.  The index-space gradient at a lattice point, per axis: 0.5 (d[+1] - d[-1]) when both neighbours exist and are
 *   usable; otherwise the one-sided difference towards the usable neighbour (d[+1] - d[0], or d[0] - d[-1]); otherwise 0.
 *   At a vertex gr = gr_a + t (gr_b - gr_a);  m_c = (A[c][0] gr_0 + A[c][1] gr_1) + A[c][2] gr_2 with A the inverse transpose
 *   of [du dv dw] (nine HOST floats, row-major; the caller computes them in float64);  n = -m / sqrtf((m_0 m_0 + m_1 m_1) +
 *   m_2 m_2).  A zero or non-finite n is written as (0, 0, 0).
 * Cells and tetrahedra.  Cell p exists when i < nu-1, j < nv-1, k < nw-1 and is emitted at its origin g.  Its six tetrahedra
 *   come in the order of the axis permutations (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0); permutation (x, y, z) has
 *   the corners v0 = p, v1 = p + e_x, v2 = p + e_x + e_y, v3 = p + (1,1,1).  A tetrahedron emits only when all four corners
 *   are usable.  (Every edge v_a v_b, a < b, of a tetrahedron is one of the seven edges its lower corner owns.)
 * Triangles.  I the in corners, O the out corners, each sorted by local index 0 .. 3; "xy" is the vertex on edge v_x v_y.
 *   One corner a alone on its side, the others b < c < d:  (ab, ac, ad).
 *   I = {a < b}, O = {c < d}:  the quad ac, ad, bd, bc as (ac, ad, bd) and (ac, bd, bc).
 *   Every triangle is wound so that its right-hand normal points from the in corners to the out corners in a right-handed
 *   frame (det [du dv dw] > 0): a triangle (x, y, z) that is not, is emitted as (x, z, y).  `flip` != 0 reverses every
 *   winding the same way (a left-handed frame).  The winding depends only on the case and the parity of the permutation.
 *   A corner with d == iso gives zero-area triangles; they stay, because the topology must.
 * Triangle order.  toff[g] is the exclusive prefix sum of each cell's triangle count (at most 12): cell order, then
 *   tetrahedron order, then the order above.
 * Holes.  A vertex next to an unusable point may be referenced by no triangle.  That is documented, not repaired. */
#ifndef DURF_MESH_H
#define DURF_MESH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_MESH_BLOCK 256        /* lattice points per workgroup and per block sum */
#define DURF_MESH_MAX_POINTS (1 << 27)

/* The workspace of nu nv nw lattice points, every part on a 256-byte boundary in this order: voff int32 [n], toff int32 [n],
 * mask uint8 [n], then the scan's block sums, int32 [2, nb + 1] with nb = ceil(n / DURF_MESH_BLOCK).  0 for a refused shape. */
size_t durf_mesh_workspace_bytes(int nu, int nv, int nw);

/* ---- classify, count, scan (k_mesh_classify, k_mesh_scan, k_mesh_offsets) -----------------------------------------------
 * One thread per lattice point, adjacent lanes along k: the point's density and its seven forward neighbours give mask[g],
 * the cell's triangle count and the workgroup's two sums; ONE workgroup scans the block sums exclusively, looping over as many
 * as there are; a third pass turns the per-point counts into voff and toff.  counts [2] int32 on the device = (vertices,
 * triangles), the true totals.
 * Refused: nu, nv or nw < 2, n >= 2^27 (7 n and 12 n stay inside int32), NaN iso, a NULL density, workspace (256-byte
 * aligned) or counts, a workspace smaller than durf_mesh_workspace_bytes (both sizes named). */
int durf_mesh_count(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid /* nullable */, float iso,
                    void* workspace, size_t workspace_bytes, int32_t* counts);

/* ---- emit (k_mesh_emit) ---------------------------------------------------------------------------------------------------
 * Reads the workspace as durf_mesh_count left it for the same lattice and iso.  vertices [max_vertices,3]; normals
 * [max_vertices,3] NULLABLE (then normal_xform_host may be NULL); vertex_edge [max_vertices,2] int32 NULLABLE: (g, e) of each
 * vertex; vertex_t [max_vertices] NULLABLE; triangles [max_triangles,3] int32.  Nothing at or past a capacity is written: a
 * vertex row with id >= max_vertices is not, a triangle with index >= max_triangles is not, and a triangle is written whole
 * or not at all (its ids may then name vertices past max_vertices: compare the capacities with `counts`).
 * Refused: the shape as above, NaN iso, a NULL density, workspace, origin or axis, normals without normal_xform_host, negative
 * capacities, NULL vertices with max_vertices > 0, NULL triangles with max_triangles > 0, a small workspace. */
int durf_mesh_emit(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid /* nullable */, float iso,
                   const float* origin_host /* 3 */, const float* du_host /* 3 */, const float* dv_host /* 3 */,
                   const float* dw_host /* 3 */, const float* normal_xform_host /* 9, nullable */, int flip, const void* workspace,
                   size_t workspace_bytes, int max_vertices, int max_triangles, float* vertices, float* normals /* nullable */,
                   int32_t* vertex_edge /* nullable */, float* vertex_t /* nullable */, int32_t* triangles);

/* ---- lattice attributes at the vertices (k_mesh_gather) ---------------------------------------------------------------------
 * For vertex v < min(counts[0], max_vertices) on edge (g, e) = vertex_edge[v] with t = vertex_t[v], a = g, b = g + o_e:
 *   out_f [max_vertices,C] row v = attr_f[a] + t (attr_f[b] - attr_f[a]) per channel (attr_f [n,C] NULLABLE with out_f);
 *   out_i [max_vertices] = attr_i[the IN end of the edge] (attr_i int32 [n] NULLABLE with out_i; density, valid, iso decide
 *   which end is in, and are needed only then): how a vertex learns its owner.
 * A row whose (g, e) does not name an edge of the lattice is skipped.
 * Refused: the shape, max_vertices < 0, NULL counts, vertex_edge or vertex_t, neither attribute, attr_f without out_f or
 * C < 1, attr_i without out_i or density, NaN iso with attr_i. */
int durf_mesh_gather(void* stream, int nu, int nv, int nw, const int32_t* counts, int max_vertices, const int32_t* vertex_edge,
                     const float* vertex_t, int C, const float* attr_f /* nullable */, float* out_f /* nullable */,
                     const int32_t* attr_i /* nullable */, const float* density /* nullable */, const uint8_t* valid /* nullable */,
                     float iso, int32_t* out_i /* nullable */);

#ifdef __cplusplus
}
#endif
#endif
