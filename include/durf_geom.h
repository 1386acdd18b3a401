/* C ABI of durf_amd/libdurf_geom.so: how far two unordered point sets lie from each other, on the device -- the nearest point
 * within a radius over a cell-sorted set, the deterministic statistics of the distances (accuracy, completeness, Chamfer,
 * precision / recall at thresholds are sums of them) and area-uniform samples of a triangle mesh, so that a surface
 * (include/durf_mesh.h) can be held against a cloud (include/durf_lidar.h, a back-projected depth map).  A library of its own
 * beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs that library for
 * durf_last_error alone and takes plain arrays.  The house rules of durf_hip.h hold: device pointers of caller-owned buffers
 * unless marked HOST, asynchronous on `stream` (hipStream_t), 0 or nonzero with the text in durf_last_error(), every argument
 * checked before anything is launched, no stream synchronisation and no device-to-host copy anywhere.  No atomics: the same
 * inputs give the same bits.  fp32 arithmetic is unfused, in the order written here; float64 where it says so.
 *
 * Grid.  origin [3] HOST, inv_cell, (nx, ny, nz), each 1 .. DURF_GEOM_MAX_CELLS.  The cell of a point x, per axis:
 *   t = (x - origin) * inv_cell (two fp32 roundings), c = floorf(t).  A point is IN the grid when 0 <= c < n on every axis
 *   (a NaN or infinite coordinate, or t, never is); its key is then (int64) ((cx ny) + cy) nz + cz, else -1.
 * Reference set.  ref_sorted [m,3], ref_keys [m] int64, ref_index [m] int32: the points in ascending order of their keys
 *   (the caller sorts: a stable sort of durf_geom_keys' output and a gather), their keys, and the index each had before.
 *   No dense cell table exists: the run of a cell is found by binary search (lower bound) in ref_keys, so any grid within
 *   the limit works and nothing is counted with atomics.  Keys of -1 sort first and are never reached.
 * Search.  The query's cell (cx, cy, cz) as above.  A query with a coordinate, or t, that is not finite, or with c < -1 or
 *   c > n on any axis (more than one cell outside) is UNUSABLE: dist = NaN, index = -2.  Otherwise, for a = -1, 0, 1 (outer)
 *   and b = -1, 0, 1 (inner) with 0 <= cx + a < nx and 0 <= cy + b < ny, the keys of cells (cx + a, cy + b, zlo .. zhi),
 *   zlo = max(cz - 1, 0), zhi = min(cz + 1, nz - 1), are one contiguous range [lower_bound(key(zlo)), lower_bound(key(zhi) + 1))
 *   of ref_keys; every point in it is a candidate.
 * Distance.  dx = qx - rx, dy = qy - ry, dz = qz - rz;  d2 = (dx dx + dy dy) + dz dz.
 * Acceptance.  A candidate COUNTS when d2 <= md2, md2 = max_dist * max_dist computed once on the host in fp32; the comparison
 *   is exact.  The winner has the smallest d2; among equal d2 the smallest ref_index.  (The result is therefore independent of
 *   the order within a cell and of the order of the queries.)  dist = sqrtf(d2), index = ref_index of the winner; when no
 *   candidate counts dist = max_dist and index = -1.
 *
 * Grid rule (the caller builds the grid so, durf_geom_nearest refuses one that is not):
 *   cell = max_dist (1 + 2^-10) in float64, inv_cell = (float) (1 / cell): refused unless
 *   (double) inv_cell * max_dist * (1 + 2^-10) <= 1 + 2^-22;  1e-18 <= max_dist <= 1e18 (md2 is a normal fp32 number);
 *   origin = the per-axis minimum of the reference points' finite coordinates; n = floorf(t(maximum)) + 1 on every axis, so
 *   every finite reference point is in the grid (t is monotone in x); at most DURF_GEOM_MAX_CELLS = 2048 cells per axis.
 * What the rule guarantees: a reference point r in the grid that counts for a usable query q lies in q's 27 cells AS
 *   COMPUTED, so the search above equals the brute-force search over all m points, bit for bit.  Proof, per axis, with
 *   e = 2^-24 and fdx = fl(qx - rx):  d2 >= fl(fdx^2) (adding non-negative terms and rounding are monotone), so
 *   fl(fdx^2) <= fl(max_dist^2), that is fdx^2 (1 - e) <= max_dist^2 (1 + e) and |fdx| < max_dist (1 + 2e); with
 *   |qx - rx| <= |fdx| / (1 - e):  |qx - rx| < max_dist (1 + 2^-21).  With u(x) = (x - origin) inv_cell in real arithmetic,
 *   |u(q) - u(r)| < max_dist inv_cell (1 + 2^-21) <= (1 + 2^-22) (1 + 2^-21) / (1 + 2^-10) < 1 - 2^-10 + 2^-19.  The computed
 *   t = u (1 + d1) (1 + d2), |d| <= e, and |u| < 2050 for a point in the grid or one cell outside, so
 *   |t - u| < 2050 * 2^-23 (1 + e) < 2^-12 (1 + 2^-9).  Therefore |t(q) - t(r)| < 1 - 2^-10 + 2^-19 + 2^-11 (1 + 2^-9)
 *   < 1 - 2^-12 < 1, and two numbers less than 1 apart have floors at most 1 apart.  (The margin 2^-10 is what the limit of
 *   2^11 cells needs: the two computed coordinates together err by almost 2^-11; 4096 cells would need 2^-9.)
 *
 * Statistics.  Row of DURF_GEOM_STAT_DOUBLES float64, over the q queries (USABLE: index != -2; FOUND: index >= 0):
 *   [0] usable  [1] found  [2] sum of dist over found  [3] sum of dist dist (in float64) over found  [4] sum of dist over
 *   usable (a query that found nothing holds max_dist: the truncated mean)  [5 + k] usable with index >= 0 and
 *   dist <= thresholds[k] (an exact fp32 comparison), k < n_thresholds; the rest 0.
 *   Order: workgroup w sums queries [w B, (w + 1) B), B = DURF_GEOM_STAT_CHUNK: thread j of DURF_GEOM_BLOCK adds j, j + 256, ...
 *   in turn, then the workgroup folds its 256 values pairwise (stride 128, 64, ... 1); ONE workgroup adds the partials the same
 *   way (thread j: partials j, j + 256, ...).  Fixed by q alone: two runs give the same bits.
 *
 * Mesh samples.  vertices [V,3], triangles [T,3] int32.  area_i = 0.5f * sqrtf((cx cx + cy cy) + cz cz), c the cross product
 *   of e1 = b - a and e2 = c - a (cx = e1y e2z - e1z e2y, cy = e1z e2x - e1x e2z, cz = e1x e2y - e1y e2x), fp32; a triangle
 *   with an index outside [0, V) or an area that is not finite has area 0.  cum_i: the inclusive prefix sum of the areas in
 *   float64, by the three passes of durf_mesh_count (block sums, one workgroup over them, offsets); its additions are ordered
 *   as a tree, so cum agrees with a sequential sum to float64 rounding (exactly, where the areas' sums are exact).
 *   total = the scan's own sum of the block sums (cum_{T-1} to float64 rounding).
 *   Sample s of n:  target = ((s + 0.5) * total) / n in float64; triangle = the first i with cum_i > target; u = frac(0.5 + s * 0.7548776662466927), v = frac(0.5 + s * 0.5698402909980532) in float64
 *   (frac x = x - floor x; the R2 sequence), (u, v) -> (1 - u, 1 - v) when u + v > 1, then cast to fp32;
 *   point = a + (u (b - a) + v (c - a)) per component.  total == 0 (or T == 0): n rows of NaN with id -1. */
#ifndef DURF_GEOM_H
#define DURF_GEOM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_GEOM_BLOCK 256          /* threads per workgroup, and points per block sum of the area scan */
#define DURF_GEOM_STAT_CHUNK 1024    /* queries per workgroup of the statistics */
#define DURF_GEOM_MAX_CELLS 2048     /* per axis */
#define DURF_GEOM_MAX_THRESHOLDS 8
#define DURF_GEOM_STAT_DOUBLES 13    /* 5 + DURF_GEOM_MAX_THRESHOLDS */

/* The workspace of durf_geom_stats over n_queries and of durf_geom_sample_mesh over n_triangles (either may be 0), every part
 * on a 256-byte boundary in this order: the partials, float64 [ceil(n_queries / DURF_GEOM_STAT_CHUNK), DURF_GEOM_STAT_DOUBLES];
 * cum, float64 [n_triangles]; the scan's block sums, float64 [ceil(n_triangles / DURF_GEOM_BLOCK) + 1].  durf_geom_stats checks
 * against (q, 0) and durf_geom_sample_mesh against (0, n_triangles).  0 for a negative count. */
size_t durf_geom_workspace_bytes(int n_queries, int n_triangles);

/* ---- cell keys (k_geom_keys) ---------------------------------------------------------------------------------------------
 * One thread per point: keys [n] int64 as above.
 * Refused: n < 0, NULL points or keys with n > 0, a NULL origin, a dimension outside 1 .. DURF_GEOM_MAX_CELLS, an inv_cell
 * that is not a positive finite number. */
int durf_geom_keys(void* stream, int n, const float* points, const float* origin_host /* 3 */, float inv_cell, int nx, int ny, int nz,
                   int64_t* keys);

/* ---- nearest point within max_dist (k_geom_nearest) ------------------------------------------------------------------------
 * One thread per query: dist [q], index [q] int32 as above.  m = 0 is an empty reference set (nothing is found).
 * Refused: q < 0 or m < 0, NULL query, dist or index with q > 0, a NULL reference array with m > 0, a NULL origin, a dimension
 * outside 1 .. DURF_GEOM_MAX_CELLS ("at most 2048 cells per axis"), max_dist that is NaN or outside [1e-18, 1e18], an
 * inv_cell that breaks the grid rule (both numbers named). */
int durf_geom_nearest(void* stream, int q, const float* query, int m, const float* ref_sorted, const int64_t* ref_keys,
                      const int32_t* ref_index, const float* origin_host /* 3 */, float inv_cell, int nx, int ny, int nz, float max_dist,
                      float* dist, int32_t* index);

/* ---- statistics (k_geom_stats_partial, k_geom_stats_final) --------------------------------------------------------------------
 * stats [DURF_GEOM_STAT_DOUBLES] float64 on the device.  q = 0 gives a row of zeros (one launch).
 * Refused: q < 0, NULL dist or index with q > 0, n_thresholds outside 0 .. 8, NULL thresholds with n_thresholds > 0, a NaN
 * threshold, NULL stats, a NULL or misaligned (256 bytes) workspace, one smaller than durf_geom_workspace_bytes(q, 0). */
int durf_geom_stats(void* stream, int q, const float* dist, const int32_t* index, int n_thresholds, const float* thresholds_host,
                    void* workspace, size_t workspace_bytes, double* stats);

/* ---- points on a mesh (k_geom_areas, k_geom_scan, k_geom_offsets, k_geom_sample) ------------------------------------------
 * points [n,3], tri [n] int32 (the triangle each sample lies on: the caller carries normals, colours or the owner label by
 * it), total_area [1] float64 on the device.
 * Refused: n, n_vertices or n_triangles < 0, NULL vertices with n_vertices > 0, NULL triangles with n_triangles > 0, NULL
 * points or tri with n > 0, NULL total_area, a NULL or misaligned workspace, one smaller than
 * durf_geom_workspace_bytes(0, n_triangles). */
int durf_geom_sample_mesh(void* stream, int n_vertices, const float* vertices, int n_triangles, const int32_t* triangles, int n,
                          void* workspace, size_t workspace_bytes, float* points, int32_t* tri, double* total_area);

#ifdef __cplusplus
}
#endif
#endif
