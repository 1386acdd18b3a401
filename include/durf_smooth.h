/* C ABI of durf_amd/libdurf_smooth.so: which vertices of a triangle mesh are neighbours, whether the mesh is closed and manifold,
 * Laplacian / Taubin smoothing as a deterministic gather over that adjacency, and area-weighted vertex normals of the result.
 * What marching tetrahedra on a lattice leaves is terraced at the lattice's period; every other library takes a mesh as a triangle
 * soup.  A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs
 * that library for durf_last_error alone.  The house rules of durf_hip.h hold: device pointers of caller-owned buffers,
 * asynchronous on `stream` (hipStream_t), 0 or nonzero with the text in durf_last_error(), every argument checked before anything
 * is launched, no stream synchronisation and no device-to-host copy anywhere.  All float arithmetic is fp32, unfused, in the order
 * written here, with IEEE division and sqrtf; subnormals are kept.  The mesh is the one of csrc/triangles.h: vertices [V,3] float32,
 * triangles [T,3] int32.
 *
 * THE DEFINITIONS name no schedule, and every output is an integer or a written-out fp32 expression: a numpy oracle holds the
 * device to every bit (tests/smooth_ref.py).
 *
 * CONTRIBUTING TRIANGLE.  Triangle t = (a, b, c) contributes when each of its indices lies in 0 .. V-1 and a != b, b != c,
 *   c != a.  Coordinates play no part: adjacency is combinatorial.  A triangle that does not contribute is ignored by every
 *   definition below (it is still a triangle of the mesh: nothing here removes it).
 *
 * KEYS.  For a contributing triangle t: edge_keys[6t + 0 .. 5] = key(a,b), key(b,a), key(b,c), key(c,b), key(c,a), key(a,c) with
 *   key(p,q) = ((int64) p << 32) | q, and corner_keys[3t + 0 .. 2] = key(a,t), key(b,t), key(c,t).  A triangle that does not
 *   contribute writes DURF_SMOOTH_NO_KEY = INT64_MAX in all nine places.  The CALLER sorts both arrays ascending (any sort: equal
 *   keys are indistinguishable) and hands them to durf_smooth_adjacency.
 *
 * ADJACENCY (CSR).  Of a sorted key array, the UNIQUE keys below DURF_SMOOTH_NO_KEY in ascending order, each with its
 *   multiplicity (how often it occurs), split by their high word: row v holds the low words of the keys whose high word is v.
 *   Edges:   offsets [V+1]; neighbours[offsets[v] .. offsets[v+1]) the vertices q that share an edge with v, ascending;
 *            multiplicity, alongside: the number of contributing triangles that hold the undirected edge {v,q} (a contributing
 *            triangle writes each direction of each of its edges once).  offsets[V] <= 6T entries are written, none beyond.
 *   Corners: corner_offsets [V+1]; corner_tri[corner_offsets[v] .. corner_offsets[v+1]) the contributing triangles with a corner
 *            at v, ascending (every such key is unique).  corner_offsets[V] <= 3T entries are written, none beyond.
 *
 * VERTEX CLASS (uint8 [V]), from the edge rows:  DURF_SMOOTH_ISOLATED 0: the row is empty;  DURF_SMOOTH_NONMANIFOLD 3: some
 *   multiplicity in the row is > 2;  DURF_SMOOTH_BOUNDARY 2: otherwise, some multiplicity is 1;  DURF_SMOOTH_INTERIOR 1: every
 *   multiplicity is exactly 2.
 *
 * CENSUS (int32 [DURF_SMOOTH_CENSUS_INTS]):  [0 .. 3] the number of vertices of class 0 .. 3;  [4] contributing triangles
 *   (corner_offsets[V] / 3);  [5] undirected edges (offsets[V] / 2);  [6] boundary edges (multiplicity 1);  [7] non-manifold
 *   edges (multiplicity > 2).  An undirected edge {p,q} is counted once, at its entry with q > p.  The mesh is CLOSED when [6]
 *   and [7] are 0; its Euler characteristic is (V - [0]) - [5] + [4].  Both are the host's to derive.
 *
 * ONE SMOOTHING STEP.  in [V,3] -> out [V,3] with a factor in [-1, 1], boundary = DURF_SMOOTH_PIN or DURF_SMOOTH_SLIDE and
 *   fixed (NULLABLE uint8 [V]).  Neighbour j of vertex i (an entry of row i) COUNTS when its three coordinates in `in` are finite
 *   and either class[i] is 1, or class[i] is 2, boundary is DURF_SMOOTH_SLIDE and the entry's multiplicity is 1 (a boundary
 *   vertex slides along the boundary curve).  Vertex i is PINNED -- out_i = in_i bit for bit -- when fixed[i] != 0, a coordinate
 *   of in_i is not finite, class[i] is 0 or 3, class[i] is 2 under DURF_SMOOTH_PIN, or no neighbour counts.  Otherwise, per axis a,
 *   with j1 < j2 < ... < jn the counting neighbours:
 *   1 s = in[j1,a]; then s = s + in[jk,a] for k = 2 .. n, in that order;
 *   2 m = s / (float) n;
 *   3 out[i,a] = in[i,a] + factor * (m - in[i,a])         (the product is rounded before the sum).
 *
 * TAUBIN.  iters >= 0, lambda and mu in [-1, 1].  The sequence of steps is lambda, mu, lambda, mu, ... (2 iters steps), or with
 *   mu == 0 lambda alone (iters steps: plain Laplacian smoothing).  Bit-identical to that sequence of durf_smooth_step calls.  Of S
 *   steps, step k = 0 .. S-1 writes `out` when S - 1 - k is even and `tmp` when it is odd, and reads what step k - 1 wrote (step
 *   0 reads `in`): the last step writes `out` whatever the parity.  S == 0 copies in to out.  tmp is not read or written when S < 2.
 *
 * NORMALS.  normals [V,3]: for vertex v, over corner_tri's row of v in ascending triangle id, a triangle t = (a, b, c) with
 *   vertices (A, B, C), all nine coordinates finite (any other contributes nothing):
 *   1 e1 = B - A;  e2 = C - A  (the triangle's own vertex order, whichever corner v is);
 *   2 N = e1 x e2 in the component order of durf_shade.h's N: area-weighted, and oriented as durf_mesh_emit orients;
 *   3 S_a = N_a of the first such triangle; then S_a = S_a + N_a, in that order, per axis;
 *   4 len2 = (S_0 S_0 + S_1 S_1) + S_2 S_2;
 *   5 the normal is 0 when no triangle contributed, !(len2 > 0) or len2 is not finite;
 *   6 otherwise S * (1.0f / sqrtf(len2)), one division and three products (durf_shade.h's surface rule).
 *
 * The kernels: one thread per triangle (keys), per key (heads, scatter), per vertex (offsets, class, census, step, normals),
 *   workgroups of DURF_SMOOTH_BLOCK.  The CSR build is head flags over the sorted keys, the three-pass scan of csrc/scan.h, a
 *   scatter of the heads' positions, and per-vertex offsets by a binary search of (v << 32) among the unique keys; one routine,
 *   run once for the edges and once for the corners.  Every loop is bounded by a count read before it starts; the only atomics
 *   are integer adds on the census counters; only ordinary vector memory operations.  The caller's vertex order is kept.
 *
 * WHAT THE CALLER OWES.  durf_smooth_adjacency is given SORTED keys.  With keys that are not sorted its five arrays are
 *   unspecified, but it reads and writes nothing outside the buffers it was given: a head position that is no index into the
 *   keys is not followed.  Every later entry is given the arrays durf_smooth_adjacency and durf_smooth_classify wrote for the same
 *   V and T (rows inside the arrays, neighbours in 0 .. V-1); they are read as they are.
 */
#ifndef DURF_SMOOTH_H
#define DURF_SMOOTH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_SMOOTH_BLOCK 256
#define DURF_SMOOTH_MAX_TRIANGLES 357913942     /* T of every call is below this: 6 T < 2^31 */
#define DURF_SMOOTH_CENSUS_INTS 8
#define DURF_SMOOTH_ISOLATED 0
#define DURF_SMOOTH_INTERIOR 1
#define DURF_SMOOTH_BOUNDARY 2
#define DURF_SMOOTH_NONMANIFOLD 3
#define DURF_SMOOTH_PIN 0
#define DURF_SMOOTH_SLIDE 1
#define DURF_SMOOTH_NO_KEY 0x7fffffffffffffff

/* ---- keys (k_smooth_keys) -----------------------------------------------------------------------------------------------------------
 * edge_keys [6T] and corner_keys [3T] int64, as defined above.  T == 0 succeeds with no launch.
 * Refused: V < 0, T outside 0 .. DURF_SMOOTH_MAX_TRIANGLES - 1, NULL triangles, edge_keys or corner_keys with T > 0. */
int durf_smooth_keys(void* stream, int V, int T, const int32_t* triangles /* [T,3] */, int64_t* edge_keys /* [6T] */,
                     int64_t* corner_keys /* [3T] */);

/* ---- adjacency (k_smooth_heads, k_scan_block_sums, k_smooth_starts, k_smooth_unique, k_smooth_offsets; twice) ------------------------
 * The two CSR structures from the SORTED keys, as defined above.  cap: the entries neighbours and multiplicity hold; cap >= 6T
 * is required, which always suffices, so nothing is read back.  workspace: durf_smooth_workspace_bytes(T) bytes of the call's own.
 * T == 0 writes zeros to offsets and corner_offsets.
 * Refused: V < 0, T outside 0 .. DURF_SMOOTH_MAX_TRIANGLES - 1, cap < 6T, NULL edge_keys, corner_keys or corner_tri with T > 0,
 * NULL neighbours or multiplicity with cap > 0 and T > 0, NULL offsets or corner_offsets, a NULL workspace, one not aligned to 256
 * bytes or smaller than durf_smooth_workspace_bytes(T) (both sizes named). */
size_t durf_smooth_workspace_bytes(int T);                   /* 0 for a refused T */

int durf_smooth_adjacency(void* stream, int V, int T, const int64_t* edge_keys /* [6T] sorted */, const int64_t* corner_keys /* [3T] sorted */,
                          int cap, void* workspace, size_t workspace_bytes, int32_t* offsets /* [V+1] */, int32_t* neighbours /* [cap] */,
                          int32_t* multiplicity /* [cap] */, int32_t* corner_offsets /* [V+1] */, int32_t* corner_tri /* [3T] */);

/* ---- vertex class (k_smooth_classify) ------------------------------------------------------------------------------------------------
 * vertex_class [V] uint8 from the edge rows.  V == 0 succeeds with no launch.
 * Refused: V < 0, NULL offsets, NULL vertex_class with V > 0.  (multiplicity may be NULL only when every row is empty; the caller
 * of a mesh without triangles passes what it has.) */
int durf_smooth_classify(void* stream, int V, const int32_t* offsets /* [V+1] */, const int32_t* multiplicity,
                         uint8_t* vertex_class /* [V] */);

/* ---- census (k_smooth_census) --------------------------------------------------------------------------------------------------------
 * census [DURF_SMOOTH_CENSUS_INTS] int32 ON THE DEVICE, as defined above: zeroed on the stream, then one launch.
 * Refused: V < 0, NULL offsets, corner_offsets or census, NULL vertex_class with V > 0. */
int durf_smooth_census(void* stream, int V, const int32_t* offsets /* [V+1] */, const int32_t* neighbours, const int32_t* multiplicity,
                       const int32_t* corner_offsets /* [V+1] */, const uint8_t* vertex_class /* [V] */, int32_t* census);

/* ---- one step (k_smooth_step) --------------------------------------------------------------------------------------------------------
 * out [V,3] from in [V,3], as defined above.  V == 0 succeeds with no launch.
 * Refused: V < 0, a factor that is not finite or lies outside [-1, 1], boundary outside 0 .. 1, in == out, NULL offsets, NULL in,
 * out or vertex_class with V > 0. */
int durf_smooth_step(void* stream, int V, const float* in /* [V,3] */, const int32_t* offsets /* [V+1] */, const int32_t* neighbours,
                     const int32_t* multiplicity, const uint8_t* vertex_class /* [V] */, float factor, int boundary,
                     const uint8_t* fixed /* [V], nullable */, float* out /* [V,3] */);

/* ---- Taubin (k_smooth_step, S times) -------------------------------------------------------------------------------------------------
 * out [V,3] after the steps defined above; tmp [V,3] is the caller's.  V == 0 succeeds with no launch.
 * Refused: as durf_smooth_step for lambda and mu in the place of factor, iters < 0, iters >= 2^30, in == out, and with two or more
 * steps and V > 0 a NULL tmp, tmp == in or tmp == out. */
int durf_smooth_taubin(void* stream, int V, const float* in /* [V,3] */, const int32_t* offsets /* [V+1] */, const int32_t* neighbours,
                       const int32_t* multiplicity, const uint8_t* vertex_class /* [V] */, int iters, float lambda, float mu, int boundary,
                       const uint8_t* fixed /* [V], nullable */, float* tmp /* [V,3] */, float* out /* [V,3] */);

/* ---- normals (k_smooth_normals) ------------------------------------------------------------------------------------------------------
 * normals [V,3], as defined above.  V == 0 succeeds with no launch.
 * Refused: V < 0, T outside 0 .. DURF_SMOOTH_MAX_TRIANGLES - 1, NULL vertices or normals with V > 0, NULL triangles or corner_tri
 * with T > 0, NULL corner_offsets. */
int durf_smooth_normals(void* stream, int V, int T, const float* vertices /* [V,3] */, const int32_t* triangles /* [T,3] */,
                        const int32_t* corner_offsets /* [V+1] */, const int32_t* corner_tri, float* normals /* [V,3] */);

#ifdef __cplusplus
}
#endif
#endif
