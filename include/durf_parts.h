/* C ABI of durf_amd/libdurf_parts.so: the connected solid regions of a density lattice, on the device -- label them, number
 * them, measure them, and drop the small ones from the lattice's iso-surface (include/durf_mesh.h) by compaction.  A radiance
 * field leaves detached blobs of density in free space; each is a closed shell of the surface and counts against its accuracy.
 * A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is, as it leaves
 * libdurf_mesh.so's; it needs libdurf_hip.so for durf_last_error alone and takes plain arrays.  The house rules of durf_hip.h
 * hold: device pointers of caller-owned buffers unless marked HOST, asynchronous on `stream` (hipStream_t), 0 or nonzero with
 * the text in durf_last_error(), every argument checked before anything is launched, no stream synchronisation and no
 * device-to-host copy anywhere.  Everything here is integer: there is no rounding and no tolerance.
 *
 * Definitions.  The lattice density [nu,nv,nw] float32 with valid uint8 NULLABLE, the index g = (i nv + j) nw + k, n = nu nv nw,
 *   USABLE, IN (usable and density >= iso) and the seven edges a point owns (e = 0 .. 6 towards p + o_e, (di, dj, dk) the bits
 *   of e + 1: three axis edges, the three (+,+) face diagonals, the (+,+,+) body diagonal) are durf_mesh.h's, word for word.
 *   Two IN points are ADJACENT when one owns an edge to the other: 14 neighbours, +-o_e -- not 6, 18 or 26.  A COMPONENT is a
 *   class of the transitive closure of ADJACENT; its LABEL is the smallest g in it; a point that is not IN has label -1.
 *   Components are NUMBERED 0 .. C-1 in ascending order of their labels.
 * Why these 14.  They are the edges of the Kuhn tetrahedra durf_mesh.h marches: it puts a vertex on an edge exactly when one
 *   end is in and the other is not.  So two IN points it does not separate by the surface share a label, two it separates do
 *   not.  Every pair of corners of a tetrahedron is one of these edges, so all IN corners of a tetrahedron lie in ONE component
 *   and every emitted triangle belongs to exactly one: the component of the IN end of any of its three vertices' edges.
 *   Dropping a component from a mesh is therefore a compaction of its vertices and triangles (durf_parts_select_mesh):
 *   nothing is re-meshed and no density is overwritten (which would move the normals of neighbouring shells).
 *
 * How the labels are found (durf_parts_label): a union-find by minimum index in three launches.  L [n] int32 in the workspace
 *   holds, for every IN point, a LINK to a point of its own component with an index no larger than its own (-1: not IN); a
 *   ROOT is a point with L[g] == g.
 *   (a) Tile pass (k_parts_tile).  One workgroup per tile of DURF_PARTS_TILE_I x _J x _K points, adjacent lanes along k.  The
 *       tile's points hold their tile-local index in LDS; a round replaces every point's value by the minimum over itself and
 *       its adjacent points inside the tile, then by that point's own value (one pointer jump); a workgroup-wide vote ends the
 *       loop when no value changed.  L[g] = the global index of the value left: the smallest index of g's component within
 *       the tile (local and global order agree inside a tile).
 *   (b) Border pass (k_parts_border).  One thread per lattice point; a point whose owned edges all stay inside its tile leaves
 *       at once.  For each owned edge that leaves the tile with both ends IN: unite(a, b), a and b the ends of the two
 *       points' link chains -- while a != b: order them a > b; old = atomicMin(&L[a], b); stop if old == a, else a = old.
 *       A link is only ever written under a smaller index.
 *   (c) Flatten (k_parts_flatten).  A launch of its own, so the kernel boundary orders it after every union:
 *       labels[g] = the end of g's link chain (it reads L and writes labels, two different arrays), or -1.
 *   Same inputs, same bits, despite the atomics.  Every value ever stored in L[x] indexes a point of x's true component (the
 *   tile pass and unite only ever connect ADJACENT-connected points).  Take the graph of the links plus, for every thread
 *   inside unite, its pending pair (a, b): atomicMin replaces the link a - old and the pending pair a - b by the link
 *   a - min(old, b) and the pending pair old - b (or by the link a - b alone when old == a), which leaves its connectivity as it
 *   was; connectivity therefore only grows, and when (b) has ended it is the tile pass's plus every border edge: the true
 *   components.  Links lead from larger to smaller indices, so a component connected by n - 1 links has exactly one root, and
 *   the root is its minimum.  The labels are that minimum whatever the schedule.
 *   A stale read costs a retry, never a wrong union: a stale L[x] is a value L[x] held earlier, so it names a point of the same
 *   component that is still connected to x in the graph above; uniting from there is right, only longer.  In (b) L is read
 *   with relaxed atomic loads at agent scope and changed with agent-scope atomicMin: the L2 caches of the chip's dies are not
 *   coherent with each other and a compute unit's L1 is not refreshed by other units' stores, so a plain load could keep
 *   returning one old value.  Only ordinary vector atomics on global memory and LDS are used.
 *   Every loop is bounded by construction.  A link chain follows strictly decreasing indices, so it ends within n steps.
 *   unite retries only with a strictly smaller larger-index: after old = atomicMin(&L[a], b) with old != a the next pair is
 *   (old, b) with old < a and b < a.  The tile loop runs at most DURF_PARTS_TILE_POINTS rounds: a round that changes nothing
 *   ends it, values only decrease, and the code also counts the rounds.  No workgroup waits for another: there are no spin
 *   loops and no flags polled inside a kernel.
 */
#ifndef DURF_PARTS_H
#define DURF_PARTS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_PARTS_TILE_I 4        /* the tile of the tile pass: 4 x 4 x 16 lattice points, one workgroup of 256 */
#define DURF_PARTS_TILE_J 4
#define DURF_PARTS_TILE_K 16
#define DURF_PARTS_TILE_POINTS (DURF_PARTS_TILE_I * DURF_PARTS_TILE_J * DURF_PARTS_TILE_K)
#define DURF_PARTS_BLOCK 256       /* elements per workgroup and per block sum of every other kernel */

/* The workspace of nu nv nw lattice points, every part on a 256-byte boundary in this order: link int32 [n] (durf_parts_label:
 * L above; durf_parts_number: the exclusive scan of the roots), then the scan's block sums int32 [nb + 1] with
 * nb = ceil(n / DURF_PARTS_BLOCK).  0 for a refused shape (a dimension < 2, n >= DURF_MESH_MAX_POINTS = 2^27).
 * durf_parts_select_mesh reads the workspace as block sums alone, int32 [2, nm + 1] with
 * nm = ceil(max(max_vertices, max_triangles) / DURF_PARTS_BLOCK), rounded up to 256 bytes; the workspace of the mesh's own
 * lattice is never smaller (V <= 7 n, T <= 12 n). */
size_t durf_parts_workspace_bytes(int nu, int nv, int nw);

/* ---- label (k_parts_tile, k_parts_border, k_parts_flatten) --------------------------------------------------------------------
 * labels [n] int32: every point's label as defined above.
 * Refused: nu, nv or nw < 2, n >= 2^27, NaN iso, a NULL density, labels or workspace, a workspace not aligned to 256 bytes or
 * smaller than durf_parts_workspace_bytes (both sizes named). */
int durf_parts_label(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid /* nullable */, float iso,
                     void* workspace, size_t workspace_bytes, int32_t* labels);

/* ---- number (k_parts_roots, k_scan_block_sums, k_parts_rank, k_parts_number) ---------------------------------------------------
 * The roots are the g with labels[g] == g.  The exclusive scan of the roots in g order (the three passes of csrc/scan.h) is
 * each root's number; comp [n] int32 = the number of labels[g]'s root, one gather through the label, or -1 where labels[g] is
 * not in 0 .. n-1; count [1] int32 on the device = C.
 * Refused: n < 1 or n >= 2^27, a NULL labels, comp, count or workspace, a workspace misaligned or smaller than
 * 256 ceil(4 n / 256) + 256 ceil(4 (nb + 1) / 256) bytes (what durf_parts_workspace_bytes gives for n points; both named). */
int durf_parts_number(void* stream, int n, const int32_t* labels, void* workspace, size_t workspace_bytes, int32_t* comp,
                      int32_t* count);

/* ---- stats (k_parts_stats_init, k_parts_stats) -----------------------------------------------------------------------------------
 * size [max_components] int32: the points of every component; bbox [max_components,6] int32: its inclusive index bounds
 * (imin, jmin, kmin, imax, jmax, kmax).  Rows of numbers no component has hold size 0 and (INT32_MAX x 3, -1 x 3).  Components
 * numbered at or past max_components are not written.  Integer adds, minima and maxima are exact in any order, so the atomics
 * that collect them leave the result deterministic (a wave first folds the lanes that share a component, a workgroup collects
 * a few components in LDS, and a bound that an earlier read shows to be as good already is not sent: one component of millions
 * of points costs a few thousand atomics).  There are no float sums: a volume is size times the cell volume, on the host.
 * Refused: the shape as above, max_components < 0, a NULL comp, NULL size or bbox with max_components > 0. */
int durf_parts_stats(void* stream, int nu, int nv, int nw, const int32_t* comp, int max_components, int32_t* size, int32_t* bbox);

/* ---- keep some components of a mesh (k_parts_select_sums, k_scan_block_sums, k_parts_select_vertices, _triangles) --------------
 * counts [2] int32 = durf_mesh_count's (vertices, triangles); V = min(counts[0], max_vertices), T = min(counts[1],
 * max_triangles), the capacities of every per-vertex and per-triangle array here.  vertex_comp [max_vertices] int32 is what
 * durf_mesh_gather(attr_i = comp) returns: the component of each edge's IN end.  keep [n_components] uint8.
 * A vertex v < V is KEPT when 0 <= vertex_comp[v] < n_components and keep[vertex_comp[v]] != 0 (a vertex of component -1, the
 * IN end of a hole's edge next to an unusable point never is: it is dropped).  A triangle t < T is kept when its first vertex
 * is (its other two then are: one component per triangle).  Kept vertices and kept triangles keep their relative order.
 * vertex_map [max_vertices] int32: the new id of v, or -1 (also for V <= v);  vertex_src [max_vertices] int32: row v' < V' holds
 * the old id of new vertex v' (the caller gathers positions, normals, colours with it; later rows are left as they are);
 * triangles_out [max_triangles,3] int32: the kept triangles through vertex_map, rows past T' left as they are (an id outside
 * 0 .. V-1 maps to -1);  counts_out [2] int32 = (V', T').
 * Refused: max_vertices or max_triangles < 0, n_components < 0, a NULL counts or counts_out, NULL vertex_comp, vertex_map or
 * vertex_src with max_vertices > 0, NULL triangles or triangles_out with max_triangles > 0, NULL keep with n_components > 0, a
 * NULL or misaligned workspace, a workspace smaller than stated at durf_parts_workspace_bytes (both sizes named). */
int durf_parts_select_mesh(void* stream, const int32_t* counts, int max_vertices, int max_triangles, const int32_t* vertex_comp,
                           const int32_t* triangles, const uint8_t* keep, int n_components, void* workspace, size_t workspace_bytes,
                           int32_t* vertex_map, int32_t* vertex_src, int32_t* triangles_out, int32_t* counts_out);

#ifdef __cplusplus
}
#endif
#endif
