/* C ABI of durf_amd/libdurf_closest.so: the closest point of a triangle mesh to arbitrary points, on the device -- the exact
 * distance between a surface and measured points (accuracy and completeness without a sample spacing), mesh-to-mesh distance,
 * the mesh's attributes carried to points, and the unsigned distance field of a mesh over a lattice.  A library of its own
 * beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs that library for
 * durf_last_error alone, takes plain arrays and calls no other library.  It READS the workspace durf_cast_build
 * (include/durf_cast.h) leaves, by the layout that header documents, and builds no tree of its own: durf_cast_workspace_bytes
 * is the size of the workspace here too.  The house rules of durf_hip.h hold: device pointers of caller-owned buffers,
 * asynchronous on `stream` (hipStream_t), 0 or nonzero with the text in durf_last_error(), every argument checked before
 * anything is launched, no stream synchronisation and no device-to-host copy anywhere.  All float arithmetic is fp32, unfused,
 * in the order written here, with IEEE division and square root; subnormals are kept.  Sums of three are (x + y) + z; a dot
 * product x . y is (x_0 y_0 + x_1 y_1) + x_2 y_2.
 *
 * THE DEFINITION names no tree: the result of a query is a minimum over ALL triangles, and the box bound is part of it.
 *
 * Query.  A point P is USABLE when its three coordinates are finite; an unusable point gives tri = -2, dist = NaN and NaN in
 *   bary and point.  max_dist is a scalar, +inf or a number in [1e-18, 1e18]; cap2 = max_dist * max_dist.
 * Valid triangle, box of a triangle.  Exactly durf_cast.h's: three indices in 0 .. V-1 and nine finite coordinates; per axis
 *   lo_a = nextafterf(min of the three, -inf), hi_a = nextafterf(max of the three, +inf).  An invalid triangle never counts and
 *   contributes to no box.
 * Box bound, for a box [lo, hi] and a usable point:
 *   e_a = fmaxf(fmaxf(lo_a - P_a, P_a - hi_a), 0.0f) per axis;  lb = (e_0 e_0 + e_1 e_1) + e_2 e_2.
 *   The empty box (lo = +inf, hi = -inf) gives +inf by the same formula.  No e_a is NaN: P_a is finite and lo_a, hi_a are
 *   numbers or infinities.
 *   Monotone: for boxes B inside B' (lo' <= lo, hi <= hi' per axis), fp32 subtraction with P_a fixed is monotone in the other
 *   operand, so lo'_a - P_a <= lo_a - P_a and P_a - hi'_a <= P_a - hi_a; fmaxf is monotone in each argument, so 0 <= e'_a <=
 *   e_a; the rounded square of a non-negative number and rounded addition are monotone; hence lb' <= lb.
 * Triangle rule, for vertices A, B, C of a valid triangle.  Every candidate is a point of the triangle given by weights (w, u,
 *   v) in the rasteriser's order (durf_raster.h); the rule takes the nearest of at most four candidates:
 *   e1 = B - A;  e2 = C - A;  s = P - A;  f = C - B;  r = P - B;
 *   a = e1 . e1;  b = e1 . e2;  c = e2 . e2;  d = e1 . s;  e = e2 . s;  l = f . f;  g = f . r;
 *   0 the interior projection: det = a c - b b; only if det > 0: u = (c d - b e) / det, v = (a e - b d) / det,
 *     w = (1.0f - u) - v, and only if u >= 0 && v >= 0 && w >= 0 (a NaN fails);
 *   1 the segment AB: x = a > 0 ? fminf(fmaxf(d / a, 0.0f), 1.0f) : 0.0f;  (w, u, v) = (1.0f - x, x, 0);
 *   2 the segment AC: x = c > 0 ? fminf(fmaxf(e / c, 0.0f), 1.0f) : 0.0f;  (w, u, v) = (1.0f - x, 0, x);
 *   3 the segment BC: x = l > 0 ? fminf(fmaxf(g / l, 0.0f), 1.0f) : 0.0f;  (w, u, v) = (0, 1.0f - x, x).
 *   (fmaxf and fminf return the other operand for a NaN: a quotient that is NaN clamps to 0.)
 *   The point of a candidate: C_k = (A_k + u e1_k) + v e2_k per axis;  q = P - C;  its d2 = q . q.
 *   The rule starts from (w, u, v) = (1, 0, 0), C = A, d2_0 = +inf and takes candidates 0, 1, 2, 3 in this order, each only if
 *   its d2 < d2_0 (strictly: the earlier candidate keeps a tie, a NaN is never taken).
 *   No 0 / 0: every division is guarded by its divisor being > 0, the interior projection is consulted only where it lies
 *   inside, and the three clamped segments always stand, so a DEGENERATE triangle is its longest segment (three collinear
 *   vertices, two coincident vertices: det is 0 or rounding noise that the segments undercut) or its point (a = c = l = 0:
 *   every x is 0).  For coordinates of magnitude up to 2^30 nothing overflows and d2_0 is finite for every valid triangle and
 *   usable point; beyond, a product may overflow, the rule stays defined (candidates that are NaN are not taken) and d2_0 may
 *   be +inf.  Where det underflows to 0 (edges shorter than about 1e-10) the triangle is measured by its outline.
 * The clamp.  d2_i = fmaxf(d2_0, lb_i) + 0.0f, lb_i the bound of the triangle's OWN box.  In real arithmetic it is the
 *   identity, because the triangle lies in its box.  In fp32 it makes lb_i <= d2_i true by construction -- the whole of the
 *   proof obligation.
 * A triangle i COUNTS iff it is valid and d2_i <= cap2.
 * The winner.  The counting triangle with the smallest d2; among equal d2 the smallest id, in the mesh's own numbering.
 * Outputs: tri int32, the winner's id; dist = sqrtf(d2); bary [.,3] = (w, u, v) NULLABLE, which durf_raster_interp consumes
 *   unchanged; point [.,3] = C NULLABLE.  Where nothing counts: tri = -1, dist = max_dist, bary and point 0 -- durf_geom_nearest's
 *   convention (include/durf_geom.h), so durf_geom_stats consumes dist and tri unchanged.  dist <= max_dist always: d2 <= cap2
 *   = fl(max_dist max_dist), sqrtf is monotone and correctly rounded, and sqrtf(fl(x x)) == x for every fp32 x whose square is
 *   a normal number, which [1e-18, 1e18] guarantees.
 *
 * WHY NO TREE CAN CHANGE AN ANSWER.  Let every node's box be the union of its children's boxes, the leaves' of their valid
 *   triangles' boxes (durf_cast.h).  A walk skips a node N only for lb_N > cap2 or for lb_N > d2_best, strictly, d2_best the
 *   smallest d2 found so far (+inf at the start), and measures every triangle of a visited leaf by the triangle rule.  Suppose
 *   triangle i counts with d2_i.  Every ancestor N of i contains box_i, so by monotonicity lb_N <= lb_i <= d2_i <= cap2: N is
 *   not skipped for cap2, and if it is skipped for lb_N > d2_best then d2_best < d2_i: i neither wins nor ties.  So every
 *   triangle that would win or tie is measured, whatever the tree, the order of the children and the order of the leaves: the
 *   walk's minimum of (d2, id) is the minimum over all triangles, bit for bit.
 *
 * The walk reads durf_cast.h's workspace of T triangles: the leaf records (A, B, C and the id's bits, 40 bytes each, -1 for an
 *   invalid triangle and for padding) and the node boxes of the heap-numbered implicit tree.  One thread per query, workgroups
 *   of DURF_CLOSEST_BLOCK, a stack of at most DURF_CLOSEST_STACK node numbers per thread in LDS (one entry per level at most),
 *   the child with the smaller lb first (the lower on a tie), a popped node tested again against the d2_best of that moment.
 *   Every loop is bounded by a count read before it starts; no atomics at all, no spin loops, only ordinary vector memory
 *   operations.  The order of the queries affects speed only: the caller keeps neighbours together (durf_amd/closest.py sorts
 *   them by a Morton key of their own).
 */
#ifndef DURF_CLOSEST_H
#define DURF_CLOSEST_H
#include <stddef.h>
#include <stdint.h>
#include "durf_cast.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_CLOSEST_BLOCK 256           /* queries per workgroup: DURF_CAST_BLOCK */
#define DURF_CLOSEST_STACK 32            /* levels: DURF_CAST_STACK; DURF_CLOSEST_STACK DURF_CLOSEST_BLOCK int32 of LDS, 32 KB */
#define DURF_CLOSEST_BRICK 4             /* durf_closest_grid: a wave of 64 walks a brick of 4 x 4 x 4 lattice points */

/* ---- points (k_closest_points) -------------------------------------------------------------------------------------------------------
 * n points in the caller's order against the workspace durf_cast_build left for the same T: tri [n] int32, dist [n], bary
 * [n,3] = (w, u, v) NULLABLE, point [n,3] NULLABLE, as defined above.  n == 0 succeeds with no launch; T == 0 is legal (an
 * empty tree: -1 / max_dist for every usable point).
 * Refused: n < 0, T outside 0 .. DURF_CAST_MAX_TRIANGLES - 1, a max_dist that is neither +inf nor in [1e-18, 1e18] (a NaN
 * too), NULL points, tri or dist with n > 0, a NULL workspace, one not aligned to 256 bytes or smaller than
 * durf_cast_workspace_bytes(T) (both sizes named). */
int durf_closest_points(void* stream, int n, const float* points /* [n,3] */, float max_dist, int T, const void* workspace,
                        size_t workspace_bytes, int32_t* tri /* [n] */, float* dist /* [n] */, float* bary /* [n,3], nullable */,
                        float* point /* [n,3], nullable */);

/* ---- lattice (k_closest_grid) --------------------------------------------------------------------------------------------------------
 * The same walk for the points of a lattice, generated in the kernel and never stored: point (i, j, k) of nu x nv x nw lies at
 * durf_tsdf.h's P_c = ((origin_c + (float) i du_c) + (float) j dv_c) + (float) k dw_c (origin, du, dv, dw: three HOST floats
 * each) and has index g = (i nv + j) nw + k.  dist [nu,nv,nw], tri [nu,nv,nw] int32 NULLABLE: bit-identical to
 * durf_closest_points on the same points (a lattice point that is not finite is unusable).  A wave walks a brick of
 * DURF_CLOSEST_BRICK^3 points, so that its lanes stay together; that order affects speed only.
 * Refused: nu, nv or nw < 1, nu nv nw >= 2^31, an origin or a step component that is not finite, a NULL dist, and T, max_dist
 * and the workspace as durf_closest_points. */
int durf_closest_grid(void* stream, int nu, int nv, int nw, const float* origin /* [3] host */, const float* du /* [3] host */,
                      const float* dv /* [3] host */, const float* dw /* [3] host */, float max_dist, int T, const void* workspace,
                      size_t workspace_bytes, float* dist /* [nu,nv,nw] */, int32_t* tri /* [nu,nv,nw], nullable */);

#ifdef __cplusplus
}
#endif
#endif
