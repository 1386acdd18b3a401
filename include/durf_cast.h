/* C ABI of durf_amd/libdurf_cast.so: the nearest triangle of a mesh along arbitrary rays, on the device -- a LIDAR sweep of an
 * extracted surface, depth from a camera that stands inside the mesh (a ray has no near plane), and visibility between points.
 * A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs that
 * library for durf_last_error alone and takes plain arrays.  The house rules of durf_hip.h hold: device pointers of
 * caller-owned buffers, asynchronous on `stream` (hipStream_t), 0 or nonzero with the text in durf_last_error(), every argument
 * checked before anything is launched, no stream synchronisation and no device-to-host copy anywhere.  All float arithmetic is
 * fp32, unfused, in the order written here, with IEEE division; subnormals are kept.  Sums of three are (x + y) + z.
 *
 * THE DEFINITION names no tree: the result of a cast is a minimum over ALL triangles, and the box test is part of it.
 *
 * Ray.  (o, d), d of any length: t is in units of |d| (camera depth for the ray generator's z = -1 directions, range for
 *   durf_lidar_rays' unit directions), with bounds tmin <= t <= tmax per ray or per call.  A ray is UNUSABLE when a component of
 *   o or d is not finite, d is all zero, !(tmin >= 0), or tmax is NaN: tri = -2, t = NaN, bary = NaN.  tmax = +inf is legal.
 * Valid triangle.  Its three indices lie in 0 .. V-1 and its nine coordinates are finite.  An invalid triangle never counts and
 *   contributes to no box.
 * Box of a triangle.  Per axis lo_a = nextafterf(min of the three, -inf), hi_a = nextafterf(max of the three, +inf).
 * Box rule, for a box [lo, hi] and a usable ray:
 *   1 a box with lo_a > hi_a on any axis FAILS (the empty box is lo = +inf, hi = -inf);
 *   2 inv_a = 1.0f / d_a; axis a is a ZERO axis when d_a == 0 or inv_a is not finite.  A zero axis passes iff
 *     lo_a <= o_a && o_a <= hi_a, and bounds nothing;
 *   3 any other axis: x1 = (lo_a - o_a) * inv_a, x2 = (hi_a - o_a) * inv_a, n_a = fminf(x1, x2), f_a = fmaxf(x1, x2);
 *   4 bn = the maximum of the n_a (-inf over no axis), bf = the minimum of the f_a (+inf over no axis);
 *   5 the box PASSES iff every zero axis passes and bn <= bf && bf >= tmin && bn <= tmax.
 *   Monotone: for boxes B inside B' (lo' <= lo, hi <= hi' per axis), fp32 subtraction of o_a and multiplication by the fixed
 *   inv_a are monotone, so whichever of x1, x2 is the smaller only gets smaller and the larger only larger: n_a' <= n_a,
 *   f_a' >= f_a, hence bn' <= bn and bf' >= bf, a zero axis that passes B passes B', and a pass for B is a pass for B'.  No
 *   x is NaN: lo_a - o_a is a finite number or an infinity, and inv_a is finite and not zero.
 * Triangle rule (Moller-Trumbore), for vertices A, B, C:
 *   e1 = B - A;  e2 = C - A;
 *   p = d x e2:  p_0 = d_1 e2_2 - d_2 e2_1;  p_1 = d_2 e2_0 - d_0 e2_2;  p_2 = d_0 e2_1 - d_1 e2_0;
 *   det = (e1_0 p_0 + e1_1 p_1) + e1_2 p_2;  det != 0;  inv = 1.0f / det, finite;
 *   cull: det > 0 is a FRONT face -- d . (e1 x e2) < 0, the right-hand normal points back along the ray, the triangle is
 *     counter-clockwise as the ray's origin sees it: the rasteriser's front face (durf_raster.h).  cull == 1 drops det < 0 (back
 *     faces), cull == 2 drops det > 0 (front faces), cull == 0 keeps both;
 *   s = o - A;  u = ((s_0 p_0 + s_1 p_1) + s_2 p_2) * inv;
 *   q = s x e1:  q_0 = s_1 e1_2 - s_2 e1_1;  q_1 = s_2 e1_0 - s_0 e1_2;  q_2 = s_0 e1_1 - s_1 e1_0;
 *   v = ((d_0 q_0 + d_1 q_1) + d_2 q_2) * inv;  w = (1.0f - u) - v;  t0 = ((e2_0 q_0 + e2_1 q_1) + e2_2 q_2) * inv.
 * A triangle i COUNTS iff it is valid, its own box passes (with interval [bn_i, bf_i]), det and inv are as above and not culled,
 *   u >= 0 && v >= 0 && w >= 0 (a NaN fails), t0 is not NaN, and tmin <= t && t <= tmax for
 *   t = fminf(fmaxf(t0, bn_i), bf_i) + 0.0f   (the + 0.0f turns -0 into +0: fmaxf does not order the two zeros).
 * The clamp.  In real arithmetic it is the identity, because the hit point lies in the box.  In fp32 it makes bn_i <= t true
 *   by construction (bn_i <= bf_i, since the box passed).  On an axis-aligned flat triangle it pins t to the slab value.
 * The winner.  The counting triangle with the smallest t; among equal t the smallest id, in the mesh's own numbering.
 * Outputs, in the rasteriser's conventions (durf_raster_interp consumes them unchanged): tri int32, the winner's id, -1 where
 *   nothing counts, -2 for an unusable ray; t, 0 and NaN there; bary [.,3] = (w, u, v) NULLABLE, 0 and NaN there.
 * Watertightness is NOT promised: Moller-Trumbore in fp32 can lose a ray through a shared edge, and so can the box rule at a
 *   box's rim.  It is measured.
 *
 * WHY NO TREE CAN CHANGE AN ANSWER.  Let every node's box be the union (per-axis min of lo, max of hi: exact in fp32) of its
 *   children's boxes, the leaves' of their valid triangles' boxes.  A walk visits a node only if the node's box passes the box
 *   rule for (tmin, tmax) and !(bn_node > t_best), t_best the smallest t found so far (+inf at the start), and tests every
 *   triangle of a visited leaf by the triangle rule.  Suppose triangle i counts with t_i.  Every ancestor N of i contains
 *   box_i, so by monotonicity N passes for (tmin, tmax) and bn_N <= bn_i <= t_i.  If the walk skipped N for bn_N > t_best,
 *   then t_best < t_i: i neither wins nor ties.  So every triangle that would win or tie is tested, whatever the tree, the
 *   order of the children and the order of the leaves: the walk's minimum of (t, id) is the minimum over all triangles, bit for
 *   bit.  For durf_cast_any the walk skips by (tmin, tmax) alone and existence does not depend on order.
 *
 * The tree is IMPLICIT.  The caller sorts the triangles (durf_cast_keys and a stable sort; any permutation gives the same
 *   answers) and passes the permutation `order` [T].  Leaf l holds sorted slots [l L, (l + 1) L), L = DURF_CAST_LEAF; n_0 =
 *   ceil(T / L) leaves, n_{k+1} = ceil(n_k / 2) nodes on level k + 1 until a level has one node; node j of level k + 1 is the
 *   union of nodes 2 j and 2 j + 1 of level k, a missing sibling being empty.  No child pointers, no arrival counters: the
 *   build is one launch for the leaves, one per level while a level has more than DURF_CAST_TOP nodes, and one workgroup for
 *   all the levels above.  An entry of `order` outside 0 .. T-1 is an invalid triangle.
 * Workspace of T triangles, every part on a 256-byte boundary in this order:
 *   leaf records float [n_0 L, DURF_CAST_RECORD_FLOATS]: A, B, C (nine floats) and the bits of the triangle's id as int32,
 *     -1 for an invalid triangle and for the padding of the last leaf -- a cast reads the workspace alone;
 *   nodes float [sum of n_k, DURF_CAST_NODE_FLOATS]: lo_0 lo_1 lo_2 0 hi_0 hi_1 hi_2 0, level 0 first.
 *   That is 40 bytes per triangle of records and about 16 of nodes.
 * The walk: one thread per ray, workgroups of DURF_CAST_BLOCK, a stack of at most DURF_CAST_STACK node numbers per thread in LDS
 *   (one entry per level at most), the child with the smaller bn first (the lower on a tie), a popped node tested again
 *   against the t_best of that moment.  Every loop is bounded by a count read before it starts (the node count); no atomics
 *   at all, no spin loops, only ordinary vector memory operations.
 */
#ifndef DURF_CAST_H
#define DURF_CAST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_CAST_LEAF 4                 /* triangles per leaf */
#define DURF_CAST_BLOCK 256              /* rays, triangles, leaves or nodes per workgroup */
#define DURF_CAST_STACK 32               /* levels: DURF_CAST_STACK DURF_CAST_BLOCK int32 of LDS, 32 KB */
#define DURF_CAST_TOP 256                /* a level of at most this many nodes, and all above it, are built by one workgroup */
#define DURF_CAST_RECORD_FLOATS 10       /* 40 bytes per sorted slot */
#define DURF_CAST_NODE_FLOATS 8          /* 32 bytes per node */
#define DURF_CAST_KEY_BITS 21            /* per axis: a 63-bit Morton key */
#define DURF_CAST_MAX_TRIANGLES (1 << 30)  /* T below this: a node number fits an int32 */

/* The workspace described above; 256 for T == 0 (an empty tree).  0 for a refused T: T < 0 or T >= DURF_CAST_MAX_TRIANGLES. */
size_t durf_cast_workspace_bytes(int T);

/* ---- keys (k_cast_keys) -----------------------------------------------------------------------------------------------------------
 * One thread per triangle: keys [T] int64, the Morton key of the centroid inside bounds [6] floats ON THE DEVICE (lo_0 lo_1
 * lo_2 hi_0 hi_1 hi_2, e.g. torch.aminmax of the vertices: no read-back).  Per axis a: c = ((A_a + B_a) + C_a) / 3.0f;
 * ext = hi_a - lo_a; x = ((c - lo_a) / ext) * 2097152.0f; g_a = 0 if !(ext > 0) or !(x >= 0), 2097151 if x >= 2097151.0f, else
 * (int) x (truncated).  Bit i of g_0, g_1, g_2 is bit 3 i + 2, 3 i + 1, 3 i of the key.  An invalid triangle gets INT64_MAX and
 * sorts last.  Keys affect speed only, never a result.
 * Refused: V < 0, T outside 0 .. DURF_CAST_MAX_TRIANGLES - 1, NULL vertices with V > 0, NULL triangles, bounds or keys with
 * T > 0. */
int durf_cast_keys(void* stream, int V, int T, const float* vertices /* [V,3] */, const int32_t* triangles /* [T,3] */,
                   const float* bounds /* [6] device */, int64_t* keys /* [T] */);

/* ---- build (k_cast_leaves, k_cast_level, k_cast_top) --------------------------------------------------------------------------------
 * The leaf records and the node boxes of the implicit tree over `order` [T] int32, into the workspace.  T == 0 succeeds with
 * no launch: every cast finds nothing.
 * Refused: V, T as above, NULL vertices with V > 0, NULL triangles or order with T > 0, a NULL workspace, one not aligned to 256
 * bytes or smaller than durf_cast_workspace_bytes(T) (both sizes named). */
int durf_cast_build(void* stream, int V, int T, const float* vertices, const int32_t* triangles, const int32_t* order /* [T] */,
                    void* workspace, size_t workspace_bytes);

/* ---- nearest hit (k_cast_rays) ------------------------------------------------------------------------------------------------------
 * n rays in the caller's order against the workspace durf_cast_build left for the same T.  The bounds of ray i are
 * tmin_rays[i] / tmax_rays[i] where the array is given (NULLABLE, each on its own), else the scalar tmin / tmax.
 * tri [n] int32, t [n], bary [n,3] NULLABLE, as defined above.  n == 0 succeeds with no launch.
 * Refused: n < 0, T as above, cull outside 0 .. 2, NULL origins, directions, tri or t with n > 0, a scalar bound in use with
 * !(tmin >= 0) or a NaN tmax, the workspace as above. */
int durf_cast_rays(void* stream, int n, const float* origins /* [n,3] */, const float* directions /* [n,3] */,
                   const float* tmin_rays /* [n], nullable */, const float* tmax_rays /* [n], nullable */, float tmin, float tmax,
                   int cull, int T, const void* workspace, size_t workspace_bytes, int32_t* tri /* [n] */, float* t /* [n] */,
                   float* bary /* [n,3], nullable */);

/* ---- any hit (k_cast_rays, the walk that stops at the first counting triangle) --------------------------------------------------------
 * hit [n] int32: 1 where some triangle counts, 0 where none does, -2 for an unusable ray: exactly tri >= 0 of durf_cast_rays.
 * The segment between points a and b is the ray o = a, d = b - a with tmin = 0, tmax = 1.  Refusals as durf_cast_rays. */
int durf_cast_any(void* stream, int n, const float* origins, const float* directions, const float* tmin_rays /* nullable */,
                  const float* tmax_rays /* nullable */, float tmin, float tmax, int cull, int T, const void* workspace,
                  size_t workspace_bytes, int32_t* hit /* [n] */);

/* ---- cameras (k_cast_cameras) -------------------------------------------------------------------------------------------------------
 * F camera rows cams_dev [F,DURF_CAM_FLOATS] floats ON THE DEVICE (durf_hip.h, THE CAMERA ROW), all of the call's h x w.  Pixel
 * (y, x) of frame f is cast along the ray csrc/camera.h's pinhole_ray gives for pixel y w + x of row f -- generated in the
 * kernel, never stored -- with the scalar bounds: tri [F,h,w], depth [F,h,w] (t: camera depth), bary [F,h,w,3] NULLABLE,
 * bit-identical to durf_cast_rays on durf_camera_rays' rays of the same rows.  A row whose (int) H, W are not h, w makes its
 * whole frame unusable (-2 / NaN).  F == 0 succeeds with no launch.
 * Refused: F < 0, h < 1, w < 1, F h w >= 2^31, NULL cams_dev, tri or depth with F > 0, and the rest as durf_cast_rays. */
int durf_cast_cameras(void* stream, int F, int h, int w, const float* cams_dev /* [F,DURF_CAM_FLOATS] device */, float tmin, float tmax,
                      int cull, int T, const void* workspace, size_t workspace_bytes, int32_t* tri /* [F,h,w] */,
                      float* depth /* [F,h,w] */, float* bary /* [F,h,w,3], nullable */);

#ifdef __cplusplus
}
#endif
#endif
