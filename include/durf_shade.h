/* C ABI of durf_amd/libdurf_shade.so: a shaded picture of a triangle mesh, on the device -- flat normals, a sun shadow and ambient
 * occlusion from short any-hit rays at the primary hit, composed into one colour per sample.  A depth ramp hides floaters, holes
 * and the staircase of a coarse lattice; a shaded picture with contact shadows shows them.  A library of its own beside
 * libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs that library for durf_last_error
 * alone.  It builds no tree: it reads the workspace durf_cast_build (include/durf_cast.h) leaves, as libdurf_closest.so does.
 * The house rules of durf_hip.h hold: device pointers of caller-owned buffers, asynchronous on `stream` (hipStream_t), 0 or
 * nonzero with the text in durf_last_error(), every argument checked before anything is launched, no stream synchronisation and
 * no device-to-host copy anywhere.  All float arithmetic is fp32, unfused, in the order written here, with IEEE division and
 * sqrtf; subnormals are kept.  Sums of three are (x + y) + z.  dot(x, y) below is (x_0 y_0 + x_1 y_1) + x_2 y_2.
 *
 * THE DEFINITIONS name no tree, and every output is an integer or a written-out fp32 expression: a numpy oracle holds the
 * device to every bit (tests/shade_ref.py).
 *
 * SURFACE.  Sample i with tri[i] = t and bary[i] = (w, u, v), the rasteriser's order, as durf_cast_* and durf_raster_draw write
 *   them.  The sample is VALID when 0 <= t < T, the three indices of triangles[t] lie in 0 .. V-1 and the nine coordinates are
 *   finite (durf_cast.h's valid triangle); otherwise point = normal = 0 (tri = -1 and -2 among them; bary is not read then).
 *   For a valid sample, with (A, B, C) the vertices of triangles[t]:
 *   1 e1 = B - A;  e2 = C - A;
 *   2 point_a = (A_a + u e1_a) + v e2_a          (durf_closest.h's C);
 *   3 N = e1 x e2 in the component order of durf_cast.h's q:  N_0 = e1_1 e2_2 - e1_2 e2_1;  N_1 = e1_2 e2_0 - e1_0 e2_2;
 *     N_2 = e1_0 e2_1 - e1_1 e2_0;
 *   4 len2 = (N_0 N_0 + N_1 N_1) + N_2 N_2;
 *   5 the triangle is FLAT when !(len2 > 0) or len2 is not finite: normal = 0 (the point is still written);
 *   6 otherwise n = N * (1.0f / sqrtf(len2)), one division and three products;
 *   7 with `toward` given ([n,3]: the directions of the rays that found the samples), n is negated iff dot(n, toward[i]) > 0:
 *     the normal faces the viewer.  A NaN there negates nothing.
 *
 * OCCLUSION.  points, normals [n,3]; S directions dirs [S,3] ON THE DEVICE; bias >= 0; reach = +inf or > 0; cull; the cast
 *   workspace.  Sample i is LIVE when its three normal components are finite and not all zero and its three point components
 *   are finite.  For a live sample and s = 0 .. S-1, with d = dirs[s]:
 *   1 c = dot(normal, d);
 *   2 the ray is USED iff c > 0 (a direction in the tangent plane, below it, all zero or with a NaN is not used);
 *   3 its origin is o_a = p_a + bias * n_a, its direction d, its bounds tmin = 0 and tmax = reach;
 *   4 a used ray that is UNUSABLE by durf_cast.h's rule (an infinite component of d with c > 0, an origin that overflowed)
 *     counts as used and not blocked;
 *   5 it is BLOCKED iff durf_cast_any would say 1 for it: some triangle counts on it, by durf_cast.h's box and triangle rules.
 *   used [n] and blocked [n], int32, count the used and the blocked rays of the sample; both are 0 for a sample that is not
 *   live.  Nothing else is written.  By durf_cast.h's proof (WHY NO TREE CAN CHANGE AN ANSWER, the any-hit sentence) no tree,
 *   child order or schedule can change either integer.
 *
 * COMPOSE.  Per sample, with a HOST light [3] (a direction towards the light; it is used as given, not normalised), ambient in
 *   [0, 1] and a HOST background [3]:
 *   1 ao = used > 0 ? (float) (used - blocked) / (float) used : 1.0f;
 *   2 lam = fmaxf(dot(normal, light), 0.0f)                  (a NaN gives 0);
 *   3 sun = 1.0f, except 0.0f where sun_blocked (NULLABLE [n] int32) is > 0;
 *   4 shade = ambient * ao + (1.0f - ambient) * (lam * sun);
 *   5 channel k is albedo ? albedo[i,k] * shade : shade; for tri[i] < 0 it is background[k];
 *   6 out_f [n,3] float and / or out_u8 [n,3] bytes, the latter by k_frame_pack's rule (durf_hip.h): rintf(c * 255.0f) with
 *     c = fminf(fmaxf(x, 0.0f), 1.0f), and 0 for a NaN.
 *
 * The occlusion walk: one thread per sample, workgroups of DURF_CAST_BLOCK, the loop over the directions inside the thread, each
 *   used direction one any-hit walk of durf_cast.h's tree over the same stack in LDS.  Neighbouring lanes hold neighbouring
 *   samples and walk the same direction at the same time.  Every loop is bounded by a count read before it starts; no atomics,
 *   no spin loops, only ordinary vector memory operations.  The order of the samples affects speed only.
 */
#ifndef DURF_SHADE_H
#define DURF_SHADE_H
#include <stddef.h>
#include <stdint.h>
#include "durf_cast.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_SHADE_MAX_DIRS 256          /* S of one occlusion call */

/* ---- surface (k_shade_surface) ------------------------------------------------------------------------------------------------------
 * point [n,3] and normal [n,3] of n samples (tri [n] int32, bary [n,3]) on the mesh, as defined above; toward [n,3] NULLABLE.
 * n == 0 succeeds with no launch.
 * Refused: n < 0, V < 0, T outside 0 .. DURF_CAST_MAX_TRIANGLES - 1, NULL vertices with V > 0, NULL triangles with T > 0, NULL
 * tri, bary, point or normal with n > 0. */
int durf_shade_surface(void* stream, int n, int V, int T, const float* vertices /* [V,3] */, const int32_t* triangles /* [T,3] */,
                       const int32_t* tri /* [n] */, const float* bary /* [n,3] */, const float* toward /* [n,3], nullable */,
                       float* point /* [n,3] */, float* normal /* [n,3] */);

/* ---- occlusion (k_shade_occlusion) --------------------------------------------------------------------------------------------------
 * used [n] and blocked [n] int32 of n samples against the workspace durf_cast_build left for the same T, as defined above.
 * n S may be anything: the loop over the directions is per thread.  n == 0 succeeds with no launch; T == 0 is legal (nothing
 * blocks).
 * Refused: n < 0, S outside 1 .. DURF_SHADE_MAX_DIRS, a bias that is negative or NaN, a reach that is neither +inf nor
 * > 0 (a NaN too), cull outside 0 .. 2, T outside 0 .. DURF_CAST_MAX_TRIANGLES - 1, NULL dirs, NULL points, normals, used or
 * blocked with n > 0, a NULL workspace, one not aligned to 256 bytes or smaller than durf_cast_workspace_bytes(T) (both sizes
 * named). */
int durf_shade_occlusion(void* stream, int n, const float* points /* [n,3] */, const float* normals /* [n,3] */, int S,
                         const float* dirs /* [S,3] device */, float bias, float reach, int cull, int T, const void* workspace,
                         size_t workspace_bytes, int32_t* used /* [n] */, int32_t* blocked /* [n] */);

/* ---- compose (k_shade_compose) ------------------------------------------------------------------------------------------------------
 * The colour of n samples, as defined above: out_f [n,3] NULLABLE, out_u8 [n,3] NULLABLE, not both NULL.  n == 0 succeeds with
 * no launch.
 * Refused: n < 0, an ambient outside [0, 1] (a NaN too), a NULL light or background or a component of either that is not finite,
 * NULL tri, normals, used or blocked with n > 0, out_f and out_u8 both NULL with n > 0. */
int durf_shade_compose(void* stream, int n, const int32_t* tri /* [n] */, const float* normals /* [n,3] */, const int32_t* used /* [n] */,
                       const int32_t* blocked /* [n] */, const int32_t* sun_blocked /* [n], nullable */, const float* albedo /* [n,3], nullable */,
                       const float* light /* [3] host */, float ambient, const float* background /* [3] host */,
                       float* out_f /* [n,3], nullable */, uint8_t* out_u8 /* [n,3], nullable */);

/* ---- cameras (k_shade_primary, k_shade_occlusion, k_shade_compose) ------------------------------------------------------------------
 * The whole picture for F camera rows cams_dev [F,DURF_CAM_FLOATS] ON THE DEVICE, all of the call's h x w.  Defined as, and
 * bit-identical to, this sequence over the F h w pixels:
 *   1 durf_cast_cameras(F, h, w, cams_dev, tmin, tmax, cull, T, cast_ws) -> tri, depth, bary;
 *   2 durf_shade_surface on (tri, bary) with the pixel's ray direction (csrc/camera.h's pinhole_ray) as `toward` -> point, normal;
 *   3 durf_shade_occlusion(point, normal, S, dirs, bias, reach, cull) -> ao_used, ao_blocked;
 *   4 when sun != 0, durf_shade_occlusion(point, normal, 1, light, bias, +inf, cull) -> sun_blocked (else NULL);
 *   5 when albedo_vertex [V,3] is given, albedo = durf_raster_interp's rule on it: (w a_0 + u a_1) + v a_2 of the triangle's
 *     three vertices, 0 where the sample is not valid (else NULL);
 *   6 durf_shade_compose(tri, normal, ao_used, ao_blocked, sun_blocked, albedo, light, ambient, background) -> out_f, out_u8.
 * One launch for steps 1 and 2 (the rays are generated in the kernel), one for 3, one for 4, one for 5 and 6.  A wave takes a tile
 * of 8 x 8 pixels, not 64 of a row, so that the rays of a wave stay together; that order affects speed only.  A row whose (int)
 * H, W are not h, w makes its whole frame unusable: tri = -2, depth = NaN, normal = 0, counts 0, the background.
 * Outputs: tri [F,h,w] int32, depth [F,h,w], normal [F,h,w,3] NULLABLE, ao_used and ao_blocked [F,h,w] int32, out_f [F,h,w,3]
 * NULLABLE, out_u8 [F,h,w,3] NULLABLE (not both NULL).  workspace: durf_shade_workspace_bytes(F, h, w) bytes of the call's own
 * (bary, point, normal and the sun's two counts per pixel, point and normal once more per slot of the tiles).  F == 0 succeeds with no launch.
 * Refused: F < 0, h < 1, w < 1, F h w >= 2^31, V < 0, NULL vertices with V > 0, NULL triangles with T > 0, !(tmin >= 0), a NaN
 * tmax, sun outside 0 .. 1, NULL cams_dev, tri, depth, ao_used or ao_blocked with F > 0, a NULL workspace, one not aligned to 256
 * bytes or smaller than durf_shade_workspace_bytes(F, h, w) (both sizes named), and the rest as durf_shade_occlusion (the cast
 * workspace is cast_ws) and durf_shade_compose. */
size_t durf_shade_workspace_bytes(int F, int h, int w);      /* 0 for a refused shape */

int durf_shade_cameras(void* stream, int F, int h, int w, const float* cams_dev /* [F,DURF_CAM_FLOATS] device */, float tmin, float tmax,
                       int cull, int V, int T, const float* vertices /* [V,3] */, const int32_t* triangles /* [T,3] */,
                       const void* cast_ws, size_t cast_ws_bytes, int S, const float* dirs /* [S,3] device */, float bias, float reach,
                       const float* light /* [3] host */, int sun, float ambient, const float* albedo_vertex /* [V,3], nullable */,
                       const float* background /* [3] host */, void* workspace, size_t workspace_bytes, int32_t* tri /* [F,h,w] */,
                       float* depth /* [F,h,w] */, float* normal /* [F,h,w,3], nullable */, int32_t* ao_used /* [F,h,w] */,
                       int32_t* ao_blocked /* [F,h,w] */, float* out_f /* [F,h,w,3], nullable */, uint8_t* out_u8 /* [F,h,w,3], nullable */);

#ifdef __cplusplus
}
#endif
#endif
