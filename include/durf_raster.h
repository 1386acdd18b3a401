/* C ABI of durf_amd/libdurf_raster.so: a triangle mesh seen through pinhole cameras, on the device -- per pixel the nearest
 * triangle, its camera depth and its perspective-correct barycentric weights, and from those any vertex attribute (colour,
 * normals, the owner or component label).  The cameras are the rows of durf_camera_rays (durf_hip.h), whose directions have
 * z = -1: the renderer's `distance` is camera depth, so this depth map compares with it pixel by pixel.
 * A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs that
 * library for durf_last_error alone and takes plain arrays, so it draws any mesh a caller brings.  The house rules of
 * durf_hip.h hold: device pointers of caller-owned buffers, asynchronous on `stream` (hipStream_t), 0 or nonzero with the text
 * in durf_last_error(), every argument checked before anything is launched, no stream synchronisation and no device-to-host
 * copy anywhere.  All float arithmetic is fp32, unfused, in the order written here, with IEEE division; coverage is integer.
 *
 * Inputs.  cams_dev [F,DURF_CAM_FLOATS] floats ON THE DEVICE (durf_hip.h, THE CAMERA ROW) -- the frame size is the h and w of
 *   the call, shared by all F cameras; the last two floats of a row are not read.  vertices [V,3] float, triangles [T,3] int32.  A PAIR is a (frame f, triangle t).
 * Projection (csrc/camera.h's order).  d = P - o;  pc_j = (R_c[0][j] d_0 + R_c[1][j] d_1) + R_c[2][j] d_2;  z = -pc_2;
 *   x = ppx + (focal pc_0) / z;  y = ppy - (focal pc_1) / z.  Pixel centres are at integer coordinates.
 * Cull.  A pair is counted once, under the first rule that applies, in this order:
 *   1 INVALID     a vertex id outside 0 .. V-1, a vertex coordinate that is not finite, or a pc_j that is not finite
 *   2 BEHIND      all three z < znear
 *   3 CROSSING    some but not all z < znear.  The triangle is DROPPED, not clipped: a surface that passes through the
 *                 camera's near plane loses the triangles that straddle it (clipping is out of scope; the tally says how many)
 *   4 RANGE       a vertex with !(fabsf(256 x) <= 2^29), likewise y
 *   5 DEGENERATE  A2 == 0 after the snap
 *   6 CULLED      cull == 1 and A2 > 0 (a BACK face), or cull == 2 and A2 < 0 (a FRONT face).  Picture y points down, so
 *                 A2 < 0 is a triangle whose right-hand normal points at the camera (counter-clockwise as the camera sees it)
 *   otherwise DRAWN, whether or not it touches a pixel of the frame.  The seven tallies add up to F T.
 * Snap.  X = (int32) rintf(256 x), Y likewise: DURF_RASTER_SUBPIXEL = 256, 8 sub-pixel bits, |X|, |Y| <= DURF_RASTER_MAX_COORD.
 * Coverage, exact in int64 (a coordinate difference is below 2^31, a product below 2^61, an edge function below 2^62).
 *   A2 = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0).  If A2 < 0 vertices 1 and 2 are EXCHANGED for everything up to the weights q, which
 *   are mapped back.  For the edge a -> b opposite vertex i (0: 1->2, 1: 2->0, 2: 0->1) at pixel (px, py):
 *   E_i = (Xb-Xa)(256 py - Ya) - (Yb-Ya)(256 px - Xa).  The pixel is COVERED when for every i: E_i > 0, or E_i == 0 and the edge
 *   has dY > 0 || (dY == 0 && dX < 0) with dX = Xb-Xa, dY = Yb-Ya.  E_0 + E_1 + E_2 == |A2| exactly.  A pixel centre on an edge
 *   shared by two triangles on opposite sides of it belongs to exactly one of them: the two see the edge with (dX, dY) negated,
 *   and exactly one of (dX, dY), (-dX, -dY) passes the rule ((0, 0) is an edge of a degenerate triangle).
 * Depth, perspective-correct, in the exchanged order:  w_i = (float) E_i / (float) |A2| (int64 -> float rounds to nearest);
 *   iz_i = 1.0f / z_i;  s = (w_0 iz_0 + w_1 iz_1) + w_2 iz_2;  depth = 1.0f / s;  q_i = (w_i iz_i) * depth.
 * Owner.  Of the triangles covering a pixel, the one with the smallest (bits of depth, t) in lexicographic order: depth is
 *   positive, so bit order is value order; ties go to the lowest triangle id.  It is a minimum over a set: it does not depend
 *   on any order of evaluation.
 * Outputs per frame.  tri [F,h,w] int32, -1 where nothing covers; depth [F,h,w] float, 0 there; bary [F,h,w,3] float NULLABLE:
 *   q in the mesh's own vertex order, 0 there.
 *
 * How it is drawn: a binned gather, not a frame-sized atomic z-buffer.
 *   1 k_raster_setup   one thread per pair: project, cull, snap; a RECORD of DURF_RASTER_RECORD_INTS int32 into the workspace
 *                      (X0 Y0 X1 Y1 X2 Y2, the bits of iz_0 iz_1 iz_2, and the inclusive bounds of the tiles it touches, 8 bits
 *                      each: tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24; tx0 > tx1 marks a pair that draws nothing); +1 to the count
 *                      of every DURF_RASTER_TILE x DURF_RASTER_TILE tile that the pixel bounds ceil(min X / 256) ..
 *                      floor(max X / 256), clamped to the frame, touch; the tallies, folded per workgroup first.
 *   2 the scan         exclusive scan of the F th tw tile counts in int64 (csrc/scan.h): each tile's range in `pairs`; the
 *                      total, saturated at INT32_MAX, is counts[0].
 *   3 k_raster_fill    one thread per pair: a slot in every touched tile's range through an integer cursor per tile.
 *   4 k_raster_tile    one workgroup of 256 per tile, one pixel per thread; the tile's list goes through LDS in batches of
 *                      DURF_RASTER_BATCH records; a thread rejects by the record's bounds, evaluates the three edge functions
 *                      and keeps the minimum in registers; writes tri, depth, bary.
 *   5 k_raster_interp  the gather below.
 *   Same inputs, same bits, despite the atomics.  The only atomics are integer adds on global (and LDS) counters, exact in any
 *   order: the tile counts, the tallies and therefore the scan are the same whatever the schedule.  The cursor hands the slots
 *   of a tile's range out in an order that varies, so the ORDER of a tile's list varies -- its SET does not (each touching
 *   pair takes exactly one slot of the range, the range has exactly that many) and the owner is a minimum over the set.  No
 *   float atomics, no spin loops, no flags polled; no workgroup waits for another; every loop is bounded by a count read
 *   before it starts (a record's tile bounds, a tile's count).  Only ordinary vector memory operations are used.
 */
#ifndef DURF_RASTER_H
#define DURF_RASTER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_RASTER_SUBPIXEL 256         /* snapped coordinates per pixel */
#define DURF_RASTER_MAX_COORD (1 << 29)  /* |X|, |Y| of a drawn vertex */
#define DURF_RASTER_TILE 16              /* a tile is 16 x 16 pixels, one workgroup of 256 */
#define DURF_RASTER_BATCH 256            /* records of a tile's list in LDS at a time */
#define DURF_RASTER_BLOCK 256            /* pairs, tiles or pixels per workgroup of every other kernel */
#define DURF_RASTER_MAX_SIZE 4096        /* h and w at most: 256 tiles along an axis, 8 bits in a record */
#define DURF_RASTER_RECORD_INTS 10       /* 40 bytes per pair */
#define DURF_RASTER_COUNTS 8             /* counts: pairs, drawn, invalid, behind, crossing, range, degenerate, culled */

/* The workspace of F frames of h x w and T triangles, every part on a 256-byte boundary in this order: records int32
 * [F T, DURF_RASTER_RECORD_INTS]; tile counts int32 [n]; cursors int32 [n]; tile starts int64 [n]; the scan's block sums and the total
 * int64 [nb + 2]; with th = ceil(h / 16), tw = ceil(w / 16), n = F th tw, nb = ceil(n / DURF_RASTER_BLOCK).
 * 0 for a refused shape: F < 0, T < 0, h or w outside 1 .. DURF_RASTER_MAX_SIZE, F T >= 2^31 or F h w >= 2^31. */
size_t durf_raster_workspace_bytes(int F, int T, int h, int w);

/* ---- setup (k_raster_clear, k_raster_setup, k_raster_sums, k_scan_block_sums, k_raster_offsets) ---------------------------------
 * Steps 1 and 2.  counts [DURF_RASTER_COUNTS] int32 on the device: the number of (tile, pair) entries durf_raster_draw needs
 * room for in `pairs` (INT32_MAX: more than can be had), then the seven tallies in the order of the cull list, DRAWN first.
 * cull: 0 keeps both faces, 1 drops back faces, 2 drops front faces.  F T == 0 succeeds with counts all 0.
 * Refused: the shape as above (every value named), V < 0, !(znear >= FLT_MIN) (znear > 0, and 1 / znear finite), cull outside
 * 0 .. 2, a NULL cams_dev with F > 0, NULL vertices with V > 0, NULL triangles with T > 0, a NULL counts or workspace, a workspace
 * not aligned to 256 bytes or smaller than durf_raster_workspace_bytes (both sizes named). */
int durf_raster_setup(void* stream, int F, int h, int w, const float* cams_dev /* [F,DURF_CAM_FLOATS] device */, int V, int T,
                      const float* vertices /* [V,3] */, const int32_t* triangles /* [T,3] */, float znear, int cull, void* workspace,
                      size_t workspace_bytes, int32_t* counts /* [DURF_RASTER_COUNTS] */);

/* ---- draw (k_raster_begin, k_raster_fill, k_raster_tile) -----------------------------------------------------------------------------
 * Steps 3 and 4 on the workspace durf_raster_setup left for the same F, T, h, w.  pairs [max_pairs] int32 is scratch.  If the
 * workspace's total exceeds max_pairs NOTHING is drawn: every pixel gets tri = -2, depth = NaN (and bary = NaN), never a
 * partial picture, and nothing is written to `pairs` at all -- never at or past max_pairs in any case.  May be called again on
 * the same workspace (with a larger `pairs`).  F T == 0: tri = -1, depth = 0 everywhere.  F == 0: success, no launch.
 * Refused: the shape, max_pairs < 0 (max_pairs is an int: a capacity of 2^31 cannot be asked for), NULL pairs with
 * max_pairs > 0, a NULL tri or depth with F > 0, the workspace as above. */
int durf_raster_draw(void* stream, int F, int T, int h, int w, const void* workspace, size_t workspace_bytes, int32_t* pairs,
                     int max_pairs, int32_t* tri /* [F,h,w] */, float* depth /* [F,h,w] */, float* bary /* [F,h,w,3], nullable */);

/* ---- interpolate (k_raster_interp) -----------------------------------------------------------------------------------------------
 * A pure gather, one thread per pixel p of n_pixels = F h w, t = tri[p], (v0, v1, v2) = triangles[t], q = bary[p]:
 *   out_f [n_pixels,C] = (q_0 a_0 + q_1 a_1) + q_2 a_2 per channel, a_i = attr_f[v_i] (attr_f [V,C] float, NULLABLE with out_f;
 *   needs bary), 0 where nothing covers;
 *   out_i [n_pixels] int32 = attr_i[v0], the triangle's FIRST vertex (attr_i int32 [V], NULLABLE with out_i), `fill` where
 *   nothing covers: right for the owner and the component label, since durf_parts.h proves one component per triangle.
 * "Nothing covers" is t outside 0 .. T-1 (-1, and the -2 of an overflow) or a vertex id outside 0 .. V-1.
 * Refused: n_pixels < 0, V < 0, T < 0, neither attribute, attr_f without out_f or bary, C < 1 with attr_f, attr_i without
 * out_i, NULL tri with n_pixels > 0, NULL triangles with T > 0. */
int durf_raster_interp(void* stream, int n_pixels, int V, int T, const int32_t* triangles, const int32_t* tri,
                       const float* bary /* nullable */, int C, const float* attr_f /* nullable */, float* out_f /* nullable */,
                       const int32_t* attr_i /* nullable */, int fill, int32_t* out_i /* nullable */);

/* ---- all of it (durf_raster_setup, durf_raster_draw, durf_raster_interp when an attribute is given) --------------------------------
 * F cameras in one call with a pair capacity the caller chose; the same launches, hence the same bits, as the three calls.
 * A capacity that proves too small gives the -2 / NaN picture and counts[0] says what was needed.  Every refusal of the
 * three calls applies and is made before the first launch. */
int durf_render_mesh(void* stream, int F, int h, int w, const float* cams_dev, int V, int T, const float* vertices,
                     const int32_t* triangles, float znear, int cull, void* workspace, size_t workspace_bytes, int32_t* pairs,
                     int max_pairs, int32_t* counts, int32_t* tri, float* depth, float* bary /* nullable */, int C,
                     const float* attr_f /* nullable */, float* out_f /* nullable */, const int32_t* attr_i /* nullable */, int fill,
                     int32_t* out_i /* nullable */);

#ifdef __cplusplus
}
#endif
#endif
