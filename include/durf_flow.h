/* C ABI of durf_amd/libdurf_flow.so: how the scene moves between two rendered frames -- optical flow, scene flow, the
 * backward warp of one frame onto another with its occlusion mask, a temporal-consistency number and the flow picture.  Nothing
 * is learned or approximated and no MLP runs: a sample moves rigidly with the box that contains it, everything else is static.
 * A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is and which it
 * calls through that header alone (durf_camera_rays, durf_ray_setup_masked).  The house rules of durf_hip.h hold: device
 * pointers of caller-owned buffers, asynchronous on `stream` (hipStream_t), 0 or -1 with the text in durf_last_error() -- the
 * one of libdurf_hip.so, which this library links against -- every argument checked before anything is launched, no stream
 * synchronisation and no device-to-host copy anywhere.  All arithmetic is fp32, unfused, in the order written here. */
#ifndef DURF_FLOW_H
#define DURF_FLOW_H
#include <stddef.h>
#include <stdint.h>
#include "durf_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- where a pixel goes (csrc/flow.hip k_flow_poses, k_flow_points) -------------------------------------------------------
 * n pixels [first, first + n) of source frame a, row-major in its w-wide image (w = cam_a_host[DURF_CAM_W]); pixel p = first + i is
 * (x, y) = (p mod w, p div w).  origins_s, dirs_s [n,3] and hit [n,K] int32 are durf_ray_setup_masked's outputs for that
 * frame's rays at pose_a; t [n] is the renderer's `distance` and acc [n] its `acc`.  distance is sum_j w_j t_mid_j -- NOT
 * divided by acc -- measured along dirs_s, which on a ray that hit a box is the UNIT direction in that box's frame and
 * elsewhere the un-normalised world direction of the pixel (-z component 1 in the camera: t is then depth along the axis).
 * cam_a_host, cam_b_host: one camera row of HOST floats each (durf_hip.h, THE CAMERA ROW).  pose_a, pose_b [K,6]
 * (centre, rotation vector) and ext [K,3] (half extents) on the device.  Per pixel:
 *   tt = normalise ? t / acc : t,   P_j = origins_s_j + tt dirs_s_j            (a point in the frame the ray was marched in)
 *   nh = the number of k with hit[k] != 0, k = the largest such
 *   nh == 0:  X_a = X_b = P, moving = -1
 *   nh == 1:  R = aa2matrix(rotvec) is the world->object matrix (csrc/aa2matrix.h: the one of the box overlay),
 *             X_a_j = c_a_j + ((R_a[0][j] P_0 + R_a[1][j] P_1) + R_a[2][j] P_2)                         (c_a + R_a^T P)
 *             inside = |P_j| <= ext_kj * (1 + inside_tol) for j = 0, 1, 2
 *             inside:  X_b = c_b + R_b^T P likewise, moving = k           (the point rides the box)
 *             else:    X_b = X_a (the same bits), moving = -1             (scenery seen through the box)
 *   nh >= 2:  invalid (the model's sum of several boxes' frames is no geometry anyone can reproject)
 *   camera c of a world point X, in csrc/camera.h's order: d = X - o_c, pc_j = (R_c[0][j] d_0 + R_c[1][j] d_1) +
 *     R_c[2][j] d_2, z = -pc_2, x' = ppx + (focal pc_0) / z, y' = ppy - (focal pc_1) / z
 *   target = (x', y', z_b) of X_b in camera b,  flow = (x' - (float) x, y' - (float) y),  zcam = z of X_a in camera a
 *   scene_flow = X_b - X_a (world frame; exactly 0 where nothing moved),  xyz = X_a
 *   valid = acc >= min_acc && nh <= 1 && isfinite(tt) && z_b >= znear
 * An invalid pixel gets NaN in every float output, moving = -2 and valid = 0.  Outputs, each NULLABLE (not written when NULL),
 * at least one required: flow [n,2] (8-byte aligned: one store per pixel), scene_flow, xyz, target [n,3], zcam [n], moving,
 * valid [n] int32.
 * The 2 K rotation matrices and centres come from a one-wave launch in front (k_flow_poses: thread s K + k writes, for s = 0
 * (pose_a), 1 (pose_b), the twelve floats R row-major then c at pose_scratch + (s K + k) 12) into the caller-owned
 * pose_scratch of DURF_FLOW_POSE_FLOATS(K) floats, so the per-pixel kernel has no sinf / cosf; it walks k = 0 .. K-1 and reads
 * box k's rows -- the same address in every lane -- only where some pixel of its wave hit box k.  One thread per pixel.
 * 0 <= K <= DURF_MAX_OBJ; n == 0: success, no launch; K == 0: hit, pose_a, pose_b, ext and pose_scratch may be NULL.
 * Refused: n < 0, first < 0, first + n beyond cam_a's image, w < 1, znear <= 0, inside_tol < 0 (or NaN), no output. */
#define DURF_FLOW_POSE_FLOATS(K) (2 * (K) * 12)
int durf_flow_points(void* stream, int n, int first, int K, const float* origins_s, const float* dirs_s,
                     const int32_t* hit /* nullable when K == 0 */, const float* t, const float* acc,
                     const float* cam_a_host, const float* cam_b_host, const float* pose_a, const float* pose_b,
                     const float* ext, int normalise, float min_acc, float znear, float inside_tol, float* pose_scratch,
                     float* flow /* nullable */, float* scene_flow /* nullable */, float* xyz /* nullable */,
                     float* target /* nullable */, float* zcam /* nullable */, int32_t* moving /* nullable */,
                     int32_t* valid /* nullable */);

/* ---- backward warp with an occlusion test (k_flow_warp) --------------------------------------------------------------------
 * One thread per pixel i of frame a: target [n,3] = (x', y', z_b) and valid [n] from durf_flow_points, img_b [h,w,C] float
 * (C 1 or 3), zcam_b [h,w] frame b's own zcam (durf_flow_points with b as source AND target).
 *   in-frame = 0 <= x' <= w - 1 && 0 <= y' <= h - 1                          (a NaN fails it; -0.0 passes)
 *   x0 = max(min((int) floorf(x'), w - 2), 0), x1 = min(x0 + 1, w - 1), fx = x' - (float) x0 (w == 1: fx = 0); y likewise
 *   value_c = (1 - fy) ((1 - fx) v00 + fx v10) + fy ((1 - fx) v01 + fx v11),  v_ab = img_b[y_b, x_a, c]
 *     (an integer target reproduces the pixel's bits: the other weight is exactly 0)
 *   zs = zcam_b[(int) rintf(y'), (int) rintf(x')]                            (in range by the in-frame test)
 *   visible = valid != 0 && in-frame && isfinite(zs) && z_b <= zs (1 + occ_rel) + occ_abs
 * Outputs, NULLABLE, at least one: warped [n,C] (NaN where not visible), mask [n] int32 (visible).  n == 0: success, no launch.
 * Refused: n < 0, h < 1, w < 1, h w >= 2^31, C not 1 or 3, occ_rel < 0, occ_abs < 0, no output. */
int durf_flow_warp(void* stream, int n, int h, int w, int C, const float* target, const int32_t* valid, const float* img_b,
                   const float* zcam_b, float occ_rel, float occ_abs, float* warped /* nullable */, int32_t* mask /* nullable */);

/* ---- temporal consistency: a deterministic reduction, no atomics (k_flow_cons_partial, k_flow_cons_final) ------------------
 * P pairs of m pixels of C channels (1 or 3): warped, img_a [P,m,C], mask [P,m] int32.  out [P,DURF_FLOW_CONS_FLOATS] =
 *   count = the pixels with mask != 0,  sse = sum over them and their channels of (warped - a)^2,  sae = sum of |warped - a|,
 *   psnr = -10 log10(sse / (count C))       (NaN when count == 0, +inf when sse == 0 and count > 0)
 * Two passes in this order.  Pass 1: workgroup g of pair p (256 threads) owns pixels [g S, min((g + 1) S, m)) with S =
 * DURF_FLOW_CONS_SPAN; thread t visits g S + t, g S + t + 256, ... in that order and adds, per masked pixel, for c = 0 .. C-1
 * in order, d = warped - a (fp32), sse += d d, sae += |d|, and count += 1, all in fp32 (a count of at most S / 256 is exact);
 * then the 64 lanes of a wave add butterfly-wise, v += shuffle_xor(v, o) for o = 32, 16, .., 1, and the four waves' sums are
 * added (w0 + w1) + (w2 + w3): one triple per workgroup at scratch[(p G + g) 3], G = DURF_FLOW_CONS_GROUPS(m).  Pass 2: one
 * workgroup per pair adds its G triples in index order in double and rounds count, sse, sae and psnr (evaluated in double) to
 * float.  The same inputs give the same bits on every run.  scratch: DURF_FLOW_CONS_SCRATCH(P, m) floats, caller-owned.
 * P == 0: success, no launch.  Refused: P < 0, P > 65535, m < 1, C not 1 or 3, a NULL buffer. */
#define DURF_FLOW_CONS_FLOATS 4
#define DURF_FLOW_CONS_SPAN 4096
#define DURF_FLOW_CONS_GROUPS(m) (((m) + DURF_FLOW_CONS_SPAN - 1) / DURF_FLOW_CONS_SPAN)
#define DURF_FLOW_CONS_SCRATCH(P, m) ((size_t)(P) * DURF_FLOW_CONS_GROUPS(m) * 3)
int durf_flow_consistency(void* stream, int P, int m, int C, const float* warped, const float* img_a, const int32_t* mask,
                          float* out, float* scratch);

/* ---- the flow picture: the Middlebury colour wheel (Baker et al., "A Database and Evaluation Methodology for Optical Flow",
 * k_flow_color).  The wheel has DURF_FLOW_WHEEL = 55 entries of levels 0 .. 255: 15 from red to yellow (255, floor(255 i / 15),
 * 0), 6 yellow to green (255 - floor(255 i / 6), 255, 0), 4 green to cyan (0, 255, floor(255 i / 4)), 11 cyan to blue
 * (0, 255 - floor(255 i / 11), 255), 13 blue to magenta (floor(255 i / 13), 0, 255), 6 magenta to red (255, 0, 255 -
 * floor(255 i / 6)).  For flow [n,2] = (u, v) and max_mag > 0:
 *   rad = sqrtf(u u + v v) / max_mag          (not clamped: beyond 1 it only selects the dimmed branch below)
 *   a = atan2f(-v, -u) / pi (pi rounded to float),  fk = ((a + 1) / 2) 54,  k0 = min((int) fk, 54),  k1 = (k0 + 1) mod 55,
 *   f = fk - (float) k0;  per channel: c0 = wheel[k0] / 255, c1 = wheel[k1] / 255,  col = (1 - f) c0 + f c1,
 *   col = rad <= 1 ? 1 - rad (1 - col) : col 0.75
 * rgb [n,3] float and rgb8 [n,3] uint8 = (uint8) rintf(col 255), each NULLABLE, at least one.  A flow with a NaN or an
 * infinity in it (an invalid pixel) gives 0 in both.  n == 0: success, no launch.  Refused: n < 0, max_mag <= 0 (or NaN). */
#define DURF_FLOW_WHEEL 55
int durf_flow_color(void* stream, int n, const float* flow, float max_mag, float* rgb /* nullable */, uint8_t* rgb8 /* nullable */);

/* ---- P pairs of frames in one call -----------------------------------------------------------------------------------------
 * F frames of one size h x w (n = h w) seen from cams_host [F,DURF_CAM_FLOATS] with the boxes at poses [F,K,6] on the DEVICE
 * (durf_render_trajectory's poses_out), their distance and acc planes [F,n] (durf_render_trajectory's), and P pairs
 * pairs_host [P,2] HOST ints (source frame, target frame; source == target is legal and is how a frame's own zcam is had).
 * Per pair and per chunk of `chunk` pixels (the last one the remainder): durf_camera_rays of the source camera, then
 * durf_ray_setup_masked at the source pose under box_enable (nullable) into the workspace, then k_flow_points; k_flow_poses
 * once per pair.  Outputs as durf_flow_points', [P,n,.], each NULLABLE, at least one required; every output is bit-identical
 * to durf_flow_points on the whole frame and independent of `chunk`.
 * workspace: durf_render_flow_workspace_bytes(chunk, K) bytes, 256-byte aligned: one chunk of rays, of durf_ray_setup_masked's
 * outputs and the pose table -- it grows with neither the image nor F.  Refused (-1, durf_last_error) before any launch and
 * without a device: F <= 0, P <= 0, a pair index outside [0, F), frames of different sizes, K > DURF_MAX_OBJ, znear <= 0,
 * inside_tol < 0, chunk <= 0, no output, a workspace smaller than that (both sizes named). */
size_t durf_render_flow_workspace_bytes(int chunk, int K);
int durf_render_flow(void* stream, int F, int K, const float* cams_host /* F rows */, const float* poses /* device [F,K,6] */,
                     const float* ext, const int32_t* box_enable /* nullable */, const float* distance, const float* acc, int P,
                     const int* pairs_host /* P x 2 */, float near, float far, int chunk, int normalise, float min_acc,
                     float znear, float inside_tol, float* flow /* nullable */, float* scene_flow /* nullable */,
                     float* xyz /* nullable */, float* target /* nullable */, float* zcam /* nullable */,
                     int32_t* moving /* nullable */, int32_t* valid /* nullable */, void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
