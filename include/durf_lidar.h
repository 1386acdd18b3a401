/* C ABI of durf_amd/libdurf_lidar.so: LIDAR sweeps of the scene -- the rays of a spinning multi-beam sensor in front of the
 * renderer, a robust return model behind it, and the returns as a point cloud.  A library of its own beside libdurf_hip.so
 * (include/durf_hip.h), whose set of entry points it leaves as it is and which it calls through that header alone
 * (durf_forward_masked, durf_forward_workspace_bytes).  The house rules of durf_hip.h hold: device pointers of caller-owned
 * buffers, asynchronous on `stream` (hipStream_t), 0 or an error code with the text in durf_last_error() -- the one of
 * libdurf_hip.so, which this library links against -- every argument checked before anything is launched, no stream
 * synchronisation and no device-to-host copy anywhere. */
#ifndef DURF_LIDAR_H
#define DURF_LIDAR_H
#include <stddef.h>
#include <stdint.h>
#include "durf_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the sensor (csrc/lidar.hip k_lidar_rays) -----------------------------------------------------------------------------
 * sensor_host: DURF_LIDAR_SENSOR_FLOATS HOST floats: H (beams), W (azimuth columns), az0, az_span (radians, signed: Waymo's
 * range images run from +pi downwards), radius_scale, max_range.  inclinations: [H] DEVICE floats, radians, any order.
 * sweeps_host: DURF_LIDAR_SWEEP_FLOATS HOST floats per sweep: pose_start [3,4] row-major (R_start | p_start, sensor to world;
 * sensor frame x forward, y left, z up), omega [3] and dp [3] -- the sensor's motion over the sweep, relative to pose_start.
 * Ray r = h W + w (row-major: the output is a range image), all in fp32, unfused, in this order:
 *   s = ((float) w + 0.5f) / (float) W,  phi = az0 + s az_span,  theta = inclinations[h]
 *   d = (cos theta cos phi, cos theta sin phi, sin theta)
 *   v = s omega,  t2 = (vx vx + vy vy) + vz vz,  t = sqrt(t2),  a = sin t / t,  b = 2 sin(t / 2)^2 / t2   (t2 < 1e-12: a = 1, b = 1/2)
 *   c = v x d,  e = v x c,  d' = (d + a c) + b e                                   (Rodrigues: rodrigues(s omega) d)
 *   direction_i = (R_i0 d'_0 + R_i1 d'_1) + R_i2 d'_2,  origin_i = p_i + s dp_i
 * directions == viewdirs (the same bits; unit length up to rounding, so t along a ray is Euclidean range in scene units);
 * radii = (float) (radius_scale |az_span| / W * 2 / sqrt(12)) evaluated in double on the host -- mip-NeRF's pixel-footprint
 * rule on the azimuth step, the same for every beam; near_out / far_out are copies of near / far.
 * durf_lidar_rays writes the six fields of rays [first, first + count) of one sweep: origins / directions / viewdirs [count,3],
 * radii / near_out / far_out [count]; one thread per ray.  count == 0: success, no launch. */
#define DURF_LIDAR_SENSOR_FLOATS 6
#define DURF_LIDAR_SWEEP_FLOATS 18
int durf_lidar_rays(void* stream, const float* sensor_host /* 6 */, const float* inclinations /* device [H] */,
                    const float* sweeps_host /* 18 */, int first, int count, float near, float far, float* origins,
                    float* directions, float* viewdirs, float* radii, float* near_out, float* far_out);

/* ---- the return model (k_lidar_returns) -----------------------------------------------------------------------------------
 * A LIDAR return of a ray is a quantile of its weight distribution, not the weight-averaged t the renderer's `distance` is:
 * at a depth edge the mean lands between the two surfaces ("flying points"), the median on one of them.  For n rays of N
 * samples, weights [n,N] (non-negative), t_vals [n,N+1], acc [n] (any such buffers: the last level's outputs of durf_forward):
 *   W = sum_j w_j,  c_j = sum_{i<=j} w_i;  for a quantile p: j* = the smallest j with c_j >= p W and w_j > 0,
 *   range(p) = t_{j*} + (p W - c_{j*-1}) / w_{j*} (t_{j*+1} - t_{j*})      (the fraction clamped to [0, 1])
 *   range_q = range(q),  spread = range(q_hi) - range(q_lo)  (a per-return uncertainty out of the same scan; 0 when W == 0)
 *   range_mean = sum_j w_j (t_j + t_{j+1}) / 2 / W   (0 when W == 0): the mean over the weights alone -- comparable to the
 *     renderer's distance, which it does not replace (that one is not normalised by W and is nan_to_num'd and clipped)
 *   valid = acc >= min_acc && W > 0 && range_q <= max_range;  an invalid ray gets range_q = 0
 *   xyz = origin + range_q direction, per component o + r d in fp32 (world frame); with to_sensor_host (12 HOST floats, a
 *     [3,4] world-to-sensor row M) the point M (xyz, 1) instead: (M_i0 x + M_i1 y) + M_i2 z + M_i3.
 * One wavefront per ray: lane l owns samples [floor(l N / 64), floor((l + 1) N / 64)) -- for N = 32 every other lane owns one
 * sample and the others none (half the lanes idle; rays do not share a wave) --, sums its own, an inclusive scan across the
 * lanes gives c at every lane's end, a ballot finds the crossing lane of each quantile and that lane interpolates: all three
 * quantiles out of ONE scan, no LDS, no atomics.  Sums are fp32 in that order: c_j is within (N - 1) 2^-24 W of the exact one.
 * Every output is nullable (not written when NULL), at least one is required; origins / directions [n,3] are read for xyz
 * alone.  N a multiple of 32 in [32, 256]; 0 < q < 1, 0 < q_lo < q_hi < 1; n == 0: success, no launch. */
int durf_lidar_returns(void* stream, int n, int N, const float* weights, const float* t_vals, const float* acc,
                       const float* origins /* nullable */, const float* directions /* nullable */,
                       const float* to_sensor_host /* nullable, 12 */, float q, float q_lo, float q_hi, float min_acc,
                       float max_range, float* range_q, float* range_mean, int32_t* valid, float* xyz, float* spread);

/* ---- the point cloud (k_lidar_count, k_lidar_scan, k_lidar_scatter) -------------------------------------------------------
 * Order-preserving compaction of the valid returns of n rays (0 <= n < 2^27): point m is the m-th ray with valid != 0, its row
 * of points [.,DURF_LIDAR_POINT_FLOATS] = x, y, z, range, r, g, b, dynamic ((float) dyn_mask: the number of boxes the ray hit),
 * source[m] its ray index, count[0] the number of points M -- which stays on the device.  Rows at and beyond M are not
 * touched.  Three plain passes: the valid rays of every block of DURF_LIDAR_COMPACT_BLOCK rays counted, ONE workgroup's
 * exclusive scan over the block counts, scatter; deterministic, no atomics, no look-back.  points (16-byte aligned) and
 * source have room for n rows; scratch: DURF_LIDAR_COMPACT_SCRATCH(n) int32 on the device, caller-owned.
 * rgb [n,3] and dyn_mask [n] are nullable (the columns are then 0).  n == 0: count[0] = 0 is all that is written. */
#define DURF_LIDAR_COMPACT_BLOCK 256
#define DURF_LIDAR_POINT_FLOATS 8
#define DURF_LIDAR_COMPACT_SCRATCH(n) (((n) + DURF_LIDAR_COMPACT_BLOCK - 1) / DURF_LIDAR_COMPACT_BLOCK + 1)
int durf_lidar_compact(void* stream, int n, const int32_t* valid, const float* xyz /* [n,3] */, const float* range /* [n] */,
                       const float* rgb /* nullable [n,3] */, const int32_t* dyn_mask /* nullable [n] */,
                       float* points /* [n,8] */, int32_t* source /* [n] */, int32_t* count /* [1] */, int32_t* scratch);

/* ---- F sweeps in one call -------------------------------------------------------------------------------------------------
 * `args` as for durf_render_image (durf_hip.h) with the ray fields AND args->pose ignored; sweep f is sweeps_host[f] seen by
 * the sensor, with the boxes frozen at poses[f] ([F,K,6] on the DEVICE: durf_render_trajectory's poses_out serves fractional
 * times).  Per sweep and per chunk of `chunk` rays (the last one the remainder): k_lidar_rays into the workspace,
 * durf_forward_masked (test mode, under box_enable, nullable), k_lidar_returns on the last level's weights / t_vals / acc.
 * Outputs [F, H W, .], each NULLABLE and not written when NULL, at least one required:
 *   range, range_mean, spread [F,n], valid [F,n] int32, xyz [F,n,3] (world frame)      durf_lidar_returns' planes
 *   distance, acc [F,n], rgb [F,n,3]       the renderer's own last-level planes, untouched: bit-identical to durf_render_layers
 *                                          on durf_lidar_rays' rays with args->pose = poses[f]
 *   dynamic [F,n] int32                    dyn_mask: the number of boxes the ray hit
 * max_range is the sensor row's.  workspace: durf_render_lidar_workspace_bytes(chunk, N, K, num_levels) bytes, 256-byte
 * aligned: durf_forward_workspace_bytes(chunk, N, K) plus one chunk of rays and of per-level outputs -- it grows neither with
 * H W nor with F.  Refused (-1, durf_last_error) before any launch and without a device: F <= 0, H <= 0, W <= 0, q outside
 * (0, 1), q_lo >= q_hi, K > DURF_MAX_OBJ, an unsupported N, no output, a workspace smaller than that (both sizes named). */
size_t durf_render_lidar_workspace_bytes(int chunk, int N, int K, int num_levels);
int durf_render_lidar(void* stream, const durf_forward_args* args, const int32_t* box_enable /* nullable */, int F,
                      const float* sensor_host /* 6 */, const float* inclinations /* device [H] */,
                      const float* sweeps_host /* F x 18 */, const float* poses /* device [F,K,6] */, float near, float far,
                      int chunk, float q, float q_lo, float q_hi, float min_acc, float* range /* nullable */,
                      float* range_mean /* nullable */, float* distance /* nullable */, float* acc /* nullable */,
                      float* rgb /* nullable */, float* spread /* nullable */, int32_t* dynamic /* nullable */,
                      int32_t* valid /* nullable */, float* xyz /* nullable */, void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif
