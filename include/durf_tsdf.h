/* C ABI of durf_amd/libdurf_tsdf.so: depth frames fused into a truncated signed distance (TSDF) volume, on the device -- F frames
 * of camera depth (the renderer's `distance`, durf_raster.h's depth) into a lattice of (distance, weight, colour) in one
 * launch, the lattice as durf_mesh_count takes it (the surface is the zero level), and the signed distance at arbitrary points.
 * A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is; it needs that
 * library for durf_last_error alone and takes plain arrays, so it fuses any depth a caller brings.  The house rules of
 * durf_hip.h hold: device pointers of caller-owned buffers unless marked HOST, asynchronous on `stream` (hipStream_t), 0 or
 * nonzero with the text in durf_last_error(), every argument checked before anything is launched, no stream synchronisation
 * and no device-to-host copy anywhere.  All arithmetic is fp32, unfused, in the order written here, with IEEE division.  No
 * atomics of any kind, no spin loops, no workgroup waits for another; only ordinary vector loads and stores.  It is a gather
 * per voxel, not a scatter per pixel: the same inputs give the same bits, and no memory depends on the number of frames.
 *
 * Lattice (durf_mesh.h's).  nu, nv, nw >= 2, n = nu nv nw < DURF_TSDF_MAX_POINTS (= DURF_MESH_MAX_POINTS); voxel (i, j, k) has
 *   index g = (i nv + j) nw + k and lies at P_c = ((origin_c + (float) i du_c) + (float) j dv_c) + (float) k dw_c (origin, du, dv,
 *   dw: three HOST floats each) -- durf_mesh_emit's position at t = 0, so a mesh vertex there lands on the voxel.
 * State, three caller-owned arrays; a NEW VOLUME IS ALL ZERO BYTES.
 *   tsdf   [n] float    D: the distance in units of trunc, in [-1, 1], positive in front of the surface (towards the observer)
 *   weight [n] float    W
 *   colour [n,4] float  NULLABLE: r, g, b and the colour's own weight Wc; ALIGNED TO 16 BYTES (a row is one 16-byte access)
 *
 * Integration.  cams_dev [F,DURF_CAM_FLOATS] floats ON THE DEVICE (durf_hip.h, THE CAMERA ROW), projected in csrc/camera.h's
 *   order; the last two floats of a row are not read, the frame size is the h and w of the call.  depth [F,h,w] float: camera depth.  acc [F,h,w] float NULLABLE.  rgb [F,h,w,3] float
 *   NULLABLE.  label [F,h,w] int32 NULLABLE.  xform [F,3,4] float ON THE DEVICE, NULLABLE: M maps the volume's coordinates to
 *   frame f's world, X_c = ((M[c][0] P_0 + M[c][1] P_1) + M[c][2] P_2) + M[c][3]; NULL: X = P.  (A volume in a box's frame follows
 *   the box: X = c_f + R_f^T P.)  frame_weight [F] float ON THE DEVICE, NULLABLE: NULL means 1.
 *   For every voxel the frames are taken in ascending f.  Frame f is SKIPPED for the voxel, the state left as it is, under the
 *   first rule that applies:
 *   1 INVALID   an X_c, or a pc_j, that is not finite, with d = X - o;  pc_j = (R_c[0][j] d_0 + R_c[1][j] d_1) + R_c[2][j] d_2
 *   2 BEHIND    !(z >= znear), z = -pc_2
 *   3 RANGE     !(fabsf(x) <= DURF_TSDF_MAX_COORD), likewise y:  x = ppx + (focal pc_0) / z;  y = ppy - (focal pc_1) / z
 *   4 OUTSIDE   px = (int) rintf(x) outside 0 .. w-1 or py = (int) rintf(y) outside 0 .. h-1.  The NEAREST pixel centre, ties to
 *               even as rintf has them (x = -0.5 is pixel 0, 0.5 is pixel 0, 1.5 is pixel 2); depth is never interpolated,
 *               which is what makes the result restatable bit for bit
 *   5 HOLE      dep = depth[f,py,px] is not finite, or !(dep > 0)
 *   6 FAINT     acc is given and !(acc[f,py,px] >= min_acc)
 *   7 OCCLUDED  sdf = dep - z is below -trunc: the voxel is hidden behind the surface by more than the band
 *   8 OTHER     label is given and label[f,py,px] != select, and other_mode == 0; or other_mode == 1 and !(sdf >= trunc).  With
 *               other_mode == 1 a pixel that shows something else lying beyond the voxel by at least trunc is an observation
 *               of FREE SPACE: it goes on, without colour
 *   9 WEIGHT    wf = frame_weight[f] is not finite or !(wf > 0)
 *   Otherwise the state is UPDATED:
 *     dn = fminf(sdf / trunc, 1.0f);  Wn = W + wf;  D = (W D + wf dn) / Wn;  W = fminf(Wn, max_weight)
 *     and, if colour and rgb are both given, the pixel's label is `select` (or no label is given) and sdf <= trunc:
 *     C_c = (Wc C_c + wf rgb[f,py,px,c]) / (Wc + wf) for c = 0, 1, 2, then Wc = fminf(Wc + wf, max_weight).
 *   Frames are applied in order per voxel and a voxel sees nothing of any other: ONE CALL OVER F FRAMES GIVES THE SAME BITS AS
 *   ANY SPLIT OF THOSE FRAMES INTO CONSECUTIVE CALLS.
 *
 * The lattice for durf_mesh_count.  density[g] = -D;  valid[g] = (W >= min_weight);  rgb_out[g] = the colour where Wc > 0, else
 *   0.  With iso = 0 a point is IN when it is at or behind the surface, so mesh normals, which point from in to out, face
 *   the observer.
 *
 * The signed distance at a point P.  e = P - origin;  q_c = (inv[c][0] e_0 + inv[c][1] e_1) + inv[c][2] e_2, inv the inverse of
 *   [du dv dw] (nine HOST floats, row-major; the caller computes them in float64).  P is OUTSIDE when a q_c is not finite, < 0
 *   or > n_c - 1 (n_0 = nu, ...).  Otherwise the cell is i = min((int) floorf(q_0), nu - 2), so that q_0 == nu - 1 falls in the
 *   last cell, likewise j, k;  t_c = q_c - (float) cell_c;  with d_abc the value at (i + a, j + b, k + c), lerp(x, y, t) = x + t (y - x):
 *     v_ab = lerp(d_ab0, d_ab1, t_2);  v_a = lerp(v_a0, v_a1, t_1);  v = lerp(v_0, v_1, t_0)
 *   (t = 0 gives x exactly: at a lattice point that is not on the lattice's last faces v is D itself).  ok = inside and all
 *   eight corners have W >= min_weight;  sdf = v trunc when ok, else NaN.  rgb_out: the same lerp per colour channel when the
 *   point is inside and all eight corners have Wc > 0, else 0.
 *
 * How it runs.  k_tsdf_integrate: one thread per voxel, adjacent lanes along k, DURF_TSDF_BLOCK per workgroup.  The frame loop
 *   runs INSIDE the kernel with D, W and the four colour floats in registers: the volume is read once and written once per
 *   call whatever F is (a voxel no frame updated is not stored).  The camera, xform and frame_weight rows are the same for
 *   every lane and are read through wave-uniform addresses; the depth, acc, label and rgb gathers of neighbouring k land on
 *   neighbouring pixels.  k_tsdf_lattice and k_tsdf_sample: one thread per voxel / per point. */
#ifndef DURF_TSDF_H
#define DURF_TSDF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_TSDF_BLOCK 256              /* voxels or points per workgroup */
#define DURF_TSDF_MAX_POINTS (1 << 27)   /* n below this: DURF_MESH_MAX_POINTS, the lattice goes on to durf_mesh_count */
#define DURF_TSDF_MAX_SIZE 4096          /* h and w at most, as durf_raster.h has them */
#define DURF_TSDF_MAX_COORD (1 << 20)    /* |x|, |y| of a projected voxel that is looked up */

/* ---- integrate (k_tsdf_integrate) ----------------------------------------------------------------------------------------------
 * F frames into the volume, one launch.  F == 0 succeeds with no launch.
 * Refused: nu, nv or nw < 2, n >= 2^27, F < 0, h or w outside 1 .. DURF_TSDF_MAX_SIZE, F h w >= 2^31, !(trunc > 0) or trunc not
 * finite, !(max_weight > 0), !(znear >= FLT_MIN), NaN min_acc with acc, other_mode outside 0 .. 1, other_mode == 1 without label,
 * a NULL origin_host, du_host, dv_host, dw_host, tsdf or weight, a NULL cams_dev or depth with F > 0 (each named), a
 * colour not aligned to 16 bytes.  rgb without colour is allowed: the colour is simply not kept. */
int durf_tsdf_integrate(void* stream, int nu, int nv, int nw, const float* origin_host /* 3 */, const float* du_host /* 3 */,
                        const float* dv_host /* 3 */, const float* dw_host /* 3 */, int F, int h, int w,
                        const float* cams_dev /* [F,DURF_CAM_FLOATS] device */, const float* depth /* [F,h,w] */, const float* acc /* nullable */,
                        float min_acc, const float* rgb /* [F,h,w,3], nullable */, const int32_t* label /* nullable */, int select,
                        int other_mode, const float* xform /* [F,3,4] device, nullable */, const float* frame_weight /* [F], nullable */,
                        float trunc, float max_weight, float znear, float* tsdf /* [n] */, float* weight /* [n] */,
                        float* colour /* [n,4], nullable */);

/* ---- the lattice durf_mesh_count takes (k_tsdf_lattice) ----------------------------------------------------------------------------
 * density [n] float, valid [n] uint8, rgb_out [n,3] float NULLABLE.
 * Refused: the shape, NaN min_weight, a NULL tsdf, weight, density or valid, rgb_out without colour, a colour not aligned
 * to 16 bytes. */
int durf_tsdf_lattice(void* stream, int nu, int nv, int nw, const float* tsdf, const float* weight, const float* colour /* nullable */,
                      float min_weight, float* density, uint8_t* valid, float* rgb_out /* nullable */);

/* ---- the signed distance at points (k_tsdf_sample) -----------------------------------------------------------------------------------
 * points [m,3] float -> sdf [m] float, ok [m] uint8, rgb_out [m,3] float NULLABLE.  m == 0 succeeds with no launch.
 * Refused: the shape, m < 0, !(trunc > 0) or trunc not finite, NaN min_weight, a NULL origin_host, inv_host, tsdf or weight,
 * NULL points, sdf or ok with m > 0, rgb_out without colour, a colour not aligned to 16 bytes. */
int durf_tsdf_sample(void* stream, int nu, int nv, int nw, const float* origin_host /* 3 */, const float* inv_host /* 9 */,
                     const float* tsdf, const float* weight, const float* colour /* nullable */, float trunc, float min_weight, int m,
                     const float* points /* [m,3] */, float* sdf /* [m] */, uint8_t* ok /* [m] */, float* rgb_out /* [m,3], nullable */);

#ifdef __cplusplus
}
#endif
#endif
