/* C ABI of durf_amd/libdurf_overlay.so: the scene's boxes drawn on rendered frames.  A library of its own beside
 * libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is: it renders nothing, it takes the frames
 * and the box poses durf_render_trajectory returned.  The house rules of durf_hip.h hold: device pointers of caller-owned
 * buffers, asynchronous on `stream` (hipStream_t), 0 or an error code with the text in durf_last_error() -- the one of
 * libdurf_hip.so, which this library links against -- and every argument checked before anything is launched. */
#ifndef DURF_OVERLAY_H
#define DURF_OVERLAY_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the scene's boxes on rendered frames (csrc/overlay.hip -> libdurf_overlay.so; by hand in the reference: notebooks/waymo_labels.ipynb
 * project_point / show_camera_image) ----------------------------------------------------------------
 * durf_project_boxes: the twelve edges of box k of frame f as the camera of row f of cams_dev ([F,DURF_CAM_FLOATS] DEVICE floats:
 * durf_hip.h, THE CAMERA ROW) sees them.  World corner c in 0..7 (bit 0 / 1 / 2: the sign on the box's
 * x / y / z half extent, 0 = -, 1 = +): P_c = centre + R^T (s_c * ext[k]), (centre, rotvec) = poses[f,k], R = aa2matrix(rotvec)
 * the world->object matrix of the box test (durf_ray_setup, durf_hip.h).  Camera space pc = R_c^T (P - o), depth z = -pc_z; picture
 * x = ppx + (focal pc_x) / z, y = ppy - (focal pc_y) / z, in csrc/camera.h's order: the inverse of the ray generator.  Edge e = 4 axis + j joins the two corners that differ in bit `axis`, j counting the four such pairs by
 * increasing corner index, from the corner with the bit clear to the corner with it set.  Edges are clipped in camera space
 * against z >= znear (znear > 0): both ends nearer -- the edge is culled, its four floats are NaN; one end nearer -- it is cut
 * at z = znear.
 *   segments [F,K,12,4]: x0, y0, x1, y1 of every edge.
 *   rect [F,K,DURF_BOX_RECT_FLOATS]: xmin, ymin, xmax, ymax, zc, visible -- the bounds of the kept segments' end points (every
 *     vertex of the part of the box in front of znear is one) intersected with [0, w - 1] x [0, h - 1]; zc the depth of the box
 *     centre; visible 1.0 when a segment is kept and the intersection is not empty, else 0.0 and the four bounds NaN.
 * box_enable (nullable, int32 [K] on the device): a box with 0 is culled whole.  K <= DURF_MAX_OBJ; F * K == 0: success, no launch.
 *
 * durf_draw_boxes: the segments as lines of width 2 half_width on F frames of h x w, as a gather: a workgroup owns a tile of
 * one frame, lists the frame's segments whose bounds grown by half_width touch the tile, and every pixel (x, y) of the tile
 * takes per box the least point-segment distance, in fp32: e = b - a, L = e.e, t = L > 0 ? clamp(((p - a).e) / L, 0, 1) : 0,
 * d = sqrt(|p - (a + t e)|^2).  The pixel belongs to the lowest k with d <= half_width (a NaN segment never matches); no
 * atomics, no dependence on any order.  Targets, all nullable (at least one given), written at owned pixels only:
 *   frames8 [F,h,w,3] uint8 in place: rintf(src + opacity (col - src)); any alignment.
 *   framesf [F,h,w,3] float in place: src + opacity (col / 255 - src), and col / 255 itself at opacity == 1.
 *   label [F,h,w] int32: the owning k -- here EVERY pixel is written, -1 where no box owns it.
 * colors [K,3] uint8 on the device; 0 <= opacity <= 1; half_width >= 0.  A tile no segment touches reads and writes
 * nothing of the frames.  K == 0 with a label fills it with -1. */
#define DURF_BOX_EDGES 12
#define DURF_BOX_RECT_FLOATS 6
int durf_project_boxes(void* stream, int F, int K, const float* cams_dev /* [F,DURF_CAM_FLOATS] device */, const float* poses /* [F,K,6] */,
                       const float* ext /* [K,3] */, const int32_t* box_enable /* nullable */, float znear,
                       float* segments /* [F,K,12,4] */, float* rect /* [F,K,6] */);
int durf_draw_boxes(void* stream, int F, int h, int w, int K, const float* segments /* [F,K,12,4] */,
                    const uint8_t* colors /* [K,3] */, float half_width, float opacity, uint8_t* frames8 /* nullable */,
                    float* framesf /* nullable */, int32_t* label /* nullable */);

#ifdef __cplusplus
}
#endif
#endif
