// The scene's boxes on rendered frames (include/durf_overlay.h: durf_project_boxes, durf_draw_boxes; libdurf_overlay.so): two small kernels with a
// table between them.  k_project_boxes turns (camera row, box pose, half extents) into the twelve picture-space edges of every
// box, clipped against the near plane, and the box's 2D rectangle; k_draw_boxes rasterises that table onto frames as a gather
// -- a workgroup owns a tile, a pixel asks which box's edge it lies on -- so there are no atomics and no order to depend on.
// Plain fp32 in the order the header states; nothing here synchronises or copies to the host.
#include "durf_common.h"
#include "aa2matrix.h"
#include "camera.h"
#include "../../include/durf_overlay.h"

// ---- projection ----------------------------------------------------------------------------------------------------------
// overlay_aa2matrix, the world->object matrix of a box pose: aa2matrix.h (shared with flow.hip and field.hip); cam_to_camera and
// cam_pixel, the two halves of the projection, with the near-plane clip between them: camera.h

// one thread per (frame, box)
__global__ void __launch_bounds__(64)
k_project_boxes(int FK, int K, const float* __restrict__ cams, const float* __restrict__ poses, const float* __restrict__ ext,
                const int32_t* __restrict__ enable, float znear, float* __restrict__ segments, float* __restrict__ rect) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= FK) return;
    const int f = i / K, k = i - f * K;
    float cam[DURF_CAM_FLOATS];
#pragma unroll
    for (int j = 0; j < DURF_CAM_FLOATS; j++) cam[j] = cams[(size_t)f * DURF_CAM_FLOATS + j];
    const float* pose = poses + (size_t)i * 6;
    const float xhi = cam[DURF_CAM_W] - 1.0f, yhi = cam[DURF_CAM_H] - 1.0f;
    const float nan = __builtin_nanf("");
    const bool on = enable ? (enable[k] != 0) : true;

    float R[9];
    overlay_aa2matrix(pose[3], pose[4], pose[5], R);
    const float c[3] = {pose[0], pose[1], pose[2]};
    float pc[8][3];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const float v0 = (q & 1) ? ext[k * 3 + 0] : -ext[k * 3 + 0];
        const float v1 = (q & 2) ? ext[k * 3 + 1] : -ext[k * 3 + 1];
        const float v2 = (q & 4) ? ext[k * 3 + 2] : -ext[k * 3 + 2];
        float P[3];
#pragma unroll
        for (int a = 0; a < 3; a++) P[a] = c[a] + ((R[0 * 3 + a] * v0 + R[1 * 3 + a] * v1) + R[2 * 3 + a] * v2);     // c + R^T v
        cam_to_camera(cam, P[0], P[1], P[2], pc[q]);
    }
    float pcc[3];
    cam_to_camera(cam, c[0], c[1], c[2], pcc);

    float xmin = nan, ymin = nan, xmax = nan, ymax = nan;        // fminf / fmaxf return the other operand of a NaN
    bool any = false;
    float* seg = segments + (size_t)i * (DURF_BOX_EDGES * 4);
#pragma unroll
    for (int e = 0; e < DURF_BOX_EDGES; e++) {
        const int axis = e >> 2, j = e & 3;
        // the two other bits of the corner index hold j, in increasing corner index
        const int lo = axis == 0 ? (j << 1) : (axis == 1 ? ((j & 1) | ((j & 2) << 1)) : j);
        const int hi = lo | (1 << axis);
        float ax = pc[lo][0], ay = pc[lo][1], az = -pc[lo][2];
        float bx = pc[hi][0], by = pc[hi][1], bz = -pc[hi][2];
        const bool a_in = az >= znear, b_in = bz >= znear;
        float o[4] = {nan, nan, nan, nan};
        if (on && (a_in || b_in)) {
            if (!a_in || !b_in) {
                const float t = (znear - az) / (bz - az);
                const float cx = ax + t * (bx - ax), cy = ay + t * (by - ay);
                if (!a_in) { ax = cx; ay = cy; az = znear; }
                else { bx = cx; by = cy; bz = znear; }
            }
            cam_pixel(cam, ax, ay, az, o[0], o[1]);
            cam_pixel(cam, bx, by, bz, o[2], o[3]);
            any = true;
            xmin = fminf(xmin, fminf(o[0], o[2])); xmax = fmaxf(xmax, fmaxf(o[0], o[2]));
            ymin = fminf(ymin, fminf(o[1], o[3])); ymax = fmaxf(ymax, fmaxf(o[1], o[3]));
        }
        *(f32x4*)(seg + e * 4) = f32x4{o[0], o[1], o[2], o[3]};     // (16-byte aligned: 48 floats per box)
    }
    xmin = fmaxf(xmin, 0.0f); ymin = fmaxf(ymin, 0.0f);
    xmax = fminf(xmax, xhi); ymax = fminf(ymax, yhi);
    const bool vis = any && xmin <= xmax && ymin <= ymax;
    float* r = rect + (size_t)i * DURF_BOX_RECT_FLOATS;
    r[0] = vis ? xmin : nan; r[1] = vis ? ymin : nan; r[2] = vis ? xmax : nan; r[3] = vis ? ymax : nan;
    r[4] = -pcc[2];
    r[5] = vis ? 1.0f : 0.0f;
}

// ---- rasteriser ----------------------------------------------------------------------------------------------------------
#define OVL_TW 32                   // a tile: 32 x 8 pixels, one per lane (a wave covers two rows of 32)
#define OVL_TH 8
#define OVL_MAX_SEG (DURF_MAX_OBJ * DURF_BOX_EDGES)       // 192: the list holds every segment of a frame, it cannot overflow

__global__ void __launch_bounds__(OVL_TW * OVL_TH)
k_draw_boxes(int h, int w, int K, int tiles_x, const float* __restrict__ segments, const uint8_t* __restrict__ colors,
             float half_width, float opacity, uint8_t* __restrict__ frames8, float* __restrict__ framesf,
             int32_t* __restrict__ label) {
    __shared__ float s_seg[OVL_MAX_SEG][4];
    __shared__ int s_box[OVL_MAX_SEG];
    __shared__ int s_wave[OVL_TW * OVL_TH / DURF_WAVE];
    const int t = threadIdx.x, lane = t & (DURF_WAVE - 1), wave = t / DURF_WAVE;
    const int f = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * OVL_TW, y0 = ty * OVL_TH;
    const int x1 = min(x0 + OVL_TW, w) - 1, y1 = min(y0 + OVL_TH, h) - 1;       // the tile's last pixel, inside the frame

    // the frame's segments whose bounds grown by half_width touch the tile, in segment order (ballot + prefix count per wave)
    const int nseg = K * DURF_BOX_EDGES;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    bool keep = false;
    if (t < nseg) {
        s = *(const f32x4*)(segments + ((size_t)f * nseg + t) * 4);
        // a NaN fails every comparison: a culled segment is never listed
        keep = fminf(s[0], s[2]) - half_width <= (float)x1 && fmaxf(s[0], s[2]) + half_width >= (float)x0 &&
               fminf(s[1], s[3]) - half_width <= (float)y1 && fmaxf(s[1], s[3]) + half_width >= (float)y0 &&
               s[0] == s[0] && s[1] == s[1] && s[2] == s[2] && s[3] == s[3];
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int v = 0; v < OVL_TW * OVL_TH / DURF_WAVE; v++) {
        if (v < wave) base += s_wave[v];
        total += s_wave[v];
    }
    if (keep) {
        const int slot = base + __popcll(m & ((1ull << lane) - 1ull));          // < total <= nseg <= OVL_MAX_SEG
        s_seg[slot][0] = s[0]; s_seg[slot][1] = s[1]; s_seg[slot][2] = s[2]; s_seg[slot][3] = s[3];
        s_box[slot] = t / DURF_BOX_EDGES;
    }
    __syncthreads();
    if (total == 0 && !label) return;            // (uniform over the workgroup) nothing of the frame is read or written

    const int x = x0 + (t & (OVL_TW - 1)), y = y0 + t / OVL_TW;
    if (x >= w || y >= h) return;
    const float px = (float)x, py = (float)y;
    // the list is in box order: the first segment within half_width is of the lowest such box
    int owner = -1;
    for (int i = 0; i < total; i++) {
        const float ax = s_seg[i][0], ay = s_seg[i][1];
        const float ex = s_seg[i][2] - ax, ey = s_seg[i][3] - ay;
        const float L = ex * ex + ey * ey;
        float u = 0.0f;
        if (L > 0.0f) u = fminf(fmaxf(((px - ax) * ex + (py - ay) * ey) / L, 0.0f), 1.0f);
        const float dx = px - (ax + u * ex), dy = py - (ay + u * ey);
        const float d = sqrtf(dx * dx + dy * dy);
        if (d <= half_width) { owner = s_box[i]; break; }
    }
    const size_t p = ((size_t)f * h + y) * w + x;
    if (label) label[p] = owner;
    if (owner < 0) return;
    const float c0 = (float)colors[owner * 3], c1 = (float)colors[owner * 3 + 1], c2 = (float)colors[owner * 3 + 2];
    if (frames8) {
        uint8_t* q = frames8 + p * 3;
        const float a0 = (float)q[0], a1 = (float)q[1], a2 = (float)q[2];
        q[0] = (uint8_t)rintf(a0 + opacity * (c0 - a0));
        q[1] = (uint8_t)rintf(a1 + opacity * (c1 - a1));
        q[2] = (uint8_t)rintf(a2 + opacity * (c2 - a2));
    }
    if (framesf) {
        float* q = framesf + p * 3;
        const float g0 = c0 / 255.0f, g1 = c1 / 255.0f, g2 = c2 / 255.0f;
        if (opacity == 1.0f) { q[0] = g0; q[1] = g1; q[2] = g2; }
        else {
            const float a0 = q[0], a1 = q[1], a2 = q[2];
            q[0] = a0 + opacity * (g0 - a0);
            q[1] = a1 + opacity * (g1 - a1);
            q[2] = a2 + opacity * (g2 - a2);
        }
    }
}

extern "C" {

int durf_project_boxes(void* stream, int F, int K, const float* cams_dev, const float* poses, const float* ext,
                       const int32_t* box_enable, float znear, float* segments, float* rect) {
    DURF_REQUIRE(F >= 0 && K >= 0 && K <= DURF_MAX_OBJ, "F >= 0, 0 <= K <= DURF_MAX_OBJ");
    DURF_REQUIRE(znear > 0.0f, "znear > 0");
    if (F == 0 || K == 0) return 0;
    DURF_REQUIRE((size_t)F * K <= 0x7fffffffu / (DURF_BOX_EDGES * 4), "F * K * 48 < 2^31");
    DURF_REQUIRE(cams_dev && poses && ext && segments && rect, "cams_dev, poses, ext, segments and rect are given");
    DURF_REQUIRE(((size_t)segments & 15) == 0, "segments is 16-byte aligned");
    const int FK = F * K;
    hipLaunchKernelGGL(k_project_boxes, dim3(durf_cdiv(FK, 64)), dim3(64), 0, (hipStream_t)stream, FK, K, cams_dev, poses, ext,
                       box_enable, znear, segments, rect);
    DURF_CHECK_LAUNCH("durf_project_boxes");
    return 0;
}

int durf_draw_boxes(void* stream, int F, int h, int w, int K, const float* segments, const uint8_t* colors, float half_width,
                    float opacity, uint8_t* frames8, float* framesf, int32_t* label) {
    DURF_REQUIRE(F >= 0 && h >= 1 && w >= 1 && (size_t)h * w <= 0x7fffffffu, "F >= 0, h, w >= 1, h * w < 2^31");
    DURF_REQUIRE(K >= 0 && K <= DURF_MAX_OBJ, "0 <= K <= DURF_MAX_OBJ");
    DURF_REQUIRE(half_width >= 0.0f && half_width < __builtin_inff(), "half_width is finite and >= 0");
    DURF_REQUIRE(opacity >= 0.0f && opacity <= 1.0f, "0 <= opacity <= 1");
    if (F == 0) return 0;
    DURF_REQUIRE(frames8 || framesf || label, "at least one of frames8, framesf and label is given");
    if (K == 0 && !label) return 0;
    DURF_REQUIRE(K == 0 || (segments && colors), "segments and colors are given");
    DURF_REQUIRE(((size_t)segments & 15) == 0 && ((size_t)framesf & 3) == 0 && ((size_t)label & 3) == 0,
                 "segments is 16-byte aligned, framesf and label 4-byte");
    DURF_REQUIRE(F <= 65535, "F <= 65535 (the frame is the grid's y)");
    const int tiles_x = (int)durf_cdiv(w, OVL_TW), tiles_y = (int)durf_cdiv(h, OVL_TH);
    hipLaunchKernelGGL(k_draw_boxes, dim3((unsigned)tiles_x * tiles_y, F), dim3(OVL_TW * OVL_TH), 0, (hipStream_t)stream, h, w, K,
                       tiles_x, segments, colors, half_width, opacity, frames8, framesf, label);
    DURF_CHECK_LAUNCH("durf_draw_boxes");
    return 0;
}

}  // extern "C"
