// durf_forward: MipNerfModel.__call__ in inference (obbpose_model.py:68-261 as render_eval_fn runs it, train_boxpose.py:377-390)
// as ONE C call -- the orchestration durf_amd/obbpose_model.py does in Python for `train=False`, for hosts that are not Python
// (SURVEY 8b proposed it; INTEGRATION.md shows the binding).  No kernel of its own: the stage entry points of this library
// in the order the Python path issues them, on one stream, with every intermediate carved out of a caller-owned workspace
// (workspace.h).  bf16 MLPs; with boxes the background forward evaluates each ray class once and writes raw in the full
// layout itself (DURF_FWD_RAW_FULL); K = 0 is the static model.  Results are bit-identical to MipNerfModel.apply
// (tests/test_gpu_forward_call.py).  The image, layer and trajectory calls below are loops over forward_chunk, the one place
// that points a chunk's outputs at the caller's planes or at the workspace.
#include "durf_common.h"
#include "side_stream.h"
#include "workspace.h"
#include "../../include/durf_hip.h"

namespace {

using durf::Carver;

struct FwdWs : durf::RayHeadWs {
    float *raw_b, *obj_raw, *u_rand;
    void *wf_bkgd, *wf_obj, *enc, *obj_enc;
    size_t total;
};

FwdWs carve(void* workspace, int B, int N, int K) {
    Carver c{(char*)workspace, 0};         // (every buffer on 256 bytes)
    FwdWs w{};
    const size_t rows = (size_t)B * N, Kc = K > 0 ? K : 1;
    durf::carve_ray_head(c, w, B, K);
    w.wf_bkgd = c.take(durf_wpack_fwd_bytes(256));
    w.wf_obj = c.take(Kc * durf_wpack_fwd_bytes(128));
    w.enc = c.take(((rows + 31) / 32 * 32) * 64 * 2);
    w.raw_b = (float*)c.take(rows * 4 * 4);
    w.obj_enc = c.take(K > 0 ? (size_t)K * durf_obj_enc_stride(B, N) : 0);
    w.obj_raw = (float*)c.take(K > 0 ? (size_t)K * rows * 4 * 4 : 0);
    w.u_rand = (float*)c.take((size_t)3 * B * (N + 1) * 4);              // draw_noise: the resampling draws of the prologue
    w.total = c.total();
    return w;
}

// the image calls: one chunk's FwdWs + its per-level outputs (only the last level's rgb / distance / acc leave the workspace)
struct ImgWs { FwdWs f; float *rgb[DURF_FORWARD_MAX_LEVELS], *depth[DURF_FORWARD_MAX_LEVELS], *acc[DURF_FORWARD_MAX_LEVELS],
               *weights[DURF_FORWARD_MAX_LEVELS], *t_vals[DURF_FORWARD_MAX_LEVELS], *t_mids[DURF_FORWARD_MAX_LEVELS],
               *t_dists[DURF_FORWARD_MAX_LEVELS], *zo; int32_t* dyn; size_t total; };
ImgWs carve_image(void* workspace, int chunk, int N, int K, int L) {
    ImgWs w{};
    w.f = carve(workspace, chunk, N, K);
    Carver c{(char*)workspace, w.f.total};
    for (int l = 0; l < L; l++) {
        w.rgb[l] = (float*)c.take((size_t)chunk * 3 * 4); w.depth[l] = (float*)c.take((size_t)chunk * 4);
        w.acc[l] = (float*)c.take((size_t)chunk * 4); w.weights[l] = (float*)c.take((size_t)chunk * N * 4);
        w.t_vals[l] = (float*)c.take((size_t)chunk * (N + 1) * 4); w.t_mids[l] = (float*)c.take((size_t)chunk * N * 4);
        w.t_dists[l] = (float*)c.take((size_t)chunk * N * 4);
    }
    w.zo = (float*)c.take((size_t)chunk * 4);
    w.dyn = (int32_t*)c.take((size_t)chunk * 4);
    w.total = c.total();
    return w;
}
// the per-image layer outputs a chunk's bookkeeping launch fills (csrc/layers.hip; instance is never null here)
struct LayerOuts { int32_t* instance; float *bg_rgb, *bg_dist, *bg_acc, *obj_rgba; };

// durf_render_layers: + the per-image buffers of the second pass
struct LayerWs { ImgWs img; int32_t *instance, *idx, *count; float* rays[6]; float *rgb2, *dist2, *acc2; size_t total; };
LayerWs carve_layers(void* workspace, size_t n_rays, int chunk, int N, int K, int L) {
    LayerWs w{};
    w.img = carve_image(workspace, chunk, N, K, L);         // (the second pass re-carves the same bytes for K = 0: never larger)
    Carver c{(char*)workspace, w.img.total};
    w.instance = (int32_t*)c.take(n_rays * 4);
    w.idx = (int32_t*)c.take(n_rays * 4);
    w.count = (int32_t*)c.take(64 * 4);
    for (int f = 0; f < 6; f++) w.rays[f] = (float*)c.take(n_rays * (f < 3 ? 3 : 1) * 4);
    w.rgb2 = (float*)c.take(n_rays * 3 * 4); w.dist2 = (float*)c.take(n_rays * 4); w.acc2 = (float*)c.take(n_rays * 4);
    w.total = c.total();
    return w;
}

// durf_render_trajectory: + one chunk of rays and the frames' poses
struct TrajWs { ImgWs img; float* rays[6]; float* poses; size_t total; };
TrajWs carve_trajectory(void* workspace, int F, int chunk, int N, int K, int L) {
    TrajWs w{};
    w.img = carve_image(workspace, chunk, N, K, L);
    Carver c{(char*)workspace, w.img.total};
    for (int f = 0; f < 6; f++) w.rays[f] = (float*)c.take((size_t)chunk * (f < 3 ? 3 : 1) * 4);       // one chunk's rays
    w.poses = (float*)c.take((size_t)(F > 0 ? F : 0) * (K > 0 ? K : 0) * 6 * 4);                        // (when poses_out is NULL)
    w.total = c.total();
    return w;
}

}  // namespace

extern "C" {

size_t durf_forward_workspace_bytes(int B, int N, int K) { return carve(nullptr, B, N, K).total; }

static int check_forward_args(const durf_forward_args* a, void* workspace) {
    DURF_REQUIRE(a != nullptr && workspace != nullptr, "arguments and workspace");
    const int B = a->B, N = a->N, K = a->K, L = a->num_levels;
    DURF_REQUIRE(B > 0 && N % 32 == 0 && N >= 32 && N <= 256, "B > 0, num_samples a multiple of 32 in [32, 256]");
    DURF_REQUIRE(K >= 0 && K <= DURF_MAX_OBJ, "0 <= K <= DURF_MAX_OBJ");
    DURF_REQUIRE(L >= 1 && L <= DURF_FORWARD_MAX_LEVELS, "1 <= num_levels <= DURF_FORWARD_MAX_LEVELS");
    DURF_REQUIRE(((size_t)workspace & 255) == 0, "workspace aligned to 256 bytes");
    DURF_REQUIRE(!a->draw_noise || (a->t_rand == nullptr && a->u_rand == nullptr), "draw_noise: the library makes the draws");
    for (int l = 0; l < L && a->density_noise != 0.0f; l++)
        DURF_REQUIRE(a->density_rand[l] != nullptr || a->draw_noise, "density_noise: density_rand[level] or draw_noise");
    return 0;
}

// the launches of one chunk (arguments checked, workspace carved by the caller)
static int forward_launches(void* stream, const durf_forward_args* a, const FwdWs& w, const int32_t* box_enable = nullptr) {
    const int B = a->B, N = a->N, K = a->K, L = a->num_levels;
    const size_t rows = (size_t)B * N;
    int rc;
#define STEP(call) do { rc = (call); if (rc != 0) return rc; } while (0)
    // ray setup + view encoding + level-0 sample positions (obbpose_model.py:99-131, mip.py:330-370) + the bf16 weight
    // streams of every MLP: one launch
    STEP(durf_ray_prologue_pack_masked(stream, B, K, N, a->origins, a->directions, a->pose, a->ext, w.o_s, w.d_s, w.hit, a->zo, a->viewdirs,
                                w.view, a->near, a->far, a->t_rand, a->lindisp, a->t_vals[0], nullptr, nullptr, 0, a->seed_lo, a->seed_hi,
                                a->draw_noise ? w.u_rand : nullptr, a->bkgd_params, 60, w.wf_bkgd, nullptr, K, a->obj_params,
                                a->obj_param_stride, 63, w.wf_obj, nullptr, K == 0 ? (float*)a->dyn_mask : nullptr, K == 0 ? (size_t)B : 0,
                                       K > 0 ? box_enable : nullptr));
    if (K > 0)      // per-object hit lists + the ray classes of the de-duplicated background evaluation: one launch
        STEP(durf_compact_all(stream, B, K, N, w.hit, w.idx_obj, w.count_obj, w.slot_obj, w.idx_cls, w.count_cls, w.slot_cls,
                              a->dyn_mask));
    const float* raw_obj[DURF_MAX_OBJ > 0 ? DURF_MAX_OBJ : 1];
    for (int k = 0; k < K; k++) raw_obj[k] = w.obj_raw + (size_t)k * rows * 4;
    // (a large chunk's object MLPs on the library's side stream, issued before the persistent background launch: side_stream.h)
    const durf::Overlap ov = durf::overlap_for(stream, durf::step_policy(rows), K);
    const auto obj_fwd = [&](void* s, const float* t_vals) {          // the K object MLPs of one level, hit rays only
        return durf_obj_fwd_batch(s, K, B, N, w.idx_obj, w.count_obj, t_vals, w.o_s, w.d_s, a->radii, a->barf_w,
                                  a->enc_flags & (DURF_ENC_NO_INTEGRATION | DURF_ENC_CYLINDER), w.view, w.wf_obj, w.obj_enc, w.obj_raw,
                                  nullptr, nullptr, nullptr);
    };
    for (int lvl = 0; lvl < L; lvl++) {
        float* t_vals = a->t_vals[lvl];
        if (K > 0) {
            STEP(ov.fork());
            if (ov.sd) STEP(obj_fwd(ov.obj(), t_vals));
            STEP(durf_mlp_fwd_enc(stream, rows, N, t_vals, w.o_s, w.d_s, a->radii, w.hit, K, a->enc_flags | DURF_FWD_RAW_FULL, w.enc, w.view, w.idx_cls, w.count_cls,
                                  w.wf_bkgd, w.raw_b, nullptr, nullptr, w.idx_cls + B, w.count_cls + 1, nullptr));
            if (!ov.sd) STEP(obj_fwd(stream, t_vals));
            STEP(ov.join());
        } else {
            STEP(durf_mlp_fwd_enc(stream, rows, N, t_vals, w.o_s, w.d_s, a->radii, nullptr, 0, a->enc_flags, w.enc, w.view, nullptr, nullptr, w.wf_bkgd, w.raw_b, nullptr, nullptr, nullptr,
                              nullptr, nullptr));
        }
        if (a->density_noise != 0.0f)      // obbpose_model.py:236-240
            STEP(durf_density_noise(stream, rows, w.raw_b, a->density_noise, a->density_rand[lvl], a->seed_lo, a->seed_hi, lvl));
        STEP(durf_composite_fwd(stream, B, N, K, w.raw_b, raw_obj, w.slot_obj, t_vals, w.d_s, a->density_bias, a->bkgd_mode,
                                a->rgb[lvl], a->depth[lvl], a->acc[lvl], a->weights[lvl], a->t_mids[lvl], a->t_dists[lvl]));
        if (lvl + 1 < L)
            STEP(durf_resample(stream, B, N, t_vals, a->weights[lvl], a->resample_padding, a->draw_noise ? w.u_rand + (size_t)lvl * B * (N + 1) : a->u_rand, a->t_vals[lvl + 1]));
    }
#undef STEP
    return 0;
}

int durf_forward_masked(void* stream, const durf_forward_args* a, const int32_t* box_enable, void* workspace, size_t workspace_bytes) {
    int rc = check_forward_args(a, workspace);
    if (rc != 0) return rc;
    const FwdWs w = carve(workspace, a->B, a->N, a->K);
    rc = durf::check_workspace("durf_forward", workspace_bytes, w.total, "durf_forward_workspace_bytes(%d, %d, %d)", a->B, a->N, a->K);
    return rc != 0 ? rc : forward_launches(stream, a, w, box_enable);
}

int durf_forward(void* stream, const durf_forward_args* a, void* workspace, size_t workspace_bytes) {
    return durf_forward_masked(stream, a, nullptr, workspace, workspace_bytes);
}

// the test-mode and level-count requirements of the render calls (who: "render_image", ...)
static int require_render_mode(const durf_forward_args* a, const char* who) {
    if (a->t_rand != nullptr || a->u_rand != nullptr || a->draw_noise || a->density_noise != 0.0f) {
        durf_set_error("durf_%s: requirement failed: %s is test mode: randomized = False (obbpose_model.py:421-479)", who, who);
        return -1;
    }
    if (a->num_levels < 1 || a->num_levels > DURF_FORWARD_MAX_LEVELS) {
        durf_set_error("durf_%s: requirement failed: 1 <= num_levels <= DURF_FORWARD_MAX_LEVELS", who);
        return -1;
    }
    return 0;
}

// One chunk of a render call: `a` is the call's argument block (render mode required by the caller); B rays at the six ray
// fields under `pose`; the last level's rgb / distance / acc go to the given planes, a null plane keeps that output in the
// workspace -- as every other per-level output of the chunk is.
static int forward_chunk(void* stream, const durf_forward_args* a, const int32_t* box_enable, int B, const float* const rays[6],
                         const float* pose, float* rgb, float* distance, float* acc, const ImgWs& w, void* workspace) {
    durf_forward_args c = *a;
    const int L = a->num_levels;
    c.B = B;
    c.origins = rays[0]; c.directions = rays[1]; c.viewdirs = rays[2]; c.radii = rays[3]; c.near = rays[4]; c.far = rays[5];
    c.pose = pose;
    for (int l = 0; l < L; l++) {
        const bool last = l == L - 1;
        c.rgb[l] = last && rgb ? rgb : w.rgb[l]; c.depth[l] = last && distance ? distance : w.depth[l]; c.acc[l] = last && acc ? acc : w.acc[l];
        c.weights[l] = w.weights[l]; c.t_vals[l] = w.t_vals[l]; c.t_mids[l] = w.t_mids[l]; c.t_dists[l] = w.t_dists[l];
    }
    c.zo = w.zo; c.dyn_mask = w.dyn;
    const int rc = check_forward_args(&c, workspace);
    return rc != 0 ? rc : forward_launches(stream, &c, w.f, box_enable);
}

// ---- one C call per IMAGE (obbpose_model.py:421-479 render_image on one device) --------------------------------------
// The reference walks the image in chunks from Python, one pmapped call and one host round trip per chunk; here the chunk
// loop is this function: the rays of the whole image stay where they are on the device, every chunk runs durf_forward's
// launch sequence on slices of them, the levels' per-chunk outputs live in the workspace, and the LAST level's rgb /
// distance / acc land in the image planes in place -- what render_image returns (:476-479).
// the chunk loop of durf_render_image / durf_render_layers over rays resident on the device (arguments checked, workspace
// carved by the caller; the three planes are never null here)
static int render_chunks(void* stream, const durf_forward_args* a, const int32_t* box_enable, size_t n_rays, int chunk, float* rgb,
                         float* distance, float* acc, const ImgWs& w, void* workspace, const LayerOuts* lo) {
    for (size_t i = 0; i < n_rays; i += (size_t)chunk) {
        const int B = (int)(n_rays - i < (size_t)chunk ? n_rays - i : (size_t)chunk);        // (the last chunk is the remainder, :451-453)
        const float* const rays[6] = {a->origins + i * 3, a->directions + i * 3, a->viewdirs + i * 3, a->radii + i, a->near + i, a->far + i};
        int rc = forward_chunk(stream, a, box_enable, B, rays, a->pose, rgb + i * 3, distance + i, acc + i, w, workspace);
        if (rc != 0) return rc;
        if (lo) {         // instance map, bg_* pre-filled with the composite, obj_rgba: one launch behind the chunk's composite
            rc = durf::launch_layer_chunk(stream, B, a->K, w.f.hit, rgb + i * 3, distance + i, acc + i, a->bkgd_mode, lo->instance + i,
                                          lo->bg_rgb ? lo->bg_rgb + i * 3 : nullptr, lo->bg_dist ? lo->bg_dist + i : nullptr,
                                          lo->bg_acc ? lo->bg_acc + i : nullptr, lo->obj_rgba ? lo->obj_rgba + i * 4 : nullptr);
            if (rc != 0) return rc;
        }
    }
    return 0;
}

size_t durf_render_image_workspace_bytes(int chunk, int N, int K, int num_levels) {
    return carve_image(nullptr, chunk, N, K, num_levels).total;
}

int durf_render_image(void* stream, const durf_forward_args* a, size_t n_rays, int chunk, float* rgb, float* distance, float* acc,
                      void* workspace, size_t workspace_bytes) {
    DURF_REQUIRE(a != nullptr && rgb && distance && acc, "arguments and the three image planes");
    DURF_REQUIRE(chunk > 0 && n_rays > 0, "chunk > 0, n_rays > 0");
    int rc = require_render_mode(a, "render_image");
    if (rc != 0) return rc;
    const int L = a->num_levels;
    const ImgWs w = carve_image(workspace, chunk, a->N, a->K, L);
    rc = durf::check_workspace("durf_render_image", workspace_bytes, w.total, "durf_render_image_workspace_bytes(%d, %d, %d, %d)", chunk,
                               a->N, a->K, L);
    if (rc != 0) return rc;
    return render_chunks(stream, a, nullptr, n_rays, chunk, rgb, distance, acc, w, workspace, nullptr);
}

// ---- scene layers (include/durf_hip.h durf_render_layers; kernels: csrc/layers.hip) -------------------------------------
size_t durf_render_layers_workspace_bytes(size_t n_rays, int chunk, int N, int K, int num_levels) {
    return carve_layers(nullptr, n_rays, chunk, N, K, num_levels).total;
}

int durf_render_layers(void* stream, const durf_forward_args* a, const int32_t* box_enable, size_t n_rays, int chunk, float* rgb,
                       float* distance, float* acc, int32_t* instance, float* bg_rgb, float* bg_distance, float* bg_acc,
                       float* obj_rgba, void* workspace, size_t workspace_bytes) {
    DURF_REQUIRE(a != nullptr && rgb && distance && acc, "arguments and the three image planes");
    DURF_REQUIRE(chunk > 0 && n_rays > 0 && n_rays < ((size_t)1 << 27), "chunk > 0, 0 < n_rays < 2^27");
    int rc = require_render_mode(a, "render_layers");
    if (rc != 0) return rc;
    DURF_REQUIRE((bg_rgb != nullptr) == (bg_distance != nullptr) && (bg_rgb != nullptr) == (bg_acc != nullptr),
                 "bg_rgb, bg_distance and bg_acc go together");
    DURF_REQUIRE(((size_t)obj_rgba & 15) == 0, "obj_rgba aligned to 16 bytes");
    const int L = a->num_levels;
    const LayerWs w = carve_layers(workspace, n_rays, chunk, a->N, a->K, L);
    rc = durf::check_workspace("durf_render_layers", workspace_bytes, w.total, "durf_render_layers_workspace_bytes(%zu, %d, %d, %d, %d)",
                               n_rays, chunk, a->N, a->K, L);
    if (rc != 0) return rc;
    const ImgWs w0 = carve_image(workspace, chunk, a->N, 0, L);          // the second pass re-carves the image part for K = 0
    DURF_REQUIRE(w0.total <= w.img.total, "the K = 0 workspace fits inside the K one");
    const bool any = instance || bg_rgb || obj_rgba;
    LayerOuts lo{instance ? instance : w.instance, bg_rgb, bg_distance, bg_acc, obj_rgba};
    rc = render_chunks(stream, a, box_enable, n_rays, chunk, rgb, distance, acc, w.img, workspace, any ? &lo : nullptr);
    if (rc != 0 || !bg_rgb || a->K == 0) return rc;          // (K = 0: no box-hit rays, bg_* is the composite)
    // the box-hit rays of the whole image, in ray order, and their number -- read back once per image: it sizes the second
    // pass exactly (chunks, grids, the persistent kernels' row counts), where an upper bound would launch the whole
    // forward sequence over n_rays / chunk mostly empty chunks
    rc = durf::launch_layer_compact(stream, (int)n_rays, lo.instance, w.idx, w.count);
    if (rc != 0) return rc;
    int32_t n_hit = 0;
    DURF_REQUIRE(hipMemcpyAsync(&n_hit, w.count, sizeof(n_hit), hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess &&
                 hipStreamSynchronize((hipStream_t)stream) == hipSuccess, "reading the number of box-hit rays");
    DURF_REQUIRE(n_hit >= 0 && (size_t)n_hit <= n_rays, "0 <= box-hit rays <= n_rays");
    if (n_hit == 0) return 0;
    const float* src[6] = {a->origins, a->directions, a->viewdirs, a->radii, a->near, a->far};
    rc = durf::launch_layer_gather(stream, n_hit, w.idx, src, w.rays);
    if (rc != 0) return rc;
    durf_forward_args s = *a;                                 // the same model without boxes, over the dense buffer
    s.K = 0; s.pose = nullptr; s.ext = nullptr; s.obj_params = nullptr;
    s.origins = w.rays[0]; s.directions = w.rays[1]; s.viewdirs = w.rays[2]; s.radii = w.rays[3]; s.near = w.rays[4]; s.far = w.rays[5];
    rc = render_chunks(stream, &s, nullptr, (size_t)n_hit, chunk, w.rgb2, w.dist2, w.acc2, w0, workspace, nullptr);
    if (rc != 0) return rc;
    return durf::launch_layer_scatter(stream, n_hit, w.idx, w.rgb2, w.dist2, w.acc2, bg_rgb, bg_distance, bg_acc);
}

// ---- a camera trajectory (include/durf_hip.h durf_render_trajectory; kernels: csrc/trajectory.hip) ----------------------
int durf_camera_rays(void* stream, const float* cams_host, int first, int count, float near, float far, float* origins,
                     float* directions, float* viewdirs, float* radii, float* near_out, float* far_out) {
    DURF_REQUIRE(cams_host && origins && directions && viewdirs && radii && near_out && far_out, "the camera row and the six ray fields");
    DURF_REQUIRE(cams_host[DURF_CAM_H] >= 2 && cams_host[DURF_CAM_W] >= 1, "camera height >= 2, width >= 1");
    const long n = (long)(int)cams_host[DURF_CAM_H] * (int)cams_host[DURF_CAM_W];
    DURF_REQUIRE(first >= 0 && count >= 0 && (long)first + count <= n, "pixels [first, first + count) inside the image");
    float* const rays[6] = {origins, directions, viewdirs, radii, near_out, far_out};
    return durf::launch_camera_rays(stream, cams_host, first, count, near, far, rays);
}

size_t durf_render_trajectory_workspace_bytes(int F, int chunk, int N, int K, int num_levels) {
    return carve_trajectory(nullptr, F, chunk, N, K, num_levels).total;
}

int durf_render_trajectory(void* stream, const durf_forward_args* a, const int32_t* box_enable, const float* box_centers, int T, int F,
                           const float* cams_host, const float* times_host, float near, float far, int chunk, uint8_t* rgb8, float* rgb,
                           float* distance, float* acc, float* poses_out, void* workspace, size_t workspace_bytes) {
    DURF_REQUIRE(a != nullptr && workspace != nullptr, "arguments and workspace");
    DURF_REQUIRE(F > 0 && times_host != nullptr, "F > 0 frames and their times");
    const bool image = rgb8 || rgb || distance || acc;
    DURF_REQUIRE(image || poses_out, "at least one output");
    DURF_REQUIRE(chunk > 0, "chunk > 0");
    int rc = require_render_mode(a, "render_trajectory");
    if (rc != 0) return rc;
    const int L = a->num_levels, K = a->K;
    DURF_REQUIRE(K >= 0 && K <= DURF_MAX_OBJ, "0 <= K <= DURF_MAX_OBJ");
    DURF_REQUIRE(T >= 1 && (K == 0 || box_centers != nullptr), "T >= 1 timesteps of box_centers");
    for (int f = 0; f < F; f++)
        if (!(times_host[f] >= 0.0f && times_host[f] <= (float)(T - 1))) {
            durf_set_error("durf_render_trajectory: time %g of frame %d is outside [0, %d] (T = %d timesteps)", (double)times_host[f], f,
                           T - 1, T);
            return -1;
        }
    int h = 0, wd = 0;
    if (image) {
        DURF_REQUIRE(cams_host != nullptr, "the camera rows");
        h = (int)cams_host[DURF_CAM_H]; wd = (int)cams_host[DURF_CAM_W];
        DURF_REQUIRE(cams_host[DURF_CAM_H] >= 2 && cams_host[DURF_CAM_W] >= 1, "camera height >= 2, width >= 1");
        DURF_REQUIRE((size_t)h * wd < ((size_t)1 << 27), "h * w < 2^27");
        for (int f = 1; f < F; f++) {
            const float* cam = cams_host + (size_t)f * DURF_CAM_FLOATS;
            if ((int)cam[DURF_CAM_H] != h || (int)cam[DURF_CAM_W] != wd) {
                durf_set_error("durf_render_trajectory: frame %d is %d x %d, frame 0 is %d x %d: all frames share one image size", f,
                               (int)cam[DURF_CAM_H], (int)cam[DURF_CAM_W], h, wd);
                return -1;
            }
        }
    }
    const TrajWs w = carve_trajectory(workspace, F, chunk, a->N, K, L);
    rc = durf::check_workspace("durf_render_trajectory", workspace_bytes, w.total,
                               "durf_render_trajectory_workspace_bytes(%d, %d, %d, %d, %d)", F, chunk, a->N, K, L);
    if (rc != 0) return rc;
    if (image) {                                    // (every chunk passes the same checks: nothing is refused after a launch)
        durf_forward_args c0 = *a;
        c0.B = 1;
        if ((rc = check_forward_args(&c0, workspace)) != 0) return rc;
    }
    float* poses = poses_out ? poses_out : w.poses;
    rc = durf::launch_pose_interp(stream, F, K, times_host, box_centers, poses);
    if (rc != 0 || !image) return rc;
    const size_t n = (size_t)h * wd;
    for (int f = 0; f < F; f++) {
        for (size_t i = 0; i < n; i += (size_t)chunk) {
            const int B = (int)(n - i < (size_t)chunk ? n - i : (size_t)chunk);
            rc = durf::launch_camera_rays(stream, cams_host + (size_t)f * DURF_CAM_FLOATS, (int)i, B, near, far, w.rays);
            if (rc != 0) return rc;
            const size_t at = (size_t)f * n + i;          // (an output that is not asked for stays in the workspace, per chunk)
            rc = forward_chunk(stream, a, box_enable, B, w.rays, K > 0 ? poses + (size_t)f * K * 6 : nullptr, rgb ? rgb + at * 3 : nullptr,
                               distance ? distance + at : nullptr, acc ? acc + at : nullptr, w.img, workspace);
            if (rc != 0) return rc;
            if (rgb8) {
                rc = durf::launch_frame_pack(stream, B, rgb ? rgb + at * 3 : w.img.rgb[L - 1], rgb8 + at * 3);
                if (rc != 0) return rc;
            }
        }
    }
    return 0;
}

}  // extern "C"
