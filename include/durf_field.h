/* C ABI of durf_amd/libdurf_field.so: the field itself at world points -- density and colour at any position, over regular
 * grids, and top-down maps of a grid's columns.  Everything the renderer ships is a picture of the field along rays; this is
 * the question behind them: what is at this point of the world?
 * A library of its own beside libdurf_hip.so (include/durf_hip.h), whose set of entry points it leaves as it is and which it
 * calls through that header alone (durf_view_enc, durf_mlp_fwd_f32, durf_objf32_fwd_batch, durf_bkgd_hit_rays_f32).  The house
 * rules of durf_hip.h hold: device pointers of caller-owned buffers unless marked HOST, asynchronous on `stream`
 * (hipStream_t), 0 or nonzero with the text in durf_last_error() -- the one of libdurf_hip.so, which this library links
 * against --, every argument checked before anything is launched, no stream synchronisation and no device-to-host copy
 * anywhere; n == 0 is a successful no-op.  All arithmetic is fp32, unfused, in the order written here.
 *
 * What "the field at X" means.  The model masks per RAY (obbpose_model.py:112-122, 167-234): on a ray that hits box k every
 * sample goes through BoxMLP_k in the box's frame and the background MLP sees a zero-masked Gaussian (constant encoding
 * [0 x 30, 1 x 30]); the two raws are added.  Point-wise, with P = R_k (X - c_k) the object frame of k_ray_setup (R =
 * aa2matrix(rotvec) of csrc/aa2matrix.h, world->object) and the owner rule of durf_flow.h ("rides the box"):
 *   X in exactly one enabled box k (|P_j| <= ext_kj (1 + inside_tol), j = 0, 1, 2):
 *       raw = MLP_0(const encoding, view) + BoxMLP_k(weighted_ipe(P), view),  owner = k
 *   X in no box:       raw = MLP_0(integrated_pos_enc(new_space(X)), view),   owner = -1
 *   X in several:      owner = -2, every float output NaN, valid = 0   (the model's sum of several frames is no geometry)
 * The view direction is the world-frame one for both networks (:193-199).  A sample outside the box on a box-hit ray is
 * evaluated by the BoxMLP in a render and by the background here: that difference is intended.
 * The Gaussian of a point is isotropic: mean X, covariance sigma^2 I, var_j = sigma * sigma (one fp32 product on the host),
 * the same in every box frame; sigma = 0 is the plain positional encoding.  The MLPs are the exact-fp32 kernels of
 * csrc/mlp_f32.hip; the bf16 kernels take a tile layout this library cannot produce through durf_hip.h and are out of scope. */
#ifndef DURF_FIELD_H
#define DURF_FIELD_H
#include <stddef.h>
#include <stdint.h>
#include "durf_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define DURF_FIELD_POSE_FLOATS(K) ((K) * 12)
#define DURF_FIELD_ENC_BKGD 60
#define DURF_FIELD_ENC_OBJ 63

/* ---- which box a point lies in (csrc/field.hip k_field_poses, k_field_classify) ---------------------------------------------
 * points [n,3], pose [K,6] (centre, rotation vector), ext [K,3] half extents, box_enable [K] int32 NULLABLE (0: the box is
 * absent).  A one-wave launch in front (thread k < K) writes R row-major then c, twelve floats, at pose_scratch + 12 k
 * (DURF_FIELD_POSE_FLOATS(K) floats, caller-owned); the per-point kernel has no trigonometry and walks k = 0 .. K-1, the same
 * in every lane.  Per point and enabled box:
 *   d_j = X_j - c_j,   P_i = (R[i][0] d_0 + R[i][1] d_1) + R[i][2] d_2,   inside = |P_j| <= ext_kj * (1 + inside_tol) for all j
 * owner [n] int32 = the one box the point is inside of, -1 for none, -2 for several; local [n,3] = P of the owner for
 * owner >= 0 and X (the same bits) otherwise.  K == 0: every owner is -1, pose / ext / pose_scratch may be NULL.
 * Refused: n < 0, K outside [0, DURF_MAX_OBJ], inside_tol < 0 (or NaN), a NULL buffer. */
int durf_field_classify(void* stream, int n, const float* points, int K, const float* pose, const float* ext,
                        const int32_t* box_enable /* nullable */, float inside_tol, float* pose_scratch, int32_t* owner,
                        float* local);

/* ---- ordered lists (k_field_lists): K + 1 ordered, deterministic compactions of owner [n]: list c < K holds the indices i
 * (ascending) with owner[i] == c, list K those with owner[i] == -1; a point with owner -2 is in no list.  idx [(K+1), n] int32
 * (list c at idx + c n; entries at or past count[c] are not written), count [K+1] int32 on the device.  One workgroup per
 * list walks the points in order with a ballot scan: no atomics, no scratch, no read-back.  Refused: n < 0, n >= 2^27, K. */
int durf_field_lists(void* stream, int n, int K, const int32_t* owner, int32_t* idx, int32_t* count);

/* The object-owned points as ONE list (k_field_owned): lists 0 .. K-1 one after the other -- owned[off_c + r] = idx[c][r]
 * with off_c = count[0] + .. + count[c-1] -- and owned_count [1] their total: the idx / count durf_bkgd_hit_rays_f32 takes. */
int durf_field_owned(void* stream, int n, int K, const int32_t* idx, const int32_t* count, int32_t* owned, int32_t* owned_count);

/* ---- the two encodings as fp32 rows (k_field_encode) ------------------------------------------------------------------------
 * Row r < count[c] of list c encodes point i = idx[c][r] of points_or_local [n,3] (durf_field_classify's `local`) with
 * var_j = sigma * sigma:
 *   list K -> enc_bkgd [n,60]: new_space (csrc/enc_lane.h contract_gaussian) when enc_flags has DURF_ENC_CONTRACT, then
 *             feature f = (c 30 + deg 3 + j): expf(-0.5 (var_j s s)) safe_sin(x_j s [+ fl32(pi/2) for c = 1]), s = 2^deg
 *             (csrc/gauss.h ipe_feature: safe_sin's period and threshold are the float32-rounded 100 pi);
 *   list c < K -> enc_obj [K, n, 63] (row r of box c at (c n + r) 63): no contraction; x_0, x_1, x_2, then barf_w[f / 6]
 *             times feature f of the above (csrc/gauss.h obj_features8; barf_w HOST float[10]: the BARF weights of alpha).
 * Rows at or past count[c] are not written.  Eight lanes per row, eight consecutive features each: a wave stores eight
 * consecutive rows.  enc_bkgd or enc_obj may be NULL (that side is skipped); K == 0: enc_obj and barf_w may be NULL.
 * Refused: n < 0, K, sigma < 0 (or NaN), enc_flags other than 0 / DURF_ENC_CONTRACT, a NULL buffer. */
int durf_field_encode(void* stream, int n, int K, const float* points_or_local, const int32_t* idx, const int32_t* count,
                      float sigma, int enc_flags, const float* barf_w /* HOST float[10] */, float* enc_bkgd /* nullable */,
                      float* enc_obj /* nullable */);

/* ---- merge, activations, back to point order (k_field_activate) -------------------------------------------------------------
 * raw_bkgd [n,4] row r = list K's row r; raw_obj [K,n,4] row r of box c at (c n + r) 4; raw_const [n,4] row off_c + r = the
 * background's constant-encoding evaluation of the same point (durf_field_owned's order); all (r, g, b, density) as
 * durf_mlp_fwd_f32 writes them.  Per list row, for point i = idx[c][r]:
 *   m = raw_bkgd[r]  (c == K)   or   m_q = raw_const[off_c + r]_q + raw_obj[c][r]_q  (c < K)
 *   density[i] = softplus(m_3 + density_bias) = fmaxf(x, 0) + log1pf(expf(-|x|)),   rgb[i]_q = 1 / (1 + expf(-m_q))
 *   -- the compositor's activations (csrc/render.hip composite_ray: a plain sigmoid, no rgb_padding term) --,
 *   raw[i] = m,  valid[i] = 1;  a point with owner[i] == -2: NaN in density, rgb and raw, valid[i] = 0.
 * density [n], valid [n] uint8; rgb [n,3] and raw [n,4] NULLABLE.  There is no density noise (randomized = False).
 * Refused: n < 0, K, a NULL buffer (raw_obj and raw_const may be NULL when K == 0). */
int durf_field_activate(void* stream, int n, int K, const int32_t* idx, const int32_t* count, const float* raw_bkgd,
                        const float* raw_obj, const float* raw_const, const int32_t* owner, float density_bias, float* density,
                        float* rgb /* nullable */, float* raw /* nullable */, uint8_t* valid);

/* ---- n points in one call ---------------------------------------------------------------------------------------------------
 * Walks the points in chunks of `chunk` (the last one the remainder).  Per chunk of B points: durf_field_classify,
 * durf_field_lists, durf_field_owned, durf_field_encode, durf_view_enc, durf_mlp_fwd_f32(256, 60, B, N = 1, enc_bkgd, ...,
 * ray_idx = list K, count = its count), durf_objf32_fwd_batch(K, B, N = 1, idx, count, enc_obj, ...) when K > 0 -- the
 * staged buffers ARE its [K, B, .] slabs --, durf_bkgd_hit_rays_f32 on the owned list, durf_field_activate.  Launch extents
 * come from B, the row counts stay on the device; nothing is synchronised or read back.  (durf_mlp_fwd_f32 guards every row
 * against the device count, so the lists need no padding to 32-row tiles.)  Every output row is a function of its point
 * alone: the result is bit-identical to the staged calls and independent of `chunk`.
 * viewdirs == NULL is a density-only query: rgb must be NULL, the view rows are zeros (the density does not depend on
 * them) and the constant term is still added.
 * workspace: durf_field_workspace_bytes(chunk, K) bytes, 256-byte aligned; it grows with chunk and K, never with n.
 * Refused before any launch: n < 0, chunk <= 0, K outside [0, DURF_MAX_OBJ], sigma < 0, inside_tol < 0, enc_flags, a NULL
 * parameter pointer, rgb without viewdirs, no density, a workspace smaller than that (both sizes named). */
typedef struct {
    int K;
    int enc_flags;                 /* 0 or DURF_ENC_CONTRACT */
    float sigma;                   /* >= 0 */
    float inside_tol;              /* >= 0 */
    float density_bias;
    float barf_w[10];              /* the BARF weights of alpha (mip.py:217-218); alpha >= 10: all 1 */
    const float* bkgd_params;      /* MLP_0, flax layout */
    const float* obj_params;       /* BoxMLP_0 .. BoxMLP_{K-1}, param_stride floats apart (K == 0: NULL) */
    size_t param_stride;
    const float* bkgd_wstream;     /* durf_mlp_f32_pack(256, 60, 1, ...) */
    const float* obj_wstream;      /* durf_mlp_f32_pack(128, 63, K, ...) (K == 0: NULL) */
    const float* const_trunk;      /* durf_bkgd_const_trunk_f32's trunk [257] (K == 0: NULL) */
    const float* pose;             /* [K,6] */
    const float* ext;              /* [K,3] */
    const int32_t* box_enable;     /* nullable [K] */
    const float* points;           /* [n,3] (durf_field_grid: ignored) */
    const float* viewdirs;         /* nullable [n,3] (durf_field_grid: ignored) */
    float* density;                /* [n] */
    float* rgb;                    /* nullable [n,3] */
    float* raw;                    /* nullable [n,4] */
    int32_t* owner;                /* nullable [n] */
    uint8_t* valid;                /* nullable [n] */
} durf_field_args;
size_t durf_field_workspace_bytes(int chunk, int K);
int durf_field_query(void* stream, const durf_field_args* args, int n, int chunk, void* workspace, size_t workspace_bytes);

/* ---- a regular grid (k_field_grid_points) -----------------------------------------------------------------------------------
 * durf_field_query over X(i, j, k) = origin + i du + j dv + k dw, cell g = (i nv + j) nw + k (k fastest), evaluated as
 *   X_c = ((origin_c + (float) i * du_c) + (float) j * dv_c) + (float) k * dw_c
 * by a kernel that builds each chunk's points in the workspace: no point buffer of the grid's size exists unless points_out
 * [nu nv nw, 3] (NULLABLE) asks for it.  One view direction for the whole grid by value; has_view == 0: a density-only
 * query (args->rgb NULL).  Outputs of args are [nu nv nw, .].  Refused: nu, nv or nw < 1 or > 2^24, nu nv nw >= 2^31. */
int durf_field_grid(void* stream, const durf_field_args* args, const float* origin_host /* 3 */, const float* du_host /* 3 */,
                    const float* dv_host /* 3 */, const float* dw_host /* 3 */, int nu, int nv, int nw, int has_view, float view_x,
                    float view_y, float view_z, int chunk, void* workspace, size_t workspace_bytes, float* points_out /* nullable */);

/* ---- the top-down map (k_field_columns) -------------------------------------------------------------------------------------
 * One thread per column (i, j) walks k = 0 .. nw-1 in order over density, valid [nu nv nw].  A cell counts when valid != 0
 * and its density is not NaN.  col_max = the largest counted density (NaN when the column has none); s = the counted
 * densities added in k order starting from 0, col_opacity = 1 - expf(-(step * s)); col_first int32 = the first counted k with
 * density >= threshold, -1 when there is none.  The order is fixed: the same inputs give the same bits.
 * Each output NULLABLE, at least one.  Refused: nu, nv, nw < 1, nu nv nw >= 2^31, step < 0, a NULL input. */
int durf_field_columns(void* stream, int nu, int nv, int nw, const float* density, const uint8_t* valid, float step, float threshold,
                       float* col_max /* nullable */, float* col_opacity /* nullable */, int32_t* col_first /* nullable */);

#ifdef __cplusplus
}
#endif
#endif
