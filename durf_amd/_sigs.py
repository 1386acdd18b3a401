"""Argument types of every entry point of libdurf_hip.so, and the constants, macros and structs of its header -- GENERATED from
include/durf_hip.h by tools/gen_integration_stub.py (do not edit; `--check` runs in the CPU test-suite)."""
import ctypes as C

vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t

SIGS = {
    'durf_last_error': (C.c_char_p, []),
    'durf_version': (i32, []),
    'durf_dispatch_seen': (i32, []),
    'durf_dispatch_reset': (i32, []),
    'durf_step_policy': (C.c_uint, [u64]),
    'durf_overlap_min_rows': (u64, []),
    'durf_mlp_param_count': (u64, [i32, i32]),
    'durf_mlp_layer_offset': (u64, [i32, i32, i32, i32]),
    'durf_wpack_fwd_bytes': (u64, [i32]),
    'durf_wpack_bwd_bytes': (u64, [i32]),
    'durf_pack_weights': (i32, [vp, i32, i32, vp, vp, vp]),
    'durf_pack_weights_all': (i32, [vp, vp, i32, vp, vp, i32, vp, u64, i32, vp, vp]),
    'durf_ray_setup': (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_ray_setup_masked': (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_compact_hits': (i32, [vp, i32, i32, vp, vp, vp, vp]),
    'durf_compact_classes': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    'durf_compact_all': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_ray_prologue': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, u64, C.c_uint32, C.c_uint32, vp]),
    'durf_ray_prologue_pack': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, i32, vp, vp, i32, vp, u64, i32, vp, vp, vp, u64]),
    'durf_ray_prologue_pack_masked': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, u64, C.c_uint32, C.c_uint32, vp, vp, i32, vp, vp, i32, vp, u64, i32, vp, vp, vp, u64, vp]),
    'durf_sample_t': (i32, [vp, i32, i32, vp, vp, vp, i32, vp]),
    'durf_density_noise': (i32, [vp, u64, vp, f32, vp, C.c_uint32, C.c_uint32, i32]),
    'durf_view_enc': (i32, [vp, i32, vp, vp, vp]),
    'durf_encode_bkgd': (i32, [vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    'durf_encode_obj': (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(f32), i32, vp, vp]),
    'durf_mlp_stash_bytes': (u64, [i32, u64]),
    'durf_mlp_mask_bytes': (u64, [u64]),
    'durf_mlp_fwd': (i32, [vp, i32, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_mlp_fwd_enc': (i32, [vp, u64, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_mlp_fwd_enc_obj': (i32, [vp, u64, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, C.POINTER(f32), i32, vp, vp, vp, vp, vp, vp]),
    'durf_composite_fwd': (i32, [vp, i32, i32, i32, vp, C.POINTER(vp), vp, vp, vp, f32, i32, vp, vp, vp, vp, vp, vp]),
    'durf_composite_resample': (i32, [vp, i32, i32, i32, vp, C.POINTER(vp), vp, vp, vp, f32, i32, vp, vp, vp, vp, vp, vp, f32, vp, vp, vp, vp, vp, vp, vp, f32, f32, i32, i32, vp, vp, vp, vp]),
    'durf_resample': (i32, [vp, i32, i32, vp, vp, f32, vp, vp]),
    'durf_sorted_piecewise_constant_pdf': (i32, [vp, i32, i32, vp, vp, vp, vp]),
    'durf_loss_prep': (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, i32, i32, vp, vp]),
    'durf_loss_bwd': (i32, [vp, i32, i32, i32, vp, C.POINTER(vp), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, C.POINTER(f32), f32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_loss_bwd_levels': (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, f32, i32, f32, f32]),
    'durf_train_stats': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(f32), i32, vp, C.POINTER(vp), i32]),
    'durf_mlp_bwd': (i32, [vp, i32, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_expand_view': (i32, [vp, u64, i32, vp, vp, vp, vp, vp, vp]),
    'durf_dw_part_floats': (u64, [i32]),
    'durf_dw_bpart_floats': (u64, [i32]),
    'durf_mlp_dw': (i32, [vp, i32, u64, i32, vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]),
    'durf_mlp_dw_finalize': (i32, [vp, i32, i32, u64, i32, vp, i32, vp, vp, vp, vp]),
    'durf_mlp_dw_levels': (i32, [vp, i32, i32, C.POINTER(u64), C.POINTER(i32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]),
    'durf_mlp_dw_finalize_levels': (i32, [vp, i32, i32, i32, C.POINTER(u64), C.POINTER(i32), C.POINTER(vp), vp, vp, vp, vp]),
    'durf_expand_raw': (i32, [vp, i32, i32, vp, vp, vp, vp, vp]),
    'durf_forward_workspace_bytes': (u64, [i32, i32, i32]),
    'durf_forward': (i32, [vp, vp, vp, u64]),
    'durf_render_image_workspace_bytes': (u64, [i32, i32, i32, i32]),
    'durf_render_image': (i32, [vp, vp, u64, i32, vp, vp, vp, vp, u64]),
    'durf_forward_masked': (i32, [vp, vp, vp, vp, u64]),
    'durf_render_layers_workspace_bytes': (u64, [u64, i32, i32, i32, i32]),
    'durf_render_layers': (i32, [vp, vp, vp, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64]),
    'durf_camera_rays': (i32, [vp, C.POINTER(f32), i32, i32, f32, f32, vp, vp, vp, vp, vp, vp]),
    'durf_render_trajectory_workspace_bytes': (u64, [i32, i32, i32, i32, i32]),
    'durf_render_trajectory': (i32, [vp, vp, vp, vp, i32, i32, C.POINTER(f32), C.POINTER(f32), f32, f32, i32, vp, vp, vp, vp, vp, vp, u64]),
    'durf_train_workspace_bytes': (u64, [i32, i32, i32, i32, u64]),
    'durf_train_workspace_bytes_flags': (u64, [i32, i32, i32, i32, u64, i32]),
    'durf_prefetch_join': (i32, [vp]),
    'durf_loss_backward': (i32, [vp, vp, vp, u64]),
    'durf_train_step': (i32, [vp, vp, vp, u64]),
    'durf_comm_available': (i32, []),
    'durf_comm_unique_id': (i32, [vp]),
    'durf_comm_init': (i32, [i32, i32, vp, C.POINTER(vp)]),
    'durf_comm_destroy': (i32, [vp]),
    'durf_allreduce_sum': (i32, [vp, vp, vp, u64]),
    'durf_mlp_f32_act_floats': (u64, [i32, i32]),
    'durf_mlp_f32_dz_floats': (u64, [i32, i32]),
    'durf_mlp_f32_dw_scratch_floats': (u64, [i32, i32, i32]),
    'durf_mlp_f32_wstream_floats': (u64, [i32]),
    'durf_mlp_f32_pack': (i32, [vp, i32, i32, i32, vp, u64, vp]),
    'durf_mlp_fwd_f32': (i32, [vp, i32, i32, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_mlp_bwd_f32': (i32, [vp, i32, i32, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_mlp_dw_f32': (i32, [vp, i32, i32, u64, i32, vp, vp, vp, i32, vp, vp]),
    'durf_bkgd_const_trunk_f32': (i32, [vp, vp, vp]),
    'durf_bkgd_hit_rays_f32': (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    'durf_objf32_act_stride': (u64, [i32, i32]),
    'durf_objf32_dz_stride': (u64, [i32, i32]),
    'durf_encode_obj_f32_batch': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(f32), i32, vp]),
    'durf_objf32_fwd_batch': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, vp, C.POINTER(f32), i32]),
    'durf_objf32_bwd_batch': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, u64, vp, vp, vp, vp]),
    'durf_mlp_f32_pack_x3': (i32, [vp, i32, vp, u64, vp]),
    'durf_objf32_bwd_batch_x3': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, u64, vp, vp, vp, vp]),
    'durf_objf32_dw_batch': (i32, [vp, i32, i32, i32, vp, i32, C.POINTER(vp), C.POINTER(vp), i32, vp, vp, u64]),
    'durf_obj_enc_stride': (u64, [i32, i32]),
    'durf_obj_view_stride': (u64, [i32, i32]),
    'durf_obj_dzout_stride': (u64, [i32, i32]),
    'durf_pack_weights_batch': (i32, [vp, i32, i32, i32, vp, u64, vp, vp]),
    'durf_obj_fwd_batch': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(f32), i32, vp, vp, vp, vp, vp, vp, vp]),
    'durf_obj_bwd_batch': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_obj_bwd_batch_levels': (i32, [vp, i32, i32, i32, i32, vp, vp, C.POINTER(vp), vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    'durf_mlp_bwd_obj': (i32, [vp, u64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, C.POINTER(vp), vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    'durf_obj_dw_batch': (i32, [vp, i32, i32, i32, vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i32, vp, vp, vp, u64, vp]),
    'durf_obj_dw_partials': (i32, [vp, i32, i32, i32, vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]),
    'durf_dw_finalize_all': (i32, [vp, i32, i32, C.POINTER(u64), C.POINTER(i32), C.POINTER(vp), vp, vp, vp, vp, i32, i32, i32, vp, i32, i32, vp, vp, vp, u64, vp]),
    'durf_encode_obj_bwd': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(f32), vp, vp, i32, i32]),
    'durf_encode_obj_bwd_batch': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(f32), vp, vp, i32, i32]),
    'durf_encode_obj_bwd_levels': (i32, [vp, i32, i32, i32, i32, vp, vp, C.POINTER(vp), C.POINTER(vp), vp, vp, vp, vp, vp, vp, C.POINTER(f32), vp, vp, i32, i32]),
    'durf_encode_bkgd_bwd_batch': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, i32]),
    'durf_pose_finish': (i32, [vp, i32, vp, vp, i32, i32, vp]),
    'durf_optim_scratch_floats': (u64, [u64]),
    'durf_stats_scrub': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(f32), i32, vp, C.POINTER(vp), i32, u64, vp, f32, f32, vp, vp, u64, i32, u64, u64]),
    'durf_adam_apply': (i32, [vp, u64, vp, vp, vp, vp, f32, f32, i32, vp, vp]),
    'durf_poison_multi_hit': (i32, [vp, u64, vp, vp, u64, i32, u64, u64]),
    'durf_clip_adam': (i32, [vp, u64, vp, vp, vp, vp, f32, f32, f32, f32, i32, vp, vp]),
    'durf_weight_decay': (i32, [vp, u64, vp, vp, u64, u64, f32, vp, vp]),
    'durf_gen_batch': (i32, [vp, i32, i32, C.POINTER(f32), vp, f32, f32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'durf_ssim_scratch_floats': (u64, [i32, i32, i32, i32]),
    'durf_ssim': (i32, [vp, i32, i32, i32, vp, vp, f32, i32, vp, f32, f32, vp, vp, vp]),
    'durf_eval_scratch_bytes': (u64, [i32, i32, i32]),
    'durf_eval_frames': (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, u64]),
    'durf_vis_scratch_bytes': (u64, [i32, i32, i32]),
    'durf_vis_stats': (i32, [vp, i32, i32, i32, vp, vp, vp, u64]),
    'durf_vis_depth': (i32, [vp, i32, i32, i32, vp, vp, vp, i32, i32, f32, vp, vp, vp]),
    'durf_vis_normals': (i32, [vp, i32, i32, i32, vp, vp, vp, i32, i32, vp, vp]),
    'durf_vis_sinebow': (i32, [vp, u64, vp, vp, vp]),
    'durf_vis_turbo_lut': (i32, [vp]),
}


DURF_MAX_OBJ = 16
DURF_MAX_LEVELS = 8
DURF_MAX_CAMS = 8
DURF_W_BKGD = 256
DURF_W_OBJ = 128
DURF_ENC_CONTRACT = 1
DURF_ENC_NO_INTEGRATION = 2
DURF_ENC_CYLINDER = 4
DURF_FWD_RAW_FULL = 8
DURF_ENC_DIM = 64
DURF_VIEW_DIM = 32
DURF_DISPATCH_FWD256_8W = 0x1
DURF_DISPATCH_FWD256_4W = 0x2
DURF_DISPATCH_FWD128_SAMPLE = 0x4
DURF_DISPATCH_FWD128_MSPLIT = 0x8
DURF_DISPATCH_BWD256_8W = 0x10
DURF_DISPATCH_BWD256_4W = 0x20
DURF_DISPATCH_BWD128_SAMPLE = 0x40
DURF_DISPATCH_BWD128_MSPLIT = 0x80
DURF_DISPATCH_DW256_256WG = 0x100
DURF_DISPATCH_DW256_512WG = 0x200
DURF_DISPATCH_DW128_128WG = 0x400
DURF_DISPATCH_DW128_256WG = 0x800
DURF_DISPATCH_FWD_ENC = 0x1000
DURF_DISPATCH_FWD_RAW_FULL = 0x2000
DURF_DISPATCH_FWD_TAIL = 0x4000
DURF_DISPATCH_F32_DW_TILE = 0x8000
DURF_DISPATCH_F32_DW_B2 = 0x10000
DURF_DISPATCH_BWD_POSE = 0x20000
DURF_DISPATCH_FWD_MIX = 0x40000
DURF_DISPATCH_BWD_MIX = 0x80000
DURF_LAYERLOG_SELECT = 0x100000
DURF_LAYERLOG_PASS2 = 0x200000
DURF_LAYERLOG_BOX_MASK = 0x400000
DURF_LAYERLOG_TRAJ_RAYS = 0x800000
DURF_LAYERLOG_TRAJ_POSE = 0x1000000
DURF_LAYERLOG_TRAJ_PACK = 0x2000000
DURF_OVERLAP_MIN_ROWS = 262144          # ((size_t)2048 * 128)
DURF_POLICY_SIDE_FWD = 0x1
DURF_POLICY_SIDE_BWD = 0x2
DURF_POLICY_SIDE_DW = 0x4
DURF_POLICY_MSPLIT = 0x8
DURF_POLICY_MIX = 0x10


class durf_loss_level(C.Structure):
    _fields_ = [
        ('raw_bkgd', vp),
        ('raw_obj', vp * DURF_MAX_OBJ),
        ('t_vals', vp),
        ('norm', vp),
        ('mults', f32 * 6),
        ('level', i32),
        ('draw', vp),
        ('terms', vp),
        ('rgb_out', vp),
        ('depth_out', vp),
        ('acc_out', vp),
        ('weights_out', vp),
        ('t_mids_out', vp),
        ('t_dists_out', vp),
        ('draw_ray_sum', vp),
    ]


DURF_FORWARD_MAX_LEVELS = 4


class durf_forward_args(C.Structure):
    _fields_ = [
        ('B', i32),
        ('N', i32),
        ('K', i32),
        ('num_levels', i32),
        ('enc_flags', i32),
        ('lindisp', i32),
        ('bkgd_mode', i32),
        ('density_bias', f32),
        ('resample_padding', f32),
        ('barf_w', f32 * 10),
        ('origins', vp),
        ('directions', vp),
        ('viewdirs', vp),
        ('radii', vp),
        ('near', vp),
        ('far', vp),
        ('pose', vp),
        ('ext', vp),
        ('bkgd_params', vp),
        ('obj_params', vp),
        ('obj_param_stride', u64),
        ('t_rand', vp),
        ('u_rand', vp),
        ('rgb', vp * DURF_FORWARD_MAX_LEVELS),
        ('depth', vp * DURF_FORWARD_MAX_LEVELS),
        ('acc', vp * DURF_FORWARD_MAX_LEVELS),
        ('weights', vp * DURF_FORWARD_MAX_LEVELS),
        ('t_vals', vp * DURF_FORWARD_MAX_LEVELS),
        ('t_mids', vp * DURF_FORWARD_MAX_LEVELS),
        ('t_dists', vp * DURF_FORWARD_MAX_LEVELS),
        ('dyn_mask', vp),
        ('zo', vp),
        ('draw_noise', i32),
        ('seed_lo', C.c_uint32),
        ('seed_hi', C.c_uint32),
        ('density_noise', f32),
        ('density_rand', vp * DURF_FORWARD_MAX_LEVELS),
    ]


DURF_CAM_FLOATS = 17
DURF_CAM_FOCAL = 12
DURF_CAM_PPX = 13
DURF_CAM_PPY = 14
DURF_CAM_H = 15
DURF_CAM_W = 16
DURF_TRAIN_OBJ_FP32 = 1
DURF_TRAIN_POSE_OPT = 2
DURF_TRAIN_OBJ_X3 = 4
DURF_TIMED_FWD = 0
DURF_TIMED_BWD = 4
DURF_TIMED_COMPOSITE = 8
DURF_TIMED_DW = 12
DURF_TIMED_STAGES = 13


class durf_step_timing(C.Structure):
    _fields_ = [
        ('begin', vp * DURF_TIMED_STAGES),
        ('end', vp * DURF_TIMED_STAGES),
    ]


class durf_train_args(C.Structure):
    _fields_ = [
        ('f', durf_forward_args),
        ('lossmult', vp),
        ('pixels', vp),
        ('gt_depth', vp),
        ('sky', vp),
        ('target6', vp),
        ('prev6', vp),
        ('eps', f32),
        ('box_loss_mult', f32),
        ('bg', f32),
        ('disable_multiscale', i32),
        ('level_mults', (f32 * 6) * DURF_FORWARD_MAX_LEVELS),
        ('stat_mults', f32 * 6),
        ('params', vp),
        ('n_params', u64),
        ('box_floats', u64),
        ('mlp0_floats', u64),
        ('obj_floats', u64),
        ('grad', vp),
        ('stats', vp),
        ('adam_m', vp),
        ('adam_v', vp),
        ('lr', f32),
        ('max_val', f32),
        ('max_norm', f32),
        ('step', i32),
        ('grad_stats', vp),
        ('flags', i32),
        ('want_pos', i32),
        ('want_rot', i32),
        ('tv_loss_mult', f32),
        ('comm', vp),
        ('world', i32),
        ('reduce_stats', i32),
        ('weight_decay_mult', f32),
        ('pose_used', vp),
        ('cls_count', vp),
        ('timing', vp),
        ('const_trunk', vp),
        ('const_trunk_valid', i32),
        ('prefetch_const_trunk', i32),
    ]


DURF_COMM_ID_BYTES = 128
DURF_F32_X3 = 16
DURF_EVAL_FLOATS = 10
DURF_EVAL_MSE = 0
DURF_EVAL_PSNR = 1
DURF_EVAL_SSIM = 2
DURF_EVAL_OBJ_COUNT = 3
DURF_EVAL_OBJ_MSE = 4
DURF_EVAL_OBJ_PSNR = 5
DURF_EVAL_DEPTH_COUNT = 6
DURF_EVAL_DEPTH_ABS = 7
DURF_EVAL_DEPTH_RMSE = 8
DURF_EVAL_NONFINITE = 9
DURF_VIS_CURVE_NEGLOG = 0
DURF_VIS_CURVE_IDENTITY = 1
DURF_VIS_CURVE_INVERSE = 2
DURF_VIS_STATS_FLOATS = 8
DURF_VIS_NORMALS_RAW = 1
