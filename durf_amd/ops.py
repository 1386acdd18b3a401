"""Stage-level operators: torch tensors in, torch tensors out, every one a call through the
C ABI of libdurf_hip.so on the current HIP stream.  PyTorch is used for device memory and
streams only.  Reference lines each op replaces are cited in include/durf_hip.h."""
import collections
import ctypes as C
import math
import os

import torch

from . import _lib, camera
from . import _sigs as _H, _field_sigs, _flow_sigs, _geom_sigs, _lidar_sigs, _mesh_sigs, _overlay_sigs, _parts_sigs, _raster_sigs, _tsdf_sigs, _cast_sigs, _closest_sigs, _shade_sigs, _smooth_sigs



def _by_prefix(table, prefix):
    """{X: value} of a generated table's integer constants named <prefix>X, in header order"""
    return {k[len(prefix):]: v for k, v in vars(table).items() if k.startswith(prefix) and type(v) is int}


# The headers are the one place a constant or an argument struct is written (tools/gen_integration_stub.py renders them into
# the tables imported above; tests/test_headers_host.py holds the tables to the C compiler).  Every `#define DURF_X <integer>`
# of include/durf_hip.h and include/durf_<name>.h is ops.X: ENC_DIM, MAX_OBJ, TRAIN_OBJ_FP32, TIMED_STAGES, MESH_BLOCK, PARTS_TILE_K, ...
# -- all but OVERLAP_MIN_ROWS, launch policy that the library is asked for (__getattr__ below).
for _table in (_H, _overlay_sigs, _lidar_sigs, _flow_sigs, _field_sigs, _mesh_sigs, _geom_sigs, _parts_sigs, _raster_sigs, _tsdf_sigs, _cast_sigs, _closest_sigs, _shade_sigs, _smooth_sigs):
    globals().update(_by_prefix(_table, 'DURF_'))
del OVERLAP_MIN_ROWS


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional per-op timing with HIP events recorded on the launch stream (bench.py's live
# roofline measurement).  TIMERS = None disables it (default: zero overhead).
TIMERS = None
TIMED_NAMES = None       # optional set of op names to time (None: every wrapped op)
TIMERS_ACTIVE = True     # bench.py samples: an event record stalls the stream for ~3-6 us on either side of the launch it
                         # brackets (the next packet waits for the marker's signal), so only every n-th step is timed


class _Timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.on = TIMERS is not None and TIMERS_ACTIVE and (TIMED_NAMES is None or self.name in TIMED_NAMES)
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if self.on:
            self.e1.record()
            TIMERS.setdefault(self.name, []).append((self.e0, self.e1))


EVENT_POOL = []          # timing events that exist already (created by a record outside any timed region): _step_timing takes
                         # them from here first, because handing an event to the C call needs its handle, torch creates the
                         # handle on the first record, and a record costs the stream 3-6 us (bench.py parks its pre-warm events here)


def recycle_timers():
    """the events of the collected TIMERS go back to EVENT_POOL (call after timer_totals())"""
    for pairs in (TIMERS or {}).values():
        for pair in pairs:
            EVENT_POOL.extend(pair)
    if TIMERS is not None:
        TIMERS.clear()


def _timing_event():
    if EVENT_POOL:
        return EVENT_POOL.pop()
    e = torch.cuda.Event(enable_timing=True)
    e.record()                              # (torch creates the underlying event on its first record; the call re-records it)
    return e


def timer_totals():
    """{name: (calls, total_seconds)}; synchronises."""
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) * 1e-3) for k, v in (TIMERS or {}).items()}


def _p(t):
    return None if t is None else t.data_ptr()


def _z(t):
    """a tensor's address, or None for no tensor and for one of zero elements (it has no address to hand over)"""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _up256(b):
    return (b + 255) // 256 * 256


def _ws(ws, need, dev):
    return torch.empty(max(need, 256), dtype=torch.uint8, device=dev) if ws is None else ws


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), (t.dtype, t.device, t.is_contiguous())
    return t


def _i32(t, n, what):
    assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == n, (what, t.dtype, tuple(t.shape), n)
    return t


def _enable(box_enable, K, dev):
    """box_enable (None or K values 0 / 1) -> None or a contiguous int32 [K] tensor on `dev`: the device-side switch of the box
    test (durf_ray_setup_masked).  A tensor already on the device is used where it is: no copy, no synchronisation."""
    if box_enable is None:
        return None
    e = torch.as_tensor(box_enable)
    if e.dim() != 1 or e.shape[0] != K:
        raise ValueError('box_enable: %d values for K = %d boxes' % (e.numel(), K))
    return e.to(device=dev, dtype=torch.int32).contiguous()


def ray_setup(origins, dirs, pose, ext, box_enable=None):
    """-> origins_s[B,3], dirs_s[B,3], hit[B,K] int32, zo[B]; box_enable: durf_ray_setup_masked (a box with 0 is a miss)"""
    B, K = origins.shape[0], pose.shape[0]
    dev = origins.device
    o_s = torch.empty(B, 3, device=dev)
    d_s = torch.empty(B, 3, device=dev)
    hit = torch.empty(B, K, dtype=torch.int32, device=dev)
    zo = torch.empty(B, device=dev)
    if box_enable is not None:
        en = _enable(box_enable, K, dev)
        _lib.check(_lib.lib().durf_ray_setup_masked(_stream(), B, K, _p(_f32(origins)), _p(_f32(dirs)), _p(_f32(pose)),
                                                    _p(_f32(ext)), _p(en), _p(o_s), _p(d_s), _p(hit), _p(zo)),
                   'durf_ray_setup_masked')
        return o_s, d_s, hit, zo
    _lib.check(_lib.lib().durf_ray_setup(_stream(), B, K, _p(_f32(origins)), _p(_f32(dirs)),
                                         _p(_f32(pose)), _p(_f32(ext)), _p(o_s), _p(d_s), _p(hit),
                                         _p(zo)), 'durf_ray_setup')
    return o_s, d_s, hit, zo


def ray_prologue(origins, dirs, pose, ext, viewdirs, near, far, N, t_rand=None, lindisp=False, pose_copy=None, zero=None,
                 seed=None, pack=None, box_enable=None):
    """ray_setup + view_enc (bf16) + sample_t as ONE launch (durf_ray_prologue)
    box_enable (int32 [K] on the device): the box test of durf_ray_setup_masked (durf_ray_prologue_pack_masked)
    -> origins_s[B,3], dirs_s[B,3], hit[B,K] int32, zo[B], view[B,32] bf16, t_vals[B,N+1]
    pose_copy [K,6]: receives a snapshot of `pose`; zero: a contiguous fp32 tensor the launch zero fills (the gradient)
    seed (int, instead of t_rand): the launch draws the step's stratified-sampling noise itself (Philox under this key) and
    also returns u_rand [3,B,N+1], the resampling draws behind levels 0, 1, 2 (Philox words 1, 2, 3) -> (..., t_vals, u_rand)
    pack = (bkgd_params, K, obj_params, obj_param_stride, want_bwd): pack_weights_all's work rides in the same launch
    (durf_ray_prologue_pack); its result ((bkgd_fwd, bkgd_bwd), (obj_fwd, obj_bwd) or None) is appended to the tuple"""
    B, K = origins.shape[0], pose.shape[0]
    dev = origins.device
    if zero is not None:
        assert zero.is_contiguous() and zero.dtype == torch.float32
    o_s = torch.empty(B, 3, device=dev)
    d_s = torch.empty(B, 3, device=dev)
    hit = torch.empty(B, K, dtype=torch.int32, device=dev)
    zo = torch.empty(B, device=dev)
    view = torch.empty(B, VIEW_DIM, dtype=torch.bfloat16, device=dev)
    t = torch.empty(B, N + 1, device=dev)
    u_out = None
    if seed is not None:
        assert t_rand is None
        u_out = torch.empty(3, B, N + 1, device=dev)
    lo, hi = (0, 0) if seed is None else split_seed(seed)
    common = (_stream(), B, K, N, _p(_f32(origins)), _p(_f32(dirs)), _p(_f32(pose)),
              _p(_f32(ext)), _p(o_s), _p(d_s), _p(hit), _p(zo), _p(_f32(viewdirs)), _p(view),
              _p(_f32(near)), _p(_f32(far)), _p(None if t_rand is None else _f32(t_rand)),
              int(lindisp), _p(t), _p(pose_copy if K else None), _p(zero),
              0 if zero is None else zero.numel(), lo, hi, _p(u_out))
    out = (o_s, d_s, hit, zo, view, t) if seed is None else (o_s, d_s, hit, zo, view, t, u_out)
    if pack is None:
        if box_enable is not None:        # (no weight streams to pack: the masked launch with an empty packing list)
            _lib.check(_lib.lib().durf_ray_prologue_pack_masked(*common, None, 0, None, None, 0, None, 0, 0, None, None, None, 0,
                                                                _p(box_enable)), 'durf_ray_prologue_pack_masked')
            return out
        _lib.check(_lib.lib().durf_ray_prologue(*common), 'durf_ray_prologue')
        return out
    bkgd_params, Kp, obj_params, obj_param_stride, want_bwd = pack
    L = _lib.lib()
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)
    bf = u8(L.durf_wpack_fwd_bytes(W_BKGD_))
    bb = u8(L.durf_wpack_bwd_bytes(W_BKGD_)) if want_bwd else None
    of = ob = None
    if Kp:
        of = u8(Kp * int(L.durf_wpack_fwd_bytes(W_OBJ_)))
        ob = u8(Kp * int(L.durf_wpack_bwd_bytes(W_OBJ_))) if want_bwd else None
    pack_args = (_p(_f32(bkgd_params)), IN_BKGD, _p(bf), _p(bb), int(Kp), _p(obj_params) if Kp else None, int(obj_param_stride),
                 IN_OBJ_, _p(of), _p(ob), None, 0)
    if box_enable is not None:
        _lib.check(L.durf_ray_prologue_pack_masked(*common, *pack_args, _p(box_enable)), 'durf_ray_prologue_pack_masked')
    else:
        _lib.check(L.durf_ray_prologue_pack(*common, *pack_args), 'durf_ray_prologue_pack')
    return out + (((bf, bb), ((of, ob) if Kp else None)),)


def split_seed(seed):
    """host PRNG key (any Python int) -> the two 32-bit key words of the in-kernel Philox stream"""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def compact_all(hit, N):
    """compact_hits + compact_classes as ONE launch -> (idx, count, slot), (idx2, count4, slot2, dyn)"""
    B, K = hit.shape
    dev = hit.device
    i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device=dev)
    idx, count, slot = i32(K, B), i32(K), i32(B, K)
    idx2, count4, slot2, dyn = i32(2, B), i32(5), i32(B, 2), i32(B)
    _lib.check(_lib.lib().durf_compact_all(_stream(), B, K, N, _p(hit), _p(idx), _p(count), _p(slot), _p(idx2),
                                           _p(count4), _p(slot2), _p(dyn)), 'durf_compact_all')
    return (idx, count, slot), (idx2, count4, slot2, dyn)


_CONST = {}


def const_tensor(device, shape, dtype=torch.float32, value=0):
    """A cached, READ-ONLY constant tensor (the K = 0 model's empty hit lists, zero dyn_mask / box_rot / multi-hit count):
    a torch.zeros / torch.full per step is a fill launch each -- five of them were 5 % of a cfg1 step."""
    key = (str(device), tuple(shape), dtype, value)
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.full(tuple(shape), value, dtype=dtype, device=device)
    return t


def compact_hits(hit):
    """-> idx[K,B] int32, count[K] int32, slot[B,K] int32"""
    B, K = hit.shape
    dev = hit.device
    if K == 0:
        return (const_tensor(dev, (1, B), torch.int32), const_tensor(dev, (1,), torch.int32),
                const_tensor(dev, (B, 1), torch.int32, -1))
    # the kernel writes every slot and count entry, and idx[k, :count[k]] is all anyone reads
    idx = torch.empty(K, B, dtype=torch.int32, device=dev)
    count = torch.empty(K, dtype=torch.int32, device=dev)
    slot = torch.empty(B, K, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().durf_compact_hits(_stream(), B, K, _p(hit), _p(idx), _p(count), _p(slot)),
               'durf_compact_hits')
    return idx, count, slot


def compact_classes(hit, N):
    """-> idx[2,B], count[5] (class-0 rays, class-1 rays, valid compacted rows, multi-hit rays, bit mask of the boxes
    they hit), slot[B,2], dyn[B]:
    the ray classes of the de-duplicated background evaluation (class 1 = rays that hit exactly one box)"""
    B, K = hit.shape
    dev = hit.device
    idx = torch.empty(2, B, dtype=torch.int32, device=dev)
    count = torch.empty(5, dtype=torch.int32, device=dev)
    slot = torch.empty(B, 2, dtype=torch.int32, device=dev)
    dyn = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().durf_compact_classes(_stream(), B, K, N, _p(hit), _p(idx), _p(count), _p(slot), _p(dyn)),
               'durf_compact_classes')
    return idx, count, slot, dyn


def sample_t(near, far, N, t_rand=None, lindisp=False):
    B = near.shape[0]
    t = torch.empty(B, N + 1, device=near.device)
    _lib.check(_lib.lib().durf_sample_t(_stream(), B, N, _p(_f32(near)), _p(_f32(far)),
                                        _p(None if t_rand is None else _f32(t_rand)), int(lindisp), _p(t)),
               'durf_sample_t')
    return t


def view_enc(viewdirs, want_f32=False):
    B = viewdirs.shape[0]
    out = torch.empty(B, VIEW_DIM, dtype=torch.bfloat16, device=viewdirs.device)
    o32 = torch.empty(B, 27, device=viewdirs.device) if want_f32 else None
    _lib.check(_lib.lib().durf_view_enc(_stream(), B, _p(_f32(viewdirs)), _p(out), _p(o32)),
               'durf_view_enc')
    return (out, o32) if want_f32 else out


def tile_rows(rows):
    return (rows + 31) // 32 * 32


# the kernel variants the launchers choose by size (tests/test_gpu_dispatch_matrix.py)
DISPATCH = _by_prefix(_H, 'DURF_DISPATCH_')
# marks of the scene-layer launches in the same log word (tests/test_gpu_layers.py)
LAYER_LOG = _by_prefix(_H, 'DURF_LAYERLOG_')


def dispatch_reset():
    _lib.lib().durf_dispatch_reset()


def dispatch_seen():
    """names of the size-selected kernel variants launched since dispatch_reset() (durf_dispatch_seen)"""
    m = int(_lib.lib().durf_dispatch_seen())
    return {k for k, b in DISPATCH.items() if m & b}


def layer_log_seen():
    """which scene-layer launches ran since dispatch_reset() (DURF_LAYERLOG_*)"""
    m = int(_lib.lib().durf_dispatch_seen())
    return {k for k, b in LAYER_LOG.items() if m & b}


def encode_bkgd(t_vals, origins_s, dirs_s, radii, hit, contraction=True, tile=True, f32=False,
                disable_integration=False, cylinder=False, idx=None, count=None):
    """hit=None: no object masking of the samples (MipNerfModel.dynamics=False);
    idx / count: encode only rays idx[:count] into compacted rows (bf16 tiles)"""
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    K = 0 if hit is None else hit.shape[1]
    dev = t_vals.device
    ot = torch.empty(tile_rows(B * N), ENC_DIM, dtype=torch.bfloat16, device=dev) if tile else None
    of = torch.empty(B * N, 60, device=dev) if f32 else None
    with _Timed('encode_bkgd'):
        _lib.check(_lib.lib().durf_encode_bkgd(_stream(), B, N, _p(_f32(t_vals)), _p(_f32(origins_s)),
                                               _p(_f32(dirs_s)), _p(_f32(radii)), _p(hit), K,
                                               (ENC_CONTRACT if contraction else 0) | (ENC_NO_INTEGRATION if disable_integration else 0) |
                                               (ENC_CYLINDER if cylinder else 0),
                                               _p(ot), _p(of), _p(idx), _p(count)), 'durf_encode_bkgd')
    return ot, of


def barf_weights(alpha, max_deg=10):
    """mip.py:217-218 evaluated on the host in float32 arithmetic."""
    import numpy as np
    k = np.arange(max_deg, dtype=np.float32)
    a = np.clip(np.float32(alpha) - k, 0, 1).astype(np.float32) * np.float32(math.pi)
    return ((np.float32(1) - np.cos(a, dtype=np.float32)) / np.float32(2)).astype(np.float32)


def encode_obj(max_rays, idx_k, count_k, t_vals, origins_s, dirs_s, radii, alpha, tile=True, f32=False,
               disable_integration=False, cylinder=False):
    N = t_vals.shape[1] - 1
    dev = t_vals.device
    ot = torch.empty(tile_rows(max_rays * N), ENC_DIM, dtype=torch.bfloat16, device=dev) if tile else None
    of = torch.zeros(max_rays * N, 63, device=dev) if f32 else None
    w = barf_weights(alpha)
    wa = (C.c_float * 10)(*[float(x) for x in w])
    _lib.check(_lib.lib().durf_encode_obj(_stream(), max_rays, N, _p(idx_k), _p(count_k),
                                          _p(_f32(t_vals)), _p(_f32(origins_s)), _p(_f32(dirs_s)),
                                          _p(_f32(radii)), wa,
                                          (ENC_NO_INTEGRATION if disable_integration else 0) | (ENC_CYLINDER if cylinder else 0),
                                          _p(ot), _p(of)), 'durf_encode_obj')
    return ot, of


def mlp_param_count(width, in_dim):
    return int(_lib.lib().durf_mlp_param_count(width, in_dim))


def mlp_layer_offset(width, in_dim, layer, bias):
    return int(_lib.lib().durf_mlp_layer_offset(width, in_dim, layer, int(bias)))


def pack_weights(width, in_dim, mlp_params, want_bwd=False):
    """fp32 flax-layout params of one MLP -> bf16 fragment streams (fwd[, bwd])."""
    dev = mlp_params.device
    wf = torch.empty(int(_lib.lib().durf_wpack_fwd_bytes(width)), dtype=torch.uint8, device=dev)
    wb = None
    if want_bwd:
        wb = torch.empty(int(_lib.lib().durf_wpack_bwd_bytes(width)), dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib().durf_pack_weights(_stream(), width, in_dim, _p(_f32(mlp_params)), _p(wf),
                                            _p(wb)), 'durf_pack_weights')
    return (wf, wb) if want_bwd else wf


def pack_weights_all(bkgd_params, K, obj_params, obj_param_stride, want_bwd=False):
    """Every weight stream of the model in one launch (durf_pack_weights_all): the background MLP and the K object MLPs
    (obj_params: BoxMLP_0 .. BoxMLP_{K-1} back to back, obj_param_stride floats apart).  Returns
    ((bkgd_fwd, bkgd_bwd), (obj_fwd, obj_bwd)); the bwd streams are None without want_bwd, the obj pair is None at K = 0."""
    L = _lib.lib()
    dev = bkgd_params.device
    u8 = lambda n: torch.empty(int(n), dtype=torch.uint8, device=dev)
    bf = u8(L.durf_wpack_fwd_bytes(W_BKGD_))
    bb = u8(L.durf_wpack_bwd_bytes(W_BKGD_)) if want_bwd else None
    of = ob = None
    if K:
        of = u8(K * int(L.durf_wpack_fwd_bytes(W_OBJ_)))
        ob = u8(K * int(L.durf_wpack_bwd_bytes(W_OBJ_))) if want_bwd else None
    _lib.check(L.durf_pack_weights_all(_stream(), _p(_f32(bkgd_params)), IN_BKGD, _p(bf), _p(bb), int(K),
                                       _p(obj_params) if K else None, int(obj_param_stride), IN_OBJ_, _p(of), _p(ob)),
               'durf_pack_weights_all')
    return (bf, bb), ((of, ob) if K else None)


def mlp_stash_bytes(width, rows):
    return int(_lib.lib().durf_mlp_stash_bytes(width, rows))


def mlp_mask_bytes(rows):
    return int(_lib.lib().durf_mlp_mask_bytes(rows))


def mlp_fwd(width, rows, N, enc_tile, view_bf16, wpack_fwd, ray_idx=None, count=None, stash=None,
            raw=None, relu_mask=None, tail_idx=None, tail_count=None):
    """tail_idx / tail_count: once-per-ray rows of a de-duplicated batch after the count*N compacted rows"""
    dev = enc_tile.device
    if raw is None:
        raw = torch.empty(rows, 4, device=dev)
    with _Timed('mlp_fwd_%d%s' % (width, '_train' if stash is not None else '')):
        _lib.check(_lib.lib().durf_mlp_fwd(_stream(), width, rows, N, _p(enc_tile), _p(view_bf16),
                                           _p(ray_idx), _p(count), _p(wpack_fwd), _p(raw), _p(stash),
                                           _p(relu_mask), _p(tail_idx), _p(tail_count)),
                   'durf_mlp_fwd')
    return raw


# DURF_FUSED_ENCODE=0: the background encoding as its own launch in front of the forward (A/B switch; same results).
FUSED_ENCODE = os.environ.get('DURF_FUSED_ENCODE', '1') != '0'
# False: a de-duplicated forward writes compacted raw rows and expand_raw makes the full layout (the parity test of the
# scattered store toggles it: tests/test_gpu_fused_encode.py; not an environment switch any more)
FWD_SCATTER_RAW = True


def mlp_fwd_enc(rows, N, t_vals, origins_s, dirs_s, radii, hit, view_bf16, wpack_fwd, contraction=True,
                disable_integration=False, cylinder=False, ray_idx=None, count=None, stash=None, raw=None, relu_mask=None,
                tail_idx=None, tail_count=None, view_tile=None, raw_full=False):
    """durf_mlp_fwd_enc: the background forward that encodes its own tiles (encode_bkgd + mlp_fwd(256) as one launch)
    -> (raw, enc_tile); enc_tile is what encode_bkgd would have returned (the weight-gradient GEMMs read it).
    view_tile (training): a [tile_rows, 32] bf16 buffer the launch fills with expand_view's output; raw_full (with
    ray_idx / tail_idx): raw comes back in the full [B*N,4] layout -- expand_raw's output, without that launch"""
    dev = t_vals.device
    K = 0 if hit is None else hit.shape[1]
    if raw is None:
        raw = torch.empty(rows, 4, device=dev)
    enc_tile = torch.empty(tile_rows(rows), ENC_DIM, dtype=torch.bfloat16, device=dev)
    flags = ((ENC_CONTRACT if contraction else 0) | (ENC_NO_INTEGRATION if disable_integration else 0) |
             (ENC_CYLINDER if cylinder else 0) | (FWD_RAW_FULL if raw_full else 0))
    with _Timed('mlp_fwd_256%s' % ('_train' if stash is not None else '')):
        _lib.check(_lib.lib().durf_mlp_fwd_enc(_stream(), rows, N, _p(_f32(t_vals)), _p(_f32(origins_s)), _p(_f32(dirs_s)),
                                               _p(_f32(radii)), _p(hit), K, flags, _p(enc_tile), _p(view_bf16),
                                               _p(ray_idx), _p(count), _p(wpack_fwd), _p(raw), _p(stash), _p(relu_mask),
                                               _p(tail_idx), _p(tail_count), _p(view_tile)), 'durf_mlp_fwd_enc')
    return raw, enc_tile


# The K object MLPs touch ~10 % of the rays: their launches are small and latency-bound.  DURF_OVERLAP_OBJECTS issues the
# object work of a stage on a side HIP stream, forked after the background encode / the loss kernel and joined before its
# results are consumed:
#   2 forward + backward + weight gradients;   0 everything on one stream;   1 the object forward;   3 forward + backward.
# The persistent background forward / backward (one workgroup per CU) leave the object launches no CU until their own
# tail, so 1 and 3 measure like 0; what pays is that the objects' weight-gradient launch, queued behind their backward on
# the side stream, starts in the tail of the background backward instead of after it.  Round 3, three interleaved runs per
# mode on one box, k rays/s: cfg3 0: 949 / 948 / 950, 2: 960 / 961 / 954;  cfg2 0: 958 / 960 / 947, 2: 972 / 962 / 961;
# cfg5 0: 704 / 712 / 709, 2: 721 / 702 / 721;  cfg4 (objects on the fp32 kernels, main stream): no change.  The
# background weight-gradient launch then shares its first ~100 us with the objects' (1444-1452 -> 1506-1515 us, HIP events),
# which is what bench.py's roofline line reports.  Moving ONLY the objects' weight gradients to the side stream, started
# together with the background ones, is destructive (background launch 1725-1777 us, 898-910 k rays/s): measured, dropped.
# The same switch costs at small batches, where every kernel is one latency-bound round and a fork / join is one more
# dependency in the chain (cfg3 shape, k rays/s, 0 vs 2: 512 rays 595 -> 545-559, 1024 rays 750-756 -> 745, 2048 rays 883
# -> 902-908, 4096 rays above): 'auto' (default) = 2 from OVERLAP_MIN_ROWS sample rows per step (4 rounds of background blocks), else 0.
# The rule itself -- this switch, DURF_OBJ_MSPLIT and DURF_OBJ_MIX, read from the environment on every call -- is the library's
# (durf_step_policy, include/durf_hip.h DURF_POLICY_*); everything below reads it from there.
class StepPolicy(collections.namedtuple('StepPolicy', 'side_fwd side_bwd side_dw msplit mix_enabled')):      # (in bit order)
    @property
    def mix(self):
        """the bf16 object MLPs ride in the background MLP's persistent launches: enabled, and the step runs on one stream"""
        return self.mix_enabled and not (self.side_fwd or self.side_bwd or self.side_dw)


def step_policy(rows):
    """the launch policy of a step (or a render chunk) of `rows` sample rows per level"""
    m = int(_lib.lib().durf_step_policy(rows))
    return StepPolicy(*(bool(m & (1 << i)) for i in range(5)))


def __getattr__(name):
    if name == 'OVERLAP_MIN_ROWS':          # include/durf_hip.h DURF_OVERLAP_MIN_ROWS
        return int(_lib.lib().durf_overlap_min_rows())
    if name == '_MODE':                     # what set_overlap_mode() takes to restore the present setting
        small, large = overlap_mode(0), overlap_mode(1 << 62)
        return small if small == large else 'auto'
    raise AttributeError('module %r has no attribute %r' % (__name__, name))


def set_overlap_mode(mode):
    """'auto' / '0' .. '3'; the one-call C step runs '1' and '3' (experiment modes of this file) as '2' (csrc/side_stream.h)"""
    os.environ['DURF_OVERLAP_OBJECTS'] = mode


def overlap_mode(rows):
    """'0' .. '3' for a step (or a render chunk) of `rows` sample rows per level"""
    p = step_policy(rows)
    return '2' if p.side_dw else '3' if p.side_bwd else '1' if p.side_fwd else '0'


def overlap_forward(rows):
    return step_policy(rows).side_fwd


def overlap_backward(rows):
    return step_policy(rows).side_bwd


def overlap_dw(rows):
    return step_policy(rows).side_dw


_SIDE = {}


def side_stream(device):
    key = (device.type, device.index)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


class on_side:
    """with on_side(device, enabled): ... -- launches inside go to the side stream (no-op when disabled).  fork():
    the side stream waits for everything issued so far on the current stream; join(): the reverse."""

    def __init__(self, device, enabled=True):
        self.enabled = bool(enabled) and device.type == 'cuda'
        self.side = side_stream(device) if self.enabled else None
        self.ctx = None

    def fork(self):
        if self.enabled:
            self.side.wait_stream(torch.cuda.current_stream())

    def join(self):
        if self.enabled:
            torch.cuda.current_stream().wait_stream(self.side)

    def __enter__(self):
        if self.enabled:
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
        return self

    def __exit__(self, *a):
        if self.enabled:
            self.ctx.__exit__(*a)


# Evaluate the background MLP once per box-hit ray instead of once per sample (exact: see durf_expand_raw in
# include/durf_hip.h).  Module switch for A/B measurements and tests.
DEDUP_HIT_RAYS = os.environ.get('DURF_DEDUP_HIT_RAYS', '1') != '0'


def expand_raw(B, N, raw_c, slot2, count2, raw_tail=None):
    """compacted raw (count2[0]*N rows of the sample-by-sample rays, then one row per box-hit ray) -> [B*N,4];
    raw_tail [B,4]: fp32 re-evaluation of the box-hit rays' rows (mlp_fwd_f32 with enc=None), used instead of them"""
    raw_full = torch.empty(B * N, 4, device=raw_c.device)
    # the tail starts at row count2[0]*N: hand the kernel a pointer to that row (device-side count -> device-side offset
    # is not available on the host, so the kernel takes the base and the slot of the tail separately)
    _lib.check(_lib.lib().durf_expand_raw(_stream(), B, N, _p(_f32(raw_c)), _p(count2), _p(slot2), _p(raw_full),
                                          _p(raw_tail)), 'durf_expand_raw')
    return raw_full


BKGD_GREY, BKGD_WHITE, BKGD_RAND = 0, 1, 2


def composite_fwd(raw_bkgd, raw_obj, slot, t_vals, dirs_s, density_bias=-1.0, bkgd_mode=BKGD_GREY,
                  want_t=True):
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    K = len(raw_obj)
    dev = t_vals.device
    rgb = torch.empty(B, 3, device=dev)
    depth = torch.empty(B, device=dev)
    acc = torch.empty(B, device=dev)
    weights = torch.empty(B, N, device=dev)
    t_mids = torch.empty(B, N, device=dev) if want_t else None
    t_dists = torch.empty(B, N, device=dev) if want_t else None
    ptrs = (C.c_void_p * max(K, 1))(*[r.data_ptr() for r in raw_obj])
    with _Timed('composite_fwd'):
        _lib.check(_lib.lib().durf_composite_fwd(_stream(), B, N, K, _p(_f32(raw_bkgd)), ptrs, _p(slot),
                                                 _p(_f32(t_vals)), _p(_f32(dirs_s)), density_bias,
                                                 bkgd_mode, _p(rgb), _p(depth), _p(acc), _p(weights),
                                                 _p(t_mids), _p(t_dists)), 'durf_composite_fwd')
    return rgb, depth, acc, weights, t_mids, t_dists


def composite_resample(raw_bkgd, raw_obj, slot, t_vals, dirs_s, density_bias=-1.0, bkgd_mode=BKGD_GREY,
                       padding=0.01, u_rand=None, want_t=True, prep=None):
    """composite_fwd + resample in one launch (bit-identical to the two calls) -> (rgb, depth, acc, weights,
    t_mids, t_dists, t_vals_next).  prep = dict(lossmult, gt_depth, sky, dyn, zo, eps, box_loss_mult, level,
    disable_multiscale, norms [L,5]) also fills norms[level] (when level == 0) and norms[level + 1]: durf_loss_prep's
    job for both levels."""
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    K = len(raw_obj)
    dev = t_vals.device
    rgb = torch.empty(B, 3, device=dev)
    depth = torch.empty(B, device=dev)
    acc = torch.empty(B, device=dev)
    weights = torch.empty(B, N, device=dev)
    t_mids = torch.empty(B, N, device=dev) if want_t else None
    t_dists = torch.empty(B, N, device=dev) if want_t else None
    t_next = torch.empty(B, N + 1, device=dev)
    ptrs = (C.c_void_p * max(K, 1))(*[r.data_ptr() for r in raw_obj])
    pa = [None] * 5 + [0.0, 0.0, 0, 0] + [None] * 4
    if prep is not None:
        lvl = int(prep['level'])
        norms = prep['norms']
        buf = torch.empty(2, PREP_ROWS, B, device=dev)
        pa = [_p(_f32(prep['lossmult'])), _p(_f32(prep['gt_depth'])), _p(_f32(prep['sky'])), _p(prep['dyn']),
              _p(_f32(prep['zo'])), float(prep['eps']), float(prep['box_loss_mult']), lvl,
              int(prep['disable_multiscale']),
              _p(buf[0]) if lvl == 0 else None, _p(norms[lvl]) if lvl == 0 else None, _p(buf[1]), _p(norms[lvl + 1])]
    with _Timed('composite_resample'):
        _lib.check(_lib.lib().durf_composite_resample(
            _stream(), B, N, K, _p(_f32(raw_bkgd)), ptrs, _p(slot), _p(_f32(t_vals)), _p(_f32(dirs_s)), density_bias,
            bkgd_mode, _p(rgb), _p(depth), _p(acc), _p(weights), _p(t_mids), _p(t_dists), padding,
            _p(None if u_rand is None else _f32(u_rand)), _p(t_next), *pa), 'durf_composite_resample')
    return rgb, depth, acc, weights, t_mids, t_dists, t_next


def resample(t_vals, weights, padding=0.01, u_rand=None):
    B, N = weights.shape
    out = torch.empty(B, N + 1, device=t_vals.device)
    _lib.check(_lib.lib().durf_resample(_stream(), B, N, _p(_f32(t_vals)), _p(_f32(weights)), padding,
                                        _p(None if u_rand is None else _f32(u_rand)), _p(out)),
               'durf_resample')
    return out


def sorted_piecewise_constant_pdf(bins, weights, u_rand=None):
    """math.sorted_piecewise_constant_pdf(key, bins, weights, num_samples=N+1, randomized=u_rand is not None)"""
    B, N = weights.shape
    out = torch.empty(B, N + 1, device=bins.device)
    _lib.check(_lib.lib().durf_sorted_piecewise_constant_pdf(_stream(), B, N, _p(_f32(bins)), _p(_f32(weights)),
                                                             _p(None if u_rand is None else _f32(u_rand)), _p(out)),
               'durf_sorted_piecewise_constant_pdf')
    return out


# ---------------------------------------------------------------------------
# training ops
# ---------------------------------------------------------------------------
PREP_ROWS, TERM_ROWS = 5, 7
TERM_NAMES = ('rgb', 'obj', 'depth', 'near', 'empty', 'sky', 'dist')


def loss_prep(t_vals, lossmult, gt_depth, sky, dyn, zo, eps, box_loss_mult, level, disable_multiscale=False,
              norm=None):
    """-> norm[5] device floats: sum m, sum depth_mask, sum sky_mask, min near-dist^2, sum dyn."""
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    dev = t_vals.device
    prep = torch.empty(PREP_ROWS, B, device=dev)
    if norm is None:
        norm = torch.empty(PREP_ROWS, device=dev)
    _lib.check(_lib.lib().durf_loss_prep(_stream(), B, N, _p(_f32(t_vals)), _p(_f32(lossmult)),
                                         _p(_f32(gt_depth)), _p(_f32(sky)), _p(dyn), _p(_f32(zo)),
                                         eps, box_loss_mult, level, int(disable_multiscale), _p(prep),
                                         _p(norm)), 'durf_loss_prep')
    return norm


def loss_bwd(raw_bkgd, raw_obj, slot, t_vals, dirs_s, pixels, lossmult, gt_depth, sky, dyn, zo, norm, eps,
             mults, box_loss_mult, level, bg, density_bias=-1.0, disable_multiscale=False, sums=None, render_out=None,
             draw_ray_sum=None, defer_sums=False):
    """-> draw [B*N,4], term_sums[7] (rgb, obj, depth, near, empty, sky, dist numerators).
    defer_sums: no reduction launch here; returns (draw, terms [7,B]) for train_stats(..., terms=...) to reduce.
    render_out = (rgb [B,3], depth [B], acc [B], weights [B,N], t_mids [B,N], t_dists [B,N]) tensors to fill with the level's rendered
    outputs (what composite_fwd returns; a training step then skips that launch for the last level)."""
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    K = len(raw_obj)
    dev = t_vals.device
    draw = torch.empty(B * N, 4, device=dev)
    terms = torch.empty(TERM_ROWS, B, device=dev)
    if sums is None and not defer_sums:
        sums = torch.empty(TERM_ROWS, device=dev)
    ptrs = (C.c_void_p * max(K, 1))(*[r.data_ptr() for r in raw_obj])
    m = (C.c_float * 6)(*[float(x) for x in mults])
    _lib.check(_lib.lib().durf_loss_bwd(_stream(), B, N, K, _p(_f32(raw_bkgd)), ptrs, _p(slot),
                                        _p(_f32(t_vals)), _p(_f32(dirs_s)), _p(_f32(pixels)),
                                        _p(_f32(lossmult)), _p(_f32(gt_depth)), _p(_f32(sky)), _p(dyn),
                                        _p(_f32(zo)), _p(norm), eps, m, box_loss_mult, level,
                                        int(disable_multiscale), bg, density_bias, _p(draw), _p(terms),
                                        None if defer_sums else _p(sums), *[_p(t) for t in (render_out or (None,) * 6)],
                                        _p(draw_ray_sum)), 'durf_loss_bwd')
    return draw, (terms if defer_sums else sums)


LossLevel = _H.durf_loss_level


def loss_bwd_levels(levels, slot, dirs_s, pixels, lossmult, gt_depth, sky, dyn, zo, eps, box_loss_mult, bg, density_bias=-1.0,
                    disable_multiscale=False):
    """loss_bwd(defer_sums=True) of EVERY level as one launch (durf_loss_bwd_levels).  levels: one dict per level with
    raw_bkgd, raw_obj (list), t_vals, norm, mults, level[, render_out (6 tensors)][, draw_ray_sum]
    -> [(draw [B*N,4], terms [7,B])] per level"""
    L = len(levels)
    B, N = levels[0]['t_vals'].shape[0], levels[0]['t_vals'].shape[1] - 1
    K = len(levels[0]['raw_obj'])
    dev = levels[0]['t_vals'].device
    arr = (LossLevel * L)()
    out, keep = [], []
    for i, lv in enumerate(levels):
        a = arr[i]
        draw = torch.empty(B * N, 4, device=dev)
        terms = torch.empty(TERM_ROWS, B, device=dev)
        a.raw_bkgd, a.t_vals, a.norm = _p(_f32(lv['raw_bkgd'])), _p(_f32(lv['t_vals'])), _p(lv['norm'])
        for k, r in enumerate(lv['raw_obj']):
            a.raw_obj[k] = r.data_ptr()
        a.mults = (C.c_float * 6)(*[float(x) for x in lv['mults']])
        a.level = int(lv['level'])
        a.draw, a.terms = _p(draw), _p(terms)
        ro = lv.get('render_out') or (None,) * 6
        a.rgb_out, a.depth_out, a.acc_out, a.weights_out, a.t_mids_out, a.t_dists_out = (_p(t) for t in ro)
        a.draw_ray_sum = _p(lv.get('draw_ray_sum'))
        keep.append(lv)
        out.append((draw, terms))
    _lib.check(_lib.lib().durf_loss_bwd_levels(_stream(), B, N, K, L, C.cast(arr, C.c_void_p), _p(slot), _p(_f32(dirs_s)),
                                               _p(_f32(pixels)), _p(_f32(lossmult)), _p(_f32(gt_depth)), _p(_f32(sky)), _p(dyn),
                                               _p(_f32(zo)), float(eps), float(box_loss_mult), int(disable_multiscale),
                                               float(bg), float(density_bias)), 'durf_loss_bwd_levels')
    return out


STAT_ROWS = ('losses', 'obj_losses', 'd_losses', 'n_losses', 'e_losses', 's_losses', 'distr_losses', 'tv_losses',
             'offsets', 'offset_x', 'offset_y', 'offset_z', 'offset_yaw', 'psnrs', 'obj_psnrs')
STATS_ASSEMBLE, STATS_PSNR = 1, 2


def train_stats(norms, sums, weight_l2, pose6, prev6, target6, t_vals_levels, mults, mode, out=None, terms=None):
    """Scalars of utils.Stats in one launch; see durf_train_stats.  -> out [2 + 17 L]
    terms: per-level [7,B] tensors of loss_bwd(defer_sums=True); reduced into `sums` by the same launch."""
    L = norms.shape[0]
    K = 0 if pose6 is None else pose6.shape[0]
    N = t_vals_levels[0].shape[1] - 1
    if out is None:
        out = torch.empty(2 + 17 * L, device=norms.device)
    ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in t_vals_levels])
    m = (C.c_float * 6)(*[float(x) for x in mults])
    _lib.check(_lib.lib().durf_train_stats(_stream(), L, K, N, _p(norms), _p(sums), _p(weight_l2),
                                           _p(pose6) if K else None, _p(prev6) if K else None,
                                           _p(target6) if K else None, ptrs, m, mode, _p(out),
                                           (C.c_void_p * L)(*[t.data_ptr() for t in terms]) if terms is not None else None,
                                           int(terms[0].shape[1]) if terms is not None else 0), 'durf_train_stats')
    return out


def stats_scrub(norms, sums, weight_l2, pose6, prev6, target6, t_vals_levels, mults, mode, terms, grad, inv_world, max_val,
                poison=None):
    """train_stats + the scrub pass of clip_adam (+ the multi-hit outcome: poison = (cls_count, box_floats, K, mlp0_floats,
    obj_floats) of poison_multi_hit, single device only) as ONE launch (durf_stats_scrub) -> (out [2 + 17 L], scratch);
    adam_apply(.., scratch) finishes the update"""
    L = norms.shape[0]
    K = 0 if pose6 is None else pose6.shape[0]
    N = t_vals_levels[0].shape[1] - 1
    dev = norms.device
    out = torch.empty(2 + 17 * L, device=dev)
    n = grad.numel()
    scratch = torch.empty(int(_lib.lib().durf_optim_scratch_floats(n)), device=dev)
    ptrs = (C.c_void_p * L)(*[t.data_ptr() for t in t_vals_levels])
    m = (C.c_float * 6)(*[float(x) for x in mults])
    cls, bf, Kb, m0, of = poison if poison is not None else (None, 0, 0, 0, 0)
    _lib.check(_lib.lib().durf_stats_scrub(_stream(), L, K, N, _p(norms), _p(sums), _p(weight_l2),
                                           _p(pose6) if K else None, _p(prev6) if K else None, _p(target6) if K else None,
                                           ptrs, m, mode, _p(out),
                                           (C.c_void_p * L)(*[t.data_ptr() for t in terms]) if terms is not None else None,
                                           int(terms[0].shape[1]) if terms is not None else 0, n, _p(_f32(grad)),
                                           float(inv_world), float(max_val), _p(scratch), _p(cls), int(bf), int(Kb), int(m0),
                                           int(of)), 'durf_stats_scrub')
    return out, scratch


def adam_apply(params, m, v, grad, max_norm, lr, step, scratch):
    """the Adam pass of clip_adam behind stats_scrub's scrub pass -> stats[4] as clip_adam"""
    _bump_generation(params)
    stats = torch.empty(4, device=params.device)
    _lib.check(_lib.lib().durf_adam_apply(_stream(), params.numel(), _p(_f32(params)), _p(_f32(m)), _p(_f32(v)),
                                          _p(_f32(grad)), float(max_norm), float(lr), int(step), _p(scratch), _p(stats)),
               'durf_adam_apply')
    return stats


def weight_decay(params, grad, mult, lo=0, hi=None, want_l2=True):
    """Config.weight_decay_mult (train_boxpose.py:73-75): grad[lo:hi) += (2 mult / n) params[lo:hi); -> weight_l2 [1] =
    mult * mean(params^2) over the whole buffer (None unless want_l2)"""
    n = params.numel()
    hi = n if hi is None else hi
    L = _lib.lib()
    out = torch.empty(1, device=params.device) if want_l2 else None
    scratch = torch.empty(int(L.durf_optim_scratch_floats(n)), device=params.device) if want_l2 else None
    _lib.check(L.durf_weight_decay(_stream(), n, _p(_f32(params)), _p(_f32(grad)), int(lo), int(hi), float(mult), _p(scratch),
                                   _p(out)), 'durf_weight_decay')
    return out


def density_noise(raw, scale, normal=None, seed=None, level=0):
    """MipNerfModel.density_noise (obbpose_model.py:236-240): raw[:, 3] += scale * z in place; z = `normal` [rows] or the
    library's own draws under `seed` (Philox block (row, 1 + level, 0, 0) through Box-Muller; oracle/philox_ref.py)"""
    assert raw.dim() == 2 and raw.shape[1] == 4 and raw.is_contiguous()
    assert (normal is None) != (seed is None), 'either the draws or the key they are made under'
    if normal is not None:
        normal = _f32(normal.reshape(-1).contiguous())
        assert normal.numel() == raw.shape[0]
    lo, hi = (0, 0) if seed is None else split_seed(seed)
    _lib.check(_lib.lib().durf_density_noise(_stream(), raw.shape[0], _p(_f32(raw)), float(scale), _p(normal), lo, hi, int(level)),
               'durf_density_noise')
    return raw


class Comm:
    """A communicator of the library's own in-stream all-reduce (csrc/comm.hip: RCCL resolved at run time)"""

    def __init__(self, world, rank, uid):
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(uid), COMM_ID_BYTES)
        _lib.check(_lib.lib().durf_comm_init(int(world), int(rank), C.cast(buf, C.c_void_p), C.byref(h)), 'durf_comm_init')
        self.handle, self.world, self.rank = h, int(world), int(rank)

    def all_reduce_sum(self, t):
        """in place, on the current stream (fp32, contiguous)"""
        assert t.dtype == torch.float32 and t.is_contiguous()
        _lib.check(_lib.lib().durf_allreduce_sum(_stream(), self.handle, _p(t), t.numel()), 'durf_allreduce_sum')

    def destroy(self):
        if self.handle:
            _lib.check(_lib.lib().durf_comm_destroy(self.handle), 'durf_comm_destroy')
            self.handle = None


def comm_available():
    return bool(_lib.lib().durf_comm_available())


def comm_unique_id():
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _lib.check(_lib.lib().durf_comm_unique_id(C.cast(buf, C.c_void_p)), 'durf_comm_unique_id')
    return buf.raw


def stats_views(out, L):
    """dict of named views into the durf_train_stats buffer"""
    d = {'loss': out[0], 'sampling_stats': out[1 + 15 * L:1 + 17 * L], 'weight_l2': out[1 + 17 * L]}
    for i, name in enumerate(STAT_ROWS):
        d[name] = out[1 + i * L:1 + (i + 1) * L]
    return d


def mlp_bwd(width, rows, N, draw, wpack_bwd, relu_mask, ray_idx=None, count=None, want_d_enc=False,
            tail_idx=None, tail_count=None, draw_ray_sum=None, dz=None, dz_out=None, d_enc=None):
    """-> dz (same layout as the stash), dz_out tile [rows,16][, d_enc [rows,64] fp32]
    dz / dz_out / d_enc: the caller's buffers instead of fresh ones (as mlp_fwd's raw)"""
    dev = draw.device
    if dz is None:
        dz = torch.empty(mlp_stash_bytes(width, rows), dtype=torch.uint8, device=dev)
    if dz_out is None:
        dz_out = torch.empty(tile_rows(rows), 16, dtype=torch.bfloat16, device=dev)
    if not want_d_enc:
        d_enc = None
    elif d_enc is None:
        d_enc = torch.zeros(rows, ENC_DIM, device=dev)
    with _Timed('mlp_bwd_%d' % width):
        _lib.check(_lib.lib().durf_mlp_bwd(_stream(), width, rows, N, _p(_f32(draw)), _p(ray_idx), _p(count),
                                           _p(wpack_bwd), _p(relu_mask), _p(dz), _p(dz_out), _p(d_enc),
                                           _p(tail_idx), _p(tail_count), _p(draw_ray_sum)),
                   'durf_mlp_bwd')
    return (dz, dz_out, d_enc) if want_d_enc else (dz, dz_out)


def expand_view(rows, N, view_bf16, ray_idx=None, count=None, tail_idx=None, tail_count=None, out=None):
    if out is None:
        out = torch.empty(tile_rows(rows), VIEW_DIM, dtype=torch.bfloat16, device=view_bf16.device)
    _lib.check(_lib.lib().durf_expand_view(_stream(), rows, N, _p(view_bf16), _p(ray_idx), _p(count),
                                           _p(out), _p(tail_idx), _p(tail_count)), 'durf_expand_view')
    return out


def dw_buffers(width, device):
    part = torch.empty(int(_lib.lib().durf_dw_part_floats(width)), device=device)
    bpart = torch.empty(int(_lib.lib().durf_dw_bpart_floats(width)), device=device)
    return part, bpart


def mlp_dw(width, rows, N, enc_tiles, view_tiles, stashes, dzs, dz_outs, part, bpart, count=None):
    """Weight-gradient partials of one MLP over the samples of every level (lists: one entry per level)."""
    L = len(stashes)
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])
    with _Timed('mlp_dw_%d' % width):
        _lib.check(_lib.lib().durf_mlp_dw(_stream(), width, rows, N, _p(count), L, arr(enc_tiles), arr(view_tiles),
                                          arr(stashes), arr(dzs), arr(dz_outs), _p(part), _p(bpart)), 'durf_mlp_dw')


def _levels_args(rows_l, n_l, count_l):
    L = len(rows_l)
    return (L, (C.c_size_t * L)(*[int(r) for r in rows_l]), (C.c_int * L)(*[int(n) for n in n_l]),
            (C.c_void_p * L)(*[None if c is None else c.data_ptr() for c in count_l]))


def mlp_dw_levels(width, rows_l, n_l, count_l, enc_tiles, view_tiles, stashes, dzs, dz_outs, part, bpart):
    """mlp_dw with per-segment geometry: row capacity, rows per ray and device ray count of every segment"""
    L, rows_a, n_a, cnt_a = _levels_args(rows_l, n_l, count_l)
    arr = lambda ts: (C.c_void_p * L)(*[t.data_ptr() for t in ts])
    with _Timed('mlp_dw_%d' % width):
        _lib.check(_lib.lib().durf_mlp_dw_levels(_stream(), width, L, rows_a, n_a, cnt_a, arr(enc_tiles), arr(view_tiles),
                                                 arr(stashes), arr(dzs), arr(dz_outs), _p(part), _p(bpart)),
                   'durf_mlp_dw_levels')


def mlp_dw_finalize_levels(width, in_dim, rows_l, n_l, count_l, part, bpart, grad_mlp, mlp_params):
    L, rows_a, n_a, cnt_a = _levels_args(rows_l, n_l, count_l)
    with _Timed('mlp_dw_finalize_%d' % width):
        _lib.check(_lib.lib().durf_mlp_dw_finalize_levels(_stream(), width, in_dim, L, rows_a, n_a, cnt_a, _p(part),
                                                          _p(bpart), _p(grad_mlp), _p(_f32(mlp_params))),
                   'durf_mlp_dw_finalize_levels')


def mlp_dw_finalize(width, in_dim, rows, N, nlevels, part, bpart, grad_mlp, mlp_params, count=None):
    """rows, N, nlevels, count: as in the mlp_dw call that wrote the partials; mlp_params: the MLP's fp32 parameters
    (the linear bottleneck layer's gradients are derived from them, see durf_mlp_dw_finalize)"""
    with _Timed('mlp_dw_finalize_%d' % width):
        _lib.check(_lib.lib().durf_mlp_dw_finalize(_stream(), width, in_dim, rows, N, _p(count), nlevels, _p(part),
                                                   _p(bpart), _p(grad_mlp), _p(_f32(mlp_params))), 'durf_mlp_dw_finalize')


# ---------------------------------------------------------------------------
# the K object MLPs of one level as one call each (csrc/objects.hip)
# ---------------------------------------------------------------------------
W_OBJ_, IN_OBJ_ = W_OBJ, 63
W_BKGD_, IN_BKGD = W_BKGD, 60


class ObjSlabs:
    """[K, ...] slabs of one level for the batched object calls (strides fixed by the library)."""

    def __init__(self, K, B, N, device, train):
        L = _lib.lib()
        rows = B * N
        u8 = lambda n: torch.empty(K * int(n), dtype=torch.uint8, device=device)
        self.K, self.B, self.N = K, B, N
        self.enc = u8(L.durf_obj_enc_stride(B, N))
        self.raw = torch.empty(K, rows, 4, device=device)
        self.stash = u8(mlp_stash_bytes(W_OBJ_, rows)) if train else None
        self.mask = u8(mlp_mask_bytes(rows)) if train else None
        self.dz = self.dz_out = self.d_enc = None

    def raws(self):
        return [self.raw[k] for k in range(self.K)]


def pack_weights_batch(K, obj_params, param_stride, want_bwd=False):
    """obj_params: flat fp32 params of BoxMLP_0 .. BoxMLP_{K-1}, back to back"""
    L = _lib.lib()
    dev = obj_params.device
    wf = torch.empty(K * int(L.durf_wpack_fwd_bytes(W_OBJ_)), dtype=torch.uint8, device=dev)
    wb = torch.empty(K * int(L.durf_wpack_bwd_bytes(W_OBJ_)), dtype=torch.uint8, device=dev) if want_bwd else None
    _lib.check(L.durf_pack_weights_batch(_stream(), W_OBJ_, IN_OBJ_, K, _p(obj_params), param_stride, _p(wf), _p(wb)),
               'durf_pack_weights_batch')
    return wf, wb


def obj_fwd_batch(slabs, idx, count, t_vals, origins_s, dirs_s, radii, alpha, view_bf16, wf, view_tile=None,
                  disable_integration=False, cylinder=False):
    w = barf_weights(alpha)
    wa = (C.c_float * 10)(*[float(x) for x in w])
    with _Timed('obj_fwd_batch'):
        _lib.check(_lib.lib().durf_obj_fwd_batch(
            _stream(), slabs.K, slabs.B, slabs.N, _p(idx), _p(count), _p(_f32(t_vals)), _p(_f32(origins_s)),
            _p(_f32(dirs_s)), _p(_f32(radii)), wa,
            (ENC_NO_INTEGRATION if disable_integration else 0) | (ENC_CYLINDER if cylinder else 0), _p(view_bf16),
            _p(wf), _p(slabs.enc), _p(slabs.raw), _p(slabs.stash), _p(slabs.mask), _p(view_tile)), 'durf_obj_fwd_batch')


def obj_mix(rows):
    """whether a training step of `rows` sample rows per level issues its bf16 object MLPs as items of the background MLP's
    persistent launches (durf_mlp_fwd_enc_obj / durf_mlp_bwd_obj: one stream, the M-split regime; DURF_OBJ_MIX=0: A/B switch)"""
    return step_policy(rows).mix


def mlp_fwd_enc_obj(rows, N, t_vals, origins_s, dirs_s, radii, hit, view_bf16, wpack_fwd, slabs, obj_idx, obj_count, alpha, obj_wf,
                    ray_idx, count, tail_idx, tail_count, stash, relu_mask, contraction=True, disable_integration=False,
                    cylinder=False, view_tile=None, raw_full=True, obj_view_tile=None):
    """mlp_fwd_enc (the background MLP on the de-duplicated ray classes) + obj_fwd_batch (the K object MLPs into `slabs`) as
    ONE launch (durf_mlp_fwd_enc_obj: the heterogeneous persistent grid of a small training step) -> (raw, enc_tile);
    every output bit-identical to the two calls"""
    dev = t_vals.device
    K = hit.shape[1]
    raw = torch.empty(rows, 4, device=dev)
    enc_tile = torch.empty(tile_rows(rows), ENC_DIM, dtype=torch.bfloat16, device=dev)
    flags = ((ENC_CONTRACT if contraction else 0) | (ENC_NO_INTEGRATION if disable_integration else 0) |
             (ENC_CYLINDER if cylinder else 0) | (FWD_RAW_FULL if raw_full else 0))
    wa = (C.c_float * 10)(*[float(x) for x in barf_weights(alpha)])
    with _Timed('mlp_fwd_256%s' % ('_train' if stash is not None else '')):
        _lib.check(_lib.lib().durf_mlp_fwd_enc_obj(
            _stream(), rows, N, _p(_f32(t_vals)), _p(_f32(origins_s)), _p(_f32(dirs_s)), _p(_f32(radii)), _p(hit), K, flags,
            _p(enc_tile), _p(view_bf16), _p(ray_idx), _p(count), _p(wpack_fwd), _p(raw), _p(stash), _p(relu_mask), _p(tail_idx),
            _p(tail_count), _p(view_tile), slabs.B, _p(obj_idx), _p(obj_count), wa,
            (ENC_NO_INTEGRATION if disable_integration else 0) | (ENC_CYLINDER if cylinder else 0), _p(obj_wf), _p(slabs.enc),
            _p(slabs.raw), _p(slabs.stash), _p(slabs.mask), _p(obj_view_tile)), 'durf_mlp_fwd_enc_obj')
    return raw, enc_tile


def mlp_bwd_obj(rows, N, draw, wpack_bwd, relu_mask, ray_idx, count, tail_idx, tail_count, draw_ray_sum, slabs_levels, obj_idx,
                obj_count, obj_draws, obj_wb):
    """mlp_bwd(256) of the background MLP + obj_bwd_batch_levels of the K object MLPs (slabs_levels / obj_draws: per level)
    as ONE launch (durf_mlp_bwd_obj) -> (dz, dz_out) of the background MLP; the slabs receive dz / dz_out; bit-identical"""
    L = _lib.lib()
    dev = draw.device
    dz = torch.empty(mlp_stash_bytes(256, rows), dtype=torch.uint8, device=dev)
    dz_out = torch.empty(tile_rows(rows), 16, dtype=torch.bfloat16, device=dev)
    s0 = slabs_levels[0]
    K, B, nl = s0.K, s0.B, len(slabs_levels)
    for sl in slabs_levels:
        sl.dz = torch.empty(K * mlp_stash_bytes(W_OBJ_, B * N), dtype=torch.uint8, device=dev)
        sl.dz_out = torch.empty(K * int(L.durf_obj_dzout_stride(B, N)), dtype=torch.uint8, device=dev)
        sl.d_enc = None
    arr = lambda ts: (C.c_void_p * nl)(*[t.data_ptr() for t in ts])
    with _Timed('mlp_bwd_256'):
        _lib.check(L.durf_mlp_bwd_obj(_stream(), rows, N, _p(_f32(draw)), _p(ray_idx), _p(count), _p(wpack_bwd), _p(relu_mask),
                                      _p(dz), _p(dz_out), _p(tail_idx), _p(tail_count), _p(draw_ray_sum), K, B, nl, _p(obj_idx),
                                      _p(obj_count), arr([_f32(d) for d in obj_draws]), _p(obj_wb),
                                      arr([s.mask for s in slabs_levels]), arr([s.dz for s in slabs_levels]),
                                      arr([s.dz_out for s in slabs_levels])), 'durf_mlp_bwd_obj')
    return dz, dz_out


def obj_view_tiles(K, B, N, device):
    return torch.empty(K * int(_lib.lib().durf_obj_view_stride(B, N)), dtype=torch.uint8, device=device)


def obj_bwd_batch(slabs, idx, count, draw, wb, want_d_enc=False):
    L = _lib.lib()
    dev = draw.device
    K, B, N = slabs.K, slabs.B, slabs.N
    slabs.dz = torch.empty(K * mlp_stash_bytes(W_OBJ_, B * N), dtype=torch.uint8, device=dev)
    slabs.dz_out = torch.empty(K * int(L.durf_obj_dzout_stride(B, N)), dtype=torch.uint8, device=dev)
    slabs.d_enc = torch.empty(K, B * N, ENC_DIM, device=dev) if want_d_enc else None     # every valid row is written
    with _Timed('obj_bwd_batch'):
        _lib.check(L.durf_obj_bwd_batch(_stream(), K, B, N, _p(idx), _p(count), _p(_f32(draw)), _p(wb), _p(slabs.mask),
                                        _p(slabs.dz), _p(slabs.dz_out), _p(slabs.d_enc)), 'durf_obj_bwd_batch')


def obj_bwd_batch_levels(slabs_levels, idx, count, draws, wb):
    """obj_bwd_batch (no d(enc)) for every level of a step in one call (durf_obj_bwd_batch_levels: one launch at small batches);
    slabs_levels / draws: per level, in the order they are to be issued"""
    L = _lib.lib()
    s0 = slabs_levels[0]
    K, B, N = s0.K, s0.B, s0.N
    nl = len(slabs_levels)
    dev = draws[0].device
    for sl in slabs_levels:
        sl.dz = torch.empty(K * mlp_stash_bytes(W_OBJ_, B * N), dtype=torch.uint8, device=dev)
        sl.dz_out = torch.empty(K * int(L.durf_obj_dzout_stride(B, N)), dtype=torch.uint8, device=dev)
        sl.d_enc = None
    arr = lambda ts: (C.c_void_p * nl)(*[t.data_ptr() for t in ts])
    with _Timed('obj_bwd_batch'):
        _lib.check(L.durf_obj_bwd_batch_levels(_stream(), K, B, N, nl, _p(idx), _p(count), arr([_f32(d) for d in draws]), _p(wb),
                                               arr([s.mask for s in slabs_levels]), arr([s.dz for s in slabs_levels]),
                                               arr([s.dz_out for s in slabs_levels])), 'durf_obj_bwd_batch_levels')


def obj_dw_batch(slabs_levels, view_tile, count, grad_obj, grad_stride, obj_params):
    """weight gradients of all K object MLPs over every level -> grad_obj (flat, K x grad_stride floats);
    obj_params: their fp32 parameters with the same stride"""
    L = _lib.lib()
    s0 = slabs_levels[0]
    K, B, N = s0.K, s0.B, s0.N
    nl = len(slabs_levels)
    dev = grad_obj.device
    part = torch.empty(K * int(L.durf_dw_part_floats(W_OBJ_)), device=dev)
    bpart = torch.empty(K * int(L.durf_dw_bpart_floats(W_OBJ_)), device=dev)
    arr = lambda ts: (C.c_void_p * nl)(*[t.data_ptr() for t in ts])
    with _Timed('obj_dw_batch'):
        _lib.check(L.durf_obj_dw_batch(_stream(), K, B, N, _p(count), nl, arr([s.enc for s in slabs_levels]),
                                       arr([view_tile] * nl), arr([s.stash for s in slabs_levels]),
                                       arr([s.dz for s in slabs_levels]), arr([s.dz_out for s in slabs_levels]),
                                       IN_OBJ_, _p(part), _p(bpart), _p(grad_obj), grad_stride, _p(_f32(obj_params))),
                   'durf_obj_dw_batch')


def obj_dw_partials(slabs_levels, view_tile, count):
    """the split-K half of obj_dw_batch: returns (part, bpart) for dw_finalize_all"""
    L = _lib.lib()
    s0 = slabs_levels[0]
    K, B, N = s0.K, s0.B, s0.N
    nl = len(slabs_levels)
    dev = s0.enc.device
    part = torch.empty(K * int(L.durf_dw_part_floats(W_OBJ_)), device=dev)
    bpart = torch.empty(K * int(L.durf_dw_bpart_floats(W_OBJ_)), device=dev)
    arr = lambda ts: (C.c_void_p * nl)(*[t.data_ptr() for t in ts])
    with _Timed('obj_dw_batch'):
        _lib.check(L.durf_obj_dw_partials(_stream(), K, B, N, _p(count), nl, arr([s.enc for s in slabs_levels]),
                                          arr([view_tile] * nl), arr([s.stash for s in slabs_levels]),
                                          arr([s.dz for s in slabs_levels]), arr([s.dz_out for s in slabs_levels]),
                                          _p(part), _p(bpart)), 'durf_obj_dw_partials')
    return part, bpart


def dw_finalize_all(rows_l, n_l, count_l, part, bpart, grad_bkgd, bkgd_params, obj=None):
    """Finalize the background MLP's weight gradients (segments as in mlp_dw_levels) and, with
    obj = (K, B, N, count, nlevels, part, bpart, grad_obj, grad_stride, obj_params), those of the K object MLPs in the
    same pair of launches (durf_dw_finalize_all)."""
    L, rows_a, n_a, cnt_a = _levels_args(rows_l, n_l, count_l)
    if obj is None:
        oa = (0, 0, 0, None, 1, IN_OBJ_, None, None, None, 0, None)
    else:
        K, B, N, cnt, nl, po, bo, go, gs, pr = obj
        oa = (int(K), int(B), int(N), _p(cnt), int(nl), IN_OBJ_, _p(po), _p(bo), _p(go), int(gs), _p(_f32(pr)))
    with _Timed('mlp_dw_finalize_256'):
        _lib.check(_lib.lib().durf_dw_finalize_all(_stream(), IN_BKGD, L, rows_a, n_a, cnt_a, _p(part), _p(bpart),
                                                   _p(grad_bkgd), _p(_f32(bkgd_params)), *oa), 'durf_dw_finalize_all')


def poison_multi_hit(grad, cls_count, box_floats, K, mlp0_floats, obj_floats, upto=None):
    """reference semantics of rays that hit two boxes (durf_poison_multi_hit): NaN into the gradient segments they touch;
    upto: only the first `upto` floats of the flat buffer are touched"""
    n = grad.numel() if upto is None else int(upto)
    _lib.check(_lib.lib().durf_poison_multi_hit(_stream(), n, _p(_f32(grad)), _p(cls_count), int(box_floats), int(K),
                                                int(mlp0_floats), int(obj_floats)), 'durf_poison_multi_hit')


# Parameter updates go through ctypes data pointers, which torch's tensor version counters do not see.  Whatever caches a
# function of the parameters (MipNerfModel.prefetch_const_trunk) keys it on this generation count instead: every
# in-place update issued from this module bumps the count of the flat buffer it wrote.
_PARAM_GENERATION = {}


def param_generation(params):
    return _PARAM_GENERATION.get((params.data_ptr(), params.numel()), 0)


def _bump_generation(params):
    key = (params.data_ptr(), params.numel())
    _PARAM_GENERATION[key] = _PARAM_GENERATION.get(key, 0) + 1
    if len(_PARAM_GENERATION) > 256:                 # (buffers come and go in tests; the table need not grow with them)
        for k in list(_PARAM_GENERATION)[:128]:
            if k != key:
                del _PARAM_GENERATION[k]


def clip_adam(params, m, v, grad, inv_world, max_val, max_norm, lr, step):
    """In-place Adam step on the flat buffers; returns stats[4] (grad_norm, grad_abs_max,
    clip multiplier, grad_norm_clipped) as a device tensor."""
    _bump_generation(params)
    n = params.numel()
    dev = params.device
    scratch = torch.empty(int(_lib.lib().durf_optim_scratch_floats(n)), device=dev)
    stats = torch.empty(4, device=dev)
    _lib.check(_lib.lib().durf_clip_adam(_stream(), n, _p(_f32(params)), _p(_f32(m)), _p(_f32(v)),
                                         _p(_f32(grad)), inv_world, max_val, max_norm, lr, int(step),
                                         _p(scratch), _p(stats)), 'durf_clip_adam')
    return stats


def encode_obj_bwd(k_obj, idx_k, count_k, d_enc, t_vals, origins_s, dirs_s, radii, origins, dirs, pose, alpha,
                   sums, scratch=None, precise=False, enc_flags=0):
    """accumulates the 21 pose sums of object k (one level) into sums[k] (sums: [K,21], caller-zeroed)"""
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    if scratch is None:
        scratch = torch.empty(21 * B, device=t_vals.device)
    w = barf_weights(alpha)
    wa = (C.c_float * 10)(*[float(x) for x in w])
    _lib.check(_lib.lib().durf_encode_obj_bwd(_stream(), B, N, k_obj, _p(idx_k), _p(count_k), _p(_f32(d_enc)),
                                              _p(_f32(t_vals)), _p(_f32(origins_s)), _p(_f32(dirs_s)),
                                              _p(_f32(radii)), _p(_f32(origins)), _p(_f32(dirs)), _p(_f32(pose)),
                                              wa, _p(scratch), _p(_f32(sums)), int(precise), int(enc_flags)), 'durf_encode_obj_bwd')


def encode_obj_bwd_batch(K, idx, count, d_enc, t_vals, origins_s, dirs_s, radii, origins, dirs, pose, alpha, sums,
                         precise=False, enc_flags=0, scratch=None):
    """all K objects of one level in one launch pair: idx [K,B], count [K], d_enc [K, B*N, 64] (obj_bwd_batch's slab);
    scratch: caller-owned K*21*B floats (the per-ray rows [K][21][B], column j = compact ray index), or None"""
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    if scratch is None:
        scratch = torch.empty(K * 21 * B, device=t_vals.device)
    w = barf_weights(alpha)
    wa = (C.c_float * 10)(*[float(x) for x in w])
    _lib.check(_lib.lib().durf_encode_obj_bwd_batch(_stream(), int(K), B, N, _p(idx), _p(count), _p(_f32(d_enc)),
                                                    _p(_f32(t_vals)), _p(_f32(origins_s)), _p(_f32(dirs_s)),
                                                    _p(_f32(radii)), _p(_f32(origins)), _p(_f32(dirs)), _p(_f32(pose)),
                                                    wa, _p(scratch), _p(_f32(sums)), int(precise), int(enc_flags)),
               'durf_encode_obj_bwd_batch')


def encode_obj_bwd_levels(K, idx, count, d_enc_list, t_vals_list, origins_s, dirs_s, radii, origins, dirs, pose, alpha, sums,
                          scratch=None, precise=False, enc_flags=0):
    """all K objects of every level in one launch pair (durf_encode_obj_bwd_levels: the one-call step's form): one d_enc slab
    [K, B*N, 64] and one t_vals [B, N+1] per level, the same N; the levels' row sums are added into sums [K,21] in the order
    given.  scratch: caller-owned nlev*K*21*B floats (level l's rows [K][21][B] at l*K*21*B), or None"""
    nlev = len(d_enc_list)
    if nlev != len(t_vals_list) or nlev < 1:
        raise ValueError('encode_obj_bwd_levels: %d d_enc slabs for %d t_vals' % (nlev, len(t_vals_list)))
    B, N = t_vals_list[0].shape[0], t_vals_list[0].shape[1] - 1
    if any(tuple(t.shape) != (B, N + 1) for t in t_vals_list):
        raise ValueError('encode_obj_bwd_levels: every level takes the same [B, N+1] t_vals')
    if scratch is None:
        scratch = torch.empty(nlev * K * 21 * B, device=t_vals_list[0].device)
    w = barf_weights(alpha)
    wa = (C.c_float * 10)(*[float(x) for x in w])
    de = (C.c_void_p * nlev)(*[_p(_f32(t)) for t in d_enc_list])
    tv = (C.c_void_p * nlev)(*[_p(_f32(t)) for t in t_vals_list])
    _lib.check(_lib.lib().durf_encode_obj_bwd_levels(_stream(), int(K), B, N, nlev, _p(idx), _p(count), de, tv,
                                                     _p(_f32(origins_s)), _p(_f32(dirs_s)), _p(_f32(radii)), _p(_f32(origins)),
                                                     _p(_f32(dirs)), _p(_f32(pose)), wa, _p(scratch), _p(_f32(sums)),
                                                     int(precise), int(enc_flags)), 'durf_encode_obj_bwd_levels')


def encode_bkgd_bwd_batch(K, idx, count, d_enc, t_vals, origins_s, dirs_s, radii, origins, dirs, pose, sums, raw=None, draw=None,
                          density_bias=-1.0, denc_slot=None, enc_flags=ENC_CONTRACT, scratch=None):
    """dynamics=False: the box-pose rows of all K boxes of one level through the BACKGROUND encoding (durf_encode_bkgd_bwd_batch):
    idx [K,B], count [K] (compact_hits); d_enc [rows,64]: row b*N + n, or denc_slot[b]*N + n (the fp32 evaluation of the box-hit
    rays); raw / draw [B*N,4] add the rendering's |d_s| term.  Accumulates into sums [K,21].  scratch: caller-owned K*21*B
    floats (the per-ray rows), or None."""
    B, N = t_vals.shape[0], t_vals.shape[1] - 1
    if scratch is None:
        scratch = torch.empty(K * 21 * B, device=t_vals.device)
    _lib.check(_lib.lib().durf_encode_bkgd_bwd_batch(_stream(), int(K), B, N, _p(idx), _p(count), _p(_f32(d_enc)), _p(denc_slot),
                                                     _p(_f32(t_vals)), _p(_f32(origins_s)), _p(_f32(dirs_s)), _p(_f32(radii)),
                                                     _p(_f32(origins)), _p(_f32(dirs)), _p(_f32(pose)),
                                                     _p(None if raw is None else _f32(raw)), _p(None if draw is None else _f32(draw)),
                                                     float(density_bias), _p(scratch), _p(_f32(sums)), int(enc_flags)),
               'durf_encode_bkgd_bwd_batch')


def pose_finish(pose, sums, want_pos, want_rot, grad6):
    K = pose.shape[0]
    _lib.check(_lib.lib().durf_pose_finish(_stream(), K, _p(_f32(pose)), _p(_f32(sums)), int(want_pos),
                                           int(want_rot), _p(_f32(grad6))), 'durf_pose_finish')


# ---------------------------------------------------------------------------
# exact-fp32 MLP (csrc/mlp_f32.hip): the object branch of a step with box-pose optimisation (MipNerfModel.object_precision)
# and the parity instrument behind MipNerfModel(mlp_precision='f32')
# ---------------------------------------------------------------------------
def mlp_f32_pack(width, in_dim, mlp_params, K=1, param_stride=0, x3=False):
    """fp32 weight streams of K MLPs (durf_mlp_f32_pack): the wide Dense kernels as the chunks the fp32 forward / the
    backward (transposed) consume, in order; re-packed whenever the parameters change.  x3 (W = 128): every weight as a
    (hi, lo) bf16 pair, for the 'bf16x3' object kernels (durf_mlp_f32_pack_x3)"""
    L = _lib.lib()
    out = torch.empty(int(K) * int(L.durf_mlp_f32_wstream_floats(width)), device=mlp_params.device)
    if x3:
        assert width == W_OBJ_ and in_dim == IN_OBJ_
        _lib.check(L.durf_mlp_f32_pack_x3(_stream(), int(K), _p(_f32(mlp_params)), int(param_stride), _p(out)), 'durf_mlp_f32_pack_x3')
        return out
    _lib.check(L.durf_mlp_f32_pack(_stream(), width, in_dim, int(K), _p(_f32(mlp_params)), int(param_stride), _p(out)),
               'durf_mlp_f32_pack')
    return out


def mlp_fwd_f32(width, in_dim, rows, N, enc_f32, view27, mlp_params, ray_idx=None, count=None, want_act=False,
                wstream=None, raw=None, act=None):
    """-> raw [rows,4][, act (opaque record buffer for mlp_bwd_f32 / mlp_dw_f32)].  enc_f32 [rows,in_dim] row-major, or
    None: every row is the background MLP's constant encoding of a box-hit ray (width 256); view27 [B,27]
    raw / act: caller-owned output buffers (at least [rows,4] / tile_rows(rows) records; act implies want_act)"""
    dev = view27.device
    L = _lib.lib()
    if wstream is None:
        wstream = mlp_f32_pack(width, in_dim, mlp_params)
    want_act = want_act or act is not None
    nact = tile_rows(rows) * int(L.durf_mlp_f32_act_floats(width, in_dim))
    if raw is None:
        raw = torch.zeros(rows, 4, device=dev)
    assert _f32(raw).numel() >= rows * 4
    if want_act and act is None:
        act = torch.empty(nact, device=dev)
    assert act is None or _f32(act).numel() >= nact
    with _Timed('mlp_fwd_f32_%d' % width):
        _lib.check(L.durf_mlp_fwd_f32(_stream(), width, in_dim, rows, N, _p(None if enc_f32 is None else _f32(enc_f32)),
                                      _p(_f32(view27)), _p(ray_idx), _p(count), _p(_f32(mlp_params)), _p(wstream), _p(raw),
                                      _p(act)), 'durf_mlp_fwd_f32')
    return (raw, act) if want_act else raw


def mlp_bwd_f32(width, in_dim, rows, N, draw, mlp_params, act, ray_idx=None, count=None, want_d_enc=False, wstream=None,
                dz=None, d_enc=None):
    """-> dz (opaque record buffer)[, d_enc [rows,64]]
    dz / d_enc: caller-owned output buffers (at least tile_rows(rows) records / [rows,64]; d_enc implies want_d_enc)"""
    dev = draw.device
    L = _lib.lib()
    if wstream is None:
        wstream = mlp_f32_pack(width, in_dim, mlp_params)
    want_d_enc = want_d_enc or d_enc is not None
    ndz = tile_rows(rows) * int(L.durf_mlp_f32_dz_floats(width, in_dim))
    if dz is None:
        dz = torch.empty(ndz, device=dev)
    assert _f32(dz).numel() >= ndz
    if want_d_enc and d_enc is None:
        d_enc = torch.zeros(rows, ENC_DIM, device=dev)
    assert d_enc is None or _f32(d_enc).numel() >= rows * ENC_DIM
    with _Timed('mlp_bwd_f32_%d' % width):
        _lib.check(L.durf_mlp_bwd_f32(_stream(), width, in_dim, rows, N, _p(_f32(draw)), _p(ray_idx), _p(count),
                                      _p(_f32(mlp_params)), _p(wstream), _p(_f32(act)), _p(dz), _p(d_enc)),
                   'durf_mlp_bwd_f32')
    return (dz, d_enc) if want_d_enc else dz


def mlp_dw_f32(width, in_dim, rows, N, act, dz, grad_mlp, count=None, nsplit=32):
    """weight gradients of one MLP over `rows` samples, ADDED to grad_mlp (flax layout)"""
    dev = act.device
    L = _lib.lib()
    scratch = torch.empty(int(L.durf_mlp_f32_dw_scratch_floats(width, in_dim, nsplit)), device=dev)
    g = torch.empty_like(grad_mlp)
    with _Timed('mlp_dw_f32_%d' % width):
        _lib.check(L.durf_mlp_dw_f32(_stream(), width, in_dim, rows, N, _p(count), _p(_f32(act)), _p(_f32(dz)), nsplit,
                                     _p(scratch), _p(g)), 'durf_mlp_dw_f32')
    grad_mlp += g


def bkgd_const_trunk_f32(bkgd_params):
    """Dense_0 .. Dense_9 of the background MLP on the constant encoding every box-hit ray feeds it ([0 x 30, 1 x 30]), in
    fp32 -> trunk [257] (bottleneck, density): depends on the parameters only, once per step"""
    trunk = torch.empty(257, device=bkgd_params.device)
    _lib.check(_lib.lib().durf_bkgd_const_trunk_f32(_stream(), _p(_f32(bkgd_params)), _p(trunk)), 'durf_bkgd_const_trunk_f32')
    return trunk


def bkgd_hit_rays_f32(B, view27, bkgd_params, idx1, count1, trunk=None, raw_tail=None):
    """the background MLP's one evaluation of every box-hit ray (ray class 1: idx1 / count1), in fp32 -> raw_tail [B,4]
    (row j = ray idx1[j]): the view layer and the rgb head per ray on top of bkgd_const_trunk_f32's output
    raw_tail: a caller-owned [B,4] buffer; rows from count1 on are not written"""
    dev = view27.device
    if trunk is None:
        trunk = bkgd_const_trunk_f32(bkgd_params)
    if raw_tail is None:
        raw_tail = torch.empty(B, 4, device=dev)
    assert _f32(raw_tail).numel() >= B * 4
    with _Timed('bkgd_hit_rays_f32'):
        _lib.check(_lib.lib().durf_bkgd_hit_rays_f32(_stream(), B, _p(_f32(view27)), _p(_f32(bkgd_params)), _p(idx1),
                                                     _p(count1), _p(trunk), _p(raw_tail)), 'durf_bkgd_hit_rays_f32')
    return raw_tail


class ObjSlabsF32:
    """[K, ...] slabs of one level for the batched fp32 object calls (durf_objf32_*; strides fixed by the library)"""

    def __init__(self, K, B, N, device, train, raw=None, act=None):
        """raw [K, B * N, 4] / act (K * durf_objf32_act_stride floats): caller-owned slabs instead of fresh ones (act may
        be longer)"""
        L = _lib.lib()
        self.K, self.B, self.N = K, B, N
        self.enc = None                       # only filled by objf32_fwd_batch(fused_encode=False)
        nact = K * int(L.durf_objf32_act_stride(B, N))
        self.raw = torch.empty(K, B * N, 4, device=device) if raw is None else raw
        assert _f32(self.raw).shape == (K, B * N, 4)
        self.act = act if act is not None else (torch.empty(nact, device=device) if train else None)
        assert self.act is None or _f32(self.act).numel() >= nact
        self.dz = self.d_enc = None

    def raws(self):
        return [self.raw[k] for k in range(self.K)]


def objf32_fwd_batch(slabs, idx, count, t_vals, origins_s, dirs_s, radii, alpha, view27, obj_params, param_stride, wstream,
                     disable_integration=False, cylinder=False, fused_encode=True, x3=False):
    """accurate fp32 encodings + fp32 forward of all K object MLPs of one level: ONE launch (the forward encodes its own
    tiles); fused_encode=False: durf_encode_obj_f32_batch into slabs.enc first, then the forward reads it (bit-identical)"""
    w = barf_weights(alpha)
    wa = (C.c_float * 10)(*[float(x) for x in w])
    L = _lib.lib()
    flags = (ENC_NO_INTEGRATION if disable_integration else 0) | (ENC_CYLINDER if cylinder else 0) | (F32_X3 if x3 else 0)
    assert fused_encode or not x3
    with _Timed('objf32_fwd_batch'):
        if not fused_encode:
            slabs.enc = torch.empty(slabs.K, slabs.B * slabs.N, IN_OBJ_, device=t_vals.device)
            _lib.check(L.durf_encode_obj_f32_batch(
                _stream(), slabs.K, slabs.B, slabs.N, _p(idx), _p(count), _p(_f32(t_vals)), _p(_f32(origins_s)),
                _p(_f32(dirs_s)), _p(_f32(radii)), wa, flags & ~F32_X3, _p(slabs.enc)), 'durf_encode_obj_f32_batch')
        _lib.check(L.durf_objf32_fwd_batch(_stream(), slabs.K, slabs.B, slabs.N, _p(idx), _p(count),
                                           _p(None if fused_encode else slabs.enc), _p(_f32(view27)), _p(_f32(obj_params)),
                                           int(param_stride), _p(wstream), _p(slabs.raw), _p(slabs.act), _p(_f32(t_vals)),
                                           _p(_f32(origins_s)), _p(_f32(dirs_s)), _p(_f32(radii)), wa, flags),
                   'durf_objf32_fwd_batch')


def objf32_bwd_batch(slabs, idx, count, draw, obj_params, param_stride, wstream, want_d_enc=False, x3=False, dz=None,
                     d_enc=None):
    """dz (K * durf_objf32_dz_stride floats) / d_enc [K, B * N, 64]: caller-owned slabs instead of fresh ones (d_enc implies
    want_d_enc)"""
    L = _lib.lib()
    dev = draw.device
    K, B, N = slabs.K, slabs.B, slabs.N
    ndz = K * int(L.durf_objf32_dz_stride(B, N))
    slabs.dz = torch.empty(ndz, device=dev) if dz is None else dz
    assert _f32(slabs.dz).numel() >= ndz
    if d_enc is not None:
        assert _f32(d_enc).shape == (K, B * N, ENC_DIM)
        slabs.d_enc = d_enc
    else:
        slabs.d_enc = torch.empty(K, B * N, ENC_DIM, device=dev) if want_d_enc else None     # every valid row is written
    with _Timed('objf32_bwd_batch'):
        fn = L.durf_objf32_bwd_batch_x3 if x3 else L.durf_objf32_bwd_batch
        _lib.check(fn(_stream(), K, B, N, _p(idx), _p(count), _p(_f32(draw)), _p(_f32(obj_params)), int(param_stride), _p(wstream),
                      _p(slabs.act), _p(slabs.dz), _p(slabs.d_enc)), 'durf_objf32_bwd_batch')


def objf32_dw_batch(slabs_levels, count, grad_obj, grad_stride, nsplit=8):
    """weight gradients of all K object MLPs over every level -> grad_obj (flat, K x grad_stride floats), overwritten"""
    L = _lib.lib()
    s0 = slabs_levels[0]
    K, B, N = s0.K, s0.B, s0.N
    nl = len(slabs_levels)
    scratch = torch.empty(K * int(L.durf_mlp_f32_dw_scratch_floats(W_OBJ_, IN_OBJ_, nsplit)), device=grad_obj.device)
    arr = lambda ts: (C.c_void_p * nl)(*[t.data_ptr() for t in ts])
    with _Timed('objf32_dw_batch'):
        _lib.check(L.durf_objf32_dw_batch(_stream(), K, B, N, _p(count), nl, arr([s.act for s in slabs_levels]),
                                          arr([s.dz for s in slabs_levels]), int(nsplit), _p(scratch), _p(grad_obj),
                                          int(grad_stride)), 'durf_objf32_dw_batch')


# ---------------------------------------------------------------------------------------------------------------------
# the whole inference forward as one C call (csrc/forward.hip, include/durf_hip.h durf_forward)
# ---------------------------------------------------------------------------------------------------------------------
ForwardArgs, TrainArgs, StepTiming = _H.durf_forward_args, _H.durf_train_args, _H.durf_step_timing
_vp4 = C.c_void_p * FORWARD_MAX_LEVELS


def _step_timing(num_levels, keep):
    """the live timers of a one-call step (bench.py's roofline): HIP events the C call records around the launches the
    Python-issued path brackets with _Timed -- the same names in TIMERS.  None unless timers are armed for this step."""
    if TIMERS is None or not TIMERS_ACTIVE:
        return None
    want = lambda name: TIMED_NAMES is None or name in TIMED_NAMES
    slots = []
    if want('mlp_fwd_256_train'):
        slots += [('mlp_fwd_256_train', TIMED_FWD + l) for l in range(num_levels)]
    if want('mlp_bwd_256'):
        slots += [('mlp_bwd_256', TIMED_BWD + l) for l in range(num_levels)]
    if want('composite_resample'):
        slots += [('composite_resample', TIMED_COMPOSITE + l) for l in range(num_levels - 1)]
    if want('mlp_dw_256'):
        slots += [('mlp_dw_256', TIMED_DW)]
    if not slots:
        return None
    tm = StepTiming()
    for name, i in slots:
        pair = (_timing_event(), _timing_event())
        tm.begin[i], tm.end[i] = pair[0].cuda_event, pair[1].cuda_event
        TIMERS.setdefault(name, []).append(pair)
    keep.append(tm)
    return tm


def _fill_model_args(a, K, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags, lindisp, bkgd_mode,
                     density_bias, resample_padding):
    """the fields of durf_forward_args that say which model renders, whatever the rays"""
    a.N, a.K, a.num_levels, a.enc_flags, a.lindisp, a.bkgd_mode = N, K, num_levels, enc_flags, int(lindisp), bkgd_mode
    a.density_bias, a.resample_padding = density_bias, resample_padding
    a.barf_w = (C.c_float * 10)(*[float(x) for x in barf_weights(alpha)])
    a.bkgd_params = _p(_f32(bkgd_params))
    a.obj_params, a.obj_param_stride = (_p(_f32(obj_params)) if K else None), int(obj_param_stride)


def _fill_ray_args(a, rays, pose, ext, t_rand=None, u_rand=None, seed=None, density_noise=0.0, density_rand=None, outputs=True):
    """behind _fill_model_args: the rays, the boxes, the draws and freshly allocated output buffers of one call -> the per-level
    outputs, dyn_mask, zo (None with outputs=False: an image call keeps them in its workspace), the tensors made on the way"""
    a.B = B = rays.origins.shape[0]
    N, K, num_levels = a.N, a.K, a.num_levels
    keep = flat = [t.reshape(-1).contiguous() for t in (rays.radii, rays.near, rays.far)]
    a.origins, a.directions, a.viewdirs = _p(_f32(rays.origins)), _p(_f32(rays.directions)), _p(_f32(rays.viewdirs))
    a.radii, a.near, a.far = (_p(_f32(t)) for t in flat)
    a.pose, a.ext = (_p(_f32(pose)) if K else None), (_p(_f32(ext)) if K else None)
    a.t_rand, a.u_rand = _p(t_rand), _p(u_rand)
    a.draw_noise = int(seed is not None)
    a.seed_lo, a.seed_hi = (0, 0) if seed is None else split_seed(seed)
    a.density_noise = float(density_noise)
    if density_noise and density_rand is not None:          # the caller's standard-normal draws, [B,N] per level
        dr = [_f32(t.reshape(-1).contiguous()) for t in density_rand]
        assert len(dr) == num_levels and all(t.numel() == B * N for t in dr)
        keep.extend(dr)
        a.density_rand = _vp4(*([t.data_ptr() for t in dr] + [None] * (FORWARD_MAX_LEVELS - num_levels)))
    outs = dyn = zo = None
    if outputs:
        f = lambda *sh: torch.empty(*sh, device=rays.origins.device)
        outs = [(f(B, 3), f(B), f(B), f(B, N), f(B, N + 1), f(B, N), f(B, N)) for _ in range(num_levels)]
        dyn, zo = torch.empty(B, 1, dtype=torch.int32, device=rays.origins.device), f(B)
        for i, name in enumerate(('rgb', 'depth', 'acc', 'weights', 't_vals', 't_mids', 't_dists')):
            setattr(a, name, _vp4(*([o[i].data_ptr() for o in outs] + [None] * (FORWARD_MAX_LEVELS - num_levels))))
    a.dyn_mask, a.zo = _p(dyn), _p(zo)
    return outs, dyn, zo, keep


def _image_args(rays, chunk, pose, ext, *model):
    """a whole-image call's durf_forward_args over contiguous [n, .] ray fields (C slices them by pointer) -> a, what it points at, the chunk"""
    a = ForwardArgs()
    rays = type(rays)(*[t.contiguous() for t in rays])
    _fill_model_args(a, pose.shape[0], *model)
    keep = _fill_ray_args(a, rays, pose, ext, outputs=False)[3] + [rays]
    a.B = ck = min(chunk, rays.origins.shape[0])
    return a, keep, ck


def forward_call(rays, pose, ext, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags, lindisp=False,
                 bkgd_mode=BKGD_GREY, density_bias=-1.0, resample_padding=0.01, t_rand=None, u_rand=None, seed=None,
                 density_noise=0.0, density_rand=None, box_enable=None):
    """MipNerfModel.__call__ in inference as ONE library call (durf_forward; box_enable int32 [K]: durf_forward_masked): -> list[num_levels] of
    (rgb, depth, acc, weights, t_vals, t_mids, t_dists), dyn_mask [B,1] int32, zo [B]"""
    B, K = rays.origins.shape[0], pose.shape[0]
    dev = rays.origins.device
    L = _lib.lib()
    a = ForwardArgs()
    _fill_model_args(a, K, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags, lindisp, bkgd_mode,
                     density_bias, resample_padding)
    outs, dyn, zo, keep = _fill_ray_args(a, rays, pose, ext, t_rand, u_rand, seed, density_noise, density_rand)
    ws = _workspace(dev, int(L.durf_forward_workspace_bytes(B, N, K)))
    with _Timed('forward_call'):
        if box_enable is not None:
            _lib.check(L.durf_forward_masked(_stream(), C.byref(a), _p(box_enable), _p(ws), ws.numel()), 'durf_forward_masked')
        else:
            _lib.check(L.durf_forward(_stream(), C.byref(a), _p(ws), ws.numel()), 'durf_forward')
    return outs, dyn, zo


def render_image_call(rays, pose, ext, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags, chunk,
                      lindisp=False, bkgd_mode=BKGD_GREY, density_bias=-1.0, resample_padding=0.01):
    """render_image on one device as ONE library call (durf_render_image: the chunk loop in C over the ray buffer resident on
    the device) -> rgb [n,3], distance [n], acc [n] of the last level; rays: flattened [n, .] fields of the whole image"""
    n, K = rays.origins.shape[0], pose.shape[0]
    dev = rays.origins.device
    L = _lib.lib()
    rgb, dist_, acc = torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
    a, keep, ck = _image_args(rays, chunk, pose, ext, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags,
                              lindisp, bkgd_mode, density_bias, resample_padding)
    ws = _workspace(dev, int(L.durf_render_image_workspace_bytes(ck, N, K, num_levels)))
    with _Timed('render_image_call'):
        _lib.check(L.durf_render_image(_stream(), C.byref(a), n, ck, _p(rgb), _p(dist_), _p(acc), _p(ws), ws.numel()),
                   'durf_render_image')
    return rgb, dist_, acc


LAYER_NAMES = ('instance', 'background', 'objects')


def render_layers_call(rays, pose, ext, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags, chunk,
                       lindisp=False, bkgd_mode=BKGD_GREY, density_bias=-1.0, resample_padding=0.01, box_enable=None,
                       layers=LAYER_NAMES):
    """render_image_call plus the scene layers of the image, ONE library call (durf_render_layers) -> dict: rgb [n,3],
    distance [n], acc [n]; 'instance' in layers: instance [n] int32; 'background': bg_rgb / bg_distance / bg_acc;
    'objects': obj_rgba [n,4].  box_enable: int32 [K] on the device or None.  A layer that is not asked for costs nothing."""
    n, K = rays.origins.shape[0], pose.shape[0]
    dev = rays.origins.device
    L = _lib.lib()
    f = lambda *sh: torch.empty(*sh, device=dev)
    out = dict(rgb=f(n, 3), distance=f(n), acc=f(n))
    if 'instance' in layers:
        out['instance'] = torch.empty(n, dtype=torch.int32, device=dev)
    if 'background' in layers:
        out.update(bg_rgb=f(n, 3), bg_distance=f(n), bg_acc=f(n))
    if 'objects' in layers:
        out['obj_rgba'] = f(n, 4)
    a, keep, ck = _image_args(rays, chunk, pose, ext, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags,
                              lindisp, bkgd_mode, density_bias, resample_padding)
    ws = _workspace(dev, int(L.durf_render_layers_workspace_bytes(n, ck, N, K, num_levels)))
    with _Timed('render_layers_call'):
        _lib.check(L.durf_render_layers(_stream(), C.byref(a), _p(box_enable), n, ck, _p(out['rgb']), _p(out['distance']),
                                        _p(out['acc']), _p(out.get('instance')), _p(out.get('bg_rgb')), _p(out.get('bg_distance')),
                                        _p(out.get('bg_acc')), _p(out.get('obj_rgba')), _p(ws), ws.numel()), 'durf_render_layers')
    return out


TRAJECTORY_OUTPUTS = ('rgb8', 'rgb', 'distance', 'acc')


def render_trajectory(cams, times, box_centers, ext, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags,
                      chunk, near, far, lindisp=False, bkgd_mode=BKGD_GREY, density_bias=-1.0, resample_padding=0.01,
                      box_enable=None, outputs=('rgb8', 'distance', 'acc'), out=None):
    """A camera trajectory as ONE library call (durf_render_trajectory): cams [F,CAM_FLOATS] host rows (camera.rows, one
    image size), times [F] host floats in [0, T - 1], box_centers [T,K,6] on the device (read there: no host copy) -> dict:
    the requested `outputs` of rgb8 [F,n,3] uint8, rgb [F,n,3], distance [F,n], acc [F,n], and poses [F,K,6], the box poses
    every frame was rendered with.  outputs = (): poses only, nothing is rendered (cams may be None).  out: dict of
    preallocated contiguous tensors to write into.  The call only enqueues work."""
    import numpy as np
    outputs = tuple(outputs)
    unknown = [o for o in outputs if o not in TRAJECTORY_OUTPUTS]
    if unknown:
        raise ValueError('unknown outputs %s: choose from %s' % (unknown, list(TRAJECTORY_OUTPUTS)))
    times = np.ascontiguousarray(np.asarray(times, np.float32).reshape(-1))
    F = int(times.shape[0])
    T, K = int(box_centers.shape[0]), int(box_centers.shape[1])
    dev = box_centers.device
    L = _lib.lib()
    n = 0
    cam_arr = None
    if outputs:
        cams, h, w = camera.as_rows(cams, 'render_trajectory', one_size=False)
        if cams.shape[0] != F:
            raise ValueError('%d camera rows for %d frame times' % (cams.shape[0], F))
        n = h * w
        cam_arr = (C.c_float * cams.size)(*cams.reshape(-1).tolist())
    shapes = dict(rgb8=((F, n, 3), torch.uint8), rgb=((F, n, 3), torch.float32), distance=((F, n), torch.float32),
                  acc=((F, n), torch.float32), poses=((F, K, 6), torch.float32))
    res = {}
    for name in outputs + ('poses',):
        shape, dtype = shapes[name]
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda and t.is_contiguous(), (name, tuple(t.shape), t.dtype)
        res[name] = t
    a = ForwardArgs()
    _fill_model_args(a, K, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags, lindisp, bkgd_mode,
                     density_bias, resample_padding)
    a.B = ck = min(chunk, max(n, 1))
    a.ext = _p(_f32(ext)) if (K and ext is not None) else None      # (poses only: nothing is rendered)
    ws = _workspace(dev, int(L.durf_render_trajectory_workspace_bytes(F, ck, N, K, num_levels)))
    with _Timed('render_trajectory'):
        _lib.check(L.durf_render_trajectory(_stream(), C.byref(a), _p(box_enable), _p(_f32(box_centers)) if K else None, T, F, cam_arr,
                                            (C.c_float * max(F, 1))(*times.tolist()), float(near), float(far), ck, _p(res.get('rgb8')),
                                            _p(res.get('rgb')), _p(res.get('distance')), _p(res.get('acc')), _p(res['poses']),
                                            _p(ws), ws.numel()), 'durf_render_trajectory')
    return res


_WORKSPACE = {}


def _workspace(dev, nbytes):
    """the one-call entry points' workspace: ONE buffer per device, kept across calls and grown when a call needs more (a
    fresh torch.empty of several hundred MB per step leaves it to the caching allocator to hand the same block back; when it
    does not, the step stalls on a device allocation -- seen as one 0.5 ms step in ~8 passes of a 0.4 ms workload)"""
    # (per device AND per stream: two one-call entry points issued on different streams of one device -- an eval render beside
    # training, a second model -- must not share intermediates; calls on one stream are ordered and may)
    key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream if dev.type == 'cuda' else 0)
    ws = _WORKSPACE.get(key)
    if ws is None or ws.numel() < nbytes:
        _WORKSPACE[key] = ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert ws.data_ptr() % 256 == 0
    return ws


def release_workspace():
    """drop the cached workspaces of the one-call entry points (a large render chunk otherwise pins its buffer -- hundreds
    of MB -- for the life of the process); the next call allocates afresh"""
    _WORKSPACE.clear()


def train_call(rays, pose, ext, params_flat, m, v, box_floats, mlp0_floats, obj_floats, N, num_levels, alpha, enc_flags,
               lossmult, pixels, gt_depth, sky, target6, prev6, eps, box_loss_mult, bg, disable_multiscale, level_mults,
               stat_mults, lr, max_val, max_norm, step, lindisp=False, bkgd_mode=BKGD_GREY, density_bias=-1.0,
               resample_padding=0.01, t_rand=None, u_rand=None, update=True, obj_fp32=False, obj_x3=False, want_pos=False, want_rot=False,
               tv_loss_mult=0.0, seed=None, comm=None, world=1, reduce_stats=False, density_noise=0.0, density_rand=None,
               weight_decay_mult=0.0, const_trunk=None, const_trunk_valid=False):
    """One shard's training step as ONE library call (durf_train_step; update=False: durf_loss_backward, parameters
    untouched) -> (per-level outputs, dyn_mask, zo, grad, stats buffer, grad_stats or None, pose_used [K,6] or None -- the
    poses the step rendered with -- and the class counts [8] int32 or None: [3] = rays that hit two boxes).
    obj_fp32: the object branch on the exact-fp32 kernels; want_pos / want_rot: box-pose optimisation behind it (`pose` must
    then be a view of this timestep's rows of box_centers inside params_flat).  const_trunk [264] (obj_fp32): the caller-kept
    constant trunk -- used when const_trunk_valid (the caller vouches for the parameters), refilled for the NEXT step behind the
    update (durf_train_args.prefetch_const_trunk)"""
    if update:
        _bump_generation(params_flat)
    B, K = rays.origins.shape[0], pose.shape[0]
    dev = rays.origins.device
    L = _lib.lib()
    grad, stats, gstats = torch.empty_like(params_flat), torch.empty(2 + 17 * num_levels, device=dev), torch.empty(4, device=dev)
    a = TrainArgs()
    o0 = box_floats + mlp0_floats
    _fill_model_args(a.f, K, params_flat[box_floats:o0], params_flat[o0:] if K else None, obj_floats, N, num_levels, alpha, enc_flags,
                     lindisp, bkgd_mode, density_bias, resample_padding)
    outs, dyn, zo, keep = _fill_ray_args(a.f, rays, pose, ext, t_rand, u_rand, seed, density_noise, density_rand)
    a.weight_decay_mult = float(weight_decay_mult)
    hold = [t.reshape(-1).contiguous() for t in (lossmult, gt_depth, sky)] + [pixels.contiguous()]
    a.lossmult, a.gt_depth, a.sky, a.pixels = (_p(_f32(t)) for t in hold)
    hold += [target6.contiguous(), prev6.contiguous()] if K else []
    a.target6, a.prev6 = (_p(_f32(hold[-2])), _p(_f32(hold[-1]))) if K else (None, None)
    a.eps, a.box_loss_mult, a.bg, a.disable_multiscale = float(eps), float(box_loss_mult), float(bg), int(disable_multiscale)
    for lvl in range(num_levels):
        for i in range(6):
            a.level_mults[lvl][i] = float(level_mults[lvl][i])
    a.stat_mults = (C.c_float * 6)(*[float(x) for x in stat_mults])
    a.params, a.n_params = _p(_f32(params_flat)), params_flat.numel()
    a.box_floats, a.mlp0_floats, a.obj_floats = int(box_floats), int(mlp0_floats), int(obj_floats)
    a.grad, a.stats, a.grad_stats = _p(grad), _p(stats), _p(gstats)
    a.adam_m, a.adam_v = _p(_f32(m)), _p(_f32(v))
    a.lr, a.max_val, a.max_norm, a.step = float(lr), float(max_val), float(max_norm), int(step)
    pose_opt = bool(K) and (want_pos or want_rot)
    if pose_opt and not obj_fp32:
        raise NotImplementedError('durf_train_step: DURF_TRAIN_POSE_OPT needs DURF_TRAIN_OBJ_FP32 (csrc/train.hip)')
    a.flags = ((TRAIN_OBJ_FP32 if (K and obj_fp32) else 0) | (TRAIN_POSE_OPT if pose_opt else 0) |
               (TRAIN_OBJ_X3 if (K and obj_fp32 and obj_x3) else 0))
    a.want_pos, a.want_rot, a.tv_loss_mult = int(bool(want_pos)), int(bool(want_rot)), float(tv_loss_mult)
    a.comm, a.world, a.reduce_stats = (comm.handle if comm is not None else None), int(world), int(bool(reduce_stats))
    pose_used = torch.empty_like(pose) if K else None
    cls = torch.empty(8, dtype=torch.int32, device=dev) if K else None
    a.pose_used, a.cls_count = _p(pose_used), _p(cls)
    if const_trunk is not None and K and obj_fp32:
        assert const_trunk.numel() >= 264 and const_trunk.is_contiguous()
        a.const_trunk, a.const_trunk_valid, a.prefetch_const_trunk = _p(_f32(const_trunk)), int(bool(const_trunk_valid)), int(bool(update))
    tm = _step_timing(num_levels, keep) if update else None
    a.timing = C.cast(C.pointer(tm), C.c_void_p) if tm is not None else None
    ws = _workspace(dev, int(L.durf_train_workspace_bytes_flags(B, N, K, num_levels, params_flat.numel(), a.flags)))
    with _Timed('train_call'):
        fn = L.durf_train_step if update else L.durf_loss_backward
        _lib.check(fn(_stream(), C.byref(a), _p(ws), ws.numel()), 'durf_train_step' if update else 'durf_loss_backward')
    return outs, dyn, zo, grad, stats, (gstats if update else None), pose_used, cls


# ---- depth visualisations (csrc/vis.hip; include/durf_hip.h durf_vis_*) -----------------------------------------------------
VIS_CURVES = {k.lower(): v for k, v in _by_prefix(_H, 'DURF_VIS_CURVE_').items()}
VIS_STATS_FIELDS = ('near_auto', 'far_auto', 'normal_scale', 'count', 'var_x', 'var_y', 'var_depth', 'mean_depth')
assert len(VIS_STATS_FIELDS) == VIS_STATS_FLOATS


def _vis_outputs(shape, dev, want_float, want_u8, rgb, rgb8):
    if not (want_float or want_u8):
        raise ValueError('at least one of the float and the 8-bit output')
    if want_float and rgb is None:
        rgb = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
    if want_u8 and rgb8 is None:
        rgb8 = torch.empty(shape + (3,), dtype=torch.uint8, device=dev)
    for t, dt in ((rgb, torch.float32), (rgb8, torch.uint8)):
        assert t is None or (t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape + (3,)), (t.dtype, t.shape)
    return (rgb if want_float else None), (rgb8 if want_u8 else None)


def vis_stats(depth):
    """depth [F,H,W] -> [F, VIS_STATS_FLOATS] device record (VIS_STATS_FIELDS): durf_vis_stats, three launches, no read-back"""
    F, H, W = depth.shape
    L = _lib.lib()
    stats = torch.empty(F, VIS_STATS_FLOATS, device=depth.device)
    nbytes = int(L.durf_vis_scratch_bytes(F, H, W))
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=depth.device)
    with _Timed('vis_stats'):
        _lib.check(L.durf_vis_stats(_stream(), F, H, W, _p(_f32(depth)), _p(stats), _p(scratch), nbytes), 'durf_vis_stats')
    return stats


def vis_depth(depth, acc, rng, curve='neglog', modulus=0.0, lut=None, want_float=True, want_u8=False, rgb=None, rgb8=None):
    """durf_vis_depth: depth [F,H,W], acc [F,H,W] or None, rng [F, >= 2] (near, far in its first two columns; None with
    modulus > 0), lut None (turbo) or [256,3] -> (rgb [F,H,W,3] or None, rgb8 uint8 or None)"""
    F, H, W = depth.shape
    if curve not in VIS_CURVES:
        raise ValueError('curve_fn %r: choose from %s' % (curve, sorted(VIS_CURVES)))
    if lut is not None and (tuple(lut.shape) != (256, 3)):
        raise ValueError('colormap: a [256,3] tensor, got %s' % (tuple(lut.shape),))
    if acc is not None and acc.shape != depth.shape:
        raise ValueError('acc %s against depth %s' % (tuple(acc.shape), tuple(depth.shape)))
    if rng is not None:
        assert rng.dim() == 2 and rng.shape[0] == F and rng.shape[1] >= 2 and rng.stride(1) == 1, (rng.shape, rng.stride())
    rgb, rgb8 = _vis_outputs((F, H, W), depth.device, want_float, want_u8, rgb, rgb8)
    with _Timed('vis_depth'):
        _lib.check(_lib.lib().durf_vis_depth(_stream(), F, H, W, _p(_f32(depth)), _p(None if acc is None else _f32(acc)),
                                             _p(rng), 0 if rng is None else rng.stride(0), VIS_CURVES[curve], float(modulus),
                                             _p(None if lut is None else _f32(lut)), _p(rgb), _p(rgb8)), 'durf_vis_depth')
    return rgb, rgb8


def vis_normals(depth, acc, scale, raw=False, want_float=True, want_u8=False, rgb=None, rgb8=None):
    """durf_vis_normals: scale a float32 device tensor read at stride scale.stride(0) (one value per frame; None: 1);
    raw: the normals themselves (depth_to_normals)"""
    F, H, W = depth.shape
    if acc is not None and acc.shape != depth.shape:
        raise ValueError('acc %s against depth %s' % (tuple(acc.shape), tuple(depth.shape)))
    if scale is not None:
        assert scale.dtype == torch.float32 and scale.is_cuda and scale.shape[0] == F, (scale.dtype, scale.shape)
    rgb, rgb8 = _vis_outputs((F, H, W), depth.device, want_float, want_u8, rgb, rgb8)
    stride = 1 if scale is None else max(int(scale.stride(0)), 1)
    with _Timed('vis_normals'):
        _lib.check(_lib.lib().durf_vis_normals(_stream(), F, H, W, _p(_f32(depth)), _p(None if acc is None else _f32(acc)),
                                               _p(scale), stride, VIS_NORMALS_RAW if raw else 0, _p(rgb), _p(rgb8)),
                   'durf_vis_normals')
    return rgb, rgb8


def vis_sinebow(h, want_float=True, want_u8=False):
    rgb, rgb8 = _vis_outputs(tuple(h.shape), h.device, want_float, want_u8, None, None)
    _lib.check(_lib.lib().durf_vis_sinebow(_stream(), h.numel(), _p(_f32(h)), _p(rgb), _p(rgb8)), 'durf_vis_sinebow')
    return rgb, rgb8


def vis_turbo_lut():
    """the library's built-in colour map (matplotlib's turbo) -> [256,3] float32 numpy array; touches no device"""
    import numpy as np
    buf = (C.c_float * 768)()
    _lib.check(_lib.lib().durf_vis_turbo_lut(C.cast(buf, C.c_void_p)), 'durf_vis_turbo_lut')
    return np.ctypeslib.as_array(buf).reshape(256, 3).copy()


# ---- evaluation metrics of F frames (csrc/metrics.hip; include/durf_hip.h durf_eval_frames) --------------------------------
EVAL_INDEX = {k.lower(): v for k, v in _by_prefix(_H, 'DURF_EVAL_').items() if k != 'FLOATS'}      # mse: 0, psnr: 1, ...
EVAL_FIELDS = tuple(sorted(EVAL_INDEX, key=EVAL_INDEX.get))
assert [EVAL_INDEX[name] for name in EVAL_FIELDS] == list(range(EVAL_FLOATS))


def eval_frames(rgb, gt_rgb, distance=None, gt_depth=None, obj_mask=None):
    """rgb, gt_rgb [F,H,W,3]; distance with gt_depth [F,H,W] or neither; obj_mask [F,H,W] or None -> ([F, EVAL_FLOATS] device
    record, EVAL_FIELDS): durf_eval_frames, two launches for any F, no read-back (the fields of a plane that is None are NaN,
    its count 0)"""
    if rgb.dim() != 4 or rgb.shape[-1] != 3 or gt_rgb.shape != rgb.shape:
        raise ValueError('rgb and gt_rgb: [F,H,W,3], got %s and %s' % (tuple(rgb.shape), tuple(gt_rgb.shape)))
    F, H, W = rgb.shape[:3]
    if (distance is None) != (gt_depth is None):
        raise ValueError('distance and gt_depth are given together or not at all')
    for name, t in (('distance', distance), ('gt_depth', gt_depth), ('obj_mask', obj_mask)):
        if t is not None and tuple(t.shape) != (F, H, W):
            raise ValueError('%s: %s against frames of %s' % (name, tuple(t.shape), (F, H, W)))
    L = _lib.lib()
    dev = rgb.device
    out = torch.empty(F, EVAL_FLOATS, device=dev)
    nbytes = int(L.durf_eval_scratch_bytes(F, H, W))
    scratch = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    opt = lambda t: None if t is None else _p(_f32(t))
    with _Timed('eval_frames'):
        _lib.check(L.durf_eval_frames(_stream(), F, H, W, _p(_f32(rgb)), _p(_f32(gt_rgb)), opt(distance), opt(gt_depth),
                                      opt(obj_mask), _p(out), _p(scratch), nbytes), 'durf_eval_frames')
    return out, EVAL_FIELDS


# ---- the scene's boxes on rendered frames (csrc/overlay.hip, libdurf_overlay.so; include/durf_overlay.h) -------
BOX_RECT_FIELDS = ('xmin', 'ymin', 'xmax', 'ymax', 'zc', 'visible')
assert len(BOX_RECT_FIELDS) == BOX_RECT_FLOATS


def project_boxes(cams, poses, ext, box_enable=None, znear=1e-2):
    """cams [F,CAM_FLOATS] device rows, poses [F,K,6], ext [K,3] -> (segments [F,K,12,4], rect [F,K,BOX_RECT_FLOATS]): one launch of
    durf_project_boxes, no read-back.  box_enable: None or K values 0 / 1 (a box with 0 is culled whole)."""
    F, K = int(poses.shape[0]), int(poses.shape[1])
    dev = poses.device
    assert tuple(cams.shape) == (F, CAM_FLOATS) and tuple(poses.shape) == (F, K, 6) and tuple(ext.shape) == (K, 3), \
        (tuple(cams.shape), tuple(poses.shape), tuple(ext.shape))
    segments = torch.empty(F, K, BOX_EDGES, 4, device=dev)
    rect = torch.empty(F, K, BOX_RECT_FLOATS, device=dev)
    en = _enable(box_enable, K, dev)
    with _Timed('project_boxes'):
        _lib.check(_lib.overlay_lib().durf_project_boxes(_stream(), F, K, _p(_f32(cams)), _p(_f32(poses)), _p(_f32(ext)), _p(en),
                                                 float(znear), _p(segments), _p(rect)), 'durf_project_boxes')
    return segments, rect


def draw_boxes(segments, colors, half_width, opacity=1.0, frames8=None, framesf=None, label=None):
    """durf_draw_boxes, one launch: segments [F,K,12,4], colors [K,3] uint8 on the device; frames8 [F,h,w,3] uint8 (any byte
    offset into its storage) and / or framesf [F,h,w,3] float are decorated IN PLACE, label [F,h,w] int32 is written whole
    (the owning box, -1: none).  At least one target."""
    targets = [t for t in (frames8, framesf, label) if t is not None]
    if not targets:
        raise ValueError('at least one of frames8, framesf and label')
    F, h, w = (int(n) for n in targets[0].shape[:3])
    K = int(segments.shape[1])
    for t, dt, shape in ((frames8, torch.uint8, (F, h, w, 3)), (framesf, torch.float32, (F, h, w, 3)), (label, torch.int32, (F, h, w))):
        assert t is None or (t.dtype == dt and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape), (t.dtype, tuple(t.shape))
    assert tuple(segments.shape) == (F, K, BOX_EDGES, 4), (tuple(segments.shape), F)
    assert colors.dtype == torch.uint8 and colors.is_cuda and colors.is_contiguous() and tuple(colors.shape) == (K, 3), \
        (colors.dtype, tuple(colors.shape))
    with _Timed('draw_boxes'):
        _lib.check(_lib.overlay_lib().durf_draw_boxes(_stream(), F, h, w, K, _p(_f32(segments)), _p(colors), float(half_width), float(opacity),
                                              _p(frames8), _p(framesf), _p(label)), 'durf_draw_boxes')
    return frames8, framesf, label


# ---- LIDAR sweeps (csrc/lidar.hip, libdurf_lidar.so; include/durf_lidar.h) -------------------------------------
# (LIDAR_SENSOR_FLOATS: H, W, az0, az_span, radius_scale, max_range; LIDAR_SWEEP_FLOATS: pose_start [3,4], omega [3], dp [3])
LIDAR_POINT_FIELDS = ('x', 'y', 'z', 'range', 'r', 'g', 'b', 'dynamic')
assert len(LIDAR_POINT_FIELDS) == LIDAR_POINT_FLOATS
lidar_compact_scratch = _lidar_sigs.DURF_LIDAR_COMPACT_SCRATCH          # (n): int32 elements of durf_lidar_compact's scratch
LIDAR_OUTPUTS = ('range', 'range_mean', 'distance', 'acc', 'rgb', 'spread', 'dynamic', 'valid', 'xyz')      # in argument order


def _host_floats(values, n, what):
    import numpy as np
    a = np.ascontiguousarray(np.asarray(values, np.float32).reshape(-1))
    if a.size != n:
        raise ValueError('%s: %d floats, expected %d' % (what, a.size, n))
    return (C.c_float * n)(*a.tolist())


def _dims(shape):
    nu, nv, nw = (int(s) for s in shape)
    return nu, nv, nw


def _mesh(vertices, triangles):
    """the triangle mesh every mesh library takes: vertices float32 [V,3], triangles int32 [T,3], contiguous on the device -> (V, T)"""
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    assert _f32(vertices).numel() == 3 * V and _i32(triangles, 3 * T, 'triangles') is triangles
    return V, T


def _cams(cams):
    """cams [F,CAM_FLOATS] float32, contiguous on the device -> F"""
    assert _f32(cams).dim() == 2 and cams.shape[1] == CAM_FLOATS, tuple(cams.shape)
    return int(cams.shape[0])


def _lattice_args(origin, du, dv, dw):
    return _host_floats(origin, 3, 'origin'), _host_floats(du, 3, 'du'), _host_floats(dv, 3, 'dv'), _host_floats(dw, 3, 'dw')


def lidar_rays(sensor_row, inclinations, sweep_row, near, far, first=0, count=None):
    """rays [first, first + count) of one sweep (durf_lidar_rays, one launch): sensor_row 6 host floats, inclinations [H] on the
    device, sweep_row 18 host floats -> (origins, directions, viewdirs [count,3], radii, near, far [count])"""
    H, Wd = int(sensor_row[0]), int(sensor_row[1])
    count = H * Wd - first if count is None else count
    dev = inclinations.device
    f = lambda *sh: torch.empty(*sh, device=dev)
    out = (f(count, 3), f(count, 3), f(count, 3), f(count), f(count), f(count))
    with _Timed('lidar_rays'):
        _lib.check(_lib.lidar_lib().durf_lidar_rays(_stream(), _host_floats(sensor_row, LIDAR_SENSOR_FLOATS, 'sensor_row'),
                                                    _p(_f32(inclinations)), _host_floats(sweep_row, LIDAR_SWEEP_FLOATS, 'sweep_row'),
                                                    int(first), int(count), float(near), float(far), *[_p(t) for t in out]),
                   'durf_lidar_rays')
    return out


def lidar_returns(weights, t_vals, acc, origins=None, directions=None, q=0.5, q_lo=0.16, q_hi=0.84, min_acc=0.5,
                  max_range=float('inf'), to_sensor=None):
    """the return model on weights [n,N], t_vals [n,N+1], acc [n] (durf_lidar_returns, one launch) -> dict: range, range_mean,
    spread [n], valid [n] int32 and, with origins / directions [n,3], xyz [n,3] (world; with to_sensor, a [3,4] host
    world-to-sensor row, in that frame)"""
    n, N = int(weights.shape[0]), int(weights.shape[1])
    assert tuple(t_vals.shape) == (n, N + 1) and acc.numel() == n, (tuple(weights.shape), tuple(t_vals.shape), tuple(acc.shape))
    dev = weights.device
    f = lambda *sh: torch.empty(*sh, device=dev)
    out = dict(range=f(n), range_mean=f(n), valid=torch.empty(n, dtype=torch.int32, device=dev), spread=f(n))
    if origins is not None:
        assert tuple(origins.shape) == (n, 3) == tuple(directions.shape), (tuple(origins.shape), tuple(directions.shape))
        out['xyz'] = f(n, 3)
    M = None if to_sensor is None else _host_floats(to_sensor, 12, 'to_sensor')
    with _Timed('lidar_returns'):
        _lib.check(_lib.lidar_lib().durf_lidar_returns(
            _stream(), n, N, _p(_f32(weights)), _p(_f32(t_vals)), _p(_f32(acc)), _p(None if origins is None else _f32(origins)),
            _p(None if origins is None else _f32(directions)), M, float(q), float(q_lo), float(q_hi), float(min_acc), float(max_range),
            _p(out['range']), _p(out['range_mean']), _p(out['valid']), _p(out.get('xyz')), _p(out['spread'])), 'durf_lidar_returns')
    return out


def lidar_compact(valid, xyz, range_, rgb=None, dyn_mask=None, points=None, source=None):
    """the valid returns of n rays, in ray order (durf_lidar_compact: three launches, no read-back) -> points [n,8] (x, y, z, range,
    r, g, b, dynamic; rows from count on are untouched), source [n] int32, count [1] int32 ON THE DEVICE"""
    n = int(valid.numel())
    dev = valid.device
    assert valid.dtype == torch.int32 and valid.is_contiguous() and xyz.numel() == 3 * n and range_.numel() == n
    points = torch.empty(n, LIDAR_POINT_FLOATS, device=dev) if points is None else points
    source = torch.empty(n, dtype=torch.int32, device=dev) if source is None else source
    assert tuple(points.shape) == (n, LIDAR_POINT_FLOATS) and source.dtype == torch.int32 and source.numel() == n
    count = torch.empty(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(lidar_compact_scratch(n), dtype=torch.int32, device=dev)
    if dyn_mask is not None:
        assert dyn_mask.dtype == torch.int32 and dyn_mask.is_contiguous() and dyn_mask.numel() == n
    with _Timed('lidar_compact'):
        _lib.check(_lib.lidar_lib().durf_lidar_compact(_stream(), n, _p(valid), _p(_f32(xyz)), _p(_f32(range_)),
                                                       _p(None if rgb is None else _f32(rgb)), _p(dyn_mask), _p(_f32(points)), _p(source),
                                                       _p(count), _p(scratch)), 'durf_lidar_compact')
    return points, source, count


def render_lidar(sensor_row, inclinations, sweep_rows, poses, ext, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha,
                 enc_flags, chunk, near, far, lindisp=False, bkgd_mode=BKGD_GREY, density_bias=-1.0, resample_padding=0.01,
                 box_enable=None, q=0.5, q_lo=0.16, q_hi=0.84, min_acc=0.5, outputs=LIDAR_OUTPUTS, out=None):
    """F sweeps as ONE library call (durf_render_lidar): sensor_row 6 host floats, inclinations [H] on the device, sweep_rows
    [F,18] host floats, poses [F,K,6] on the device (the boxes of every sweep) -> dict of the requested `outputs`, [F,n,.]
    with n = H * W.  out: dict of preallocated contiguous tensors to write into.  The call only enqueues work."""
    import numpy as np
    outputs = tuple(outputs)
    unknown = [o for o in outputs if o not in LIDAR_OUTPUTS]
    if unknown:
        raise ValueError('unknown outputs %s: choose from %s' % (unknown, list(LIDAR_OUTPUTS)))
    sweep_rows = np.ascontiguousarray(np.asarray(sweep_rows, np.float32).reshape(-1, LIDAR_SWEEP_FLOATS))
    F, K = int(sweep_rows.shape[0]), int(poses.shape[1])
    if int(poses.shape[0]) != F:
        raise ValueError('%d box-pose rows for %d sweeps' % (poses.shape[0], F))
    H, Wd = int(sensor_row[0]), int(sensor_row[1])
    n = max(H, 0) * max(Wd, 0)
    dev = inclinations.device
    L = _lib.lidar_lib()
    res = {}
    for name in outputs:
        shape = (F, n, 3) if name in ('rgb', 'xyz') else (F, n)
        dtype = torch.int32 if name in ('dynamic', 'valid') else torch.float32
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda and t.is_contiguous(), (name, tuple(t.shape), t.dtype)
        res[name] = t
    a = ForwardArgs()
    _fill_model_args(a, K, bkgd_params, obj_params, obj_param_stride, N, num_levels, alpha, enc_flags, lindisp, bkgd_mode,
                     density_bias, resample_padding)
    a.B = ck = max(min(chunk, max(n, 1)), 1)
    a.ext = _p(_f32(ext)) if K else None
    ws = _workspace(dev, int(L.durf_render_lidar_workspace_bytes(ck, N, K, num_levels)))
    with _Timed('render_lidar'):
        _lib.check(L.durf_render_lidar(_stream(), C.byref(a), _p(box_enable), F, _host_floats(sensor_row, LIDAR_SENSOR_FLOATS, 'sensor_row'),
                                       _p(_f32(inclinations)), (C.c_float * max(sweep_rows.size, 1))(*sweep_rows.reshape(-1).tolist()),
                                       _p(_f32(poses)) if K else None, float(near), float(far), ck, float(q), float(q_lo), float(q_hi),
                                       float(min_acc), *[_p(res.get(name)) for name in LIDAR_OUTPUTS], _p(ws), ws.numel()),
                   'durf_render_lidar')
    return res


# ---- motion between frames (csrc/flow.hip, libdurf_flow.so; include/durf_flow.h) -------------------------------
FLOW_CONS_FIELDS = ('count', 'sse', 'sae', 'psnr')
assert len(FLOW_CONS_FIELDS) == FLOW_CONS_FLOATS
flow_pose_floats = _flow_sigs.DURF_FLOW_POSE_FLOATS             # (K): floats of durf_flow_points' pose scratch
flow_cons_scratch = _flow_sigs.DURF_FLOW_CONS_SCRATCH           # (P, m): floats of durf_flow_consistency's scratch
FLOW_OUTPUTS = ('flow', 'scene_flow', 'xyz', 'target', 'zcam', 'moving', 'valid')      # in argument order
_FLOW_COLS = dict(flow=2, scene_flow=3, xyz=3, target=3, zcam=None, moving=None, valid=None)


def _flow_outputs(outputs, lead, dev, out=None):
    outputs = tuple(outputs)
    unknown = [o for o in outputs if o not in FLOW_OUTPUTS]
    if unknown:
        raise ValueError('unknown outputs %s: choose from %s' % (unknown, list(FLOW_OUTPUTS)))
    res = {}
    for name in outputs:
        cols = _FLOW_COLS[name]
        shape = tuple(lead) + ((cols,) if cols else ())
        dtype = torch.int32 if name in ('moving', 'valid') else torch.float32
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda and t.is_contiguous(), (name, tuple(t.shape), t.dtype)
        res[name] = t
    return res


def flow_points(origins_s, dirs_s, hit, t, acc, cam_a, cam_b, pose_a, pose_b, ext, *, first=0, normalise=True, min_acc=0.5,
                znear=1e-2, inside_tol=1e-3, outputs=FLOW_OUTPUTS, out=None):
    """where n pixels [first, first + n) of frame a go (durf_flow_points: a one-wave pose launch and one per-pixel launch):
    origins_s, dirs_s [n,3], hit [n,K] int32 (ray_setup's outputs at pose_a), t, acc [n], cam_a / cam_b one camera row each, pose_a /
    pose_b [K,6], ext [K,3] -> dict of the requested `outputs` (FLOW_OUTPUTS), [n,.]"""
    n, K = int(origins_s.shape[0]), int(pose_a.shape[0])
    dev = origins_s.device
    assert tuple(dirs_s.shape) == (n, 3) and t.numel() == n and acc.numel() == n, (tuple(dirs_s.shape), tuple(t.shape), tuple(acc.shape))
    if K:
        assert hit.dtype == torch.int32 and hit.is_contiguous() and tuple(hit.shape) == (n, K), (hit.dtype, tuple(hit.shape))
        assert tuple(pose_b.shape) == (K, 6) and tuple(ext.shape) == (K, 3), (tuple(pose_b.shape), tuple(ext.shape))
    res = _flow_outputs(outputs, (n,), dev, out)
    scratch = torch.empty(max(flow_pose_floats(K), 1), device=dev)
    with _Timed('flow_points'):
        _lib.check(_lib.flow_lib().durf_flow_points(
            _stream(), n, int(first), K, _p(_f32(origins_s)), _p(_f32(dirs_s)), _p(hit) if K else None, _p(_f32(t)), _p(_f32(acc)),
            _host_floats(cam_a, CAM_FLOATS, 'cam_a'), _host_floats(cam_b, CAM_FLOATS, 'cam_b'), _p(_f32(pose_a)) if K else None,
            _p(_f32(pose_b)) if K else None, _p(_f32(ext)) if K else None, int(bool(normalise)), float(min_acc), float(znear),
            float(inside_tol), _p(scratch), *[_p(res.get(name)) for name in FLOW_OUTPUTS]), 'durf_flow_points')
    return res


def flow_warp(target, valid, img_b, zcam_b, occ_rel=0.02, occ_abs=0.0, want_warped=True, want_mask=True):
    """frame b sampled where frame a's pixels land (durf_flow_warp, one launch): target [n,3], valid [n] int32, img_b [h,w,C]
    (C 1 or 3), zcam_b [h,w] -> (warped [n,C], NaN where not visible, or None; mask [n] int32 or None)"""
    n = int(valid.numel())
    h, w, Cc = (int(x) for x in img_b.shape)
    dev = img_b.device
    assert target.numel() == 3 * n and valid.dtype == torch.int32 and valid.is_contiguous() and zcam_b.numel() == h * w, \
        (tuple(target.shape), valid.dtype, tuple(zcam_b.shape))
    warped = torch.empty(n, Cc, device=dev) if want_warped else None
    mask = torch.empty(n, dtype=torch.int32, device=dev) if want_mask else None
    with _Timed('flow_warp'):
        _lib.check(_lib.flow_lib().durf_flow_warp(_stream(), n, h, w, Cc, _p(_f32(target)), _p(valid), _p(_f32(img_b)), _p(_f32(zcam_b)),
                                                  float(occ_rel), float(occ_abs), _p(warped), _p(mask)), 'durf_flow_warp')
    return warped, mask


def flow_consistency(warped, img_a, mask):
    """warped, img_a [P,m,C], mask [P,m] int32 -> [P,FLOW_CONS_FLOATS] (count, sse, sae, psnr) on the device
    (durf_flow_consistency: two launches, no atomics, the same bits on every run)"""
    P, m, Cc = (int(x) for x in warped.shape)
    assert tuple(img_a.shape) == (P, m, Cc) and tuple(mask.shape) == (P, m) and mask.dtype == torch.int32 and mask.is_contiguous(), \
        (tuple(img_a.shape), tuple(mask.shape), mask.dtype)
    dev = warped.device
    out = torch.empty(P, FLOW_CONS_FLOATS, device=dev)
    scratch = torch.empty(max(flow_cons_scratch(P, m), 1), device=dev)
    with _Timed('flow_consistency'):
        _lib.check(_lib.flow_lib().durf_flow_consistency(_stream(), P, m, Cc, _p(_f32(warped)), _p(_f32(img_a)), _p(mask), _p(out),
                                                         _p(scratch)), 'durf_flow_consistency')
    return out


def flow_color(flow, max_mag, want_float=True, want_u8=False):
    """the Middlebury flow picture of flow [n,2] (durf_flow_color, one launch) -> (rgb [n,3] float or None, rgb8 [n,3] uint8 or None)"""
    n = int(flow.numel()) // 2
    dev = flow.device
    rgb = torch.empty(n, 3, device=dev) if want_float else None
    rgb8 = torch.empty(n, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    with _Timed('flow_color'):
        _lib.check(_lib.flow_lib().durf_flow_color(_stream(), n, _p(_f32(flow)), float(max_mag), _p(rgb), _p(rgb8)), 'durf_flow_color')
    return rgb, rgb8


def render_flow(cams, poses, ext, distance, acc, pairs, near, far, chunk, *, box_enable=None, normalise=True, min_acc=0.5, znear=1e-2,
                inside_tol=1e-3, outputs=('flow', 'valid', 'moving'), out=None):
    """P pairs of frames as ONE library call (durf_render_flow): cams [F,CAM_FLOATS] host rows, poses [F,K,6] on the device, ext [K,3],
    distance / acc [F,n] (render_trajectory's planes), pairs [P,2] host ints (source, target) -> dict of the requested `outputs`
    (FLOW_OUTPUTS), [P,n,.].  out: dict of preallocated contiguous tensors to write into.  The call only enqueues work."""
    import numpy as np
    cams, h, w = camera.as_rows(cams, 'render_flow', one_size=False)
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    F, P, K = int(cams.shape[0]), int(pairs.shape[0]), int(poses.shape[1])
    n = h * w
    dev = distance.device
    if int(poses.shape[0]) != F or tuple(distance.shape) != (F, n) or tuple(acc.shape) != (F, n):
        raise ValueError('%d camera rows of %d pixels for poses %s, distance %s, acc %s' %
                         (F, n, tuple(poses.shape), tuple(distance.shape), tuple(acc.shape)))
    L = _lib.flow_lib()
    res = _flow_outputs(outputs, (P, n), dev, out)
    ck = max(min(int(chunk), max(n, 1)), 1) if chunk > 0 else int(chunk)
    ws = _workspace(dev, int(L.durf_render_flow_workspace_bytes(ck, K)))
    with _Timed('render_flow'):
        _lib.check(L.durf_render_flow(_stream(), F, K, (C.c_float * max(cams.size, 1))(*cams.reshape(-1).tolist()),
                                      _p(_f32(poses)) if K else None, _p(_f32(ext)) if K else None, _p(box_enable), _p(_f32(distance)),
                                      _p(_f32(acc)), P, (C.c_int * max(pairs.size, 1))(*pairs.reshape(-1).tolist()), float(near),
                                      float(far), ck, int(bool(normalise)), float(min_acc), float(znear), float(inside_tol),
                                      *[_p(res.get(name)) for name in FLOW_OUTPUTS], _p(ws), ws.numel()), 'durf_render_flow')
    return res


# ---------------------------------------------------------------------------
# the field at world points (include/durf_field.h, csrc/field.hip, libdurf_field.so): staged calls and the one-call walks
# ---------------------------------------------------------------------------
FieldArgs = _field_sigs.durf_field_args
field_pose_floats = _field_sigs.DURF_FIELD_POSE_FLOATS          # (K): floats of durf_field_classify's pose scratch


def _barf_host(alpha):
    return (C.c_float * 10)(*[float(x) for x in barf_weights(alpha)])


def field_classify(points, pose, ext, box_enable=None, inside_tol=0.0):
    """durf_field_classify: points [n,3], pose [K,6], ext [K,3] -> owner [n] int32 (-1 none, -2 several), local [n,3]"""
    n, K = int(points.shape[0]), 0 if pose is None else int(pose.shape[0])
    dev = points.device
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    local = torch.empty(n, 3, device=dev)
    table = torch.empty(field_pose_floats(max(K, 1)), device=dev)
    with _Timed('field_classify'):
        _lib.check(_lib.field_lib().durf_field_classify(_stream(), n, _p(_f32(points)), K, _p(_f32(pose)) if K else None,
                                                        _p(_f32(ext)) if K else None, _p(box_enable), float(inside_tol), _p(table),
                                                        _p(owner), _p(local)), 'durf_field_classify')
    return owner, local


def field_lists(owner, K, idx=None, count=None):
    """durf_field_lists: owner [n] int32 -> idx [(K+1), n] int32 (rows past count[c] untouched), count [K+1] int32"""
    n, dev = int(owner.shape[0]), owner.device
    idx = torch.empty(K + 1, n, dtype=torch.int32, device=dev) if idx is None else idx
    count = torch.zeros(K + 1, dtype=torch.int32, device=dev) if count is None else count
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() >= (K + 1) * n and count.numel() >= K + 1
    _lib.check(_lib.field_lib().durf_field_lists(_stream(), n, K, _p(owner), _p(idx), _p(count)), 'durf_field_lists')
    return idx, count


def field_owned(idx, count, K):
    """durf_field_owned: lists 0 .. K-1 one after the other -> owned [n] int32, owned_count [1] int32"""
    n, dev = int(idx.shape[1]), idx.device
    owned = torch.empty(n, dtype=torch.int32, device=dev)
    ocount = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.field_lib().durf_field_owned(_stream(), n, K, _p(idx), _p(count), _p(owned), _p(ocount)), 'durf_field_owned')
    return owned, ocount


def field_encode(local, idx, count, K, sigma=0.0, contraction=True, alpha=10.0, enc_bkgd=None, enc_obj=None):
    """durf_field_encode -> enc_bkgd [n,60], enc_obj [K,n,63] (fresh buffers are zero filled; rows past count are untouched)"""
    n, dev = int(local.shape[0]), local.device
    enc_bkgd = torch.zeros(n, FIELD_ENC_BKGD, device=dev) if enc_bkgd is None else enc_bkgd
    enc_obj = (torch.zeros(K, n, FIELD_ENC_OBJ, device=dev) if enc_obj is None else enc_obj) if K else None
    with _Timed('field_encode'):
        _lib.check(_lib.field_lib().durf_field_encode(_stream(), n, K, _p(_f32(local)), _p(idx), _p(count), float(sigma),
                                                      ENC_CONTRACT if contraction else 0, _barf_host(alpha), _p(_f32(enc_bkgd)),
                                                      _p(enc_obj)), 'durf_field_encode')
    return enc_bkgd, enc_obj


def field_activate(idx, count, raw_bkgd, raw_obj, raw_const, owner, density_bias, want_rgb=True, want_raw=True):
    """durf_field_activate -> density [n], rgb [n,3] or None, raw [n,4] or None, valid [n] uint8"""
    n, K, dev = int(owner.shape[0]), int(idx.shape[0]) - 1, owner.device
    density = torch.empty(n, device=dev)
    rgb = torch.empty(n, 3, device=dev) if want_rgb else None
    raw = torch.empty(n, 4, device=dev) if want_raw else None
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    with _Timed('field_activate'):
        _lib.check(_lib.field_lib().durf_field_activate(_stream(), n, K, _p(idx), _p(count), _p(_f32(raw_bkgd)), _p(raw_obj),
                                                        _p(raw_const), _p(owner), float(density_bias), _p(density), _p(rgb), _p(raw),
                                                        _p(valid)), 'durf_field_activate')
    return density, rgb, raw, valid


def field_workspace_bytes(chunk, K):
    return int(_lib.field_lib().durf_field_workspace_bytes(int(chunk), int(K)))


def field_args(K, bkgd_params, bkgd_ws, obj_params, param_stride, obj_ws, trunk, pose, ext, box_enable, sigma, alpha, contraction,
               inside_tol, density_bias):
    """the parameter half of durf_field_args (the points and the outputs are filled per call) -> (FieldArgs, the tensors it
    points into: keep them alive until the call is issued)"""
    a = FieldArgs()
    a.K, a.enc_flags = int(K), ENC_CONTRACT if contraction else 0
    a.sigma, a.inside_tol, a.density_bias = float(sigma), float(inside_tol), float(density_bias)
    a.barf_w = _barf_host(alpha)
    a.bkgd_params, a.bkgd_wstream = _p(_f32(bkgd_params)), _p(bkgd_ws)
    if K:
        a.obj_params, a.param_stride, a.obj_wstream, a.const_trunk = _p(_f32(obj_params)), int(param_stride), _p(obj_ws), _p(trunk)
        a.pose, a.ext, a.box_enable = _p(_f32(pose)), _p(_f32(ext)), _p(box_enable)
    return a, (bkgd_params, bkgd_ws, obj_params, obj_ws, trunk, pose, ext, box_enable)


def _field_outputs(a, n, dev, want_rgb):
    out = dict(density=torch.empty(n, device=dev), rgb=torch.empty(n, 3, device=dev) if want_rgb else None,
               raw=torch.empty(n, 4, device=dev), owner=torch.empty(n, dtype=torch.int32, device=dev),
               valid=torch.empty(n, dtype=torch.uint8, device=dev))
    for k, v in out.items():
        setattr(a, k, _p(v))
    return out


def field_query(a, points, viewdirs, chunk):
    """durf_field_query: n points in ONE call -> dict density [n], rgb [n,3] (None without viewdirs), raw [n,4], owner [n] int32,
    valid [n] uint8.  The call only enqueues work."""
    n, dev = int(points.shape[0]), points.device
    out = _field_outputs(a, n, dev, viewdirs is not None)
    a.points, a.viewdirs = _p(_f32(points)), None if viewdirs is None else _p(_f32(viewdirs))
    ck = max(min(int(chunk), max(n, 1)), 1) if chunk > 0 else int(chunk)
    L = _lib.field_lib()
    ws = _workspace(dev, int(L.durf_field_workspace_bytes(ck, a.K)))
    with _Timed('field_query'):
        _lib.check(L.durf_field_query(_stream(), C.addressof(a), n, ck, _p(ws), ws.numel()), 'durf_field_query')
    return out


def field_grid(a, origin, du, dv, dw, shape, view, chunk, dev, want_points=False):
    """durf_field_grid: the grid origin + i du + j dv + k dw (k fastest) of shape (nu, nv, nw) in ONE call -> field_query's
    dict over the nu nv nw cells[, points [nu nv nw, 3]]; view: one direction (3 floats) or None (density only)"""
    nu, nv, nw = _dims(shape)
    n = nu * nv * nw
    if min(nu, nv, nw) < 1 or n >= 2 ** 31:
        raise ValueError('field_grid: a grid of %d x %d x %d cells' % (nu, nv, nw))
    out = _field_outputs(a, n, dev, view is not None)
    a.points = a.viewdirs = None
    out['points'] = torch.empty(n, 3, device=dev) if want_points else None
    vx, vy, vz = (float(x) for x in view) if view is not None else (0.0, 0.0, 0.0)
    ck = max(min(int(chunk), n), 1) if chunk > 0 else int(chunk)
    L = _lib.field_lib()
    ws = _workspace(dev, int(L.durf_field_workspace_bytes(ck, a.K)))
    with _Timed('field_grid'):
        _lib.check(L.durf_field_grid(_stream(), C.addressof(a), *_lattice_args(origin, du, dv, dw), nu, nv, nw, int(view is not None),
                                     vx, vy, vz, ck, _p(ws), ws.numel(), _p(out['points'])), 'durf_field_grid')
    return out


def field_columns(density, valid, shape, step, threshold):
    """durf_field_columns over density / valid [nu nv nw] -> col_max, col_opacity [nu,nv] float, col_first [nu,nv] int32"""
    nu, nv, nw = _dims(shape)
    dev = density.device
    assert density.numel() == nu * nv * nw and valid.numel() == nu * nv * nw and valid.dtype == torch.uint8 and valid.is_contiguous()
    cmax, cop = torch.empty(nu, nv, device=dev), torch.empty(nu, nv, device=dev)
    cfirst = torch.empty(nu, nv, dtype=torch.int32, device=dev)
    with _Timed('field_columns'):
        _lib.check(_lib.field_lib().durf_field_columns(_stream(), nu, nv, nw, _p(_f32(density)), _p(valid), float(step), float(threshold),
                                                       _p(cmax), _p(cop), _p(cfirst)), 'durf_field_columns')
    return cmax, cop, cfirst


# ---------------------------------------------------------------------------
# the iso-surface of a density lattice (include/durf_mesh.h, csrc/mesh.hip, libdurf_mesh.so)
# ---------------------------------------------------------------------------
def mesh_workspace_bytes(shape):
    return int(_lib.mesh_lib().durf_mesh_workspace_bytes(*_dims(shape)))


def mesh_workspace_views(ws, shape):
    """voff, toff int32 [n] and mask uint8 [n] of a workspace durf_mesh_count filled (the layout include/durf_mesh.h states)"""
    nu, nv, nw = _dims(shape)
    n = nu * nv * nw
    o1 = _up256(4 * n)
    o2 = o1 + _up256(4 * n)
    return ws[:4 * n].view(torch.int32), ws[o1:o1 + 4 * n].view(torch.int32), ws[o2:o2 + n]


def _mesh_lattice(density, valid, shape):
    nu, nv, nw = _dims(shape)
    n = nu * nv * nw
    assert density.numel() == n, (tuple(density.shape), shape)
    if valid is not None:
        assert valid.dtype == torch.uint8 and valid.is_contiguous() and valid.numel() == n and valid.is_cuda
    return nu, nv, nw


def mesh_count(density, valid, shape, iso, ws=None):
    """durf_mesh_count: classify, count, scan -> (counts int32 [2] ON THE DEVICE: vertices, triangles; the workspace, a uint8
    tensor durf_mesh_emit reads).  Three launches, no read-back."""
    nu, nv, nw = _mesh_lattice(density, valid, shape)
    dev = density.device
    L = _lib.mesh_lib()
    ws = _ws(ws, int(L.durf_mesh_workspace_bytes(nu, nv, nw)), dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    with _Timed('mesh_count'):
        _lib.check(L.durf_mesh_count(_stream(), nu, nv, nw, _p(_f32(density)), _p(valid), float(iso), _p(ws), ws.numel(), _p(counts)),
                   'durf_mesh_count')
    return counts, ws


def mesh_emit(density, valid, shape, iso, origin, du, dv, dw, ws, max_vertices, max_triangles, normal_xform=None, flip=False,
              want_edge=True, want_t=True, out=None):
    """durf_mesh_emit on the workspace of mesh_count -> dict vertices [max_vertices,3], normals (None without normal_xform),
    vertex_edge [max_vertices,2] int32, vertex_t [max_vertices], triangles [max_triangles,3] int32.  out: buffers to write
    into instead of fresh ones (rows at or past a capacity are left as they are)."""
    nu, nv, nw = _mesh_lattice(density, valid, shape)
    dev = density.device
    mv, mt = int(max_vertices), int(max_triangles)
    o = dict(out or {})
    o.setdefault('vertices', torch.empty(max(mv, 0), 3, device=dev))
    o.setdefault('normals', torch.empty(max(mv, 0), 3, device=dev) if normal_xform is not None else None)
    o.setdefault('vertex_edge', torch.empty(max(mv, 0), 2, dtype=torch.int32, device=dev) if want_edge else None)
    o.setdefault('vertex_t', torch.empty(max(mv, 0), device=dev) if want_t else None)
    o.setdefault('triangles', torch.empty(max(mt, 0), 3, dtype=torch.int32, device=dev))
    for k2, rows in (('vertices', mv), ('normals', mv), ('vertex_edge', mv), ('vertex_t', mv), ('triangles', mt)):
        assert o[k2] is None or (o[k2].is_contiguous() and o[k2].shape[0] >= rows), k2
    A = None if normal_xform is None else _host_floats(normal_xform, 9, 'normal_xform')
    with _Timed('mesh_emit'):
        _lib.check(_lib.mesh_lib().durf_mesh_emit(
            _stream(), nu, nv, nw, _p(_f32(density)), _p(valid), float(iso), *_lattice_args(origin, du, dv, dw), A, int(bool(flip)),
            _p(ws), ws.numel(), mv, mt, _p(o['vertices']), _p(o['normals']), _p(o['vertex_edge']), _p(o['vertex_t']), _p(o['triangles'])),
            'durf_mesh_emit')
    return o


def mesh_gather(shape, counts, vertex_edge, vertex_t, attr_f=None, attr_i=None, density=None, valid=None, iso=0.0, out_f=None,
                out_i=None):
    """durf_mesh_gather: lattice attributes at the vertices -> (out_f [V,C] = a + t (b - a) or None, out_i [V] int32 = the label
    of each edge's in end, or None)"""
    nu, nv, nw = _dims(shape)
    n = nu * nv * nw
    V, dev = int(vertex_edge.shape[0]), vertex_edge.device
    assert vertex_edge.dtype == torch.int32 and vertex_edge.is_contiguous() and vertex_t.numel() == V
    Cn = 1
    if attr_f is not None:
        attr_f = _f32(attr_f).reshape(n, -1)
        Cn = int(attr_f.shape[1])
        out_f = torch.empty(V, Cn, device=dev) if out_f is None else out_f
    if attr_i is not None:
        assert attr_i.dtype == torch.int32 and attr_i.is_contiguous() and attr_i.numel() == n and density.numel() == n
        out_i = torch.empty(V, dtype=torch.int32, device=dev) if out_i is None else out_i
    if V == 0:                              # an empty surface: its zero-row tensors have no address to hand over
        return out_f, out_i
    with _Timed('mesh_gather'):
        _lib.check(_lib.mesh_lib().durf_mesh_gather(
            _stream(), nu, nv, nw, _p(counts), V, _p(vertex_edge), _p(_f32(vertex_t)), Cn, _p(attr_f), _p(out_f), _p(attr_i),
            _p(None if density is None else _f32(density)), _p(valid), float(iso), _p(out_i)), 'durf_mesh_gather')
    return out_f, out_i


# ---------------------------------------------------------------------------
# connected components of a density lattice (include/durf_parts.h, csrc/parts.hip, libdurf_parts.so)
# ---------------------------------------------------------------------------
def parts_workspace_bytes(shape):
    return int(_lib.parts_lib().durf_parts_workspace_bytes(*_dims(shape)))


def parts_label(density, valid, shape, iso, ws=None, labels=None):
    """durf_parts_label: the label of every lattice point (the smallest index of its component, -1 where it is not in) ->
    (labels int32 [n], the workspace).  Three launches, no read-back."""
    nu, nv, nw = _mesh_lattice(density, valid, shape)
    n, dev = nu * nv * nw, density.device
    L = _lib.parts_lib()
    ws = _ws(ws, int(L.durf_parts_workspace_bytes(nu, nv, nw)), dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev) if labels is None else _i32(labels, n, 'labels')
    with _Timed('parts_label'):
        _lib.check(L.durf_parts_label(_stream(), nu, nv, nw, _p(_f32(density)), _p(valid), float(iso), _p(ws), ws.numel(), _p(labels)),
                   'durf_parts_label')
    return labels, ws


def parts_number(labels, ws=None):
    """durf_parts_number -> (comp int32 [n]: the number of every point's component, -1 where it has none; count int32 [1] ON
    THE DEVICE).  No read-back."""
    n, dev = int(labels.numel()), labels.device
    _i32(labels, n, 'labels')
    ws = _ws(ws, _up256(4 * n) + _up256(4 * ((n + PARTS_BLOCK - 1) // PARTS_BLOCK + 1)), dev)
    comp, count = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    with _Timed('parts_number'):
        _lib.check(_lib.parts_lib().durf_parts_number(_stream(), n, _p(labels), _p(ws), ws.numel(), _p(comp), _p(count)), 'durf_parts_number')
    return comp, count


def parts_stats(comp, shape, max_components, size=None, bbox=None):
    """durf_parts_stats -> (size int32 [max_components], bbox int32 [max_components,6]: imin, jmin, kmin, imax, jmax, kmax)"""
    nu, nv, nw = _dims(shape)
    mc, dev = int(max_components), comp.device
    _i32(comp, nu * nv * nw, 'comp')
    size = torch.empty(max(mc, 0), dtype=torch.int32, device=dev) if size is None else size
    bbox = torch.empty(max(mc, 0), 6, dtype=torch.int32, device=dev) if bbox is None else bbox
    with _Timed('parts_stats'):
        _lib.check(_lib.parts_lib().durf_parts_stats(_stream(), nu, nv, nw, _p(comp), mc, _z(size), _z(bbox)), 'durf_parts_stats')
    return size, bbox


def parts_select_mesh(counts, vertex_comp, triangles, keep, ws=None):
    """durf_parts_select_mesh: the vertices whose component is kept and the triangles that hang on them, in their order ->
    (vertex_map int32 [V], vertex_src int32 [V], triangles_out int32 [T,3], counts_out int32 [2] ON THE DEVICE).  Four
    launches, no read-back."""
    V, T, dev = int(vertex_comp.shape[0]), int(triangles.shape[0]), counts.device
    _i32(counts, 2, 'counts'), _i32(vertex_comp, V, 'vertex_comp'), _i32(triangles, 3 * T, 'triangles')
    nc = int(keep.numel())
    assert keep.dtype == torch.uint8 and keep.is_contiguous() and keep.is_cuda
    ws = _ws(ws, _up256(8 * ((max(V, T) + PARTS_BLOCK - 1) // PARTS_BLOCK + 1)), dev)
    vmap, vsrc = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.int32, device=dev)
    tri, out = torch.empty(T, 3, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    with _Timed('parts_select_mesh'):
        _lib.check(_lib.parts_lib().durf_parts_select_mesh(_stream(), _p(counts), V, T, _z(vertex_comp), _z(triangles), _z(keep), nc,
                                                           _p(ws), ws.numel(), _z(vmap), _z(vsrc), _z(tri), _p(out)),
                   'durf_parts_select_mesh')
    return vmap, vsrc, tri, out


# ---------------------------------------------------------------------------
# a triangle mesh through pinhole cameras (include/durf_raster.h, csrc/raster.hip, libdurf_raster.so)
# ---------------------------------------------------------------------------
from .raster import COUNT_FIELDS as RASTER_COUNT_FIELDS        # noqa: E402  (written once, in the host-side module, which imports no torch)
assert len(RASTER_COUNT_FIELDS) == RASTER_COUNTS


def raster_workspace_bytes(F, T, h, w):
    return int(_lib.raster_lib().durf_raster_workspace_bytes(int(F), int(T), int(h), int(w)))


def raster_setup(cams, h, w, vertices, triangles, znear, cull=0, ws=None):
    """durf_raster_setup: project, cull, snap and count per tile, scan -> (counts int32 [RASTER_COUNTS] ON THE DEVICE:
    RASTER_COUNT_FIELDS; the workspace, a uint8 tensor raster_draw reads).  No read-back."""
    F, (V, T) = _cams(cams), _mesh(vertices, triangles)
    dev = cams.device
    ws = _ws(ws, raster_workspace_bytes(F, T, h, w), dev)
    counts = torch.empty(RASTER_COUNTS, dtype=torch.int32, device=dev)
    with _Timed('raster_setup'):
        _lib.check(_lib.raster_lib().durf_raster_setup(_stream(), F, int(h), int(w), _z(cams), V, T, _z(vertices), _z(triangles), float(znear),
                                                       int(cull), _p(ws), ws.numel(), _p(counts)), 'durf_raster_setup')
    return counts, ws


def raster_draw(F, T, h, w, ws, max_pairs, pairs=None, want_bary=True):
    """durf_raster_draw on the workspace of raster_setup -> (tri int32 [F,h,w], depth [F,h,w], bary [F,h,w,3] or None).  A
    max_pairs below counts[0] gives tri = -2 and depth = NaN everywhere.  pairs: scratch of at least max_pairs int32 to reuse."""
    dev, mp = ws.device, int(max_pairs)
    if pairs is None:
        pairs = torch.empty(max(mp, 0), dtype=torch.int32, device=dev)
    assert pairs.dtype == torch.int32 and pairs.is_contiguous() and pairs.numel() >= mp
    tri = torch.empty(F, h, w, dtype=torch.int32, device=dev)
    depth = torch.empty(F, h, w, device=dev)
    bary = torch.empty(F, h, w, 3, device=dev) if want_bary else None
    with _Timed('raster_draw'):
        _lib.check(_lib.raster_lib().durf_raster_draw(_stream(), int(F), int(T), int(h), int(w), _p(ws), ws.numel(), _z(pairs), mp, _z(tri),
                                                      _z(depth), _z(bary)), 'durf_raster_draw')
    return tri, depth, bary


def _raster_attrs(V, attr_f, attr_i):
    Cn = 1
    if attr_f is not None:
        attr_f = _f32(attr_f).reshape(V, -1)
        Cn = int(attr_f.shape[1])
    if attr_i is not None:
        _i32(attr_i, V, 'attr_i')
    return Cn, attr_f, attr_i


def raster_interp(triangles, tri, bary, n_vertices, attr_f=None, attr_i=None, fill=-1):
    """durf_raster_interp: vertex attributes at the pixels -> (out_f [..., C] = (q0 a0 + q1 a1) + q2 a2 or None, out_i [...]
    int32 = attr_i of the triangle's first vertex or None); 0 and `fill` where nothing covers"""
    V, T, dev = int(n_vertices), int(triangles.shape[0]), tri.device
    n = int(tri.numel())
    _i32(tri, n, 'tri')
    Cn, attr_f, attr_i = _raster_attrs(V, attr_f, attr_i)
    out_f = torch.empty(tuple(tri.shape) + (Cn,), device=dev) if attr_f is not None else None
    out_i = torch.empty(tuple(tri.shape), dtype=torch.int32, device=dev) if attr_i is not None else None
    with _Timed('raster_interp'):
        _lib.check(_lib.raster_lib().durf_raster_interp(_stream(), n, V, T, _z(triangles), _z(tri), _z(bary), Cn, _p(attr_f), _p(out_f), _p(attr_i),
                                                        int(fill), _p(out_i)), 'durf_raster_interp')
    return out_f, out_i


def raster_render_mesh(cams, h, w, vertices, triangles, znear, max_pairs, cull=0, attr_f=None, attr_i=None, fill=-1, ws=None, pairs=None):
    """durf_render_mesh: setup, draw and (with an attribute) interp in one call, for a pair capacity the caller chose -> dict
    counts (ON THE DEVICE), tri, depth, bary, out_f, out_i.  counts[0] > max_pairs: the -2 / NaN picture."""
    F, (V, T) = _cams(cams), _mesh(vertices, triangles)
    dev, mp = cams.device, int(max_pairs)
    ws = _ws(ws, raster_workspace_bytes(F, T, h, w), dev)
    if pairs is None:
        pairs = torch.empty(max(mp, 0), dtype=torch.int32, device=dev)
    Cn, attr_f, attr_i = _raster_attrs(V, attr_f, attr_i)
    o = dict(counts=torch.empty(RASTER_COUNTS, dtype=torch.int32, device=dev), tri=torch.empty(F, h, w, dtype=torch.int32, device=dev),
             depth=torch.empty(F, h, w, device=dev), bary=torch.empty(F, h, w, 3, device=dev),
             out_f=torch.empty(F, h, w, Cn, device=dev) if attr_f is not None else None,
             out_i=torch.empty(F, h, w, dtype=torch.int32, device=dev) if attr_i is not None else None)
    with _Timed('render_mesh'):
        _lib.check(_lib.raster_lib().durf_render_mesh(
            _stream(), F, int(h), int(w), _z(cams), V, T, _z(vertices), _z(triangles), float(znear), int(cull), _p(ws), ws.numel(), _z(pairs), mp,
            _p(o['counts']), _z(o['tri']), _z(o['depth']), _z(o['bary']), Cn, _p(attr_f), _p(o['out_f']), _p(attr_i), int(fill), _p(o['out_i'])),
            'durf_render_mesh')
    return o


# ---------------------------------------------------------------------------
# distances between point sets, mesh samples (include/durf_geom.h, csrc/geom.hip, libdurf_geom.so)
# ---------------------------------------------------------------------------
GEOM_STAT_FIELDS = ('usable', 'found', 'sum_found', 'sum_sq_found', 'sum_usable')        # then one count per threshold
assert len(GEOM_STAT_FIELDS) + GEOM_MAX_THRESHOLDS == GEOM_STAT_DOUBLES


def geom_workspace_bytes(n_queries, n_triangles):
    return int(_lib.geom_lib().durf_geom_workspace_bytes(int(n_queries), int(n_triangles)))


def _geom_points(t, what):
    assert t.dim() == 2 and t.shape[1] == 3, (what, tuple(t.shape))
    return _f32(t)


def geom_keys(points, origin, inv_cell, dims):
    """durf_geom_keys: the cell key of every point [n,3] -> int64 [n] (-1: not in the grid)"""
    n = int(_geom_points(points, 'points').shape[0])
    keys = torch.empty(n, dtype=torch.int64, device=points.device)
    with _Timed('geom_keys'):
        _lib.check(_lib.geom_lib().durf_geom_keys(_stream(), n, _z(points), _host_floats(origin, 3, 'origin'), float(inv_cell),
                                                  int(dims[0]), int(dims[1]), int(dims[2]), _z(keys)), 'durf_geom_keys')
    return keys


def geom_nearest(query, ref_sorted, ref_keys, ref_index, origin, inv_cell, dims, max_dist):
    """durf_geom_nearest: per query [q,3] the nearest of the cell-sorted reference points within max_dist -> (dist [q], index [q]
    int32: the reference point's original index, -1 none within max_dist (dist = max_dist), -2 an unusable query (dist NaN))"""
    q, m = int(_geom_points(query, 'query').shape[0]), int(_geom_points(ref_sorted, 'ref_sorted').shape[0])
    assert ref_keys.dtype == torch.int64 and ref_keys.is_contiguous() and ref_keys.numel() == m
    assert ref_index.dtype == torch.int32 and ref_index.is_contiguous() and ref_index.numel() == m
    dev = query.device
    dist, index = torch.empty(q, device=dev), torch.empty(q, dtype=torch.int32, device=dev)
    with _Timed('geom_nearest'):
        _lib.check(_lib.geom_lib().durf_geom_nearest(
            _stream(), q, _z(query), m, _z(ref_sorted), _z(ref_keys), _z(ref_index), _host_floats(origin, 3, 'origin'),
            float(inv_cell), int(dims[0]), int(dims[1]), int(dims[2]), float(max_dist), _z(dist), _z(index)), 'durf_geom_nearest')
    return dist, index


def geom_stats(dist, index, thresholds=(), out=None, ws=None):
    """durf_geom_stats -> float64 [GEOM_STAT_DOUBLES] ON THE DEVICE (GEOM_STAT_FIELDS, then one count per threshold); out: the
    row to write into.  Two launches, no read-back."""
    q = int(dist.numel())
    assert index.dtype == torch.int32 and index.is_contiguous() and index.numel() == q and _f32(dist) is dist
    th = [float(t) for t in thresholds]
    L = _lib.geom_lib()
    ws = _ws(ws, int(L.durf_geom_workspace_bytes(q, 0)), dist.device)
    if out is None:
        out = torch.empty(GEOM_STAT_DOUBLES, dtype=torch.float64, device=dist.device)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == GEOM_STAT_DOUBLES
    arr = (C.c_float * max(len(th), 1))(*th)
    with _Timed('geom_stats'):
        _lib.check(L.durf_geom_stats(_stream(), q, _z(dist), _z(index), len(th), arr, _p(ws), ws.numel(),
                                     _p(out)), 'durf_geom_stats')
    return out


def geom_sample_mesh(vertices, triangles, n, ws=None):
    """durf_geom_sample_mesh: n area-uniform samples of the mesh (vertices [V,3], triangles [T,3] int32) -> (points [n,3], tri [n]
    int32: the triangle of each sample, total_area float64 [1] on the device)"""
    (V, T), n = _mesh(vertices, triangles), int(n)
    dev = vertices.device
    L = _lib.geom_lib()
    ws = _ws(ws, int(L.durf_geom_workspace_bytes(0, T)), dev)
    points, tri = torch.empty(max(n, 0), 3, device=dev), torch.empty(max(n, 0), dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    with _Timed('geom_sample_mesh'):
        _lib.check(L.durf_geom_sample_mesh(_stream(), V, _z(vertices), T, _z(triangles), n, _p(ws), ws.numel(), _z(points), _z(tri),
                                           _p(total)), 'durf_geom_sample_mesh')
    return points, tri, total


# ---------------------------------------------------------------------------
# depth frames fused into a TSDF volume (include/durf_tsdf.h, csrc/tsdf.hip, libdurf_tsdf.so)
# ---------------------------------------------------------------------------
def _tsdf_state(tsdf, weight, colour, shape):
    nu, nv, nw = _dims(shape)
    n = nu * nv * nw
    assert _f32(tsdf).numel() == n and _f32(weight).numel() == n, (tuple(tsdf.shape), tuple(weight.shape), shape)
    assert colour is None or _f32(colour).numel() == 4 * n, (tuple(colour.shape), shape)
    return nu, nv, nw, n


def tsdf_integrate(tsdf, weight, colour, shape, origin, du, dv, dw, cams, depth, trunc, acc=None, min_acc=0.5, rgb=None, label=None,
                   select=0, other_mode=0, xform=None, frame_weight=None, max_weight=64.0, znear=1e-2):
    """durf_tsdf_integrate: the F frames depth [F,h,w] (cams [F,CAM_FLOATS] on the device) into the state tsdf, weight [n] and colour
    [n,4] (or None), IN PLACE, one launch.  acc [F,h,w], rgb [F,h,w,3], label int32 [F,h,w], xform [F,3,4], frame_weight [F]:
    on the device, or None."""
    nu, nv, nw, n = _tsdf_state(tsdf, weight, colour, shape)
    assert _f32(depth).dim() == 3, tuple(depth.shape)
    F, h, w = (int(s) for s in depth.shape)
    assert _cams(cams) == F, (tuple(cams.shape), F)
    assert acc is None or _f32(acc).numel() == F * h * w
    assert rgb is None or _f32(rgb).numel() == 3 * F * h * w
    assert label is None or _i32(label, F * h * w, 'label') is label
    assert xform is None or _f32(xform).numel() == 12 * F
    assert frame_weight is None or _f32(frame_weight).numel() == F
    with _Timed('tsdf_integrate'):
        _lib.check(_lib.tsdf_lib().durf_tsdf_integrate(
            _stream(), nu, nv, nw, *_lattice_args(origin, du, dv, dw), F, h, w, _z(cams), _z(depth), _z(acc), float(min_acc), _z(rgb),
            _z(label), int(select), int(other_mode), _z(xform), _z(frame_weight), float(trunc), float(max_weight), float(znear), _p(tsdf),
            _p(weight), _p(colour)), 'durf_tsdf_integrate')


def tsdf_lattice(tsdf, weight, colour, shape, min_weight=1.0, want_rgb=True):
    """durf_tsdf_lattice -> (density [nu,nv,nw] = -D, valid uint8 [nu,nv,nw] = (W >= min_weight), rgb [nu,nv,nw,3] or None: the
    colour where its weight is positive, else 0): what mesh_count and parts_label take"""
    nu, nv, nw, n = _tsdf_state(tsdf, weight, colour, shape)
    dev = tsdf.device
    density, valid = torch.empty(nu, nv, nw, device=dev), torch.empty(nu, nv, nw, dtype=torch.uint8, device=dev)
    rgb = torch.empty(nu, nv, nw, 3, device=dev) if want_rgb and colour is not None else None
    with _Timed('tsdf_lattice'):
        _lib.check(_lib.tsdf_lib().durf_tsdf_lattice(_stream(), nu, nv, nw, _p(tsdf), _p(weight), _p(colour), float(min_weight), _p(density),
                                                     _p(valid), _p(rgb)), 'durf_tsdf_lattice')
    return density, valid, rgb


def tsdf_sample(tsdf, weight, colour, shape, origin, inv, trunc, points, min_weight=1.0, want_rgb=True):
    """durf_tsdf_sample: points [m,3] -> (sdf [m]: trilinear D times trunc, NaN outside or beside an unobserved voxel; ok uint8
    [m]; rgb [m,3] or None).  inv: the inverse of [du dv dw], nine host floats."""
    nu, nv, nw, n = _tsdf_state(tsdf, weight, colour, shape)
    m, dev = int(_geom_points(points, 'points').shape[0]), tsdf.device
    _f32(points)
    sdf, ok = torch.empty(m, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
    rgb = torch.empty(m, 3, device=dev) if want_rgb and colour is not None else None
    with _Timed('tsdf_sample'):
        _lib.check(_lib.tsdf_lib().durf_tsdf_sample(_stream(), nu, nv, nw, _host_floats(origin, 3, 'origin'), _host_floats(inv, 9, 'inv'),
                                                    _p(tsdf), _p(weight), _p(colour), float(trunc), float(min_weight), m, _z(points), _z(sdf),
                                                    _z(ok), _z(rgb)), 'durf_tsdf_sample')
    return sdf, ok, rgb


# ---------------------------------------------------------------------------
# rays against a triangle mesh (include/durf_cast.h, csrc/cast.hip, libdurf_cast.so)
# ---------------------------------------------------------------------------
def cast_workspace_bytes(T):
    return int(_lib.cast_lib().durf_cast_workspace_bytes(int(T)))


def cast_keys(vertices, triangles, bounds):
    """durf_cast_keys: the Morton key of every triangle's centroid inside bounds [6] ON THE DEVICE (lo, hi) -> int64 [T];
    INT64_MAX for an invalid triangle"""
    V, T = _mesh(vertices, triangles)
    assert _f32(bounds).numel() == 6
    keys = torch.empty(T, dtype=torch.int64, device=vertices.device)
    with _Timed('cast_keys'):
        _lib.check(_lib.cast_lib().durf_cast_keys(_stream(), V, T, _z(vertices), _z(triangles), _p(bounds), _z(keys)), 'durf_cast_keys')
    return keys


def cast_build(vertices, triangles, order, ws=None):
    """durf_cast_build: the implicit tree over the permutation order [T] int32 -> the workspace (a uint8 tensor the casts read)"""
    V, T = _mesh(vertices, triangles)
    _i32(order, T, 'order')
    if ws is None:
        ws = torch.empty(cast_workspace_bytes(T), dtype=torch.uint8, device=vertices.device)
    with _Timed('cast_build'):
        _lib.check(_lib.cast_lib().durf_cast_build(_stream(), V, T, _z(vertices), _z(triangles), _z(order), _p(ws), ws.numel()), 'durf_cast_build')
    return ws


def _cast_bound(b, n, what):
    """a bound of the cast: a number -> (None, number); a tensor [n] on the device -> (tensor, 0.0)"""
    if torch.is_tensor(b):
        assert _f32(b).numel() == n, (what, tuple(b.shape), n)
        return b, 0.0
    return None, float(b)


def _cast_rays(origins, directions, tmin, tmax):
    n = int(origins.numel() // 3)
    assert _f32(origins).numel() == 3 * n == _f32(directions).numel(), (tuple(origins.shape), tuple(directions.shape))
    return (n,) + _cast_bound(tmin, n, 'tmin') + _cast_bound(tmax, n, 'tmax')


def cast_rays(ws, T, origins, directions, tmin=0.0, tmax=float('inf'), cull=0, want_bary=True):
    """durf_cast_rays: origins, directions [..., 3] against the tree in ws -> (tri int32 [...], t [...], bary [..., 3] = (w, u, v)
    or None); tmin, tmax: numbers or tensors [...] on the device.  -1 / 0 where nothing counts, -2 / NaN for an unusable ray."""
    n, tmin_a, tmin_s, tmax_a, tmax_s = _cast_rays(origins, directions, tmin, tmax)
    lead, dev = tuple(origins.shape[:-1]), origins.device
    tri, t = torch.empty(lead, dtype=torch.int32, device=dev), torch.empty(lead, device=dev)
    bary = torch.empty(lead + (3,), device=dev) if want_bary else None
    with _Timed('cast_rays'):
        _lib.check(_lib.cast_lib().durf_cast_rays(_stream(), n, _z(origins), _z(directions), _z(tmin_a), _z(tmax_a), tmin_s, tmax_s, int(cull),
                                                  int(T), _p(ws), ws.numel(), _z(tri), _z(t), _z(bary)), 'durf_cast_rays')
    return tri, t, bary


def cast_any(ws, T, origins, directions, tmin=0.0, tmax=float('inf'), cull=0):
    """durf_cast_any -> hit int32 [...]: 1 where a triangle counts, 0 where none does, -2 for an unusable ray"""
    n, tmin_a, tmin_s, tmax_a, tmax_s = _cast_rays(origins, directions, tmin, tmax)
    hit = torch.empty(tuple(origins.shape[:-1]), dtype=torch.int32, device=origins.device)
    with _Timed('cast_any'):
        _lib.check(_lib.cast_lib().durf_cast_any(_stream(), n, _z(origins), _z(directions), _z(tmin_a), _z(tmax_a), tmin_s, tmax_s, int(cull),
                                                 int(T), _p(ws), ws.numel(), _z(hit)), 'durf_cast_any')
    return hit


def cast_cameras(ws, T, cams, h, w, tmin=0.0, tmax=float('inf'), cull=0, want_bary=True):
    """durf_cast_cameras: cams [F,CAM_FLOATS] on the device, all h x w -> (tri int32 [F,h,w], depth [F,h,w], bary [F,h,w,3] or None)"""
    F, h, w, dev = _cams(cams), int(h), int(w), cams.device
    tri, depth = torch.empty(F, h, w, dtype=torch.int32, device=dev), torch.empty(F, h, w, device=dev)
    bary = torch.empty(F, h, w, 3, device=dev) if want_bary else None
    with _Timed('cast_cameras'):
        _lib.check(_lib.cast_lib().durf_cast_cameras(_stream(), F, h, w, _z(cams), float(tmin), float(tmax), int(cull), int(T), _p(ws),
                                                     ws.numel(), _z(tri), _z(depth), _z(bary)), 'durf_cast_cameras')
    return tri, depth, bary


# ---------------------------------------------------------------------------
# the closest point of a triangle mesh (include/durf_closest.h, csrc/closest.hip, libdurf_closest.so)
# ---------------------------------------------------------------------------
def closest_points(ws, T, points, max_dist=float('inf'), want_bary=True, want_point=True):
    """durf_closest_points: points [..., 3] against the tree cast_build left in ws -> (tri int32 [...], dist [...], bary [..., 3] =
    (w, u, v) or None, point [..., 3] or None).  -1 / max_dist where nothing lies within max_dist, -2 / NaN for an unusable point."""
    n = int(points.numel() // 3)
    assert _f32(points).numel() == 3 * n and points.dim() >= 1 and points.shape[-1] == 3, tuple(points.shape)
    lead, dev = tuple(points.shape[:-1]), points.device
    tri, dist = torch.empty(lead, dtype=torch.int32, device=dev), torch.empty(lead, device=dev)
    bary = torch.empty(lead + (3,), device=dev) if want_bary else None
    point = torch.empty(lead + (3,), device=dev) if want_point else None
    with _Timed('closest_points'):
        _lib.check(_lib.closest_lib().durf_closest_points(_stream(), n, _z(points), float(max_dist), int(T), _p(ws), ws.numel(), _z(tri),
                                                          _z(dist), _z(bary), _z(point)), 'durf_closest_points')
    return tri, dist, bary, point


def closest_grid(ws, T, shape, origin, du, dv, dw, max_dist=float('inf'), want_tri=True):
    """durf_closest_grid: the lattice of shape (nu, nv, nw) at origin + i du + j dv + k dw (host floats), its points generated in
    the kernel -> (dist [nu,nv,nw], tri int32 [nu,nv,nw] or None)"""
    nu, nv, nw = _dims(shape)
    dev = ws.device
    dist = torch.empty(max(nu, 0), max(nv, 0), max(nw, 0), device=dev)
    tri = torch.empty(max(nu, 0), max(nv, 0), max(nw, 0), dtype=torch.int32, device=dev) if want_tri else None
    with _Timed('closest_grid'):
        _lib.check(_lib.closest_lib().durf_closest_grid(_stream(), nu, nv, nw, *_lattice_args(origin, du, dv, dw), float(max_dist), int(T), _p(ws),
                                                        ws.numel(), _p(dist), _p(tri)), 'durf_closest_grid')
    return dist, tri


# ---------------------------------------------------------------------------
# a shaded picture of a triangle mesh (include/durf_shade.h, csrc/shade.hip, libdurf_shade.so)
# ---------------------------------------------------------------------------
def shade_surface(vertices, triangles, tri, bary, toward=None):
    """durf_shade_surface: tri int32 [...], bary [..., 3] = (w, u, v), toward [..., 3] or None -> (point [..., 3], normal [..., 3]);
    zero where the sample is not valid, a zero normal on a flat triangle"""
    V, T = _mesh(vertices, triangles)
    n, lead, dev = int(tri.numel()), tuple(tri.shape), tri.device
    _i32(tri, n, 'tri')
    assert _f32(bary).numel() == 3 * n and (toward is None or _f32(toward).numel() == 3 * n), (tuple(bary.shape), lead)
    point, normal = torch.empty(lead + (3,), device=dev), torch.empty(lead + (3,), device=dev)
    with _Timed('shade_surface'):
        _lib.check(_lib.shade_lib().durf_shade_surface(_stream(), n, V, T, _z(vertices), _z(triangles), _z(tri), _z(bary), _z(toward), _z(point),
                                                       _z(normal)), 'durf_shade_surface')
    return point, normal


def shade_occlusion(ws, T, points, normals, dirs, bias, reach, cull=0):
    """durf_shade_occlusion: points, normals [..., 3], dirs [S,3] on the device against the tree in ws -> (used, blocked) int32 [...]"""
    n = int(points.numel() // 3)
    assert _f32(points).numel() == 3 * n == _f32(normals).numel() and points.dim() >= 1 and points.shape[-1] == 3, (tuple(points.shape), tuple(normals.shape))
    assert _f32(dirs).dim() == 2 and dirs.shape[1] == 3, tuple(dirs.shape)
    lead, dev = tuple(points.shape[:-1]), points.device
    used, blocked = torch.empty(lead, dtype=torch.int32, device=dev), torch.empty(lead, dtype=torch.int32, device=dev)
    with _Timed('shade_occlusion'):
        _lib.check(_lib.shade_lib().durf_shade_occlusion(_stream(), n, _z(points), _z(normals), int(dirs.shape[0]), _z(dirs), float(bias), float(reach),
                                                         int(cull), int(T), _p(ws), ws.numel(), _z(used), _z(blocked)), 'durf_shade_occlusion')
    return used, blocked


def shade_compose(tri, normals, used, blocked, light, ambient, background, sun_blocked=None, albedo=None, want_f=True, want_u8=True):
    """durf_shade_compose: the colour of every sample -> (out_f [..., 3] or None, out_u8 uint8 [..., 3] or None); light and
    background: three host floats each"""
    n, lead, dev = int(tri.numel()), tuple(tri.shape), tri.device
    _i32(tri, n, 'tri'), _i32(used, n, 'used'), _i32(blocked, n, 'blocked')
    assert _f32(normals).numel() == 3 * n and (albedo is None or _f32(albedo).numel() == 3 * n), tuple(normals.shape)
    if sun_blocked is not None:
        _i32(sun_blocked, n, 'sun_blocked')
    out_f = torch.empty(lead + (3,), device=dev) if want_f else None
    out_u8 = torch.empty(lead + (3,), dtype=torch.uint8, device=dev) if want_u8 else None
    with _Timed('shade_compose'):
        _lib.check(_lib.shade_lib().durf_shade_compose(_stream(), n, _z(tri), _z(normals), _z(used), _z(blocked), _z(sun_blocked), _z(albedo),
                                                       _host_floats(light, 3, 'light'), float(ambient), _host_floats(background, 3, 'background'),
                                                       _z(out_f), _z(out_u8)), 'durf_shade_compose')
    return out_f, out_u8


def shade_workspace_bytes(F, h, w):
    return int(_lib.shade_lib().durf_shade_workspace_bytes(int(F), int(h), int(w)))


def shade_cameras(cast_ws, vertices, triangles, cams, h, w, dirs, bias, reach, light, sun, ambient, background, albedo_vertex=None,
                  tmin=0.0, tmax=float('inf'), cull=0, want_normal=True, want_f=True, want_u8=True, ws=None):
    """durf_shade_cameras: cams [F,CAM_FLOATS] on the device, all h x w -> dict tri, depth, normal (or None), ao_used, ao_blocked,
    out_f, out_u8 as [F,h,w(,3)]: the cast, the surface, the two occlusions and the colour in four launches"""
    V, T = _mesh(vertices, triangles)
    assert _f32(dirs).dim() == 2 and dirs.shape[1] == 3, tuple(dirs.shape)
    assert albedo_vertex is None or _f32(albedo_vertex).numel() == 3 * V, (V,)
    F, h, w, dev = _cams(cams), int(h), int(w), cams.device
    ws = _ws(ws, shade_workspace_bytes(F, h, w), dev)
    i32 = lambda: torch.empty(F, h, w, dtype=torch.int32, device=dev)
    r = dict(tri=i32(), depth=torch.empty(F, h, w, device=dev), normal=torch.empty(F, h, w, 3, device=dev) if want_normal else None,
             ao_used=i32(), ao_blocked=i32(), out_f=torch.empty(F, h, w, 3, device=dev) if want_f else None,
             out_u8=torch.empty(F, h, w, 3, dtype=torch.uint8, device=dev) if want_u8 else None)
    with _Timed('shade_cameras'):
        _lib.check(_lib.shade_lib().durf_shade_cameras(
            _stream(), F, h, w, _z(cams), float(tmin), float(tmax), int(cull), V, T, _z(vertices), _z(triangles), _p(cast_ws), cast_ws.numel(),
            int(dirs.shape[0]), _z(dirs), float(bias), float(reach), _host_floats(light, 3, 'light'), int(sun), float(ambient), _z(albedo_vertex),
            _host_floats(background, 3, 'background'), _p(ws), ws.numel(), _z(r['tri']), _z(r['depth']), _z(r['normal']), _z(r['ao_used']),
            _z(r['ao_blocked']), _z(r['out_f']), _z(r['out_u8'])), 'durf_shade_cameras')
    return r


# ---------------------------------------------------------------------------
# vertex adjacency, census, Taubin smoothing and vertex normals of a mesh (include/durf_smooth.h, csrc/smooth.hip, libdurf_smooth.so)
# ---------------------------------------------------------------------------
def smooth_keys(triangles, V):
    """durf_smooth_keys: triangles int32 [T,3] -> (edge_keys int64 [6T], corner_keys int64 [3T]), unsorted"""
    T, dev = int(triangles.shape[0]), triangles.device
    _i32(triangles, 3 * T, 'triangles')
    ek, ck = torch.empty(6 * T, dtype=torch.int64, device=dev), torch.empty(3 * T, dtype=torch.int64, device=dev)
    with _Timed('smooth_keys'):
        _lib.check(_lib.smooth_lib().durf_smooth_keys(_stream(), int(V), T, _z(triangles), _z(ek), _z(ck)), 'durf_smooth_keys')
    return ek, ck


def smooth_workspace_bytes(T):
    return int(_lib.smooth_lib().durf_smooth_workspace_bytes(int(T)))


def smooth_adjacency(edge_keys, corner_keys, V, T, ws=None):
    """durf_smooth_adjacency: the SORTED keys -> dict offsets [V+1], neighbours [6T], multiplicity [6T], corner_offsets [V+1],
    corner_tri [3T], all int32; entries past offsets[V] (corner_offsets[V]) are not written"""
    V, T, dev = int(V), int(T), edge_keys.device
    assert edge_keys.dtype == torch.int64 and edge_keys.is_contiguous() and edge_keys.numel() == 6 * T, tuple(edge_keys.shape)
    assert corner_keys.dtype == torch.int64 and corner_keys.is_contiguous() and corner_keys.numel() == 3 * T, tuple(corner_keys.shape)
    ws = _ws(ws, smooth_workspace_bytes(T), dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    r = dict(offsets=i32(V + 1), neighbours=i32(6 * T), multiplicity=i32(6 * T), corner_offsets=i32(V + 1), corner_tri=i32(3 * T))
    with _Timed('smooth_adjacency'):
        _lib.check(_lib.smooth_lib().durf_smooth_adjacency(_stream(), V, T, _z(edge_keys), _z(corner_keys), 6 * T, _p(ws), ws.numel(), _p(r['offsets']),
                                                           _z(r['neighbours']), _z(r['multiplicity']), _p(r['corner_offsets']), _z(r['corner_tri'])),
                   'durf_smooth_adjacency')
    return r


def smooth_classify(offsets, multiplicity):
    """durf_smooth_classify -> vertex_class uint8 [V]"""
    V = int(offsets.numel()) - 1
    _i32(offsets, V + 1, 'offsets')
    cls = torch.empty(V, dtype=torch.uint8, device=offsets.device)
    with _Timed('smooth_classify'):
        _lib.check(_lib.smooth_lib().durf_smooth_classify(_stream(), V, _p(offsets), _z(multiplicity), _z(cls)), 'durf_smooth_classify')
    return cls


def smooth_census(adj):
    """durf_smooth_census -> int32 [SMOOTH_CENSUS_INTS] on the device"""
    V = int(adj['offsets'].numel()) - 1
    out = torch.empty(SMOOTH_CENSUS_INTS, dtype=torch.int32, device=adj['offsets'].device)
    with _Timed('smooth_census'):
        _lib.check(_lib.smooth_lib().durf_smooth_census(_stream(), V, _p(adj['offsets']), _z(adj['neighbours']), _z(adj['multiplicity']),
                                                        _p(adj['corner_offsets']), _z(adj['vertex_class']), _p(out)), 'durf_smooth_census')
    return out


def _smooth_rows(adj, vertices, fixed):
    V = int(adj['offsets'].numel()) - 1
    assert _f32(vertices).numel() == 3 * V, (tuple(vertices.shape), V)
    assert adj['vertex_class'].dtype == torch.uint8 and adj['vertex_class'].numel() == V
    assert fixed is None or (fixed.dtype == torch.uint8 and fixed.is_contiguous() and fixed.numel() == V), (V,)
    return V


def smooth_step(adj, vertices, factor, boundary=0, fixed=None):
    """durf_smooth_step: vertices [V,3] -> a new [V,3]"""
    V = _smooth_rows(adj, vertices, fixed)
    out = torch.empty_like(vertices)
    with _Timed('smooth_step'):
        _lib.check(_lib.smooth_lib().durf_smooth_step(_stream(), V, _z(vertices), _p(adj['offsets']), _z(adj['neighbours']), _z(adj['multiplicity']),
                                                      _z(adj['vertex_class']), float(factor), int(boundary), _z(fixed), _z(out)), 'durf_smooth_step')
    return out


def smooth_taubin(adj, vertices, iters, lam, mu, boundary=0, fixed=None):
    """durf_smooth_taubin: vertices [V,3] -> a new [V,3] after iters iterations (lam then mu; mu == 0: lam alone)"""
    V = _smooth_rows(adj, vertices, fixed)
    out, tmp = torch.empty_like(vertices), torch.empty_like(vertices)
    with _Timed('smooth_taubin'):
        _lib.check(_lib.smooth_lib().durf_smooth_taubin(_stream(), V, _z(vertices), _p(adj['offsets']), _z(adj['neighbours']), _z(adj['multiplicity']),
                                                        _z(adj['vertex_class']), int(iters), float(lam), float(mu), int(boundary), _z(fixed), _z(tmp),
                                                        _z(out)), 'durf_smooth_taubin')
    return out


def smooth_normals(adj, vertices, triangles):
    """durf_smooth_normals: area-weighted vertex normals [V,3] over the corner rows of adj"""
    V, T = _mesh(vertices, triangles)
    assert adj['corner_offsets'].numel() == V + 1, (V,)
    normals = torch.empty_like(vertices)
    with _Timed('smooth_normals'):
        _lib.check(_lib.smooth_lib().durf_smooth_normals(_stream(), V, T, _z(vertices), _z(triangles), _p(adj['corner_offsets']), _z(adj['corner_tri']),
                                                         _z(normals)), 'durf_smooth_normals')
    return normals
