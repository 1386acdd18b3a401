"""The scene's boxes on rendered frames: where every box is in a picture (its twelve edges and its 2D rectangle, for any camera)
and the frames with the boxes drawn on them -- what the reference's users do by hand in notebooks/waymo_labels.ipynb
(project_point, show_camera_image) and around notebooks/durf_render_traj.ipynb, and what its data ships as 2D_boxes.npz for the
recorded images only.  The pixels are csrc/overlay.hip's (ops.project_boxes, ops.draw_boxes): one launch for the table of
segments, one for the drawing, neither waits for the device.

The lines are drawn over the picture whatever is in front of them: the rendered `distance` plane is no single depth to test
against (it sums w * t along un-normalised world directions on background rays and along unit object-frame directions on
box-hit rays).  Lines are not anti-aliased."""
import numpy as np
import torch

from . import camera, ops

# 16 colours, one per box index (K <= 16): fixed, so that box k has one colour in every picture
PALETTE = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240],
                    [240, 50, 230], [210, 245, 60], [250, 190, 212], [0, 128, 128], [220, 190, 255], [170, 110, 40],
                    [255, 250, 200], [128, 0, 0], [170, 255, 195]], np.uint8)


def _check_k(K):
    if K > ops.MAX_OBJ:
        raise ValueError('K = %d boxes: at most %d' % (K, ops.MAX_OBJ))


def project_boxes(cams, poses, ext, box_enable=None, znear=1e-2):
    """Where the boxes are in F pictures.  cams [F,CAM_FLOATS] camera rows (numpy or a tensor: camera.rows /
    camera.row), poses [F,K,6] device tensor (centre, rotation vector: render_trajectory's `poses`, or box_centers[t]
    repeated), ext [K,3] half extents, box_enable None or K values 0 / 1, znear > 0 the plane edges are clipped against.
    -> dict: segments [F,K,12,4] (x0, y0, x1, y1 per edge, NaN where culled), rect [F,K,6] (ops.BOX_RECT_FIELDS: xmin, ymin,
    xmax, ymax clipped to the picture, zc, visible), depth [F,K] (the centre's camera depth) and visible [F,K] bool."""
    if not torch.is_tensor(poses) or poses.dim() != 3 or poses.shape[2] != 6:
        raise ValueError('poses: a [F,K,6] tensor, got %s' % (tuple(getattr(poses, 'shape', ())),))
    F, K = int(poses.shape[0]), int(poses.shape[1])
    _check_k(K)
    dev = poses.device
    cams = torch.as_tensor(np.asarray(cams, np.float32) if not torch.is_tensor(cams) else cams)
    camera.check_shape(cams.shape, 'overlay.project_boxes', frames=F)
    ext = torch.as_tensor(ext)
    if tuple(ext.shape) != (K, 3):
        raise ValueError('ext: [%d,3] half extents, got %s' % (K, tuple(ext.shape)))
    if not znear > 0:
        raise ValueError('znear = %r: must be > 0' % (znear,))
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    segments, rect = ops.project_boxes(f32(cams), f32(poses), f32(ext), box_enable, znear)
    return dict(segments=segments, rect=rect, depth=rect[..., 4], visible=rect[..., 5] > 0.5)


def _colors(colors, K, dev):
    if colors is None:
        colors = PALETTE[:K]
    c = torch.as_tensor(colors)
    if tuple(c.shape) != (K, 3):
        raise ValueError('colors: [%d,3] values 0..255, got %s' % (K, tuple(c.shape)))
    return c.to(device=dev, dtype=torch.uint8).contiguous()


def draw_boxes(frames, segments, colors=None, width=1.5, opacity=1.0, label=False, inplace=False):
    """Draw project_boxes' segments as lines `width` pixels wide.  frames [F,h,w,3] uint8 or float32 on the device (float: colours
    are col / 255), segments [F,K,12,4], colors None (PALETTE) or [K,3] values 0..255, opacity in [0, 1] blends the line over the
    picture.  Where lines of several boxes meet the lowest box index wins.  -> the decorated frames (a copy unless inplace), and
    with label=True (frames, label [F,h,w] int32: the box drawn at every pixel, -1 for none)."""
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError('frames: a [F,h,w,3] tensor, got %s' % (tuple(getattr(frames, 'shape', ())),))
    if frames.dtype not in (torch.uint8, torch.float32):
        raise ValueError('frames: uint8 or float32, got %s' % (frames.dtype,))
    F, h, w = (int(n) for n in frames.shape[:3])
    if not torch.is_tensor(segments) or segments.dim() != 4 or segments.shape[0] != F or tuple(segments.shape[2:]) != (12, 4):
        raise ValueError('segments: [%d,K,12,4] for %d frames, got %s' % (F, F, tuple(getattr(segments, 'shape', ())),))
    K = int(segments.shape[1])
    _check_k(K)
    if not width >= 0 or not 0 <= opacity <= 1:
        raise ValueError('width = %r, opacity = %r: width >= 0 and 0 <= opacity <= 1' % (width, opacity))
    dev = frames.device
    col = _colors(colors, K, dev)
    if inplace and not frames.is_contiguous():
        raise ValueError('inplace: frames must be contiguous')
    out = frames if inplace else frames.contiguous().clone()
    lab = torch.empty(F, h, w, dtype=torch.int32, device=dev) if label else None
    seg = segments.to(device=dev, dtype=torch.float32).contiguous()
    if out.dtype == torch.uint8:
        ops.draw_boxes(seg, col, width / 2.0, opacity, frames8=out, label=lab)
    else:
        ops.draw_boxes(seg, col, width / 2.0, opacity, framesf=out, label=lab)
    return (out, lab) if label else out


def overlay_trajectory(out, cams, ext, box_enable=None, znear=1e-2, colors=None, width=1.5, opacity=1.0, label=False):
    """The boxes on a rendered trajectory: `out` is MipNerfModel.render_trajectory's own result (its `poses` [F,K,6] and `rgb8`
    and / or `rgb` [F,h*w,3]), cams the camera rows it was rendered from, box_enable the switch it was rendered with.
    -> dict: decorated COPIES of rgb8 / rgb in their own shapes, rect [F,K,6] (the boxes' 2D rectangles), segments, visible,
    and with label=True label [F,h,w].  Two launches and one more per picture kind; `out` is left as it is."""
    if 'poses' not in out or not ('rgb8' in out or 'rgb' in out):
        raise ValueError('out: render_trajectory\'s result with poses and rgb8 or rgb, got %s' % (sorted(out),))
    F = int(out['poses'].shape[0])
    cams_np, h, w = camera.as_rows(cams, 'overlay.overlay_trajectory', one_size=False) if F else (np.zeros((0, camera.CAM_FLOATS), np.float32), 1, 1)
    if cams_np.shape[0] != F:
        raise ValueError('%d camera rows for %d frames' % (cams_np.shape[0], F))
    proj = project_boxes(cams_np, out['poses'], ext, box_enable, znear)
    res = dict(rect=proj['rect'], segments=proj['segments'], visible=proj['visible'])
    want_label = label
    for name in ('rgb8', 'rgb'):
        if name not in out:
            continue
        pic = out[name]
        if pic.numel() != F * h * w * 3:
            raise ValueError('%s %s against %d frames of %d x %d' % (name, tuple(pic.shape), F, h, w))
        drawn = draw_boxes(pic.reshape(F, h, w, 3), proj['segments'], colors, width, opacity, label=want_label)
        if want_label:
            drawn, res['label'] = drawn
            want_label = False
        res[name] = drawn.reshape(pic.shape)
    return res
