"""The camera row on the host: one camera is CAM_FLOATS floats -- c2w [3,4] row-major, then focal, principal point x / y,
height, width at the slots include/durf_hip.h names (THE CAMERA ROW; the constants below are generated from it).  Every module
that builds, checks or reads a row does it through here.  numpy only: the host-only modules and the commands' refusals use it
without a device."""
import numpy as np

from ._sigs import (DURF_CAM_FLOATS as CAM_FLOATS, DURF_CAM_FOCAL as CAM_FOCAL, DURF_CAM_PPX as CAM_PPX, DURF_CAM_PPY as CAM_PPY,
                    DURF_CAM_H as CAM_H, DURF_CAM_W as CAM_W)


def rows(c2w, focal, principal_point, h, w):
    """F camera-to-world matrices ([F,3,4] or [F,4,4]) -> the [F,CAM_FLOATS] float32 table.  focal, h, w: one value for all, or
    F of them; principal_point: one (x, y), or [F,2]."""
    c2w = np.stack([np.asarray(m, np.float32)[:3, :4] for m in c2w]) if len(c2w) else np.zeros((0, 3, 4), np.float32)
    out = np.zeros((c2w.shape[0], CAM_FLOATS), np.float32)
    out[:, :CAM_FOCAL] = c2w.reshape(-1, CAM_FOCAL)
    pp = np.asarray(principal_point, np.float32).reshape(-1, 2)
    out[:, CAM_FOCAL], out[:, CAM_PPX], out[:, CAM_PPY], out[:, CAM_H], out[:, CAM_W] = focal, pp[:, 0], pp[:, 1], h, w
    return out


def row(c2w, focal, principal_point, h, w):
    """one camera as its CAM_FLOATS floats"""
    return rows([c2w], focal, principal_point, h, w)[0]


def check_shape(shape, entry, frames=None):
    """the refusal of a table that is not [F,CAM_FLOATS] (frames: the F it has to have), from its shape alone"""
    shape = tuple(shape)
    if len(shape) != 2 or shape[1] != CAM_FLOATS or (frames is not None and shape[0] != frames):
        raise ValueError('%s: cams of shape %s, expected [%s,%d] camera rows (camera.rows)'
                         % (entry, shape, 'F' if frames is None else frames, CAM_FLOATS))


def as_rows(cams, entry, one_size=True, frames=None):
    """cams (numpy, a tensor or nested lists; one row or F of them) -> (float32 [F,CAM_FLOATS] contiguous host array, h, w) or
    ValueError in `entry`'s name: a table of another width, no row at all, not `frames` rows where that is given, and -- one_size
    -- rows whose heights and widths are not one pair of whole numbers.  Without one_size h, w are row 0's and the library refuses what it does not take."""
    cams = np.ascontiguousarray(cams.cpu() if hasattr(cams, 'cpu') else cams, np.float32)
    if cams.ndim == 1 and cams.size and cams.size % CAM_FLOATS == 0:
        cams = cams.reshape(-1, CAM_FLOATS)
    check_shape(cams.shape, entry, frames)
    if cams.shape[0] < 1:
        raise ValueError('%s: cams of shape %s: no camera rows' % (entry, cams.shape))
    hs, ws = np.unique(cams[:, CAM_H]), np.unique(cams[:, CAM_W])
    if one_size and (len(hs) != 1 or len(ws) != 1 or hs[0] != np.floor(hs[0]) or ws[0] != np.floor(ws[0])):
        raise ValueError('%s: the cameras of one call share one frame size, got heights %s and widths %s' % (entry, hs.tolist(), ws.tolist()))
    return (cams,) + size(cams[0])


def size(cam):
    """-> (h, w) of one row"""
    return int(cam[CAM_H]), int(cam[CAM_W])


def intrinsics(cam):
    """-> (focal, ppx, ppy, h, w) of one row, as floats"""
    return tuple(float(x) for x in cam[CAM_FOCAL:CAM_FLOATS])


def c2w(cam):
    """-> the [3,4] camera-to-world matrix of one row"""
    return np.asarray(cam[:CAM_FOCAL]).reshape(3, 4)


def scene_cameras(args, dataset, who):
    """render_traj's and fuse_tsdf's cameras -> (the dataset's rows, ext: ONE set of half extents for every frame, the first test
    image's timestep's, as the notebook renders -- boxes move, they do not resize --, and the key cameras and times of the
    synthetic sweep, else None); --cam out of range: SystemExit in `who`'s name"""
    if args.synthetic:
        cam_rows, ext = dataset.ts_data[0].cams, dataset.ext
        key_c2w, key_t = [c2w(dataset.ts_data[0].cams[0]), c2w(dataset.ts_data[-1].cams[-1])], [0.0, float(dataset.T - 1)]
    else:
        cam_rows = rows(dataset.camtoworlds, dataset.focal, dataset.principal_point, dataset.h, dataset.w)
        ext, key_c2w, key_t = dataset.peek()['ext'], None, None
    if not 0 <= args.cam < len(cam_rows):
        raise SystemExit('%s: --cam %d of %d cameras' % (who, args.cam, len(cam_rows)))
    return cam_rows, ext, key_c2w, key_t
