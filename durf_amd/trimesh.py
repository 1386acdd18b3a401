"""The triangle mesh on the host: the dict vertices [V,3], triangles [T,3] (plus per-vertex arrays) that raster, cast, closest,
shade and geometry take (csrc/triangles.h is the device side).  Every module that refuses a mesh, uploads one or
prepares its per-vertex attributes does it here, under its own entry name.  numpy only at import."""
import numpy as np


def shapes(m, entry):
    """the dict and shape refusals -> (V, T)"""
    if not isinstance(m, dict) or m.get('vertices') is None or m.get('triangles') is None:
        raise ValueError('%s: m is a dict with vertices [V,3] and triangles [T,3]' % entry)
    vs, ts = tuple(m['vertices'].shape), tuple(m['triangles'].shape)
    if len(vs) != 2 or vs[1] != 3 or len(ts) != 2 or ts[1] != 3:
        raise ValueError('%s: vertices of shape %s and triangles of shape %s, expected [V,3] and [T,3]' % (entry, vs, ts))
    return vs[0], ts[0]


def limits(V, T, entry, max_triangles=2 ** 31, words='the limit is 2^31 - 1'):
    """fewer than 2^31 vertices and fewer than max_triangles triangles; words: how the caller states its limit"""
    if V >= 2 ** 31 or T >= max_triangles:
        raise ValueError('%s: %d vertices and %d triangles, %s' % (entry, V, T, words))


def arrays(m, entry, *limit):
    """every refusal of a mesh dict, before anything touches the device -> (V, T); limit: limits()'s max_triangles and words.
    (render_mesh calls the two halves itself: it refuses its cameras between them.)"""
    V, T = shapes(m, entry)
    limits(V, T, entry, *limit)
    return V, T


def check_attrs(attrs, entry, of='the mesh'):
    if isinstance(attrs, str) or not all(isinstance(a, str) for a in attrs):
        raise ValueError('%s: attrs = %r, expected a tuple of keys of %s' % (entry, attrs, of))


def check_attribute_rows(m, attrs, label, V, entry):
    """every attribute key and the label: a string, and as many rows as vertices where m holds it"""
    for key in tuple(attrs) + ((label,) if label is not None else ()):
        if not isinstance(key, str):
            raise ValueError('%s: label = %r, expected a key of m or None' % (entry, key))
        a = m.get(key)
        if a is not None and a.shape[0] != V:
            raise ValueError('%s: m[%r] has %d rows for %d vertices' % (entry, key, a.shape[0], V))


def device_of(a):
    """where a (a mesh's vertices, a plane of samples) is if that is a device, else the current device"""
    import torch
    return a.device if torch.is_tensor(a) and a.is_cuda else torch.device('cuda', torch.cuda.current_device())


def upload(a, dtype, dev):
    """a host array (converted by numpy: whatever numpy takes) or a tensor -> a contiguous tensor of dtype on dev"""
    import torch
    if not torch.is_tensor(a):
        a = np.ascontiguousarray(a, dtype=str(dtype).split('.')[-1])
    return torch.as_tensor(a).to(device=dev, dtype=dtype).contiguous()


def on_device(m, V, T, dev):
    """-> (vertices float32 [V,3], triangles int32 [T,3]) on dev"""
    import torch
    return upload(m['vertices'], torch.float32, dev).reshape(V, 3), upload(m['triangles'], torch.int32, dev).reshape(T, 3)


def vertex_attributes(m, attrs, label, V, dev):
    """The per-vertex arrays of m as durf_raster_interp takes them -> (dict: every key of attrs that m holds as float32 [V,C], a
    uint8 colour counting as / 255; m[label] as int32 [V], or None when there is no label or m lacks it)"""
    import torch
    fattrs = {}
    for key in attrs:
        a = m.get(key)
        if a is not None:
            scale = 1.0 / 255.0 if (a.dtype == np.uint8 or a.dtype == torch.uint8) else 1.0
            fattrs[key] = (upload(a, torch.float32, dev).reshape(V, -1) * scale).contiguous()
    lab = upload(m[label], torch.int32, dev).reshape(V) if label is not None and m.get(label) is not None else None
    return fattrs, lab
