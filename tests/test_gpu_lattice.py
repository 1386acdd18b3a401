"""One lattice, five libraries (csrc/lattice.h): field, closest, tsdf, mesh and parts take the same LatticeDims and
LatticeFrame by value, decode g with the same function and place a point with the same rule.  Each is run on the same three
shapes -- (2, 2, 2), the minimum; (3, 4, 5), no dimension equal to another and none a multiple of a tile (8 / 4) or a brick (4);
(5, 3, 67), 1005 points: four workgroups of 256 with a partial last one, nw no multiple of 4 or 8 -- over one skewed, left-handed
frame with non-dyadic float32 components, and held to tests/lattice_ref.py through its own oracle, by the rule its own test file
already uses: a member that moved in one kernel's argument struct, or a decode that drifted, shows as wrong bits here."""
import numpy as np
import pytest
import torch

from durf_amd import cast, closest, field, lattice, mesh, parts, tsdf
from tests import cast_ref, lattice_ref, mesh_ref, parts_ref, tsdf_ref
from tests.test_gpu_field import _scene
from tests.test_gpu_mesh import _gate

pytestmark = pytest.mark.gpu
F32 = np.float32
SHAPES = ((2, 2, 2), (3, 4, 5), (5, 3, 67))


def _frame(shape):
    """about 2.3 scene units along every axis around the origin; the axes lean off x, z, y: skewed and left-handed"""
    s = [2.3 / (n - 1) for n in shape]
    axes = np.array([[1.0 * s[0], 0.07 * s[0], -0.04 * s[0]], [-0.06 * s[1], 0.08 * s[1], 1.0 * s[1]], [0.05 * s[2], 1.0 * s[2], -0.03 * s[2]]])
    origin = np.array([0.013, -0.021, 0.017]) - sum(0.5 * (n - 1) * a for n, a in zip(shape, axes))
    return lattice_ref.frame_of(origin, axes=axes)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).reshape(-1).view(np.int32)


def _density(shape):
    """random signs times random magnitudes: a surface through every cell; on the larger shapes one NaN and one invalid point"""
    rng = np.random.default_rng(sum(shape))
    d = mesh_ref.sign_field(shape, 3) * rng.uniform(0.1, 3.0, shape).astype(F32)
    v = None
    if d.size > 8:
        v = np.ones(shape, np.uint8)
        v[1, 1, 2], d[2, 1, 3] = 0, np.nan
    return d, v


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_the_frame_is_awkward(shape):
    frame = _frame(shape)
    assert lattice.host(frame, 'test')[5], 'left-handed'
    P32, P64 = lattice_ref.points(frame, shape, F32), lattice_ref.points(frame, shape, np.float64)
    assert (P32 != P64.astype(F32)).any() or shape == (2, 2, 2), 'float32 in the stated order is not float64 rounded'
    assert all(float(F32(x)) != x for k in ('origin', 'du', 'dv', 'dw') for x in frame[k]), 'no component is a float32'


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_field_grid_points(cuda, shape):
    s, frame = _scene(cuda), _frame(shape)
    g = field.grid(s['model'], s['variables'], frame['origin'], shape, axes=(frame['du'], frame['dv'], frame['dw']), view=(0.6, -0.64, 0.48),
                   ext=s['ext'], box_enable=s['en'], chunk=300, want_points=True)
    assert tuple(g['points'].shape) == shape + (3,)
    assert np.array_equal(_bits(g['points']), _bits(lattice_ref.points(frame, shape, F32)))


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_closest_grid_is_closest_points_at_the_lattice(cuda, shape):
    frame = _frame(shape)
    v, t = cast_ref.icosphere(2)
    b = cast.build(dict(vertices=v, triangles=t))
    g = closest.grid(b, frame['origin'], shape, 1.0, axes=[frame['du'], frame['dv'], frame['dw']])
    assert all(np.array_equal(_bits(g['frame'][k]), _bits(np.asarray(frame[k], F32))) for k in ('origin', 'du', 'dv', 'dw'))
    r = closest.points(b, lattice_ref.points(frame, shape, F32))
    assert tuple(g['density'].shape) == shape
    assert np.array_equal(_bits(g['density']), _bits(r['dist'])) and torch.equal(g['tri'].reshape(-1), r['tri'])


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_tsdf_integrate_of_one_frame(cuda, shape):
    """the rule of tests/test_gpu_tsdf.py: tsdf, weight and colour EQUAL integrate32, as int32 bits"""
    frame = _frame(shape)
    h, w = 20, 28
    cams = tsdf_ref.ring_cameras(1, h, w, 14.0, radius=4.0, height=0.7, phase=0.4)
    depth = tsdf_ref.sphere_depth(cams, h, w)
    rgb = np.random.default_rng(sum(shape)).random((1, h, w, 3)).astype(F32)
    vol = tsdf.volume(frame['origin'], shape, axes=(frame['du'], frame['dv'], frame['dw']), trunc=0.4, device=cuda)
    tsdf.integrate(vol, cams, depth, rgb=rgb)
    want = tsdf_ref.integrate32(tsdf_ref.new_state(shape), frame, shape, cams, depth, 0.4, rgb=rgb)
    assert (want['why'] == 0).sum() >= 2, 'some voxels are updated'
    for k in ('tsdf', 'weight', 'colour'):
        assert np.array_equal(_bits(vol[k]), _bits(want[k])), k


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_mesh_surface_and_parts_components(cuda, shape):
    frame = _frame(shape)
    d, v = _density(shape)
    g = dict(density=torch.as_tensor(d).to(cuda), valid=None if v is None else torch.as_tensor(v).to(cuda), frame=frame)
    m = mesh.surface(g, 0.0)
    top = mesh_ref.topology(d, v, 0.0, flip=True)
    ve = m['vertex_edge'].cpu().numpy()
    assert ve.shape[0] > 0 and np.array_equal(ve, top['vertex_edge']) and np.array_equal(m['triangles'].cpu().numpy(), top['triangles'])
    t, X, _ = mesh_ref.geometry(d, v, 0.0, frame, ve, F32, normals=False)
    assert np.array_equal(_bits(m['vertex_t']), _bits(t)) and np.array_equal(_bits(m['vertices']), _bits(X))
    # the normal transform travels in a struct of its own: the normals at tests/test_gpu_mesh.py's gate (a unit vector: ulps of 1)
    _gate(m['normals'].cpu().numpy(), mesh_ref.geometry(d, v, 0.0, frame, ve)[2], mesh_ref.geometry(d, v, 0.0, frame, ve, F32)[2], 1.0, 'normals')
    p, want = parts.components(g, 0.0), parts_ref.components(d, v, 0.0)
    assert p['n'] == want['count'] and np.array_equal(p['labels'].cpu().numpy(), want['labels']) and np.array_equal(p['comp'].cpu().numpy(), want['comp'])
    assert np.array_equal(p['size'].cpu().numpy(), want['size']) and np.array_equal(p['bbox'].cpu().numpy(), want['bbox'])
