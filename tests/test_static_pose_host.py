"""dynamics=False with box-pose optimisation on the host side: the knob check and the C ABI's new entry point (no GPU)."""
import os

import pytest

from durf_amd import _lib, _sigs, obbpose_model, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**kw):
    utils.clear_gin()
    utils.parse_gin(''.join('MipNerfModel.%s = %s\n' % (k, ('"%s"' % v) if isinstance(v, str) else v) for k, v in kw.items()))
    return utils.configured(obbpose_model.MipNerfModel)


@pytest.mark.parametrize('precision', ['bf16', 'f32'])
@pytest.mark.parametrize('obj', ['auto', 'bf16', 'f32'])
@pytest.mark.parametrize('no_pose,no_yaw', [(False, False), (True, False), (False, True)])
def test_static_boxes_with_pose_optimisation_are_accepted(precision, obj, no_pose, no_yaw):
    m = _model(dynamics=False, no_pose_opt=no_pose, no_yaw_opt=no_yaw, mlp_precision=precision, obj_precision=obj)
    m._check()
    assert m.static_hit_f32(3) == (precision == 'bf16' and obj != 'bf16')
    assert not m.static_hit_f32(0)


def test_split_bf16_objects_are_refused_with_static_boxes_and_pose_optimisation():
    with pytest.raises(NotImplementedError, match='bf16x3'):
        _model(dynamics=False, no_pose_opt=False, no_yaw_opt=True, obj_precision='bf16x3')._check()
    _model(dynamics=False, no_pose_opt=True, no_yaw_opt=True, obj_precision='bf16x3')._check()      # frozen poses: as before
    with pytest.raises(NotImplementedError):
        _model(dynamics=False, no_pose_opt=False, stop_level_grad=False)._check()
    assert not _model(dynamics=True, no_pose_opt=False).static_hit_f32(3)


def test_the_entry_point_is_declared_bound_and_exported():
    name = 'durf_encode_bkgd_bwd_batch'
    assert name in open(os.path.join(ROOT, 'include', 'durf_hip.h')).read()
    assert name in open(os.path.join(ROOT, 'include', 'durf_ctypes_stub.py')).read()
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert name in _sigs.SIGS and name in _lib.symbols()
    assert hasattr(_lib.lib(), name)
    assert _lib.lib().durf_version() == 41
