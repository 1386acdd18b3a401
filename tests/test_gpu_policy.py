"""Both orchestrations of a training step -- the Python-issued launches (train_boxpose.train_step) and the one C call
(train_step_one_call, csrc/train.hip) -- take the launch policy of the bf16 object work from ONE function (durf_step_policy,
csrc/policy.h): under every switch they dispatch the same kernel variants, those variants are the ones the policy names, and
the gradient is the same to the bit (no switch changes a result).  The threshold's far side is
tests/test_gpu_train.py::test_side_stream_modes_give_the_same_parameters and tests/test_gpu_fullsize.py."""
import pytest
import torch

from durf_amd import obbpose_model, ops, synthetic, train_boxpose, utils
from tests import helpers as H

pytestmark = pytest.mark.gpu

B, K, N = 32, 2, 32              # 2 levels of 1024 sample rows: far below DURF_OVERLAP_MIN_ROWS
OBJ = {'FWD_MIX', 'BWD_MIX', 'FWD128_MSPLIT', 'BWD128_MSPLIT', 'FWD128_SAMPLE', 'BWD128_SAMPLE'}


@pytest.fixture(scope='module')
def reference():
    """holds the first case's gradient (the default policy's, in file order) for the cases after it"""
    return {}


@pytest.mark.parametrize('env,want', [
    ({}, {'FWD_MIX', 'BWD_MIX'}),
    ({'DURF_OBJ_MIX': '0'}, {'FWD128_MSPLIT', 'BWD128_MSPLIT'}),
    ({'DURF_OBJ_MSPLIT': '0'}, {'FWD128_SAMPLE', 'BWD128_SAMPLE'}),
    ({'DURF_OVERLAP_OBJECTS': '2'}, {'FWD128_MSPLIT', 'BWD128_MSPLIT'}),
], ids=['default', 'mix0', 'msplit0', 'overlap2'])
def test_both_orchestrations_follow_the_policy(cuda, monkeypatch, reference, env, want):
    for k in ('DURF_OVERLAP_OBJECTS', 'DURF_OBJ_MSPLIT', 'DURF_OBJ_MIX'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = ops.step_policy(B * N)
    named = ({'FWD_MIX', 'BWD_MIX'} if p.mix else {'FWD128_MSPLIT', 'BWD128_MSPLIT'} if p.msplit else {'FWD128_SAMPLE', 'BWD128_SAMPLE'})
    assert named == want, p
    utils.clear_gin()
    utils.parse_gin('MipNerfModel.num_samples = %d\nMipNerfModel.num_levels = 2\nMipNerfModel.density_noise = 0.0\n'
                    'MipNerfModel.obj_precision = "bf16"\nMipNerfModel.no_pose_opt = True\nMipNerfModel.no_yaw_opt = True\n'
                    'Config.randomized = False\nConfig.rand_bkgd = False\n' % N)
    config = utils.configured(utils.Config)
    db = H.device_batch(synthetic.make_batch(B, K, seed=35), cuda)
    prev = db['init'][0:1]
    seen, flat = {}, {}
    for fn in (train_boxpose.train_step, train_boxpose.train_step_one_call):
        model, variables = obbpose_model.construct_mipnerf(4, db, device=cuda)
        state = train_boxpose.create_train_state(variables)
        ops.dispatch_reset()
        state, stats, _, _ = fn(model, config, 0, state, db, 5e-4, 3.0, 10.0, prev)
        torch.cuda.synchronize()
        seen[fn.__name__], flat[fn.__name__] = ops.dispatch_seen(), state.variables.flat.clone()
    assert seen['train_step'] == seen['train_step_one_call'], seen
    assert seen['train_step'] & OBJ == want, seen
    assert torch.equal(flat['train_step'], flat['train_step_one_call']), 'parameters after one step'
    # the gradient itself: loss_and_grad against durf_loss_backward, and against the default policy's
    model, variables = obbpose_model.construct_mipnerf(4, db, device=cuda)
    g_py, _, _ = train_boxpose.loss_and_grad(model, config, 0, variables, db, 3.0, 10.0, prev)
    g_c, _, _ = train_boxpose.train_step_one_call(model, config, 0, train_boxpose.create_train_state(variables), db, 5e-4, 3.0, 10.0,
                                                  prev, update=False)
    torch.cuda.synchronize()
    assert g_py.abs().max() > 0 and torch.equal(g_py, g_c), 'Python-issued step against the one C call'
    ref = reference.setdefault('grad', g_py.clone())
    assert torch.equal(g_py, ref), 'against the default policy'
