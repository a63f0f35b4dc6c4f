"""layers.freeze_batchnorm: the module-surface half of BatchNorm with frozen statistics (no GPU needed: modes and keys only)."""
import torch.nn as nn

from pdfnet_amd.networks import layers
from pdfnet_amd.networks.layers import BatchNorm, freeze_batchnorm


def _net():
    inner = nn.Sequential(layers.Linear(8, 8), BatchNorm(8), nn.Dropout(0.5))
    return nn.Sequential(layers.Conv2d(3, 8, 3), BatchNorm(8), inner, layers.LayerNorm(8))


def _bns(m):
    return [b for b in m.modules() if isinstance(b, BatchNorm)]


def test_frozen_batchnorm_survives_train():
    m = _net().train()
    assert freeze_batchnorm(m) is m
    assert len(_bns(m)) == 2 and not any(b.training for b in _bns(m))
    m.train()
    assert not any(b.training for b in _bns(m))
    # everything else follows the model: only the BatchNorms are held back
    assert m.training and m[2].training and m[2][2].training and m[0].training and m[3].training
    m.eval()
    m.train(True)
    m[2].train()
    assert not any(b.training for b in _bns(m))
    # the affine parameters stay trainable
    assert all(b.weight.requires_grad and b.bias.requires_grad for b in _bns(m))


def test_freeze_batchnorm_false_thaws():
    m = _net().train()
    freeze_batchnorm(m)
    freeze_batchnorm(m, False)
    assert all(b.training for b in _bns(m))              # takes the mode of the module it was called on
    m.eval()
    assert not any(b.training for b in _bns(m))
    m.train()
    assert all(b.training for b in _bns(m))
    m.eval()
    freeze_batchnorm(m)
    freeze_batchnorm(m, False)
    assert not any(b.training for b in _bns(m))
    # a sub-tree only
    m.train()
    freeze_batchnorm(m[2])
    assert m[1].training and not m[2][1].training
    m.train()
    assert m[1].training and not m[2][1].training


def test_unmarked_modules_follow_train_and_eval_as_before():
    m = _net()
    for mode in (True, False, True):
        m.train(mode)
        assert all(x.training == mode for x in m.modules())
    m.eval()
    assert not any(x.training for x in m.modules())
    b = BatchNorm(4)
    assert b.train() is b and b.training and b.eval() is b and not b.training


def test_state_dict_keys_are_unchanged_by_freezing():
    a, b = _net(), _net()
    freeze_batchnorm(b)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert sorted(k for k in b[1].state_dict()) == ['bias', 'num_batches_tracked', 'running_mean', 'running_var', 'weight']
    assert [n for n, _ in a.named_buffers()] == [n for n, _ in b.named_buffers()]
    a.load_state_dict(b.state_dict())                    # strict: no key of the frozen model is unknown to the plain one
    b.load_state_dict(a.state_dict())
    assert not any(x.training for x in _bns(b))          # loading does not thaw
