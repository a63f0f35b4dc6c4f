"""pdfnet_amd/taped.py, the host half (no GPU needed): `tape_state` -- everything a recorded tape bakes into its arguments beyond its key --
changes with every item the module docstring names and with nothing else, and `TapedSegment._revalidate` drops the tapes and checks
the parameters again when it has changed."""
import pytest
import torch
import torch.nn as nn

from pdfnet_amd import functional as F
from pdfnet_amd import taped
from pdfnet_amd.networks import layers
from pdfnet_amd.networks.layers import BatchNorm


class _Block(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv, self.bn = layers.Conv2d(c, c, 3), BatchNorm(c)


def _stages():
    """Two stand-in stages whose parameters look Trainer-owned: data and gradients are views into two flat buffers."""
    torch.manual_seed(0)
    mods = [_Block(4), _Block(8)]
    adopt(mods)
    return [p for m in mods for p in m.parameters()], [m.bn for m in mods], mods


def adopt(mods):
    """What FlatAdam.__init__ does to the parameters: fresh flat buffers, `p.data` and `p.grad` re-pointed into them."""
    ps = [p for m in mods for p in m.parameters()]
    n = sum(p.numel() for p in ps)
    flat_p, flat_g, o = torch.zeros(n), torch.zeros(n), 0
    for p in ps:
        k = p.numel()
        view = flat_p[o:o + k].view(p.shape)
        view.copy_(p.data)
        p.data = view
        p.grad = flat_g[o:o + k].view(p.shape)
        p._pdf_main_grad = True
        o += k
    return flat_p, flat_g


@pytest.fixture
def x3(monkeypatch):
    mode = [7]
    monkeypatch.setattr(taped, '_x3_mode', lambda: mode[0])
    return mode


def test_tape_state_ignores_what_the_kernels_read_through_the_addresses(x3, monkeypatch):
    ps, bns, mods = _stages()
    s0 = taped.tape_state(ps, bns)
    assert s0 == taped.tape_state(ps, bns) and hash(s0) == hash(taped.tape_state(ps, bns))
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                p.mul_(1.5)                                      # an optimizer step, a checkpoint loaded in place
                p.grad.add_(1.0)                                 # a backward pass
                p.grad.zero_()
            for b in m.buffers():
                b.add_(1)                                        # running statistics, num_batches_tracked
    sd = {k: torch.full_like(v, 0.25) for k, v in mods[0].state_dict().items()}
    mods[0].load_state_dict(sd)                                  # copies in place
    bns[0]._pending += 1
    for m in mods:
        m.eval()
        m.train()
    monkeypatch.setattr(F, 'MESH_FUSED', not F.MESH_FUSED)       # a switch no trunk Function reads
    assert taped.tape_state(ps, bns) == s0


@pytest.mark.parametrize('switch', ['WINOGRAD', 'WINOGRAD_KEEP_V', 'BN_EPILOGUE_STATS', 'BN_EPILOGUE_STATS_BF16', 'ASYNC_WGRAD_MIN_FLOP'])
def test_tape_state_follows_every_module_switch(x3, monkeypatch, switch):
    ps, bns, mods = _stages()
    s0 = taped.tape_state(ps, bns)
    assert switch in taped.SWITCHES
    old = getattr(F, switch)
    monkeypatch.setattr(F, switch, 1e9 if switch == 'ASYNC_WGRAD_MIN_FLOP' else (True if old == 'auto' else not old))
    assert getattr(F, switch) != old
    s1 = taped.tape_state(ps, bns)
    assert s1 != s0
    monkeypatch.setattr(F, switch, old)
    assert taped.tape_state(ps, bns) == s0


def test_tape_state_follows_the_x3_mode(x3):
    ps, bns, mods = _stages()
    seen = {}
    for mode in (7, 0, 1, 6):
        x3[0] = mode
        seen[mode] = taped.tape_state(ps, bns)
    assert len(set(seen.values())) == 4
    x3[0] = 7
    assert taped.tape_state(ps, bns) == seen[7]


def test_tape_state_follows_every_parameter(x3):
    """Per parameter -- each one of them, the last as well as the first: the address of the data, the address of the gradient, requires_grad."""
    ps, bns, mods = _stages()
    s0 = taped.tape_state(ps, bns)
    assert len(ps) == 8                                          # 2 x (conv weight, conv bias, bn weight, bn bias)
    for p in ps:
        data, grad = p.data, p.grad
        p.data = data.clone()
        assert taped.tape_state(ps, bns) != s0
        p.data = data
        assert taped.tape_state(ps, bns) == s0
        p.grad = grad.clone()
        assert taped.tape_state(ps, bns) != s0
        p.grad = None                                            # model.zero_grad(): nothing for the kernels to accumulate into
        assert taped.tape_state(ps, bns) != s0
        p.grad = grad
        assert taped.tape_state(ps, bns) == s0
        p.requires_grad_(False)
        assert taped.tape_state(ps, bns) != s0
        p.requires_grad_(True)
        assert taped.tape_state(ps, bns) == s0


def test_tape_state_follows_a_second_trainer(x3):
    ps, bns, mods = _stages()
    s0 = taped.tape_state(ps, bns)
    keep = adopt(mods)                                           # same values, same modules, new buffers
    s1 = taped.tape_state(ps, bns)
    x3_mode, trainers, switches, data, grads, requires_grad, hyper = range(7)
    assert s1 != s0 and all(s1[k] == s0[k] for k in (x3_mode, trainers, switches, requires_grad, hyper))
    assert all(a != b for a, b in zip(s0[data], s1[data])) and all(a != b for a, b in zip(s0[grads], s1[grads]))
    del keep
    # ... and the count of FlatAdams alone, which also covers parameters that a module swap has taken out of the segment's reach
    taped.new_trainer()
    s2 = taped.tape_state(ps, bns)
    assert s2 != s1 and all(s2[k] == s1[k] for k in range(7) if k != trainers)


def test_tape_state_follows_batchnorm_hyperparameters(x3):
    ps, bns, mods = _stages()
    s0 = taped.tape_state(ps, bns)
    for b in bns:
        for name, v in (('momentum', 0.5), ('eps', 1e-3)):
            old = getattr(b, name)
            setattr(b, name, v)
            assert taped.tape_state(ps, bns) != s0
            setattr(b, name, old)
            assert taped.tape_state(ps, bns) == s0


def test_segment_drops_its_tapes_and_rechecks_the_parameters_when_the_state_changes(x3):
    ps, bns, mods = _stages()
    seg = taped.TapedSegment([lambda x: x, lambda x: x], mods)
    assert seg._revalidate() and seg._params_ok
    pinned = torch.zeros(3)
    seg.entries['k'] = {'busy': False, 'pins': [pinned], 'pinned_bytes': 12}
    assert seg._revalidate() and list(seg.entries) == ['k']     # nothing changed: the tape stays
    with torch.no_grad():
        mods[0].conv.weight.mul_(2.0)
    assert seg._revalidate() and list(seg.entries) == ['k']     # weights changed in place: the tape stays
    # a second trainer: the tapes go, and the new parameters are looked at again
    adopt(mods)
    assert seg._revalidate() and not seg.entries and seg.pinned_bytes() == 0
    seg.entries['k'] = {'busy': False, 'pins': [pinned], 'pinned_bytes': 12}
    # ... which finds a parameter that is no trainer's
    w = mods[1].conv.weight
    w.data = w.data.clone()
    w._pdf_main_grad = False
    assert not seg._revalidate() and not seg.entries and not seg._params_ok
    assert not seg._revalidate()                                 # and keeps looking while that is so
    w._pdf_main_grad = True
    assert seg._revalidate() and seg._params_ok
    # every other item: one tape dropped per change
    changes = [lambda: x3.__setitem__(0, 0), lambda: setattr(bns[1], 'momentum', 0.5), lambda: setattr(bns[0], 'eps', 1e-3),
               lambda: mods[0].conv.weight.requires_grad_(False), lambda: setattr(w, 'grad', w.grad.clone())]
    for change in changes:
        seg.entries['k'] = {'busy': False, 'pins': [pinned], 'pinned_bytes': 12}
        assert seg._revalidate() and seg.entries
        change()
        assert seg._revalidate() and not seg.entries
