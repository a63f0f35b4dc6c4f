"""Stale replays of the taped trunk (pdfnet_amd/taped.py): a tape holds raw device addresses, workspace sizes and offsets, option structures
and scalar hyper-parameters, and is found by the input's signature alone -- so every test here records a tape, changes something the
recording pass read, and calls the trunk again.  The reference is always the EAGER trunk in the same process and state (tape switched off,
segment put aside), which tests/test_full_gradient_gpu.py pins to the float64 oracle; the comparison is bit for bit (`torch.equal`) over
the four outputs, the input gradient, the whole flat gradient buffer and every buffer of the trunk (running statistics, batch counters).
One external gradient per output, so no fan-in order can differ."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X_SMALL = (4, 64, 32, 32)
X_WINOGRAD = (8, 64, 64, 64)                                     # layer 2's 128-channel 3x3 convolutions on 32x32 maps take F(4x4): 36 x 512 tiles


class _Trunk:
    """The trunk of one model under one trainer at a time, called taped and eager from the same state."""

    def __init__(self, tr, m, shape, set_tape):
        self.tr, self.m, self.enc, self.set_tape = tr, m, m.encoder, set_tape
        m.train()
        r = self.enc.resnet
        self.layers = [r.layer1, r.layer2, r.layer3, r.layer4]
        self.bufs = [b for l in self.layers for b in l.buffers()]
        torch.manual_seed(5)
        self.x = torch.randn(*shape, device='cuda').contiguous(memory_format=torch.channels_last)
        self.gs = None
        self.set_tape(True)
        self.enc.__dict__.pop('_trunk_seg', None)

    @property
    def seg(self):
        return self.enc.__dict__['_trunk_seg']

    def call(self):
        """One forward and backward from zeroed gradients -> (outputs, dx, flat_g, buffers), all cloned."""
        from pdfnet_amd import functional as F
        from pdfnet_amd.networks.layers import BatchNorm
        self.tr.optimizer.zero_grad()
        xr = self.x.clone().requires_grad_()
        outs = self.enc.trunk_layers(xr)
        if self.gs is None:
            torch.manual_seed(1)
            self.gs = [torch.randn_like(o) for o in outs]
        torch.autograd.backward(outs, self.gs)
        F.join_wgrad()
        BatchNorm.flush_counters()
        torch.cuda.synchronize()
        return [o.detach().clone() for o in outs], xr.grad.clone(), self.tr.optimizer.flat_g.clone(), [b.clone() for b in self.bufs]

    def eager(self):
        seg = self.enc.__dict__.pop('_trunk_seg')
        self.set_tape(False)
        try:
            return self.call()
        finally:
            self.set_tape(True)
            self.enc.__dict__['_trunk_seg'] = seg

    def both(self):
        """-> (taped, eager) results of the same call from the same state; the taped call must have gone through a tape."""
        saved = [b.clone() for b in self.bufs]
        got = self.call()
        assert len(self.seg.entries) >= 1 and all(self.seg.entries.values()), "the trunk was not taped"
        for b, v in zip(self.bufs, saved):
            b.copy_(v)
        return got, self.eager()


def _same(got, ref):
    """Which parts are bit-identical: outputs, dx, flat_g, buffers."""
    return {'outs': all(torch.equal(a, b) for a, b in zip(got[0], ref[0])), 'dx': torch.equal(got[1], ref[1]),
            'flat_g': torch.equal(got[2], ref[2]), 'bufs': all(torch.equal(a, b) for a, b in zip(got[3], ref[3])),
            'live': float(ref[2].abs().max()) > 0 and float(ref[1].abs().max()) > 0}


ALL_SAME = {'outs': True, 'dx': True, 'flat_g': True, 'bufs': True, 'live': True}


def _trunk(monkeypatch, shape=X_SMALL, lr=1e-4):
    from pdfnet_amd import taped
    from pdfnet_amd.trains.base_trainer import Trainer
    from tests.test_trainer_gpu import _setup
    opt, m, crit, batch = _setup(R=128, B=2)
    tr = Trainer(opt, m, crit, lr=lr)
    t = _Trunk(tr, m, shape, lambda on: monkeypatch.setattr(taped, 'TRUNK_TAPE', on))
    return t, opt, crit, batch


def _flat_range(optimizer, params):
    """Flat offsets [lo, hi) of each of `params` in the optimizer's buffers."""
    pos = {id(p): i for i, p in enumerate(optimizer.params)}
    return [(optimizer.offsets[pos[id(p)]], optimizer.offsets[pos[id(p)]] + p.numel()) for p in params]


def test_weights_changed_in_place_are_followed_by_the_tape(monkeypatch):
    """Case a: what the kernels read THROUGH the recorded addresses may change -- a state dict loaded in place, an optimizer step.  The tape
    stays (the very same entry is replayed) and equals eager with the new weights, running statistics included."""
    from oracle import synth
    from pdfnet_amd import taped
    t, opt, crit, batch = _trunk(monkeypatch, lr=1e-3)
    t.call()                                                     # records, replays
    entry, = t.seg.entries.values()
    assert _same(*t.both()) == ALL_SAME                          # second replay
    # pinned_bytes() counts the whole entry: the pins and the buffers the replay copies its input and output gradients into
    assert t.seg.pinned_bytes() == taped._storage_bytes(entry) == taped._storage_bytes([entry[k] for k in ('pins', 'x', 'outs', 'gouts', 'gx')])
    assert t.seg.pinned_bytes() >= taped._storage_bytes([entry[k] for k in ('x', 'outs', 'gouts', 'gx')]) > 0
    before = t.eager()
    t.m.load_state_dict(synth.det_state_dict(t.m.state_dict(), salt=11))
    got, ref = t.both()
    assert _same(got, ref) == ALL_SAME
    assert not torch.equal(ref[0][0], before[0][0]) and not torch.equal(ref[2], before[2])       # the new weights were seen
    p0 = t.tr.optimizer.flat_p.clone()
    loss = float(t.tr.train_step(batch, 0))                      # one step at lr = 1e-3 (it records the step's own signature beside this one)
    assert loss == loss
    torch.cuda.synchronize()
    w = t.layers[2][0].conv2.weight
    (lo, hi), = _flat_range(t.tr.optimizer, [w])
    assert not torch.equal(p0[lo:hi], t.tr.optimizer.flat_p[lo:hi])
    got2, ref2 = t.both()
    assert _same(got2, ref2) == ALL_SAME
    assert not torch.equal(ref2[0][0], ref[0][0])
    assert any(e is entry for e in t.seg.entries.values())       # never re-recorded: the copies were in place


def test_second_trainer_on_the_same_model_gets_its_own_tape(monkeypatch):
    """Case b: a second Trainer re-points every parameter and gradient at its own flat buffers.  The tape of the first one reads the old
    weights and accumulates into the old gradient buffer: the new optimizer would see zeros for the whole trunk."""
    from pdfnet_amd.trains.base_trainer import Trainer
    t, opt, crit, _ = _trunk(monkeypatch)
    tr1 = t.tr
    t.call()                                                     # records under tr1
    assert len(t.seg.entries) == 1 and all(t.seg.entries.values())
    tr2 = Trainer(opt, t.m, crit, lr=0)
    t.tr = tr2
    w = t.layers[1][0].conv1.weight
    with torch.no_grad():
        w.mul_(1.5)                                              # tr2's buffer only: tr1.flat_p keeps the old values
    (lo, hi), = _flat_range(tr2.optimizer, [w])
    assert not torch.equal(tr1.optimizer.flat_p[lo:hi], tr2.optimizer.flat_p[lo:hi])
    g1 = tr1.optimizer.flat_g.clone()
    assert float(g1.abs().max()) > 0
    got, ref = t.both()
    assert _same(got, ref) == ALL_SAME
    for layer in t.layers:                                       # the new optimizer sees the trunk's gradients
        assert all(float(got[2][a:b].abs().max()) > 0 for a, b in _flat_range(tr2.optimizer, [q for q in layer.parameters() if q.dim() == 4]))
    assert torch.equal(tr1.optimizer.flat_g, g1)                 # nothing was written into the first trainer's gradients
    assert tr1.optimizer.flat_p.data_ptr() != tr2.optimizer.flat_p.data_ptr()


def test_batchnorm_hyperparameters_and_requires_grad_are_followed(monkeypatch):
    """Case d: momentum and eps are floats inside the recorded arguments; a frozen weight has no weight-gradient launch in eager."""
    t, _, _, _ = _trunk(monkeypatch)
    t.call()
    bn = t.layers[2][2].bn2
    k = [i for i, b in enumerate(t.bufs) if b is bn.running_mean][0]
    rm0 = bn.running_mean.clone()
    got, ref = t.both()
    assert _same(got, ref) == ALL_SAME
    mean = rm0 + (ref[3][k] - rm0) / bn.momentum                 # the batch mean of this layer: same input, same weights below
    rm1 = bn.running_mean.clone()
    bn.momentum = 0.5
    got, ref = t.both()
    assert _same(got, ref) == ALL_SAME
    assert torch.allclose(ref[3][k] - rm1, 0.5 * (mean - rm1), rtol=1e-4, atol=1e-6) and float((mean - rm1).abs().max()) > 1e-3
    bn.eps = 1e-3
    assert _same(*t.both()) == ALL_SAME
    w = t.layers[1][1].conv2.weight
    (lo, hi), = _flat_range(t.tr.optimizer, [w])
    assert float(ref[2][lo:hi].abs().max()) > 0
    w.requires_grad_(False)
    got, ref = t.both()
    assert _same(got, ref) == ALL_SAME
    assert float(got[2][lo:hi].abs().max()) == 0 and float(ref[2][lo:hi].abs().max()) == 0
    w.requires_grad_(True)
    got, ref = t.both()
    assert _same(got, ref) == ALL_SAME and float(got[2][lo:hi].abs().max()) > 0


def test_module_switches_are_followed(monkeypatch):
    """Case e: the Functions of the trunk read `functional.WINOGRAD` per call; a tape holds the launches of the value it was recorded under."""
    from pdfnet_amd import functional as F
    from pdfnet_amd import hip
    N, C, H, W = X_WINOGRAD
    assert F.WINOGRAD and hip.lib().pdf_conv2d_winograd_workspace_floats(N, H // 2, W // 2, 128, 128, 3, 3, 1, 1, 0) > 0
    t, _, _, _ = _trunk(monkeypatch, X_WINOGRAD)
    t.call()
    got, ref = t.both()
    assert _same(got, ref) == ALL_SAME
    monkeypatch.setattr(F, 'WINOGRAD', False)
    got0, ref0 = t.both()
    assert _same(got0, ref0) == ALL_SAME
    assert not torch.equal(ref0[2], ref[2])                      # the direct sum and the transform domain round differently
    monkeypatch.setattr(F, 'WINOGRAD', True)
    got1, ref1 = t.both()
    assert _same(got1, ref1) == ALL_SAME and torch.equal(ref1[2], ref[2])


X3_ENV = {'PDF_X3_MINT': '128', 'PDF_WINOGRAD_MINPT': '4096'}     # layer 3's 256-channel 3x3 convolutions on 16x16 maps (T = 128) become x3 F(4x4) launches


def _x3_child():
    """Case c, in a process of its own (the thresholds are read once, when the library meets them): prints one JSON line."""
    from pdfnet_amd import functional as F
    from pdfnet_amd import taped
    from pdfnet_amd.trains.base_trainer import Trainer
    from tests.test_trainer_gpu import _setup
    res = {'voff_default': F._wino_v_offset(8, 16, 16, 256, 256, 3, 3, 1, 1), 'mode_default': F._L().pdf_debug_x3_mode()}
    F.set_x3(0)
    res['voff_mode0'] = F._wino_v_offset(8, 16, 16, 256, 256, 3, 3, 1, 1)
    F.set_x3(None)
    opt, m, crit, _ = _setup(R=128, B=2)
    t = _Trunk(Trainer(opt, m, crit, lr=1e-4), m, X_WINOGRAD, lambda on: setattr(taped, 'TRUNK_TAPE', on))
    t.call()                                                     # records, replays
    res['pinned_first'] = t.seg.pinned_bytes()
    steps = [(None, _same(*t.both()))]
    refs = {}
    for mode in (0, None, 0, None, 0):
        F.set_x3(mode)
        got, ref = t.both()
        steps.append((mode, _same(got, ref)))
        refs.setdefault(mode, ref)
    res['steps'] = steps
    res['modes_differ'] = not torch.equal(refs[0][2], refs[None][2])
    res['entries'], res['max_entries'], res['pinned_last'] = len(t.seg.entries), t.seg.MAX_ENTRIES, t.seg.pinned_bytes()
    print(json.dumps(res))


def test_x3_mode_switches_are_followed():
    """Case c: `functional.set_x3` moves the transformed input inside the forward Winograd workspace (54 x Cin x Cout floats of x3 weights in
    front of it, or 36 x Cin x Cout of fp32 ones) and the weight gradient reads it through a recorded address.  Default mode, mode 0, and
    back and forth: every call equals eager in the mode it runs in, and the dropped tapes free what they pinned."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''), **X3_ENV)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--x3-child'], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    # the hazard is live: this layer's V sits at another offset in the two modes
    assert res['mode_default'] & 1 and res['voff_default'] == 54 * 256 * 256 and res['voff_mode0'] == 36 * 256 * 256, res
    assert [s[0] for s in res['steps']] == [None, 0, None, 0, None, 0]
    assert all(s[1] == ALL_SAME for s in res['steps']), res['steps']
    assert res['entries'] <= res['max_entries'] and 0 < res['pinned_last'] <= 2 * res['pinned_first'], res


if __name__ == '__main__' and sys.argv[1:] == ['--x3-child']:
    _x3_child()
