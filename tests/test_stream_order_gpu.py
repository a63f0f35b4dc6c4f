"""The ORDER in which the train step's work reaches the GPU: every cross-stream edge of the default schedule (F.fork sites, the weight-gradient
side streams, the backward of the forked branches, the taped trunk, the Winograd V that crosses streams) is tested by delaying one side of it.

The delay is a dependent chain of 4096^3 fp32 matmuls on buffers allocated before the step (one ping-pong pair per stream, no allocation inside
the chain), enqueued at the head of one stream's work.  It lasts at least twice the GPU time of a whole serial step, so whatever the other
stream has queued finishes first: a consumer that does not wait reads memory that is not written yet (or that the allocator handed out again),
every time, and the wrong values show as plain floats.  Nothing is provoked: every kernel reads and writes its own, allocated memory.

Reference: the SERIAL schedule (F.USE_SIDE_STREAMS = False, which also turns the weight-gradient side streams and the trunk tape off, and
simplified.FORK_DENSE_LOSS = False), same model seed, same batches, same F.manual_seed; dropout stays on (the masks are hashed from seed, step
counter and element index).  Every schedule runs two warm-up steps on batch A (with the default switches the first records the trunk tape and
the second replays it) and the measured step on a different batch B, so that stale memory of the previous step cannot hold the right answer.

Bar, from the reference alone: the serial sequence is run twice; d0 = the per-tensor spread of the two runs is what the float atomics
(scatter_rows, window_kernel mode 1) legitimately move.  A tensor passes if max|got - ref| <= 8 d0 + 1e-5 max|ref| + floor; floor is
1e-4 max|gradient of the layer's weight| for a `.bias` (the rule of tests/test_model_gpu.py: a bias in front of a normalisation holds rounding
noise only) and 0 for everything else; for the Adam moments the same rule on m, and 3e-8 max|v of the weight| on v (v is quadratic:
(g + e)^2 - g^2 <= 3 f^2 for |g|, |e| <= f = 1e-4 max|g_w|).  Integer state (num_batches_tracked, the dropout step counter) must be equal.  No
tensor is left out.

Fork sites of the step (named by the forked closure; `test_train_step...` asserts that the sites seen at run time are exactly these, so a new
F.fork call without a case fails):
    both_hands, center_features, hms_decoder, dp_decoder, other_heads, dense_terms, run_mid
The eval pass forks both_hands, center_features, hms_decoder, dp_decoder, other_heads with given clouds and center_features, hms_decoder,
other_heads with choose=None (dp_decoder is then issued in line, in front of depth2pcl).  F.parallel has no call site in the step; it is
covered at operator level.

The Adam cases (lr = 1e-4, the moments m and v after the step, which are linear and quadratic in the gradient): the two warm-up steps run at
lr = 0 like everywhere else and the measured step at 1e-4.  With all three steps at 1e-4 the sequence is chaotic -- the first Adam updates move
every element by +-lr whatever its gradient's size, and two SERIAL runs then disagree far beyond the atomics (measured: 2281 of 2371 tensors
differ, the bar 8 d0 + 1e-5 |loss| of the loss itself comes to 260), so 8 d0 of two samples is no bound: default schedules landed at 0.7 .. 3.2
of it on the loss terms whether a race was there or not.  m and v of the measured step still hold that step's gradient, so they show whether
Adam waited; the sharpness check below was made on exactly these cases.

Hardware queues: the process has 4, and a stream that shares its queue with the delayed one is held back with it, so an edge between two such
streams cannot show.  test_the_harness_sees_an_unjoined_read tries every slot of the fork pool against the launching stream and prints which
slots show an unjoined read (all three, alone and inside the whole suite).

Measured on one MI355X (every run prints these: serial step, link, chain, d0, and per case the worst ratio, the delays and the wall time):
    serial step (R = 128, B = 2, events around the measured step)      29.8 .. 31.8 ms over five runs of this file, 35.4 ms inside the whole suite
    one 4096^3 fp32 link                                                0.95 .. 0.97 ms
    chain = 2 ceil(2.5 step / link / 2) links (at least 32)             78 .. 86 links, 76 .. 78 ms alone = 2.4 .. 2.6 serial steps;
                                                                        every case asserts delay >= 2 serial steps from its own events
    d0, train lr = 0      658 .. 662 of 945 tensors differ between two serial runs; d0 / max|ref| <= 5.9e-6 outside the biases with a floor
                          (largest: pointnet_plus.netR_1.0.weight, the scatter_rows atomics), 1.0 .. 1.7 on those biases (rounding noise only)
    d0, train lr = 1e-4   1977 .. 1986 of 2371 tensors; <= 9.8e-6 outside the biases with a floor
    d0, eval (both inputs) and the Winograd pair: 0 for every tensor -- those cases are bit-exact comparisons
    worst max|got - ref| / bar per case: gradients 0.08 .. 0.29, Adam moments 0.41 .. 0.45 (v of decoder attn.w_ks), eval and Winograd 0
    wall time: 0.3 .. 0.5 s per train case, 0.09 s per eval case, 21 s for the file (reference and fixtures included)
    sharpness: with join_wgrad's waits taken out (a one-off run, not part of the suite) the three wg_side Adam cases fail at 6e4 .. 8e4 of the bar

Found by this file and fixed in functional._Linear.backward: the scale / shift vectors of a lazy BatchNorm are read by the weight-gradient kernel
on the side stream but were not recorded on it; with the side stream late and the trunk not taped the allocator handed their memory out again
(wg_side, WGRAD_GROUP 1 and 16, TRUNK_TAPE off: encoder.resnet.layer4.0.conv3.weight off by 2.9e4 and 1.9e3 at max|ref| = 4.5e3).
"""
import copy
import gc
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

SITES = ('both_hands', 'center_features', 'hms_decoder', 'dp_decoder', 'other_heads', 'dense_terms', 'run_mid')
EVAL_SITES = {'clouds': ('both_hands', 'center_features', 'hms_decoder', 'dp_decoder', 'other_heads'),
              'depth': ('center_features', 'hms_decoder', 'other_heads')}
MIN_LINKS = 32


def _site(fn):
    """Name of a forked closure: the defining function's name, or for a lambda the method it calls."""
    return fn.__name__ if fn.__name__ != '<lambda>' else '.'.join(fn.__code__.co_names)


# ---------------------------------------------------------------------------------------------- the delay
class Delay:
    """A dependent chain of `links` [N,N] x [N,N] matmuls, ping-pong between two buffers that belong to the stream it runs on."""
    N = 4096

    def __init__(self):
        g = torch.Generator(device='cuda').manual_seed(5)
        self.w = torch.randn(self.N, self.N, device='cuda', generator=g) / self.N ** 0.5       # keeps the chain's values O(1)
        self.bufs = {}
        self.links = MIN_LINKS
        self.marks = []

    def prepare(self, streams):
        """Buffers (and the BLAS handle / workspace of torch.mm) for every stream a delay may go to: before the step, in EVERY schedule."""
        for s in streams:
            if s.cuda_stream not in self.bufs:
                self.bufs[s.cuda_stream] = (torch.ones(self.N, self.N, device='cuda'), torch.empty(self.N, self.N, device='cuda'))
            with torch.cuda.stream(s):
                a, b = self.bufs[s.cuda_stream]
                torch.mm(a, self.w, out=b)
        torch.cuda.synchronize()

    def link_ms(self):
        s = torch.cuda.current_stream()
        self.prepare([s])
        a, b = self.bufs[s.cuda_stream]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            torch.mm(a, self.w, out=b)
            torch.mm(b, self.w, out=a)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 8

    def __call__(self, s=None):
        """Enqueue the chain on `s` (default: the current stream).  No allocation: the buffers must exist."""
        s = torch.cuda.current_stream() if s is None else s
        a, b = self.bufs[s.cuda_stream]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            for _ in range(self.links // 2):
                torch.mm(a, self.w, out=b)
                torch.mm(b, self.w, out=a)
            e1.record()
        self.marks.append((e0, e1))

    def took_ms(self):
        """GPU time of every chain enqueued since the last call (after a synchronize)."""
        out = [e0.elapsed_time(e1) for e0, e1 in self.marks]
        self.marks = []
        return out


class Plan:
    """One delay.  kind: None | 'side' / 'main' (at the fork site `site`) | 'wg_side' / 'wg_main' (first wgrad_stream.__enter__ of each side
    stream) | 'fork_bwd' (every stream of the fork pool, at the first wgrad_stream.__enter__ of the backward).  Acts only while `armed`."""

    def __init__(self, kind=None, site=None):
        self.kind, self.site, self.armed, self.fired, self.seen, self.done = kind, site, False, 0, [], set()

    def __str__(self):
        return "%s%s" % (self.kind, ":" + self.site if self.site else "")


_ORIG = {}


def _busy():
    """The slots of the fork pool that are taken (an earlier module's fork that nobody joined keeps its slot: compare, do not expect none)."""
    from pdfnet_amd import functional as F
    return {k: sorted(v) for k, v in F.fork._busy.items() if v}


def _fork_pool():
    from pdfnet_amd import functional as F
    return list(F._side.get(('fork', torch.cuda.current_device()), []))


def _install(mp, plan, delay):
    """Hooks on F.fork, F.parallel and F.wgrad_stream that record the sites and put `plan`'s delay in."""
    from pdfnet_amd import functional as F
    if not _ORIG:
        _ORIG.update(fork_init=F.fork.__init__, parallel=F.parallel, wg_enter=F.wgrad_stream.__enter__)
    fork_init, parallel, wg_enter = _ORIG['fork_init'], _ORIG['parallel'], _ORIG['wg_enter']       # (a second plan replaces the first one's hooks)

    def init(self, fn):
        site = _site(fn)
        hit = plan.armed and plan.site == site and F.USE_SIDE_STREAMS
        if plan.armed:
            plan.seen.append(site)
        if hit and plan.kind == 'side':
            def late():                                          # on the side stream, after its wait for the launching stream
                delay()
                plan.fired += 1
                return fn()
            fork_init(self, late)
            return
        fork_init(self, fn)
        if hit and plan.kind == 'main':                          # on the launching stream, right after the fork returned: the side runs far ahead
            delay()
            plan.fired += 1

    def par(*fns):
        if plan.armed and len(fns) > 1:
            plan.seen.append('parallel')
        if plan.armed and plan.site == 'parallel' and len(fns) > 1 and F.USE_SIDE_STREAMS:
            def late(f):
                def g():
                    delay()
                    plan.fired += 1
                    return f()
                return g
            fns = tuple(late(f) if (i > 0) == (plan.kind == 'side') else f for i, f in enumerate(fns))
        return parallel(*fns)

    def enter(self):
        launching = torch.cuda.current_stream()
        r = wg_enter(self)
        if plan.armed and self.enabled and plan.kind in ('wg_side', 'wg_main', 'fork_bwd'):
            side = torch.cuda.current_stream()
            if plan.kind == 'fork_bwd':
                if not plan.fired:
                    for s in _fork_pool():
                        delay(s)
                        plan.fired += 1
            elif side.cuda_stream not in plan.done:              # once per side stream, after its waits
                plan.done.add(side.cuda_stream)
                delay(side if plan.kind == 'wg_side' else launching)
                plan.fired += 1
        return r
    mp.setattr(F.fork, '__init__', init)
    mp.setattr(F, 'parallel', par)
    mp.setattr(F.wgrad_stream, '__enter__', enter)


def _all_streams():
    from pdfnet_amd import functional as F
    out = [torch.cuda.current_stream()] + _fork_pool()
    for k, pool in F._side.items():
        if not (isinstance(k, tuple) and k[0] == 'fork'):
            out += list(pool)
    return out + [ent[0] for ent in F._wg_streams.values()]


# ---------------------------------------------------------------------------------------------- the bar
def _floors(ref):
    mx = {n: float(t.abs().max()) if t.numel() else 0.0 for n, t in ref.items()}
    fl = {}
    for n in ref:
        f = 0.0
        kind = n.split('.', 1)[0]
        wn = n[:-4] + 'weight'
        if kind in ('grad', 'm', 'v') and n.endswith('.bias') and wn in ref:
            f = (3e-8 if kind == 'v' else 1e-4) * mx[wn]
        fl[n] = f
    return mx, fl


class Reference:
    """ref: name -> tensor of the first serial run; d0: per-tensor spread against the second; ints: the integer state."""

    def __init__(self, a, b, ints_a, ints_b, what):
        assert set(a) == set(b) and ints_a == ints_b, "two serial runs disagree on integer state"
        self.t, self.ints = a, ints_a
        self.names = sorted(a)
        self.d0 = {n: float((a[n].double() - b[n].double()).abs().max()) if a[n].numel() else 0.0 for n in self.names}
        self.mx, self.floor = _floors(a)
        self.bar = {n: 8 * self.d0[n] + 1e-5 * self.mx[n] + self.floor[n] for n in self.names}
        assert all(math.isfinite(self.mx[n]) for n in self.names)
        moved = sorted(((self.d0[n] / (self.mx[n] + 1e-30), n) for n in self.names if self.d0[n] > 0), reverse=True)
        noise = [(r, n) for r, n in moved if self.floor[n] > 0]
        rest = [(r, n) for r, n in moved if self.floor[n] == 0]
        print("\n[%s] d0: %d of %d tensors differ between two serial runs; largest d0 / max|ref| among the biases with a floor: %s; among the rest: %s"
              % (what, len(moved), len(self.names), ["%s %.2e" % (n, r) for r, n in noise[:2]], ["%s %.2e" % (n, r) for r, n in rest[:4]]))

    def check(self, got, ints, label):
        assert set(got) == set(self.names), (sorted(set(got) ^ set(self.names))[:8])
        assert ints == self.ints, (label, {k: (ints.get(k), v) for k, v in self.ints.items() if ints.get(k) != v})
        err = torch.stack([(got[n].double() - self.t[n].double()).abs().max() if self.t[n].numel() else torch.zeros((), dtype=torch.float64, device='cuda')
                           for n in self.names]).cpu().tolist()
        bad, worst = [], (0.0, None)
        for n, e in zip(self.names, err):
            bar = self.bar[n]
            ratio = e / bar if bar > 0 else (0.0 if e == 0 else float('inf'))
            if not e <= bar:
                bad.append((n, e, bar))
            if not ratio <= worst[0]:
                worst = (ratio, n)
        print("\n[%s] worst max|got - ref| / bar = %.3g (%s)" % (label, worst[0], worst[1]))
        assert not bad, (label, len(bad), sorted(bad, key=lambda x: -(x[1] / (x[2] + 1e-300)) if x[1] == x[1] else -1e300)[:8])


def _int_state(t):
    """Integer tensors compare exactly: the values of a small one, (shape, sum, weighted sum) of a large one."""
    t = t.detach().reshape(-1)
    if t.numel() <= 16:
        return t.cpu().tolist()
    d = t.double()
    return (tuple(t.shape), float(d.sum()), float((d * torch.arange(1, t.numel() + 1, device=t.device, dtype=torch.float64)).sum()))


# ---------------------------------------------------------------------------------------------- the train step
class Env:
    pass


@pytest.fixture(scope="module")
def env():
    from pdfnet_amd.synthetic import synthetic_loss_constants, synthetic_train_batch, to_device
    from tests.test_trainer_gpu import _setup
    e = Env()
    e.opt, e.template, e.crit, e.batch_a = _setup(R=128, B=2, dropout=True)                # never run: every case works on a copy of it
    consts = synthetic_loss_constants()
    e.batch_b = to_device(synthetic_train_batch(2, 128, seed=4, consts=consts), torch.device('cuda'))
    assert not torch.equal(e.batch_a['input'], e.batch_b['input']) and not torch.equal(e.batch_a['choose'], e.batch_b['choose'])
    e.delay = Delay()
    e.refs = {}
    _train_ref(e, 0.0)                                           # the reference: computed once, left unchanged
    return e


def _serial(mp):
    from pdfnet_amd import functional as F
    from pdfnet_amd.trains import simplified
    mp.setattr(F, 'USE_SIDE_STREAMS', False)
    mp.setattr(simplified, 'FORK_DENSE_LOSS', False)


def _train_sequence(e, lr, plan, mp, timed=False):
    """Two warm-up steps on batch A, the measured step on batch B -> (tensors, ints, info)."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.layers import BatchNorm
    from pdfnet_amd.trains.base_trainer import Trainer, split_parameters
    dev = torch.device('cuda', torch.cuda.current_device())
    assert torch.cuda.current_stream().cuda_stream == 0                                    # the step is issued on the default stream
    _install(mp, plan, e.delay)
    busy0 = _busy()
    m = copy.deepcopy(e.template)
    F.manual_seed(99)
    ctr = F.step_counter(dev)
    ctr.zero_()
    tr = Trainer(e.opt, m, e.crit, lr=0.0)                        # (the warm-up steps keep the weights in every case, see the Adam cases)
    cap = {}
    fwd_bwd = tr._fwd_bwd

    def keep_stats(batch, epoch):
        out = fwd_bwd(batch, epoch)
        cap['stats'] = out[1]
        return out
    tr._fwd_bwd = keep_stats
    for _ in range(2):
        tr.train_step(e.batch_a, 0)
    e.delay.prepare(_all_streams())                                                        # (synchronizes)
    e.delay.took_ms()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tr.optimizer.lr = lr
    plan.armed = True
    e0.record()
    loss = tr.train_step(e.batch_b, 0)
    e1.record()
    plan.armed = False
    m.join_deferred()
    BatchNorm.flush_counters()
    torch.cuda.synchronize()
    assert _busy() == busy0, (_busy(), busy0)                                              # every fork of the step gave its slot back
    info = {'step_ms': e0.elapsed_time(e1), 'delays_ms': e.delay.took_ms(), 'seen': list(plan.seen), 'fired': plan.fired,
            'seg': m.encoder.__dict__.get('_trunk_seg')}
    o = tr.optimizer
    t = {'loss': loss.detach().clone()}
    for k, v in cap['stats'].items():
        t['stats.' + k] = torch.as_tensor(v, device='cuda').detach().clone().float()
    early, late, dead = split_parameters(list(m.named_parameters()))
    pos = {id(p): i for i, p in enumerate(o.params)}
    for n, p in early + late:                                                              # flat_g[:n_live], tensor by tensor
        i = pos[id(p)]
        assert o.offsets[i] < tr.n_live
        t['grad.' + n] = o._view(o.flat_g, i).clone()
        if lr > 0:
            t['m.' + n] = o._view(o.flat_m, i).clone()
            t['v.' + n] = o._view(o.flat_v, i).clone()
    assert float(o.flat_g[tr.n_live:].abs().max()) == 0.0
    ints = {'step_counter': int(ctr)}
    for n, b in m.named_buffers():
        if b.is_floating_point():
            t['buf.' + n] = b.detach().clone()
        else:
            ints['buf.' + n] = _int_state(b)
    assert any(n.endswith('running_var') for n in t) and any(n.endswith('num_batches_tracked') for n in ints)
    tr._fwd_bwd = None
    m.encoder.on_trunk_output_grad = None
    del tr, m
    gc.collect()
    return t, ints, info


def _train_ref(e, lr):
    """The serial schedule, twice (module-wide: computed once per learning rate and left unchanged)."""
    if lr not in e.refs:
        with pytest.MonkeyPatch.context() as mp:
            _serial(mp)
            a, ia, info = _train_sequence(e, lr, Plan(), mp)
            b, ib, _ = _train_sequence(e, lr, Plan(), mp)
        assert sorted(set(info['seen'])) == sorted(set(SITES) - {'dense_terms'}), info['seen']       # (FORK_DENSE_LOSS off: issued in line)
        if 'step_ms' not in e.__dict__:
            e.step_ms = info['step_ms']
            e.link_ms = e.delay.link_ms()
            e.delay.links = max(MIN_LINKS, 2 * int(math.ceil(2.5 * e.step_ms / e.link_ms / 2)))       # 2.5 x: the bound asserted per case is 2 x
            print("\nserial step %.2f ms GPU time; one link %.3f ms; chain = %d links" % (e.step_ms, e.link_ms, e.delay.links))
        e.refs[lr] = Reference(a, b, ia, ib, "train lr=%g" % lr)
    return e.refs[lr]


def _train_case(e, monkeypatch, plan, lr=0.0, group=1, tape=True):
    from pdfnet_amd import functional as F
    from pdfnet_amd import taped
    ref = _train_ref(e, lr)
    t0 = time.time()
    monkeypatch.setattr(F, 'WGRAD_GROUP', group)
    monkeypatch.setattr(taped, 'TRUNK_TAPE', tape)
    got, ints, info = _train_sequence(e, lr, plan, monkeypatch)
    label = "%s lr=%g group=%d tape=%s" % (plan, lr, group, tape)
    print("\n[%s] wall %.2f s; measured step %.1f ms; delays %s ms" % (label, time.time() - t0, info['step_ms'], ["%.1f" % d for d in info['delays_ms']]))
    assert sorted(set(info['seen'])) == sorted(SITES), info['seen']                        # a new F.fork site needs a case here
    if plan.kind is not None:
        assert info['fired'] >= 1 and len(info['delays_ms']) == info['fired'], info
        assert min(info['delays_ms']) >= 2.0 * e.step_ms, (info['delays_ms'], e.step_ms)   # long enough: twice the serial step
    seg = info['seg']
    taped_now = seg is not None and len(seg.entries) == 1 and all(en is not False for en in seg.entries.values())
    assert taped_now == (tape and group == 1), "the trunk tape is replayed exactly when TRUNK_TAPE is on and WGRAD_GROUP is 1"
    ref.check(got, ints, label)


def test_default_schedule_without_a_delay_equals_the_serial_one(env, monkeypatch):
    _train_case(env, monkeypatch, Plan())


@pytest.mark.parametrize("kind", ['side', 'main'])
@pytest.mark.parametrize("site", SITES)
def test_train_step_with_one_fork_site_delayed(env, monkeypatch, site, kind):
    """Side late: the delay sits on the side stream in front of the closure's first launch.  Main late: on the launching stream right after
    the fork returned."""
    _train_case(env, monkeypatch, Plan(kind, site))


@pytest.mark.parametrize("lr", [0.0, 1e-4])
@pytest.mark.parametrize("group,tape", [(1, True), (1, False), (16, False)])
@pytest.mark.parametrize("kind", ['wg_side', 'wg_main'])
def test_train_step_with_the_weight_gradient_streams_delayed(env, monkeypatch, kind, group, tape, lr):
    """The delay goes in at the first wgrad_stream.__enter__ of every side stream in the measured backward, after its waits -- on the side
    stream (its gradients land late: join_wgrad / Adam must wait) or on its launching stream (the side stream runs far ahead: it must have
    waited for its operands).  WGRAD_GROUP = 1 with the replayed tape and without it, and 16 (what graph capture uses; the tape does not
    qualify then).  lr = 1e-4: the Adam moments after the step show whether Adam waited, without the +-lr sign noise of the parameters."""
    _train_case(env, monkeypatch, Plan(kind), lr=lr, group=group, tape=tape)


def test_train_step_with_the_backward_of_the_forks_delayed(env, monkeypatch):
    """Autograd replays each node on its forward stream: at the first weight-gradient launch of the backward every stream of the fork pool
    is delayed -- the `chain` hand-overs and the skip-gradient epilogues cross streams there."""
    _train_case(env, monkeypatch, Plan('fork_bwd'))


def test_raising_mesh_terms_gives_the_dense_fork_its_slot_back(env, monkeypatch):
    """CtdetLoss.forward joins the dense-loss fork in a finally: a raising mesh_terms leaks no slot of the fork pool, and (with the state the
    failed forward advanced put back: BatchNorm statistics, host seed) the next step is the reference step."""
    from pdfnet_amd import functional as F
    from pdfnet_amd.networks.layers import BatchNorm
    from pdfnet_amd.trains.simplified import CtdetLoss
    e = env
    ref = _train_ref(e, 0.0)
    class Boom(RuntimeError):
        pass

    # the failed attempt is made from inside the sequence: a train_step on batch B right before the measured one
    from pdfnet_amd.trains.base_trainer import Trainer
    step = Trainer.train_step
    calls = []

    def train_step(self, batch, epoch=0):
        calls.append(1)
        if len(calls) == 3:
            m = self.model
            m.join_deferred()
            BatchNorm.flush_counters()
            bufs = list(m.buffers())
            saved, seed, busy0 = [b.clone() for b in bufs], F._seed_state[0], _busy()
            with pytest.MonkeyPatch.context() as mp2:
                def boom(*a, **k):
                    raise Boom()
                mp2.setattr(CtdetLoss, 'mesh_terms', boom)
                with pytest.raises(Boom):
                    step(self, batch, epoch)
            m.join_deferred()                                     # the model's own deferred forks (mid_model) are joined by the next reader
            busy = _busy()
            BatchNorm.flush_counters()
            for b, v in zip(bufs, saved):
                b.copy_(v)
            F._seed_state[0] = seed
            assert busy == busy0, "the dense-loss fork kept its slot: %s (before the step: %s)" % (busy, busy0)
        return step(self, batch, epoch)
    monkeypatch.setattr(Trainer, 'train_step', train_step)
    got, ints, info = _train_sequence(e, 0.0, Plan(), monkeypatch)
    assert len(calls) == 3
    ref.check(got, ints, "after a raising mesh_terms")


# ---------------------------------------------------------------------------------------------- eval
def _flatten(obj, pre, out):
    if torch.is_tensor(obj):
        out[pre] = obj.detach().clone()
    elif isinstance(obj, dict):
        for k, v in obj.items():
            _flatten(v, pre + '.' + str(k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            _flatten(v, pre + '.' + str(i), out)


def _eval_pass(e, model, inputs, plan, mp):
    from pdfnet_amd import functional as F
    _install(mp, plan, e.delay)
    F.manual_seed(77)                                             # depth2pcl draws its sub-sample from the host seed
    b = e.batch_b
    ch, cl = (b['choose'], b['cloud']) if inputs == 'clouds' else (None, None)
    e.delay.prepare(_all_streams())
    e.delay.took_ms()
    plan.armed = True
    with torch.no_grad():
        res = model(b['input'], ch, cl, b['depth'], None, b['K_new'], b['valid'])
    plan.armed = False
    torch.cuda.synchronize()
    out = {}
    _flatten(res, 'out', out)
    assert len(out) > 20
    flt = {n: t for n, t in out.items() if t.is_floating_point()}
    ints = {n: _int_state(t) for n, t in out.items() if not t.is_floating_point()}
    return flt, ints, {'seen': list(plan.seen), 'fired': plan.fired, 'delays_ms': e.delay.took_ms()}


@pytest.fixture(scope="module")
def eval_env(env):
    e = env
    e.eval_model = copy.deepcopy(e.template).eval()
    e.eval_refs = {}
    with torch.no_grad():                                         # warm-up in the default schedule: streams, workspaces
        for inputs in ('clouds', 'depth'):
            with pytest.MonkeyPatch.context() as mp:
                _eval_pass(e, e.eval_model, inputs, Plan(), mp)
    for inputs in ('clouds', 'depth'):
        with pytest.MonkeyPatch.context() as mp:
            _serial(mp)
            a, ia, info = _eval_pass(e, e.eval_model, inputs, Plan(), mp)
            b, ib, _ = _eval_pass(e, e.eval_model, inputs, Plan(), mp)
        assert sorted(set(info['seen'])) == sorted(EVAL_SITES[inputs]), info['seen']
        e.eval_refs[inputs] = Reference(a, b, ia, ib, "eval " + inputs)
    return e


@pytest.mark.parametrize("kind", ['side', 'main'])
@pytest.mark.parametrize("inputs,site", [(i, s) for i in ('clouds', 'depth') for s in EVAL_SITES[i]])
def test_eval_pass_with_one_fork_site_delayed(eval_env, monkeypatch, inputs, site, kind):
    """model.eval() under no_grad, with given clouds and with choose=None (clouds from depth2pcl on the predicted masks): every returned
    tensor against the serial schedule."""
    e = eval_env
    t0 = time.time()
    plan = Plan(kind, site)
    got, ints, info = _eval_pass(e, e.eval_model, inputs, plan, monkeypatch)
    label = "eval %s %s" % (inputs, plan)
    print("\n[%s] wall %.2f s; delays %s ms" % (label, time.time() - t0, ["%.1f" % d for d in info['delays_ms']]))
    assert sorted(set(info['seen'])) == sorted(EVAL_SITES[inputs]), info['seen']
    assert info['fired'] == 1 and min(info['delays_ms']) >= 2.0 * e.step_ms, info
    e.eval_refs[inputs].check(got, ints, label)


# ---------------------------------------------------------------------------------------------- operator level
def _named(fn, name):
    fn.__name__ = name
    return fn


def _wino_pair(F, plan, delay, mode):
    """The shape of test_winograd_forwards_sharing_one_transformed_input: two convolutions on one input marked with F.share_winograd_input, the
    first on the current stream (it leaves V), the second on another stream (it reads V) -> outputs and all gradients.
    mode: 'serial' (one stream) | 'first_forward_late' (the current stream delayed in front of the forward that writes V; the second in an
    F.fork) | 'fork_late' (the fork delayed) | 'second_stream' (first forward late, the second convolution on a stream that has NOT waited for
    the current one: the event V was published with is then the only edge between the two forwards)."""
    from tests.test_gemm_dispatch_gpu import dev, rnd
    N, Cin, H, W = 2, 128, 64, 64
    cl = torch.channels_last
    x = F.share_winograd_input(dev(rnd(N, Cin, H, W, seed=1)).contiguous(memory_format=cl).requires_grad_())
    ws = [dev(rnd(co, Cin, 3, 3, seed=2 + i, scale=(Cin * 9) ** -0.5)).contiguous(memory_format=cl).requires_grad_() for i, co in enumerate((64, 128))]
    gys = [dev(rnd(N, co, H, W, seed=7 + i)).contiguous(memory_format=cl) for i, co in enumerate((64, 128))]
    s2 = torch.cuda.Stream() if mode == 'second_stream' else None
    delay.prepare(_all_streams())                                # (synchronizes: x and the weights are complete for every stream)
    delay.took_ms()
    plan.armed = True
    if mode in ('first_forward_late', 'second_stream'):
        delay()
        plan.fired += 1
    y0 = F.conv2d(x, ws[0], None, 1, 1)
    if s2 is None:
        y1 = F.fork(_named(lambda: F.conv2d(x, ws[1], None, 1, 1), 'second_conv')).join()
    else:
        cur = torch.cuda.current_stream()
        with torch.cuda.stream(s2):
            y1 = F.conv2d(x, ws[1], None, 1, 1)
        cur.wait_stream(s2)
        y1.record_stream(cur)
    shared = len(x._pdf_wino_share)
    torch.autograd.backward([y0, y1], gys)
    plan.armed = False
    torch.cuda.synchronize()
    assert shared == 1, "the first forward did not publish its V"
    return {'y0': y0.detach(), 'y1': y1.detach(), 'dx': x.grad, 'dw0': ws[0].grad, 'dw1': ws[1].grad}


@pytest.mark.parametrize("which", ['first_forward_late', 'fork_late', 'second_stream'])
def test_winograd_v_crossing_streams(env, monkeypatch, which):
    """The R = 128 step has no F(4x4) launch: the `wait_event` / `record_stream` branch of _Conv2d.forward at operator level.  Outputs and all
    gradients must equal the same two convolutions issued on one stream."""
    from pdfnet_amd import functional as F
    e = env
    monkeypatch.setattr(F, "WINOGRAD", True)
    monkeypatch.setattr(F, "WINOGRAD_KEEP_V", True)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(F, 'USE_SIDE_STREAMS', False)
        a = _wino_pair(F, Plan(), e.delay, 'serial')
        b = _wino_pair(F, Plan(), e.delay, 'serial')
    ref = Reference(a, b, {}, {}, "winograd pair")
    plan = Plan('side', 'second_conv') if which == 'fork_late' else Plan()
    _install(monkeypatch, plan, e.delay)
    got = _wino_pair(F, plan, e.delay, which)
    ms = e.delay.took_ms()
    assert plan.fired == 1 and min(ms) >= 2.0 * e.step_ms, (plan.fired, ms)
    ref.check(got, {}, "winograd pair, " + which)


def _chain(F, x, w, n=4):
    y = x
    for _ in range(n):
        y = F.linear(y, w)
    return y


@pytest.mark.parametrize("kind", ['side', 'main'])
def test_parallel_branches_with_one_side_delayed(env, monkeypatch, kind):
    """F.parallel has no call site in the step; its fork / join edges with the side branch, then the launching branch, delayed."""
    from pdfnet_amd import functional as F
    e = env
    g = torch.Generator(device='cuda').manual_seed(3)
    x = torch.randn(300, 256, device='cuda', generator=g)
    w = torch.randn(256, 256, device='cuda', generator=g) / 16
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(F, 'USE_SIDE_STREAMS', False)
        ra, rb = F.parallel(lambda: _chain(F, x, w), lambda: _chain(F, x * 2, w, 5))
        want = (ra + rb).clone()
    plan = Plan(kind, 'parallel')
    _install(monkeypatch, plan, e.delay)
    F.parallel(lambda: x + 0, lambda: x + 0)                       # the pool's stream exists before the buffers are made
    e.delay.prepare(_all_streams())
    e.delay.took_ms()
    plan.armed = True
    a, b = F.parallel(lambda: _chain(F, x, w), lambda: _chain(F, x * 2, w, 5))
    got = a + b                                                  # the consumer on the launching stream
    plan.armed = False
    torch.cuda.synchronize()
    ms = e.delay.took_ms()
    assert plan.fired == 1 and plan.seen == ['parallel'] and min(ms) >= 2.0 * e.step_ms, (plan.fired, plan.seen, ms)
    assert torch.equal(got, want)


def test_the_harness_sees_an_unjoined_read(env, monkeypatch):
    """The harness can fail: a fork whose closure writes a chain of F.linear results into a zero-filled tensor; with the side stream
    delayed, reading fork.out on the launching stream BEFORE join() gives the zeros, after join() the result.  (Initialised memory only.)
    Tried on every slot of the fork pool: the process has 4 hardware queues, and a stream that shares its queue with the delayed one is held
    back with it -- on such a slot the unjoined read waits behind the delay and sees the written tensor, so an edge between those two streams
    cannot show.  At least one slot must show it; which ones do is printed."""
    from pdfnet_amd import functional as F
    e = env
    g = torch.Generator(device='cuda').manual_seed(4)
    x = torch.randn(300, 256, device='cuda', generator=g)
    w = torch.randn(256, 256, device='cuda', generator=g) / 16
    want = _chain(F, x, w).clone()
    assert float(want.abs().max()) > 0.1
    out = torch.zeros_like(want)
    plan = Plan('side', 'writer')
    _install(monkeypatch, plan, e.delay)
    busy0 = _busy()
    F.fork(lambda: None).join()
    e.delay.prepare(_all_streams())
    e.delay.took_ms()

    def writer():
        out.copy_(_chain(F, x, w))
        return out
    visible = {}
    for k in range(max(1, len(_fork_pool()) - sum(len(v) for v in busy0.values()))):
        held = [F.fork(_named(lambda: None, 'holder')) for _ in range(k)]      # the lower free slots are taken: the writer gets the next one
        out.zero_()
        plan.armed = True
        f = F.fork(writer)
        early = f.out.clone()                                    # on the launching stream, no join: the side stream is still in its delay
        plan.armed = False
        slot = f.idx
        joined = f.join().clone()
        for h in held:
            h.join()
        torch.cuda.synchronize()
        assert min(e.delay.took_ms()) >= 2.0 * e.step_ms
        assert torch.equal(joined, want), slot                   # after join() it is the result, on every slot
        visible[slot] = float(early.abs().max()) == 0.0 and not torch.equal(early, joined)
    print("\n[harness] fork-pool slots whose unjoined read shows against the launching stream: %s" % visible)
    assert plan.fired == len(visible) and any(visible.values()), "no unjoined read saw the unwritten tensor: %s" % visible
    assert _busy() == busy0
