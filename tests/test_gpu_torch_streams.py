"""GPU: the stream ordering of ihm2_amd/torch_layer.py, made deterministic.  The layer orders the handle's non-blocking stream and torch's
current stream against each other on four edges -- forward inputs (the handle's stream behind torch's), forward outputs (torch's behind
the handle's), backward seeds, backward gradients -- and on torch's default stream, with inputs that were complete before the call, a
missing wait gives the right answer.  Here every edge gets a situation in which a missing wait reads stale but valid data: the layer
runs on a side stream, the stream that has to be waited for is held by a delay kernel (torch.cuda._sleep, 30 ms: fifty solves of a batch
of 1024, timed with events and asserted to have lasted 20 ms), and what would be read too early is
  - for an input: the true array rolled by one instance along the batch, copied over with the true values behind the delay;
  - for the symmetrised weights the layer makes itself: the rolled ones, in the blocks the allocator hands out next (rehearsed);
  - for an output or a gradient: 0.25 everywhere, in the blocks the allocator hands to the layer's torch.empty (rehearsed: tensors of
    the same shapes are allocated, filled and released in the layer's order; the layer's pointers are asserted to be those).
Never NaN, never arbitrary bytes: a missing wait gives another solve and a bit mismatch, and nothing else.  Every output and gradient
is compared bit for bit with the same call made afterwards on the default stream on synchronised inputs; the side-stream run comes
first, so no block can hold the right answer from an earlier identical run.  The table is tests/test_gpu_penalty_device.py's LAY, B = 8.

Every edge is run on four consecutive side streams of torch's pool (_on_side_streams): on one side stream alone five of the ten
removals of a wait went unnoticed, in a pattern that followed the order of the tests and not the edges -- HIP multiplexes a process's
streams onto a few hardware queues, and a pair of streams that shares one is ordered whatever the events say.  With four, each of the
ten removals is caught by the test of its edge: the table is in NOTES.md R30."""
import gc

import numpy as np
import pytest
import torch

import bitcmp
from test_gpu_penalty_device import B, N, _penalties, _Start, _t

pytestmark = pytest.mark.gpu

DELAY_MS, DELAY_MIN_MS = 30.0, 20.0
STALE = 0.25
SIDES = 4              # side streams each edge is run on (_on_side_streams)
F64, I32 = torch.float64, torch.int32
IN = ("x0", "yref", "yref_e", "W", "W_e", "soft_z", "soft_Z", "alat_z", "alat_Z")
GRAD_SHAPES = ((B, 8), (B, N, 12), (B, 8), (B, 12, 12), (B, 8, 8), (B, N + 1, 28), (B, N + 1, 28), (B, N + 1, 2), (B, N + 1, 2))


@pytest.fixture(scope="module")
def cycles_per_ms():
    """The delay kernel's cycles per millisecond, measured once with two events (as PyTorch's own tests do)."""
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); torch.cuda._sleep(1_000_000); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return 1_000_000 / float(np.median(ms))


class _Delay:
    """Enqueues DELAY_MS of the delay kernel on the current stream between two events; check(): every delay happened and lasted."""

    def __init__(self, cycles_per_ms):
        self.cycles, self.pairs = int(DELAY_MS * cycles_per_ms), []

    def __call__(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); torch.cuda._sleep(self.cycles); b.record()
        self.pairs.append((a, b))

    def check(self, n):
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in self.pairs]
        assert len(ms) == n and min(ms) >= DELAY_MIN_MS, f"{n} delays of {DELAY_MS} ms were to hold a stream, measured: {ms}"


class _LateSeed(torch.autograd.Function):
    """The identity; its backward holds torch's stream with the delay and then copies the incoming gradient into a buffer that held the
    seed rolled by one instance, and hands that buffer on: a backward that does not wait for torch's stream reads the rolled seed."""

    @staticmethod
    def forward(ctx, t, buf, delay):
        ctx.buf, ctx.delay = buf, delay
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        ctx.delay()
        ctx.buf.copy_(g)
        return ctx.buf, None, None


def _case(kind, c):
    """The call under test on the handle c.s: dict(ins, seeds (on the differentiable outputs), outs (names), call, fwd, bwd (the
    layer's allocations in their order, as (shape, dtype)), adjoint (the entry its backward calls))."""
    from ihm2_amd.torch_layer import plant_step, rti_solve, rti_solve_soft

    s = c.s
    rng = np.random.default_rng(17)
    fac = (1.0 + 0.01 * np.arange(B))[:, None, None]
    W, We = fac * np.asarray(s.data.W[0], dtype=np.float64)[None], fac * np.asarray(s.data.W_e, dtype=np.float64)[None]
    weights = [((B, 12, 12), F64), ((B, 12, 12), F64), None, ((B, 8, 8), F64), ((B, 8, 8), F64), None]      # None: the sum's block is released
    if kind == "plant":
        ins = dict(x=c.x0.copy(), u=np.stack([rng.uniform(-100.0, 200.0, B), rng.uniform(-0.2, 0.2, B)], 1))
        return dict(kind=kind, ins=ins, seeds=dict(x_next=rng.standard_normal((B, 8))), outs=("x_next", "model_used"),
                    call=lambda t: plant_step(s, t["x"], t["u"], model=0, M_sim=25),
                    fwd=[((B, 8), F64), ((B, 8, 8), F64), ((B, 8, 2), F64), ((B,), I32)], bwd=None, adjoint=None)
    ins = dict(x0=c.x0, yref=c.yref, yref_e=c.yref_e, W=W, W_e=We)
    seeds = dict(x=rng.standard_normal((B, N + 1, 8)), u=rng.standard_normal((B, N, 2)))
    if kind == "rti":
        return dict(kind=kind, ins=ins, seeds=seeds, outs=("x", "u", "status"), call=lambda t: rti_solve(s, *[t[k] for k in IN[:5]]),
                    fwd=weights + [((B, N + 1, 8), F64), ((B, N, 2), F64), ((B,), I32)],
                    # (rti_solve materialises the gradients it is not given: autograd makes zeros for status before backward runs)
                    bwd=[((B,), I32)] + [(sh, F64) for sh in GRAD_SHAPES[:5]], adjoint="eval_adjoint_weight_sensitivities_device")
    ins.update(zip(IN[5:], _penalties(s)))
    seeds.update(s=rng.standard_normal((B, N + 1, 28)), sa=rng.standard_normal((B, N + 1, 2)))
    return dict(kind=kind, ins=ins, seeds=seeds, outs=("x", "u", "s", "sa", "status"), call=lambda t: rti_solve_soft(s, *[t[k] for k in IN]),
                fwd=weights + [((B, N + 1, 8), F64), ((B, N, 2), F64), ((B, N + 1, 28), F64), ((B, N + 1, 2), F64), ((B,), I32)],
                bwd=[(sh, F64) for sh in GRAD_SHAPES], adjoint="eval_adjoint_penalty_sensitivities_device")


def _rehearse(plan, fills=None):
    """The layer's next allocations on the current stream, rehearsed: tensors of the plan's shapes and types are allocated in its order
    (None: the block before the last is released there, as the layer's temporary is), filled (``fills[i]``, default STALE everywhere)
    and released, so that the caching allocator -- best fit, deterministic -- hands the same blocks to the same requests again.  Returns
    the pointers of the blocks that stay to the end, in order."""
    held = []
    for item in plan:
        if item is None:
            del held[-2]
        else:
            held.append(torch.empty(item[0], dtype=item[1], device="cuda:0"))
    for i, t in enumerate(held):
        if fills is not None and i < len(fills):
            t.copy_(fills[i])
        else:
            t.fill_(STALE if t.dtype == F64 else 7)
    return [t.data_ptr() for t in held]


def _spy(s, name, log):
    """Notes the arguments of the solver's method ``name`` (an instance attribute in front of the method; _unspy takes it away)."""
    orig = getattr(s, name)

    def noted(*a, **kw):
        log.append(a)
        return orig(*a, **kw)

    setattr(s, name, noted)


def _unspy(s, *names):
    for n in names:
        if n in vars(s):
            delattr(s, n)


def _premise(what, got, want):
    assert list(got) == list(want), (f"{what}: the allocator did not hand the rehearsed blocks to the layer ({[hex(p) for p in got]} against "
                                      f"{[hex(p) for p in want]}), so what a missing wait would read is not the prepared stale data: the "
                                      "premise of this test is gone, and it must not pass on luck")


def _rolled_weights(case):
    sym = lambda a: (a + np.swapaxes(a, 1, 2)) * 0.5  # noqa: E731
    return [_t(np.roll(sym(case["ins"]["W"]), 1, axis=0)), _t(np.roll(sym(case["ins"]["W_e"]), 1, axis=0))]


def _reference(case, c):
    """The same call on the default stream, everything synchronised: outputs and gradients as numpy arrays."""
    torch.cuda.synchronize()
    c.restore()
    t = {k: _t(v, True) for k, v in case["ins"].items()}
    out = dict(zip(case["outs"], case["call"](t)))
    loss = sum((_t(v) * out[k]).sum() for k, v in case["seeds"].items())
    g = torch.autograd.grad(loss, list(t.values()))
    torch.cuda.synchronize()
    res = {k: v.detach().cpu().numpy() for k, v in out.items()}
    res.update({"gradient in " + k: v.cpu().numpy() for k, v in zip(t, g)})
    return res


def _finish(c, held, delay, n_delays):
    """Every delay happened; then the lifetime rule: free() refuses while a view of a layer output is held, and succeeds after."""
    delay.check(n_delays)
    gc.collect()
    with pytest.raises(RuntimeError, match="still alive"):
        c.s.free()
    held.clear()
    gc.collect()
    c.s.free()


def _on_side_streams(body):
    """The body on SIDES consecutive streams of torch's pool, one after the other: HIP multiplexes a process's streams onto a few
    hardware queues (four by default), and two streams that share a queue are ordered whatever the events say -- on such a pair a missing
    wait reads no stale data.  Consecutive streams of the pool sit on consecutive queues, so at most one of four shares the handle's.
    Returns the list of the runs' results and the views that keep the handle from being freed."""
    runs, held = [], []
    for _ in range(SIDES):
        res, h = body(torch.cuda.Stream())
        runs.append(res)
        held += h
    return runs, held


def _judge(what, runs, ref):
    assert len(runs) == SIDES and all(runs), what
    for i, res in enumerate(runs):
        bitcmp.assert_all_same_bits(f"{what} (side stream {i + 1} of {SIDES})", res, ref, keys=list(res))


# ---- forward inputs: the handle's stream behind torch's ----

@pytest.mark.parametrize("kind", ["soft", "rti", "plant"])
def test_forward_waits_for_the_inputs(track, cycles_per_ms, kind):
    """Every input holds its rolled values; on the side stream the delay, then copy_ of the true values, then the call.  A forward whose
    handle stream does not wait for torch's stream solves the rolled problem (the symmetrised weights included: their blocks hold the
    rolled ones, asserted by pointer)."""
    c = _Start(track, B)
    case, delay = _case(kind, c), _Delay(cycles_per_ms)
    seen = []

    def body(side):
        true = {k: _t(v) for k, v in case["ins"].items()}
        buf = {k: _t(np.roll(v, 1, axis=0)) for k, v in case["ins"].items()}
        stale_w = _rolled_weights(case) if kind != "plant" else None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        c.restore()
        if kind != "plant":
            _unspy(c.s, "set_instance_weights_device")
            _spy(c.s, "set_instance_weights_device", seen)
        with torch.cuda.stream(side):
            want = _rehearse(case["fwd"][:6], stale_w)[:2] if kind != "plant" else []
            delay()
            for k in buf:
                buf[k].copy_(true[k])
            for k in buf:
                buf[k].requires_grad_(True)
            out = dict(zip(case["outs"], case["call"](buf)))
            loss = sum((_t(v) * out[k]).sum() for k, v in case["seeds"].items())
            g = torch.autograd.grad(loss, list(buf.values()))
            res = {k: v.detach().cpu().numpy() for k, v in out.items()}
            res.update({"gradient in " + k: v.cpu().numpy() for k, v in zip(buf, g)})
        if kind != "plant":
            _premise("the symmetrised weights", seen[-1][:2], want)
        return res, [out[case["outs"][0]].detach()[:1]]

    runs, held = _on_side_streams(body)
    _unspy(c.s, "set_instance_weights_device")
    ref = _reference(case, c)
    _judge(f"{kind} on a side stream, inputs written behind a delay, against the default stream", runs, ref)
    _finish(c, held, delay, SIDES)


# ---- forward outputs: torch's stream behind the handle's ----

@pytest.mark.parametrize("kind", ["soft", "rti", "plant"])
def test_outputs_wait_for_the_handles_stream(track, cycles_per_ms, kind):
    """The delay sits on the handle's own stream (ihm2mpc_get_stream is there for callers that enqueue their own work) directly before the
    call; every output is cloned on the side stream directly after it.  The outputs' blocks hold 0.25 (rehearsed, asserted by pointer):
    a forward that does not make torch's stream wait for the handle's hands those out."""
    c = _Start(track, B)
    case, delay = _case(kind, c), _Delay(cycles_per_ms)

    def body(side):
        t = {k: _t(v, True) for k, v in case["ins"].items()}
        stale_w = _rolled_weights(case) if kind != "plant" else None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        c.restore()
        hs = torch.cuda.ExternalStream(c.s.get_stream())
        with torch.cuda.stream(side):
            want = _rehearse(case["fwd"], stale_w)
            with torch.cuda.stream(hs):
                delay()
            out = case["call"](t)
            clones = [o.clone() for o in out]
            res = {k: v.detach().cpu().numpy() for k, v in zip(case["outs"], clones)}
        n = len(case["outs"])
        if kind == "plant":         # x_next, (Sx, Su: kept for backward), model_used
            want = [want[0], want[3]]
        _premise("the outputs", [o.data_ptr() for o in out], want[-n:])
        return res, [out[0].detach()[:1]]

    runs, held = _on_side_streams(body)
    ref = _reference(case, c)
    _judge(f"{kind} on a side stream, the handle's stream held before the call, against the default stream", runs, ref)
    _finish(c, held, delay, SIDES)


# ---- backward seeds: the handle's stream behind torch's, in backward ----

@pytest.mark.parametrize("kind", ["soft", "rti"])
def test_backward_waits_for_the_seeds(track, cycles_per_ms, kind):
    """Between the layer's outputs and the loss sits _LateSeed: the seeds reach the layer's backward in buffers that held the rolled
    seeds until a copy behind a delay on torch's stream."""
    c = _Start(track, B)
    case, delay = _case(kind, c), _Delay(cycles_per_ms)

    def body(side):
        t = {k: _t(v, True) for k, v in case["ins"].items()}
        bufs = {k: _t(np.roll(v, 1, axis=0)) for k, v in case["seeds"].items()}
        seeds = {k: _t(v) for k, v in case["seeds"].items()}
        stale_w = _rolled_weights(case)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        c.restore()
        with torch.cuda.stream(side):
            _rehearse(case["fwd"][:6], stale_w)
            out = dict(zip(case["outs"], case["call"](t)))
            loss = sum((seeds[k] * _LateSeed.apply(out[k], bufs[k], delay)).sum() for k in seeds)
            g = torch.autograd.grad(loss, list(t.values()))
            res = {"gradient in " + k: v.cpu().numpy() for k, v in zip(t, g)}
            res.update({k: v.detach().cpu().numpy() for k, v in out.items()})
        return res, [out["x"].detach()[:1]]

    runs, held = _on_side_streams(body)
    ref = _reference(case, c)
    _judge(f"{kind} on a side stream, the seeds written behind a delay, against the default stream", runs, ref)
    _finish(c, held, delay, SIDES * len(case["seeds"]))


# ---- backward gradients: torch's stream behind the handle's, in backward; and the cold handle ----

@pytest.mark.parametrize("cold", [False, True])
@pytest.mark.parametrize("kind", ["soft", "rti"])
def test_gradients_wait_for_the_handles_stream(track, cycles_per_ms, kind, cold):
    """The delay sits on the handle's stream directly before torch.autograd.grad (the seeds go in as grad_outputs: the layer's backward
    is the first node); the gradients are cloned on the side stream directly after.  Their blocks hold 0.25 (rehearsed; the pointers the
    adjoint entry is given are asserted).  cold: the handle's first adjoint call ever is this delayed one, so the first allocation of
    the adjoint buffers (and of the penalty gradients' workspace, for rti_solve_soft) happens while the handle's stream is held --
    the state NOTES.md R29 names as a suspect; warm: one solve and one adjoint call on the host entries come before."""
    c = _Start(track, B)
    case, delay = _case(kind, c), _Delay(cycles_per_ms)
    seen = []

    def body(side):
        if not cold and not seen:
            c.s.solve()
            (c.s.eval_adjoint_penalty_sensitivities if kind == "soft" else c.s.eval_adjoint_weight_sensitivities)()
        t = {k: _t(v, True) for k, v in case["ins"].items()}
        seeds = [_t(v) for v in case["seeds"].values()]
        stale_w = _rolled_weights(case)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        c.restore()
        hs = torch.cuda.ExternalStream(c.s.get_stream())
        _unspy(c.s, case["adjoint"])
        _spy(c.s, case["adjoint"], seen)
        with torch.cuda.stream(side):
            _rehearse(case["fwd"][:6], stale_w)
            out = case["call"](t)
            # (the forward's own temporaries were marked with record_stream: the allocator takes their blocks back only once the
            # handle's stream has passed them -- before the rehearsal, not somewhere between it and backward)
            torch.cuda.synchronize()
            want = _rehearse(case["bwd"])
            with torch.cuda.stream(hs):
                delay()
            g = torch.autograd.grad(list(out[:len(seeds)]), list(t.values()), grad_outputs=seeds)
            clones = [v.clone() for v in g]
            res = {"gradient in " + k: v.cpu().numpy() for k, v in zip(t, clones)}
        want = want[-len(t):]
        _premise("the gradients", seen[-1][-len(want):], want)
        return res, [out[0].detach()[:1]]

    runs, held = _on_side_streams(body)
    _unspy(c.s, case["adjoint"])
    ref = _reference(case, c)
    _judge(f"{kind} ({'cold' if cold else 'warm'} handle) on a side stream, the handle's stream held before backward, against the default stream",
           runs, ref)
    _finish(c, held, delay, SIDES)
