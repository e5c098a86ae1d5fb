"""CPU: autograd_ops.wgrad_queue under nested, raised, back-to-back and engine-less backward passes.  The real autograd engine drives
tiny Functions whose backward parks a problem; ops.wgrad_tn_group is replaced by a recorder, so no kernel runs.  A problem is a
(dz, x, out, db) tuple; ``out`` stands for the arena slot it writes and identifies it here."""
import pytest
import torch

from vimo_clip_amd import autograd_ops as ag
from vimo_clip_amd import ops


class _Param:
    """Stands for a parameter in the hooks (the queue only hands it through)."""

    def __init__(self, name):
        self.name = name


def _problem(name):
    """A parked problem: 16-bit operands (one 256 x 256 tile) and the slot it writes."""
    dz = torch.zeros((4, 8), dtype=torch.bfloat16)
    x = torch.zeros((4, 8), dtype=torch.bfloat16)
    return dz, x, torch.zeros((8, 8)), None, [_Param(name)]


class _Push(torch.autograd.Function):
    """Identity whose backward parks the problem called `name` (and raises after it if told to)."""

    @staticmethod
    def forward(ctx, x, name, slots, fail):
        ctx.name, ctx.slots, ctx.fail = name, slots, fail
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        dz, x, out, db, params = _problem(ctx.name)
        ctx.slots[ctx.name] = out
        ag.wgrad_queue.push(dz, x, out, db, params)
        if ctx.fail:
            raise RuntimeError("backward failed on purpose")
        return dy, None, None, None


class _Nested(torch.autograd.Function):
    """Identity whose backward runs an inner engine pass (what torch.utils.checkpoint does) over two pushing Functions."""

    @staticmethod
    def forward(ctx, x, slots, fail_inner):
        ctx.slots, ctx.fail_inner = slots, fail_inner
        return x.clone()

    @staticmethod
    def backward(ctx, dy):
        with torch.enable_grad():
            leaf = dy.detach().requires_grad_(True)
            y = _Push.apply(_Push.apply(leaf, "inner_a", ctx.slots, ctx.fail_inner), "inner_b", ctx.slots, False)
        if ctx.fail_inner:
            try:
                torch.autograd.backward(y, dy)
            except RuntimeError:
                return dy, None, None           # the block is skipped; the pass around it goes on
        else:
            torch.autograd.backward(y, dy)
        return leaf.grad, None, None


@pytest.fixture()
def queue(monkeypatch):
    """(launches, fired, slots): every launch as the list of slots it writes, the names of the parameters whose hook fired."""
    launches, fired, slots = [], [], {}
    monkeypatch.setattr(ops, "wgrad_tn_group", lambda probs, dtype16: launches.append([p[2] for p in probs]))
    q = ag.wgrad_queue
    monkeypatch.setattr(q, "enabled", True)
    q.items, q.tiles, q._task, q._armed = [], 0, -1, set()
    hook = lambda p: fired.append(p.name)                     # noqa: E731
    ag.grad_ready_hooks.append(hook)
    try:
        yield launches, fired, slots
    finally:
        ag.grad_ready_hooks.remove(hook)
        q.items, q.tiles, q._task, q._armed = [], 0, -1, set()


def _names(launches, slots):
    back = {id(t): k for k, t in slots.items()}
    return [[back[id(t)] for t in launch] for launch in launches]


def test_nested_pass_launches_every_problem_once(queue):
    launches, fired, slots = queue
    x = torch.ones(3, requires_grad=True)
    y = _Push.apply(_Nested.apply(_Push.apply(x, "outer_first", slots, False), slots, False), "outer_last", slots, False)
    y.sum().backward()
    got = sorted(n for launch in _names(launches, slots) for n in launch)
    assert got == ["inner_a", "inner_b", "outer_first", "outer_last"], got      # the outer pass's parked problem survives the inner pass
    assert sorted(fired) == got                                                 # ... and every gradient-ready hook fires once
    assert not ag.wgrad_queue.items
    assert torch.equal(x.grad, torch.ones(3))


def test_nested_pass_that_raised_is_dropped_and_the_outer_pass_completes(queue):
    launches, fired, slots = queue
    x = torch.ones(3, requires_grad=True)
    y = _Push.apply(_Nested.apply(_Push.apply(x, "outer_first", slots, False), slots, True), "outer_last", slots, False)
    y.sum().backward()
    got = sorted(n for launch in _names(launches, slots) for n in launch)
    # inner_b and inner_a were parked, then inner_a raised: the inner pass is known to have failed, what it parked is not launched
    assert got == ["outer_first", "outer_last"], got
    assert sorted(fired) == got and not ag.wgrad_queue.items


def test_raised_pass_is_not_launched_with_the_next_pass(queue):
    launches, fired, slots = queue
    x = torch.ones(3, requires_grad=True)
    with pytest.raises(RuntimeError, match="on purpose"):
        _Push.apply(_Push.apply(x, "w1", slots, True), "w0", slots, False).sum().backward()
    stale = dict(slots)                                   # w0 was parked, w1 was parked and raised: no end-of-pass callback ran
    assert launches == [] and len(ag.wgrad_queue.items) == 2
    _Push.apply(_Push.apply(x, "w1", slots, False), "w0", slots, False).sum().backward()
    new = {id(t) for t in slots.values()}
    old = {id(t) for t in stale.values()}
    for launch in launches:                               # no launch mixes the stale writers with the new writers of the same slots
        ids = {id(t) for t in launch}
        assert not (ids & old and ids & new), launches
    assert [id(t) for t in launches[-1]] == [id(slots["w0"]), id(slots["w1"])]       # the clean pass leaves last, complete, once
    assert sum(len(launch) for launch in launches if {id(t) for t in launch} & new) == 2
    assert not ag.wgrad_queue.items


def test_back_to_back_passes_carry_nothing_over(queue):
    launches, fired, slots = queue
    x = torch.ones(3, requires_grad=True)
    for step in range(3):
        _Push.apply(_Push.apply(x, "b", slots, False), "a", slots, False).sum().backward()
        assert len(launches) == step + 1 and [id(t) for t in launches[-1]] == [id(slots["a"]), id(slots["b"])]
        assert not ag.wgrad_queue.items and ag.wgrad_queue.tiles == 0
    assert fired == ["a", "b"] * 3


def test_push_outside_an_engine_pass_flushes_at_once(queue):
    launches, fired, slots = queue
    assert torch._C._current_graph_task_id() < 0
    for name in ("p", "q"):
        dz, x, out, db, params = _problem(name)
        ag.wgrad_queue.push(dz, x, out, db, params)
        assert len(launches[-1]) == 1 and launches[-1][0] is out and not ag.wgrad_queue.items
    assert len(launches) == 2 and fired == ["p", "q"]
