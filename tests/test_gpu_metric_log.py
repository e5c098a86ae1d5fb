"""GPU: the device-resident epoch log (vmc_metric_append, include/vmc.h K18; metrics.DeviceMetricLog) against the numpy reference
tests/metric_log_ref.py, and a trainer that logs on the device against the trainer that keeps the host metric classes.

Every comparison is exact: the kernel copies fp32 rows, truncates labels and makes one IEEE decision per call, ``loss_sum`` is one
fp32 add per call in call order (the reference adds np.float32 sequentially), and the trainer comparison runs the same kernels on
the same values in both runs.  Log buffers are allocated here with 4 canary rows behind ``capacity`` inside the same allocation
and pre-filled, so that a write out of range or a row left unwritten shows up.
"""
import ctypes

import numpy as np
import pytest
import torch

import metric_log_ref as ref
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
CANARY = 4
FILL = (-7.25, 0xEE, 0xDD)           # value, target and squash bytes of rows nobody wrote
NEXT1 = float(np.nextafter(np.float32(1), np.float32(2)))


def _canary_log(capacity, C, task="multilabel"):
    """A DeviceMetricLog whose row buffers are views of allocations with CANARY more rows behind them, all pre-filled."""
    from vimo_clip_amd.metrics import DeviceMetricLog
    log = DeviceMetricLog(capacity, C, task, "cuda")
    log.big = (torch.full((capacity + CANARY, C), FILL[0], dtype=torch.float32, device="cuda"),
               torch.full((capacity + CANARY, C), FILL[1], dtype=torch.uint8, device="cuda"),
               torch.full((capacity + CANARY,), FILL[2], dtype=torch.uint8, device="cuda"))
    log.values, log.targets, log.squash = (b[:capacity] for b in log.big)          # before the first append builds the C struct
    return log


def _abi_append(log, v, t, loss):
    """One call through the C ABI itself (not DeviceMetricLog.append)."""
    from vimo_clip_amd import _lib
    v, t = v.cuda().contiguous(), t.cuda().contiguous()
    l = None if loss is None else torch.tensor([loss], dtype=torch.float32, device="cuda")
    rc = _lib.lib.vmc_metric_append(log._c_log(), v.data_ptr(), t.data_ptr(), None if l is None else l.data_ptr(), v.shape[0], _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()                 # v, t, l die with this frame


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)


def _check(log, calls, capacity, C):
    want = ref.apply_calls([(v.numpy(), t.numpy(), l) for v, t, l in calls], capacity, C, fill=FILL)
    vals, tgts, sq = (b.cpu().numpy() for b in log.big)
    small = log._small.cpu()
    got = dict(rows=int(small[0]), steps=int(small[1]), status=int(small[2]))
    assert got == {k: want[k] for k in got}, (got, want["rows"], want["steps"], want["status"])
    assert int(small[3]) == 0
    assert _bits(small[4:5].view(torch.float32).numpy())[0] == _bits(np.array([want["loss_sum"]], dtype=np.float32))[0]
    assert np.array_equal(_bits(vals[:capacity]), _bits(want["values"]))
    assert np.array_equal(tgts[:capacity], want["targets"]) and np.array_equal(sq[:capacity], want["squash"])
    # the canary rows
    assert np.array_equal(_bits(vals[capacity:]), _bits(np.full((CANARY, C), FILL[0], dtype=np.float32)))
    assert (tgts[capacity:] == FILL[1]).all() and (sq[capacity:] == FILL[2]).all()
    return want


def _calls(C, sizes, seed):
    """Alternating logits / inside-[0, 1] calls with a NaN, fractional labels (0.9 -> 0, 1.5 -> 1) and a loss each."""
    g = torch.Generator().manual_seed(seed)
    calls = []
    for i, B in enumerate(sizes):
        v = torch.randn(B, C, generator=g) * 3 if i % 2 == 0 else torch.rand(B, C, generator=g)
        if i % 2 == 0:
            v[-1, -1] = -2.5                              # whatever the seed drew: a logits call has a value outside [0, 1]
        if i == 2:
            v[0, 0] = float("nan")
        t = (torch.rand(B, C, generator=g) < 0.3).float()
        t[0, 0], t[-1, -1] = 0.9, 1.5
        calls.append((v, t, float(torch.randn((), generator=g)) * 3))
    return calls


@pytest.mark.parametrize("C", [1, 7, 140, 141])
def test_append_sequence_equals_the_reference(C):
    sizes = (1, 8, 3, 32)                    # the destination offset takes every alignment
    capacity = sum(sizes)
    log = _canary_log(capacity, C)
    calls = _calls(C, sizes, seed=C)
    for v, t, l in calls:
        _abi_append(log, v, t, l)
    want = _check(log, calls, capacity, C)
    assert want["rows"] == capacity and want["status"] == 0
    assert want["squash"][[0, 1, 9, 12]].tolist() == [1, 0, 1, 0]


def test_large_call_behind_an_odd_offset():
    C, capacity = 140, 3 + 4096
    log = _canary_log(capacity, C)
    calls = _calls(C, (3, 4096), seed=5)
    calls[0] = (calls[0][0], calls[0][1], None)            # a call without a loss
    for v, t, l in calls:
        _abi_append(log, v, t, l)
    want = _check(log, calls, capacity, C)
    assert want["rows"] == capacity and want["steps"] == 2 and want["squash"][3:].max() == 0 and want["squash"][:3].min() == 1


def _flag_case(name):
    base = torch.tensor([0.0, -0.0, 1.0, 0.5])
    if name == "large":
        v = torch.rand(4096, 140, generator=torch.Generator().manual_seed(3))
        v[-1, -1] = 2.0
        return v
    v = base.repeat(3 * 7 * 4)[:3 * 7].reshape(3, 7).clone() if name not in ("nan", "nan_two") else torch.full((3, 7), float("nan"))
    if name == "above":
        v[-1, -1] = NEXT1
    elif name == "below":
        v[0, 0] = -1e-30
    elif name == "nan_two":
        v[1, 3] = 2.0
    return v


@pytest.mark.parametrize("name, flag", [("inside", 0), ("above", 1), ("below", 1), ("nan", 0), ("nan_two", 1), ("large", 1)])
def test_squash_flag_edge_cases(name, flag):
    v = _flag_case(name)
    B, C = v.shape
    p = v.cuda()
    assert int(bool(((p < 0) | (p > 1)).any())) == flag          # the decision of MultilabelAveragePrecision.update, on the device
    log = _canary_log(B + 2, C)
    calls = [(v, torch.zeros(B, C), 0.5)]
    _abi_append(log, *calls[0])
    want = _check(log, calls, B + 2, C)
    assert want["squash"][:B].tolist() == [flag] * B and log.big[2][:B].cpu().tolist() == [flag] * B


def test_full_log_refuses_the_call_and_read_raises():
    C, capacity = 7, 10
    log = _canary_log(capacity, C)
    calls = _calls(C, (8, 8), seed=9)
    for v, t, l in calls:
        _abi_append(log, v, t, l)
    want = _check(log, calls, capacity, C)                 # rows 8-9 and the canaries keep their fill, loss_sum is the first loss
    assert (want["rows"], want["steps"], want["status"]) == (8, 1, 1)
    assert want["loss_sum"] == np.float32(calls[0][2])
    with pytest.raises(RuntimeError, match="refused"):
        log.read()
    log.reset()
    assert log.read() == (0, 0, 0, 0.0)
    log.append(calls[1][0].cuda(), calls[1][1].cuda())     # fits again
    assert log.read()[:3] == (8, 1, 0)


def test_label_outside_0_1_is_stored_and_reported():
    C = 7
    log = _canary_log(4, C)
    t = torch.zeros(2, C)
    t[1, 2] = 2.0
    calls = [(torch.rand(2, C), t, 1.0)]
    _abi_append(log, *calls[0])
    want = _check(log, calls, 4, C)
    assert want["status"] == 2 and int(log.targets[1, 2]) == 2
    with pytest.warns(RuntimeWarning, match="label outside"):
        assert log.read() == (2, 1, 2, 1.0)


def test_argument_errors():
    from vimo_clip_amd import _lib
    from vimo_clip_amd.metrics import MetricLogStruct
    log = _canary_log(4, 7)
    v, t = torch.zeros(2, 7, device="cuda"), torch.zeros(2, 7, device="cuda")

    def call(lg=None, values=v.data_ptr(), targets=t.data_ptr(), B=2, **fields):
        s = MetricLogStruct.from_buffer_copy(log._struct) if lg is None else lg
        for k, val in fields.items():
            setattr(s, k, val)
        return _lib.lib.vmc_metric_append(ctypes.addressof(s), values, targets, None, B, _lib.stream())
    log._c_log()
    E_ARG = -1
    assert call() == 0
    assert call(values=None) == E_ARG and call(targets=None) == E_ARG and call(B=0) == E_ARG and call(B=-1) == E_ARG
    assert _lib.lib.vmc_metric_append(None, v.data_ptr(), t.data_ptr(), None, 2, _lib.stream()) == E_ARG
    for f in ("values", "targets", "squash", "state", "loss_sum"):
        assert call(**{f: None}) == E_ARG, f
    assert call(capacity=0) == E_ARG and call(C=0) == E_ARG
    torch.cuda.synchronize()
    assert log.read()[:3] == (2, 1, 0)
    with pytest.raises(ValueError, match="do not match"):
        log.append(v, t[:1])


def test_captured_append_replays_equal_eager_appends():
    C, B = 141, 8
    calls = _calls(C, (B,) * 5, seed=21)
    eager, graphed = _canary_log(5 * B, C), _canary_log(5 * B, C)
    for v, t, l in calls:
        eager.append(v.cuda(), t.cuda(), torch.tensor(l, device="cuda"))
    from vimo_clip_amd.graphs import GraphedCallable
    x, y, l0 = torch.zeros(B, C, device="cuda"), torch.zeros(B, C, device="cuda"), torch.zeros((), device="cuda")
    g = GraphedCallable(lambda a, b, c: graphed.append(a, b, c), x, y, l0, warmup=1)       # the warm-up adds a batch ...
    assert graphed.read()[:2] == (B, 1)                    # ... and the capture runs nothing
    graphed.reset()                                        # undone, as GraphedTrainStep(extra_live=) does
    x, y, l0 = g.static_inputs
    for v, t, l in calls:
        x.copy_(v), y.copy_(t), l0.fill_(l)
        g.replay()
    torch.cuda.synchronize()
    _check(graphed, calls, 5 * B, C)
    for a, b in zip(eager.big + (eager._small,), graphed.big + (graphed._small,)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


def test_capture_runs_with_the_cyclic_collector_off_and_restores_it():
    """A collection inside a capture may destroy the captured graphs of a dropped trainer (a trainer and its GraphedTrainStep
    reference each other), which is not allowed while a stream captures: GraphedCallable keeps the collector off for the capture
    only, and leaves it as it found it."""
    import gc

    from vimo_clip_amd.graphs import GraphedCallable
    seen = []

    def fn(x):
        seen.append(gc.isenabled())
        return x + 1

    assert gc.isenabled()
    g = GraphedCallable(fn, torch.zeros(4, device="cuda"), warmup=1)
    assert seen == [True, False] and gc.isenabled()
    assert g(torch.ones(4, device="cuda")).tolist() == [2.0] * 4
    gc.disable()
    try:
        GraphedCallable(fn, torch.zeros(4, device="cuda"), warmup=1)
        assert not gc.isenabled()                          # off before, off after
    finally:
        gc.enable()


def test_compute_equals_the_host_metric_classes():
    from vimo_clip_amd.metrics import Accuracy, DeviceMetricLog, MultilabelAveragePrecision
    C = 141
    g = torch.Generator().manual_seed(4)
    inside = torch.rand(8, C, generator=g)
    edge = torch.rand(3, C, generator=g)
    edge[-1, -1] = NEXT1
    vals = [torch.randn(1, C, generator=g) * 6, inside, edge, torch.randn(32, C, generator=g) * 6]
    log, host = DeviceMetricLog(44, C, "multilabel"), MultilabelAveragePrecision(num_labels=C, average="micro")
    for v in vals:
        v, t = v.cuda(), (torch.rand(v.shape, generator=g) < 0.2).float().cuda()
        log.append(v, t)
        host.update(v, t.to(dtype=torch.int))
    assert log.squash[[0, 1, 9, 12]].tolist() == [1, 0, 1, 1]
    got, want = float(log.compute()), float(host.compute())
    print(f"multilabel: log {got!r} host {want!r}")
    assert 0.0 < want < 1.0 and got == want

    C = 12
    log, host = DeviceMetricLog(44, C, "singlelabel"), Accuracy(num_classes=C)
    for B in (1, 8, 3, 32):
        v = torch.randn(B, C, generator=g).cuda()
        t = torch.nn.functional.one_hot(torch.randint(0, C, (B,), generator=g), C).float().cuda()
        t[::2] = torch.nn.functional.one_hot(v[::2].argmax(dim=1), C).float()
        log.append(v, t)
        host.update(v, t.to(dtype=torch.int))
    got, want = float(log.compute()), float(host.compute())
    print(f"singlelabel: log {got!r} host {want!r}")
    assert 0.0 < want < 1.0 and got == want


# ---- the trainer ----------------------------------------------------------------------------------------------------------------

D, H, L, FF, BATCH = 512, 8, 1, 512, 8


def _sets(task, C):
    from vimo_clip_amd.TFAM.data.dataset import SyntheticEmbeddingDataset
    if task == "singlelabel":
        labels = [torch.nn.functional.one_hot(synth.randint(s, "cls", (n,), 0, C), C).float() for s, n in ((1, 48), (2, 16))]
    else:
        labels = [synth.multi_hot_labels(s, tag, n, C) for s, tag, n in ((1, "tr", 48), (2, "va", 16))]
    return (SyntheticEmbeddingDataset(labels[0], D, tmin=17, tmax=40, seed=5, class_seed=5),
            SyntheticEmbeddingDataset(labels[1], D, tmin=17, tmax=40, seed=6, class_seed=5))


def _trainer(tr, va, task, C, use_graphs, device_store, graph_bucket, device_metrics):
    from vimo_clip_amd import autograd_ops as ag
    from vimo_clip_amd.TFAM.models import AMO_CLIP
    from vimo_clip_amd.TFAM.train_and_eval import Config, ModelTrainer
    ag.weights.clear()
    cfg = Config(epochs=2, batch_size=BATCH, d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, device="cuda",
                 checkpoint_dir=None, task=task, dropout=0.1, mlp_dropout=0.1, use_graphs=use_graphs, graph_bucket=graph_bucket,
                 device_store=device_store, device_metrics=device_metrics)
    m = AMO_CLIP(d_model=D, nhead=H, num_layers=L, dim_feedforward=FF, num_classes=C, device="cuda", dropout=0.1, mlp_dropout=0.1).cuda()
    m.load_state_dict(synth.tfam_state_dict(D, H, L, FF, C, 83), strict=True)
    m.set_dropout_seed(cfg.seed * 1000)
    return ModelTrainer(m, tr, va, cfg)


@pytest.mark.parametrize("task, C", [("multilabel", 140), ("singlelabel", 12)])
@pytest.mark.parametrize("use_graphs, device_store, graph_bucket", [(False, False, 1), (True, False, 16), (True, True, 16)],
                         ids=["eager", "graphs", "graphs_store"])
def test_trainer_with_device_metrics_equals_trainer_without(monkeypatch, use_graphs, device_store, graph_bucket, task, C):
    """Two epochs of 6 training steps and 2 validation batches (B = 8, clips of 17..40 tokens, dropout 0.1): the four floats of
    every epoch and all parameters are those of the run that keeps the host metric classes, which the logging run never calls."""
    from vimo_clip_amd import metrics
    tr, va = _sets(task, C)
    runs = []
    for on in (False, True):
        if on:
            def boom(*a, **k):
                raise AssertionError("host metric update reached with device_metrics on")
            monkeypatch.setattr(metrics.MultilabelAveragePrecision, "update", boom)
            monkeypatch.setattr(metrics.Accuracy, "update", boom)
        t = _trainer(tr, va, task, C, use_graphs, device_store, graph_bucket, on)
        assert (t._train_log is not None) == on and (t._val_log is not None) == on
        stats = []
        for epoch in (0, 1):
            stats.append(t.train_epoch(epoch) + t.validate(epoch))
            if on:
                rows, steps, status, _ = t._train_log.read()
                assert (rows, steps, status) == (6 * BATCH, 6, 0)          # the epoch with the captures included: warm-ups added nothing
                assert t._val_log.read()[:3] == (2 * BATCH, 2, 0)
        runs.append((stats, t.arena.flat_param.detach().clone()))
    (s_off, p_off), (s_on, p_on) = runs
    print(f"{task} graphs={use_graphs} store={device_store}: off {s_off} on {s_on}")
    assert all(len(s) == 4 and all(np.isfinite(s)) for s in s_off)
    assert s_on == s_off
    assert torch.equal(p_on, p_off)
    if use_graphs:
        assert t._graphed_train.n_graphs >= 1 and t._graphed_train.extra_live == t._train_log.state_tensors()
