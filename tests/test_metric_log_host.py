"""CPU: the host side of the device-resident epoch log (vmc_metric_append; the kernel is checked on the GPU in
tests/test_gpu_metric_log.py).  The evaluation function against the host metric classes and the oracle, its data-parallel gather
over gloo, what the graph manager saves around a capture, and the trainer's option.

Tolerances.  Per-batch and whole-buffer ``torch.sigmoid`` differ in the last bit of a few elements on the CPU (vectorised body vs
scalar tail), so the AP is compared with the project's AP bound, 1e-6 (tests/test_host_logic.py); on the function's OWN scores the
float64 arithmetic is the oracle's, compared to 1e-12.  Accuracy counts integers: exact.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from metric_log_ref import apply_calls
from oracle import metrics as ometrics

C = 141
SIZES = (1, 8, 3, 32)


def _multilabel_calls(seed=0):
    """Ragged update calls: logits, a batch entirely inside [0, 1] (not squashed), a batch whose only offender is nextafter(1, 2)
    (squashed), logits again."""
    g = torch.Generator().manual_seed(seed)
    inside = torch.rand(SIZES[1], C, generator=g)
    inside[0, :4] = torch.tensor([0.0, -0.0, 1.0, 0.5])
    edge = torch.rand(SIZES[2], C, generator=g)
    edge[-1, -1] = float(np.nextafter(np.float32(1), np.float32(2)))
    vals = [torch.randn(SIZES[0], C, generator=g) * 6, inside, edge, torch.randn(SIZES[3], C, generator=g) * 6]
    return [(v, (torch.rand(v.shape, generator=g) < 0.2).float(), float(i) + 0.25) for i, v in enumerate(vals)]


def _singlelabel_calls(seed=1, classes=12):
    g = torch.Generator().manual_seed(seed)
    calls = []
    for B in SIZES:
        v = torch.randn(B, classes, generator=g)
        y = torch.nn.functional.one_hot(torch.randint(0, classes, (B,), generator=g), classes).float()
        y[::2] = torch.nn.functional.one_hot(v[::2].argmax(dim=1), classes).float()      # some rows right, some (mostly) wrong
        calls.append((v, y, 1.0))
    return calls


def _logged(calls, width):
    r = apply_calls([(v.numpy(), t.numpy(), l) for v, t, l in calls], sum(SIZES), width)
    assert r["rows"] == sum(SIZES) and r["steps"] == len(calls) and r["status"] == 0
    return torch.from_numpy(r["values"]), torch.from_numpy(r["targets"]), torch.from_numpy(r["squash"])


def test_evaluation_equals_the_host_metric_classes():
    from vimo_clip_amd.metrics import Accuracy, MultilabelAveragePrecision, evaluate_log, log_scores
    calls = _multilabel_calls()
    values, targets, squash = _logged(calls, C)
    assert [int(squash[sum(SIZES[:i])]) for i in range(4)] == [1, 0, 1, 1]
    host = MultilabelAveragePrecision(num_labels=C, average="micro")
    for v, t, _ in calls:
        host.update(v, t.to(torch.int))
    ap = evaluate_log(values, targets, squash, "multilabel")
    assert ap.dtype == torch.float32 and 0.0 < float(ap) < 1.0
    assert abs(float(ap) - float(host.compute())) < 1e-6
    ap64 = evaluate_log(values, targets, squash, "multilabel", out_dtype=torch.float64)
    want = ometrics.micro_average_precision(log_scores(values, squash).numpy(), targets.numpy())
    assert abs(float(ap64) - want) < 1e-12
    assert float(ap) == float(ap64.to(torch.float32))
    # rows the flag does not cover are taken as they are: squashing the inside batch as well moves the result
    assert float(evaluate_log(values, targets, torch.ones_like(squash), "multilabel")) != float(ap)

    calls = _singlelabel_calls()
    values, targets, squash = _logged(calls, 12)
    host = Accuracy(num_classes=12)
    for v, t, _ in calls:
        host.update(v, t.to(torch.int))
    acc = evaluate_log(values, targets, squash, "singlelabel")
    assert acc.dtype == torch.float32 and 0.0 < float(acc) < 1.0
    assert float(acc) == float(host.compute())

    empty = evaluate_log(values[:0], targets[:0], squash[:0], "multilabel", out_dtype=torch.float64)
    assert torch.isnan(empty) and empty.dtype == torch.float64 and empty.device == values.device and empty.dim() == 0
    with pytest.raises(ValueError, match="Unsupported task"):
        evaluate_log(values, targets, squash, "regression")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _host_log(values, targets, squash, task):
    """A DeviceMetricLog on the CPU holding the given rows (append needs the GPU; read and compute do not)."""
    from vimo_clip_amd.metrics import DeviceMetricLog
    n = values.shape[0]
    log = DeviceMetricLog(n + 3, values.shape[1], task, device="cpu")
    log.values[:n], log.targets[:n], log.squash[:n] = values, targets, squash
    log.values[n:], log.squash[n:] = 50.0, 1             # behind the cursor: must not be read
    log.state[0], log.state[1] = n, 4
    log.loss_sum[0] = 2.5
    return log


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist
    from vimo_clip_amd import parallel
    parallel.init_from_env("gloo")
    try:
        out = []
        for task, calls, width in (("multilabel", _multilabel_calls(), C), ("singlelabel", _singlelabel_calls(), 12)):
            values, targets, squash = _logged(calls, width)
            cut = 9 + 8                                   # unequal row counts: 17 and 27, the cut inside the unsquashed batch
            sl = slice(0, cut) if rank == 0 else slice(cut, None)
            log = _host_log(values[sl], targets[sl], squash[sl], task)
            assert log.read() == (values[sl].shape[0], 4, 0, 2.5)
            out.append(float(log.compute(distributed=True)))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_gathered_log_equals_the_single_process_log_gloo_world2():
    from vimo_clip_amd.metrics import evaluate_log
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [float(evaluate_log(*_logged(_multilabel_calls(), C), "multilabel")), float(evaluate_log(*_logged(_singlelabel_calls(), 12), "singlelabel"))]
    assert sorted(r for r, _ in res) == [0, 1]
    for _, got in res:
        assert got == want


def test_read_raises_on_a_refused_append_and_warns_on_a_bad_label():
    values, targets, squash = _logged(_singlelabel_calls(), 12)
    log = _host_log(values, targets, squash, "singlelabel")
    assert len(log.state_tensors()) == 1 and log.state_tensors()[0].numel() >= 5
    log.state[2] = 2
    with pytest.warns(RuntimeWarning, match="label outside"):
        assert log.read()[2] == 2
    log.state[2] = 3
    with pytest.raises(RuntimeError, match="refused"):
        log.read()
    with pytest.raises(RuntimeError, match="refused"):
        log.compute()
    log.reset()
    assert log.read() == (0, 0, 0, 0.0) and torch.isnan(log.compute())
    with pytest.raises(RuntimeError, match="no CPU path"):
        log.append(values[:2], targets[:2])


class _Arena:
    pass


class _Opt:           # the attribute surface GraphedTrainStep uses of optim.FusedAdam in device-state mode
    def __init__(self, n=8):
        self.arena = _Arena()
        self.arena.flat_param, self.arena.flat_grad = torch.zeros(n), torch.zeros(n)
        self.m, self.v = torch.zeros(n), torch.zeros(n)
        self.dev_state, self.dev_hyper = torch.zeros(4, dtype=torch.int64), torch.zeros(4)
        self.step_count = 0


def _warming_factory(events):
    class _Stub:          # stands in for GraphedCallable: the capture runs fn once (the warm-up), a replay runs it as well
        def __init__(self, fn, *example_inputs, warmup=1):
            events.append("capture")
            self.fn = fn
            fn(*example_inputs)

        def __call__(self, *inputs):
            events.append("replay")
            return self.fn(*inputs)
    return _Stub


def test_capture_restores_extra_live_tensors_of_the_warm_up():
    from vimo_clip_amd import graphs
    opt = _Opt()
    small = torch.tensor([16, 2, 0, 0, 7], dtype=torch.int32)            # a log mid-epoch: 16 rows, 2 steps

    def step_fn(x):
        small[0] += x.shape[0]
        small[1] += 1
        opt.arena.flat_param += 1

    events = []
    step = graphs.GraphedTrainStep(step_fn, opt, graph_factory=_warming_factory(events), extra_live=(small,))
    assert len(step._live()) == 7 and step._live()[-1] is small
    step(torch.zeros(8, 3))
    assert events == ["capture", "replay"]
    assert small.tolist() == [24, 3, 0, 0, 7] and opt.arena.flat_param.max() == 1            # one step, not two
    step(torch.zeros(4, 3))                                                # a new shape: another capture, again undone
    assert events == ["capture", "replay", "capture", "replay"] and small.tolist() == [28, 4, 0, 0, 7]
    # the default: nothing besides the optimiser's tensors
    assert len(graphs.GraphedTrainStep(step_fn, opt, graph_factory=_warming_factory(events))._live()) == 6


def _yaml_cfg():
    return dict(training=dict(mode="train", seed=1, lr=1e-4, epochs=1, batch_size=8, num_workers=0, device="cuda"),
                logging=dict(log_dir="l", checkpoint_dir="c"),
                data=dict(num_classes=4, class_names_dir=None, train_dataset_path=None, val_dataset_path=None, flow_dataset_path=None),
                model=dict(d_model=64, nhead=1, num_layers=1, dim_feedforward=64, use_cross_attention=True, concat_dim=1, dropout=0.1,
                           mlp_dropout=0.1, use_pe=False, use_only_rgb=False, use_only_flow=False))


def test_config_device_metrics_default_and_yaml(tmp_path):
    from vimo_clip_amd.TFAM.train_and_eval import Config
    assert Config().device_metrics is False
    assert Config(device_metrics=True).device_metrics is True
    import yaml
    cfg = _yaml_cfg()
    p = tmp_path / "a.yaml"
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).device_metrics is False
    cfg["training"]["device_metrics"] = True
    p.write_text(yaml.safe_dump(cfg))
    assert Config.from_yaml(str(p)).device_metrics is True
    assert Config.from_yaml(str(p), device_metrics=False).device_metrics is False     # overrides win, as for every key


def test_metric_log_struct_mirrors_the_header():
    """vmc_metric_log (include/vmc.h) is filled from Python through the ctypes.Structure mirror MetricLogStruct: same field names
    in the same order, five pointers and two ints."""
    import ctypes
    import re

    from vimo_clip_amd.metrics import MetricLogStruct
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vmc.h")).read(), flags=re.S)
    body = re.search(r"typedef struct vmc_metric_log\s*\{(.*?)\}\s*vmc_metric_log\s*;", src, flags=re.S).group(1)
    names, kinds = [], []
    for d in (d.strip() for d in body.split(";") if d.strip()):
        for n in re.sub(r"^(float|uint8_t|int)\s*\*?\s*", "", d).split(","):
            names.append(n.strip())
            kinds.append(ctypes.c_void_p if "*" in d else ctypes.c_int)
    assert names == [f[0] for f in MetricLogStruct._fields_] and kinds == [f[1] for f in MetricLogStruct._fields_]
    assert ctypes.sizeof(MetricLogStruct) == 48 and MetricLogStruct.capacity.offset == 40


def test_epoch_capacity_is_the_rows_of_the_ranks_whole_batches():
    from vimo_clip_amd.TFAM.train_and_eval import ModelTrainer, index_batches

    class _T:
        _epoch_rows = ModelTrainer._epoch_rows

    for n, bs, world in ((48, 8, 1), (50, 8, 1), (7, 8, 1), (101, 8, 2), (30, 4, 4)):
        for rank in range(world):
            t = _T()
            t.rank, t.world = rank, world
            t.config = type("Cfg", (), dict(batch_size=bs))()
            assert t._epoch_rows(n) == sum(len(ids) for _, ids in index_batches(n, bs, rank, world)), (n, bs, world, rank)
