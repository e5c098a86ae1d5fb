"""numpy reference of vmc_metric_append (include/vmc.h K18): a list of (values, targets, loss) calls applied to a log, shared by the
host and the GPU tests.  ``loss_sum`` is accumulated as sequential np.float32 adds, as the kernel's one fp32 add per call."""
import numpy as np


def apply_calls(calls, capacity, C, fill=(0.0, 0, 0)):
    """calls: (values [B, C], targets [B, C], loss or None).  Rows no call wrote keep ``fill`` = (value, target, squash).
    -> dict(values f32 [capacity, C], targets u8 [capacity, C], squash u8 [capacity], rows, steps, status, loss_sum np.float32)."""
    values = np.full((capacity, C), fill[0], dtype=np.float32)
    targets = np.full((capacity, C), fill[1], dtype=np.uint8)
    squash = np.full((capacity,), fill[2], dtype=np.uint8)
    rows = steps = status = 0
    loss_sum = np.float32(0.0)
    for v, t, loss in calls:
        v = np.asarray(v, dtype=np.float32).reshape(-1, C)
        t = np.asarray(t, dtype=np.float32).reshape(-1, C)
        B = v.shape[0]
        if rows + B > capacity:
            status |= 1                                   # refused: nothing else changes
            continue
        values[rows:rows + B] = v
        tt = np.trunc(t)                                  # labels.to(torch.int): toward zero
        if (~((tt == 0) | (tt == 1))).any():              # NaN included
            status |= 2
        targets[rows:rows + B] = np.clip(np.nan_to_num(tt, nan=0.0), 0, 255).astype(np.uint8)
        with np.errstate(invalid="ignore"):
            squash[rows:rows + B] = 1 if ((v < 0) | (v > 1)).any() else 0
        if loss is not None:
            loss_sum = np.float32(loss_sum + np.float32(loss))
        steps += 1
        rows += B
    return dict(values=values, targets=targets, squash=squash, rows=rows, steps=steps, status=status, loss_sum=loss_sum)
