"""Reference of the device scaler's state machine (vmc_loss_scale_check, include/vmc.h): torch._amp_update_scale_ in ten lines of
numpy fp32.  tests/test_loss_scale_host.py pins it to the torch op bit for bit; tests/test_gpu_loss_scale.py pins the kernel to it."""
import numpy as np


def update_scale(scale, tracker, skipped, found_inf, growth_factor, backoff_factor, growth_interval):
    """(scale, growth_tracker, skipped) after one checked step; scale is an np.float32, products are single fp32 roundings."""
    scale = np.float32(scale)
    if found_inf:
        return np.float32(scale * np.float32(backoff_factor)), 0, skipped + 1
    tracker += 1
    if tracker == growth_interval:
        with np.errstate(over="ignore"):
            grown = np.float32(scale * np.float32(growth_factor))
        return (grown if np.isfinite(grown) else scale), 0, skipped
    return scale, tracker, skipped


def run(scale, found_seq, growth_factor, backoff_factor, growth_interval, tracker=0, skipped=0):
    """The (scale, tracker, skipped) after every step of a found-inf sequence."""
    out = []
    for f in found_seq:
        scale, tracker, skipped = update_scale(scale, tracker, skipped, bool(f), growth_factor, backoff_factor, growth_interval)
        out.append((np.float32(scale), int(tracker), int(skipped)))
    return out
