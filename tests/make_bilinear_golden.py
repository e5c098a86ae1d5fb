"""Writes tests/golden/bilinear_mn.npz: u8 inputs with the f32 frames the REFERENCE's dataset_frame_diff_mn.HDF5VideoDataset
._resize_frames makes of them and the bytes of ``.mul(255).byte()`` (to_pil_image) on those.

    python tests/make_bilinear_golden.py /path/to/reference

The reference module is imported at generation time only; h5py and torchvision, which it imports at the top and which this
function never touches, are replaced by empty stand-in modules when they are not installed.  The stored arrays are what aten's CPU
kernel computed on the generating machine (torch version recorded in the file)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

CASES = {"a": ((2, 3, 37, 53), (32, 48)), "b": ((1, 3, 1, 1), (16, 16)), "c": ((1, 3, 20, 30), (64, 64))}


def _stub(name, **attrs):
    try:
        importlib.import_module(name)
    except ImportError:
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m


def main(reference_dir):
    _stub("h5py")
    _stub("torchvision")
    _stub("torchvision.io", VideoReader=None)
    sys.path.insert(0, reference_dir)
    cls = importlib.import_module("dataset_frame_diff_mn").HDF5VideoDataset
    out = {"torch_version": np.array(torch.__version__)}
    rng = np.random.default_rng(20)
    for key, (shape, size) in CASES.items():
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        x.reshape(-1)[:2] = (0, 255)
        ds = cls.__new__(cls)                       # _resize_frames reads spatial_size only
        ds.spatial_size = size
        y = ds._resize_frames(torch.from_numpy(x))
        out[key + "_in"], out[key + "_f32"], out[key + "_u8"] = x, y.numpy(), y.mul(255).byte().numpy()
        out[key + "_size"] = np.array(size)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bilinear_mn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
