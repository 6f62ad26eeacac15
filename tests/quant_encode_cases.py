"""The case list of the broadcast encoder's tests (host and GPU): one parameter dict per dtype that
mixes every size and every value pattern of the contract in one call. Test infrastructure only."""

from __future__ import annotations

import numpy as np
import torch

from distributed_learning_simulation_lib_amd import _native
from tests.quant_encode_reference import assert_same_record, expected_records

LEVELS = (1, 2, 255)
WEIGHTS = (0.01, 0.5)
SEED, DRAW = 0x1234_5678_9ABC_DEF0, 7


def tile() -> int:
    return _native.kernel_constant("quant_tile")


def sizes() -> list[int]:
    t = tile()
    return [1, 7, 8, 9, 15, 16, 17, 127, 128, 129, t - 1, t, t + 1, 2 * t + 5]


def parameter(dtype) -> dict[str, np.ndarray]:
    """Every size with random values, then the value patterns (sizes chosen off the 16- and 8-element
    boundaries so the padding rules are exercised too)."""
    dt = np.dtype(dtype).type
    rng = np.random.default_rng(20261021)
    t = tile()
    p: dict[str, np.ndarray] = {}
    for n in sizes():
        p[f"n{n}"] = rng.standard_normal(n).astype(dt)
    p["zeros"] = np.zeros(133, dtype=dt)
    p["neg_zeros"] = np.full(41, -0.0, dtype=dt)
    p["constant"] = np.full(203, 0.37, dtype=dt)
    p["neg_constant"] = np.full(19, -2.5, dtype=dt)
    x = rng.standard_normal(301).astype(dt)
    x[::7] = -0.0
    x[3::11] = 0.0
    p["signed_zeros"] = x  # -0.0 elements: their sign bit is 1 (not x < 0)
    x = (rng.standard_normal(t + 3) * 0.1).astype(dt)
    x[-1] = -9.75
    p["extremum_last_of_tail"] = x  # the norm / the minimum is the very last element of a tail tile
    x = (rng.standard_normal(2 * t + 1) * 0.1).astype(dt)
    x[-1] = 11.5
    p["maximum_last_of_tail"] = x
    k = np.arange(256, dtype=np.float64)
    p["integer_r"] = np.concatenate([k * 0.125, -k * 0.125]).astype(dt)  # r = k (level 255) where k / 255 * 255 is exact
    p["halves"] = np.array([0.0, 0.5, 1.0, -1.0, -0.5, 0.25, 0.75, -0.75, 1.0], dtype=dt)  # exact r at levels 1 and 2
    e = rng.uniform(-30, 30, 517)
    p["wide_range"] = (np.sign(rng.standard_normal(517)) * 10.0**e).astype(dt)
    p["wide_range"][5], p["wide_range"][6] = dt(1e30), dt(1e-30)
    tiny = np.finfo(dt).smallest_subnormal
    x = (rng.integers(1, 1 << 20, 263).astype(np.float64) * float(tiny)).astype(dt)
    x[::3] = -x[::3]
    x[17] = dt((1 << 20) * float(tiny))
    p["subnormals"] = x
    x = np.abs(rng.standard_normal(77)).astype(dt)
    x[[0, 9, 30]] = 0.0
    x[[4, 50]] = -0.0
    p["mixed_zero_minimum"] = x  # the one numeric comparison: NNADQ's lo is a zero of either sign
    x = -np.abs(rng.standard_normal(59)).astype(dt)
    x[[1, 8]] = 0.0
    x[[2, 40]] = -0.0
    p["mixed_zero_maximum"] = x
    p["single_neg"] = np.array([-3.0], dtype=dt)
    return p


def offset_view(x: torch.Tensor) -> torch.Tensor:
    """A contiguous copy of ``x`` whose data pointer lies one element past a 16-byte boundary."""
    base = torch.empty(x.numel() + 16, dtype=x.dtype, device=x.device)
    assert base.data_ptr() % 16 == 0
    v = base[1 : 1 + x.numel()]
    v.copy_(x.reshape(-1))
    assert v.data_ptr() % 16 == x.element_size() and v.is_contiguous()
    return v


def torch_parameter(dtype, device: torch.device | str = "cpu") -> tuple[dict[str, np.ndarray], dict[str, torch.Tensor]]:
    """The numpy dict and the same dict as torch tensors on ``device``; two entries are views one
    element off 16-byte alignment (a short one and one of more than a tile)."""
    p = parameter(dtype)
    t = tile()
    rng = np.random.default_rng(5)
    dt = np.dtype(dtype).type
    p["offset_small"] = rng.standard_normal(37).astype(dt)
    p["offset_large"] = rng.standard_normal(t + 21).astype(dt)
    tp = {k: torch.from_numpy(v.copy()).to(device) for k, v in p.items()}
    tp["offset_small"] = offset_view(tp["offset_small"])
    tp["offset_large"] = offset_view(tp["offset_large"])
    return p, tp


def check_records(records, p: dict[str, np.ndarray], scheme: str, level: int = 255, weight: float = 0.01,
                  seed: int = SEED, draw: int = DRAW, what: str = "") -> None:
    want = expected_records(p, scheme, level, weight, seed, draw)
    assert list(records) == list(p)
    for k, x in p.items():
        q = records[k]
        assert q.shape == tuple(x.shape) and q.codec.scheme == scheme
        assert q.codec.value_dtype == (torch.float64 if x.dtype == np.float64 else torch.float32)
        assert_same_record(q.record.cpu().numpy(), want[k], x, scheme, f"{what} {scheme} {x.dtype} {k}")
