"""The case list the clip-and-noise tests share (tests/test_dp_host.py on the CPU path,
tests/test_gpu_dp.py on the kernel): sizes built from ``dp_tile`` and the 16-byte group of each
dtype, values with rows below, at and above the clipping norm, and the expected bytes from
tests/dp_reference.py, computed once per case. Test infrastructure only.
"""

from __future__ import annotations

import functools

import numpy as np
import torch

from distributed_learning_simulation_lib_amd.dp import compute_dp_sigma
from tests import dp_reference as ref

SEED, DRAW = 0x9E3779B97F4A7C15, 3
C = 0.5
SIGMA = compute_dp_sigma()
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f64": torch.float64}


def list_cases() -> dict[str, tuple[tuple[int, ...], float]]:
    """name -> (sizes, C) of the whole-list cases."""
    tl = ref.tile()
    cases = {f"n{n}": ((n,), C) for n in (1, 2, 3, tl - 1, tl + 1, 2 * tl + 5)}
    cases[f"n{tl}_below"] = ((tl,), 1.0e4)  # the norm stays below C: s = 1
    cases["three"] = ((1, tl + 3, 5), C)    # the middle tensor is placed one element off 16 bytes
    cases["with_empty"] = ((7, 0, tl + 1), C)
    return cases


def row_cases() -> list[tuple[int, int]]:
    tl = ref.tile()
    return [(1, 1), (3, 1), (5, 7), (4, 64), (300, 64), (2, tl + 1)]


def values(n: int, dtype: str, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g, dtype=torch.float32).to(TORCH[dtype])


def row_values(rows: int, length: int, dtype: str) -> torch.Tensor:
    """Row 0 is zero, row 1 has norm C exactly, row 2 lies below C, the others above (where there
    are that many rows; a 2-row tensor has one below and one above)."""
    x = values(rows * length, dtype, 1000 * rows + length).reshape(rows, length) * 4
    if rows == 2:
        x[0] *= 2.0**-12
    if rows >= 3:
        x[0] = 0
        x[1] = 0
        x[1, length // 2] = -C
        x[2] = (x[2] * 2.0**-12) if length > 1 else 4 * C
    return x.reshape(-1)


def widen(x: torch.Tensor) -> np.ndarray:
    return x.to(torch.float64).numpy().reshape(-1)


def raw(x: torch.Tensor) -> bytes:
    x = x.detach().cpu().contiguous().reshape(-1)
    return x.view(torch.uint8).numpy().tobytes() if x.numel() else b""


@functools.lru_cache(maxsize=None)
def list_case(name: str, dtype: str, draw: int = DRAW) -> tuple[list[torch.Tensor], float, list[bytes]]:
    sizes, c = list_cases()[name]
    xs = [values(n, dtype, 17 * i + n) for i, n in enumerate(sizes)]
    want = ref.expected([widen(x) for x in xs], dtype, 0, c, SIGMA * c, SEED, draw)
    return xs, c, want


@functools.lru_cache(maxsize=None)
def row_case(rows: int, length: int, dtype: str, draw: int = DRAW) -> tuple[torch.Tensor, bytes]:
    x = row_values(rows, length, dtype)
    (want,) = ref.expected([widen(x)], dtype, length, C, SIGMA * C, SEED, draw, [5])
    return x, want
