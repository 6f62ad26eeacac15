"""Torch-CPU restatement of the robust aggregation rules (test-only; NOT a reference algorithm —
the reference has none besides the weighted mean — so this file is what parity means for them).

Independent of the code under test: nothing is imported from the package. Per named tensor, per
element, over the ``n`` clients that sent the tensor:

* a value is the input element converted exactly to fp64; any NaN -> ``RobustNaN("input")``;
* sorted on the int64 key of the fp64 bits (negative patterns: magnitude bits flipped), i.e. the
  IEEE total order ``-inf < ... < -0.0 < +0.0 < ... < +inf``;
* ``trimmed_mean``: ``k = floor(trim * n)``; ``sum = s_k``, then ``sum = sum + s_j`` for
  ``j = k+1 .. n-k-1`` ascending (a sequential Python loop of fp64 adds), ``result = sum / (n - 2k)``;
* ``median``: ``s_{(n-1)/2}`` (n odd) or ``(s_{n/2-1} + s_{n/2}) / 2.0`` (n even);
* a NaN result -> ``RobustNaN("result")``; ``out_dtype`` float32 rounds the fp64 result (RNE).
"""

from __future__ import annotations

import math

import torch

_MAG = 0x7FFFFFFFFFFFFFFF


class RobustNaN(Exception):
    def __init__(self, stage: str) -> None:
        super().__init__(stage)
        self.stage = stage


def trim_count(trim: float, n: int) -> int:
    return math.floor(trim * n)


def sort_total_order(x: torch.Tensor) -> torch.Tensor:
    """fp64 [n, P] sorted along dim 0 on the int64 key of the bits."""
    b = x.contiguous().view(torch.int64)
    key = torch.where(b < 0, b ^ _MAG, b)
    key, _ = torch.sort(key, dim=0)
    return torch.where(key < 0, key ^ _MAG, key).view(torch.float64)


def reduce_tensor(values: list[torch.Tensor], mode: str, trim: float = 0.0,
                  out_dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The rule over one tensor's client values (any float dtype, same shape, CPU)."""
    n = len(values)
    assert n >= 1
    x = torch.stack([v.detach().cpu().to(torch.float64).reshape(-1) for v in values])
    if torch.isnan(x).any():
        raise RobustNaN("input")
    s = sort_total_order(x)
    if mode == "median":
        if n % 2 == 1:
            out = s[(n - 1) // 2].clone()
        else:
            out = (s[n // 2 - 1] + s[n // 2]) / 2.0
    elif mode == "trimmed_mean":
        assert 0 <= trim < 0.5
        k = trim_count(trim, n)
        m = n - 2 * k
        assert m >= 1
        total = s[k].clone()
        for j in range(k + 1, n - k):
            total = total + s[j]
        out = total / float(m)
    else:
        raise ValueError(mode)
    if torch.isnan(out).any():
        raise RobustNaN("result")
    return out.to(out_dtype).reshape(values[0].shape)


def reduce_round(clients: list[dict[str, torch.Tensor] | None], mode: str, trim: float = 0.0,
                 out_dtype: torch.dtype = torch.float64) -> dict[str, torch.Tensor]:
    """A whole round: ``None`` = a skipped client; a key missing from a client does not count for
    that tensor. Keys come in first-seen order."""
    names: list[str] = []
    for c in clients:
        for name in (c or {}):
            if name not in names:
                names.append(name)
    return {name: reduce_tensor([c[name] for c in clients if c is not None and name in c], mode, trim, out_dtype)
            for name in names}
