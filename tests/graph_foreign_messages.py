"""A second wire module for the graph algorithms (test-only): the reference's message schema
(``simulation_lib/message.py:11-16, 64-71``) in classes of its own, as ``tests/foreign_messages.py``
is for the parameter messages (which has no ``FeatureMessage``). The graph plugins must recognise
these by their fields and answer with *these* classes.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any

import torch


@dataclass(kw_only=True)
class Message:
    other_data: dict[str, Any] = field(default_factory=dict)
    in_round: bool = False
    end_training: bool = False
    aggregation_weight: float | None = None


@dataclass(kw_only=True)
class FeatureMessage(Message):
    feature: torch.Tensor | None


@dataclass(kw_only=True)
class MultipleWorkerMessage(Message):
    worker_data: dict[int, Message]
