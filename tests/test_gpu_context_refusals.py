"""The refusals of ``tests/context_refusal_cases.py`` against a real context with device tensors: the
same types, texts and order as ``tests/test_context_refusals_host.py`` finds on the host, the
cases the host cannot reach (a host tensor where a device tensor is required), and that the whole
battery launched nothing: no flag is latched and the accumulator is as it was.

The client tables record real buffers (one fp32 tensor per segment, shared by every client row: a
refused call reads none of them), so a call that slipped through would read valid memory.
"""

from __future__ import annotations

import pytest
import torch

from distributed_learning_simulation_lib_amd import FedAvgContext
from tests import context_refusal_cases as cases

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope="module")
def env(hip_device):
    ctx = FedAvgContext(cases.LAYOUT, hip_device)
    ctx.accumulator.fill_(SENTINEL)
    clients = [torch.zeros(n, dtype=torch.float32, device=hip_device) for n in cases.NUMELS + (1,)]
    env = cases.Env(ctx, lambda k, t: clients[t].data_ptr(), hip_device.index)
    yield env
    ctx.close()


def test_every_refusal_and_nothing_launched(env):
    battery = cases.REFUSALS + cases.HOST_TENSOR_REFUSALS
    for case in battery:
        cases.check_refusal(env, case)
    assert len(battery) > 300
    assert env.ctx.flags() == 0
    assert not env.ctx.sparse_index_errors()
    assert bool((env.ctx.accumulator == SENTINEL).all())


@pytest.mark.parametrize("case", cases.HOST_TENSOR_REFUSALS, ids=[c.id for c in cases.HOST_TENSOR_REFUSALS])
def test_host_tensor_is_refused(env, case):
    cases.check_refusal(env, case)
