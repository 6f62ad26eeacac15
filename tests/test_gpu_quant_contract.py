"""The broadcast encoder (fedavg_quant_encode) on tensors of more than 256 tiles: the
header pass reduces a tensor's tile partials with one lane per tile, so its lanes make a second trip
there, and an extremum that lies in tile 256 or later is found in that trip alone. Records byte for
byte those of the restatement (tests/quant_encode_reference.py), then decoded on the GPU to the bits
of the oracles' ``dequantize``. The call follows a small one with nothing waiting in between and needs
more tile partials than the state's first 1024, so the partials are regrown while work is in flight.
The shapes up to two tiles are in tests/test_gpu_quant_encode.py and tests/test_gpu_quant_decode.py."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import _native
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, ModelLayout
from distributed_learning_simulation_lib_amd.quantized import codec_for
from tests.quant_decode_cases import DTYPES, SCHEMES, assert_guards_intact, assert_same_bits, guarded, torch_dtype
from tests.quant_encode_cases import DRAW, SEED, tile
from tests.quant_encode_reference import assert_same_record, expected_records

pytestmark = pytest.mark.gpu

LEVEL, WEIGHT = 255, 0.01
GUARD = 64  # bytes before and after every record


def numel() -> int:
    return (_native.kernel_constant("quant_threads") + 1) * tile() + 3


@functools.lru_cache(maxsize=None)
def parameter(dtype_name: str) -> dict[str, np.ndarray]:
    """Small values with one minimum of -5 and one maximum of 7 each. Tiles 0 .. 255 are the header
    pass's first trip; tile 256 and the tail tile of 3 elements are its second."""
    dt = np.dtype(dtype_name).type
    t, n = tile(), numel()
    lanes = _native.kernel_constant("quant_threads")
    assert n == (lanes + 1) * t + 3
    rng = np.random.default_rng(20261126)
    p = {k: (rng.standard_normal(n) * 0.01).astype(dt) for k in ("late_extremes", "early_extremes", "split", "plain")}
    p["late_extremes"][n - 2] = -5.0                # the tail tile
    p["late_extremes"][lanes * t + 20] = 7.0        # tile 256
    p["early_extremes"][t + 5] = -5.0               # tile 1
    p["early_extremes"][3 * t - 1] = 7.0            # the last element of tile 2
    p["split"][3 * t + 77] = -5.0                   # tile 3
    p["split"][n - 1] = 7.0                         # the last element of the tail tile
    return p


@functools.lru_cache(maxsize=None)
def small_parameter(dtype_name: str) -> dict[str, np.ndarray]:
    dt = np.dtype(dtype_name).type
    rng = np.random.default_rng(7)
    return {"a": rng.standard_normal(17).astype(dt), "b": rng.standard_normal(tile() + 1).astype(dt)}


@functools.lru_cache(maxsize=None)
def wanted(dtype_name: str, scheme: str, small: bool) -> dict[str, np.ndarray]:
    p = small_parameter(dtype_name) if small else parameter(dtype_name)
    return expected_records(p, scheme, LEVEL, WEIGHT, SEED, DRAW)


def _records(p, codec, device):
    bufs = [torch.full((codec.record_bytes(x.size) + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
            for x in p.values()]
    return bufs, [b[GUARD:-GUARD] for b in bufs]


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_header_over_more_than_256_tiles(hip_device, dtype, scheme):
    name = np.dtype(dtype).name
    p, small = parameter(name), small_parameter(name)
    assert sum(-(-x.size // tile()) for x in p.values()) > 1024  # the first capacity of the tile partials
    codec = codec_for(torch_dtype(dtype), scheme)
    tp, tsmall = ({k: torch.from_numpy(v).to(hip_device) for k, v in d.items()} for d in (p, small))
    (bufs, recs), (sbufs, srecs) = _records(p, codec, hip_device), _records(small, codec, hip_device)
    outs = {k: guarded(x.shape, torch_dtype(dtype), hip_device) for k, x in p.items()}
    ctx = FedAvgContext(ModelLayout.flat(1), hip_device)
    try:
        torch.cuda.synchronize(hip_device)
        ctx.quant_encode(codec.code, list(tsmall.values()), srecs, LEVEL, WEIGHT, SEED, DRAW)
        ctx.quant_encode(codec.code, list(tp.values()), recs, LEVEL, WEIGHT, SEED, DRAW)
        ctx.raise_on_nan()  # waits for the stream
        for d, want, rs, bs in ((small, wanted(name, scheme, True), srecs, sbufs), (p, wanted(name, scheme, False), recs, bufs)):
            for (k, x), r, b in zip(d.items(), rs, bs):
                assert_same_record(r.cpu().numpy(), want[k], x, scheme, f"{scheme} {name} {k}")
                assert bool((b[:GUARD] == 0xA5).all()) and bool((b[-GUARD:] == 0xA5).all()), k
        ctx.quant_decode(codec.code, recs, [view for _, view in outs.values()])
        assert ctx.flags() == 0
    finally:
        ctx.close()
    want = wanted(name, scheme, False)
    for k, x in p.items():
        buf, view = outs[k]
        assert_same_bits(view, want[k], x.shape, dtype, scheme, f"decoded {scheme} {name} {k}")
        assert_guards_intact(buf, view, k)
