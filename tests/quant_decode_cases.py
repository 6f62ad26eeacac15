"""The case list of the record decoder's tests (host and GPU). The records are the oracles' own:
``tests/quant_encode_reference.expected_records`` of the encoder's parameter dicts (every size that
crosses a packbits byte, a 16-byte group of slots and a tile boundary; every value pattern), and
hand-made records through the oracles' ``make_record`` for the byte patterns no encoder writes. The
expected values are ``oracle.qsgd_oracle.dequantize`` / ``oracle.nnadq_oracle.dequantize``, compared
as bits. Test infrastructure only."""

from __future__ import annotations

import functools

import numpy as np
import torch

from distributed_learning_simulation_lib_amd.quantized import QuantizedTensor, codec_for
from oracle import nnadq_oracle, qsgd_oracle
from tests.quant_encode_cases import DRAW, LEVELS, SEED, WEIGHTS, torch_parameter
from tests.quant_encode_reference import expected_records

DTYPES = [np.float32, np.float64]
SCHEMES = ["qsgd", "nnadq"]
GUARD = 64  # bytes before and after every output of the GPU tests


def torch_dtype(dtype) -> torch.dtype:
    return torch.float64 if np.dtype(dtype) == np.float64 else torch.float32


def oracle_dequantize(record: np.ndarray, numel: int, dtype, scheme: str) -> np.ndarray:
    oracle = nnadq_oracle if scheme == "nnadq" else qsgd_oracle
    return oracle.dequantize(record, numel, dtype)


@functools.lru_cache(maxsize=None)
def _encoded(dtype_name: str, scheme: str) -> dict[str, tuple[np.ndarray, tuple[int, ...]]]:
    dtype = np.dtype(dtype_name).type
    p, _ = torch_parameter(dtype)  # the encoder's dict plus the two offset entries
    out: dict[str, tuple[np.ndarray, tuple[int, ...]]] = {}
    settings = [("L", level, {"level": level}) for level in LEVELS] if scheme == "qsgd" else [
        ("W", weight, {"weight": weight}) for weight in WEIGHTS]
    for tag, value, kw in settings:
        recs = expected_records(p, scheme, seed=SEED, draw=DRAW, **kw)
        for k, x in p.items():
            out[f"{k}@{tag}{value}"] = (recs[k], tuple(x.shape))
    return out


def encoded_records(dtype, scheme: str) -> dict[str, tuple[np.ndarray, tuple[int, ...]]]:
    """name -> (record, shape): the encoder's whole case list at levels 1, 2, 255 / weights 0.01, 0.5.
    Computed once per (dtype, scheme) and shared: callers do not write into the records."""
    return _encoded(np.dtype(dtype).name, scheme)


def handmade_records(dtype, scheme: str) -> dict[str, tuple[np.ndarray, tuple[int, ...]]]:
    """Finite byte patterns no encoder writes: every slot / code value 0 .. 255, slots above the level,
    codes above ``levels``; sizes off the 16-element and the packbits boundaries."""
    rng = np.random.default_rng(77)
    every = np.arange(256, dtype=np.uint8)
    out: dict[str, tuple[np.ndarray, tuple[int, ...]]] = {}
    if scheme == "qsgd":
        alt = (np.arange(256) % 2).astype(np.uint8)
        out["every_slot_alternating"] = (qsgd_oracle.make_record(1.7, 255, every, alt), (256,))
        out["every_slot_random_signs"] = (
            qsgd_oracle.make_record(float(np.float32(3.25e-3)), 255, every, rng.integers(0, 2, 256)), (16, 16))
        n = 301
        out["slots_above_level_2"] = (
            qsgd_oracle.make_record(0.9, 2, rng.integers(0, 256, n).astype(np.uint8), rng.integers(0, 2, n)), (n,))
        tiny = float(np.finfo(dtype).smallest_subnormal) * 3
        out["subnormal_norm"] = (qsgd_oracle.make_record(tiny, 255, every[:77], alt[:77]), (77,))
    else:
        out["every_code_levels_1"] = (nnadq_oracle.make_record(-0.3, 0.01, 1, every), (256,))
        out["every_code_levels_255"] = (nnadq_oracle.make_record(-0.3, float(np.float32(0.0123)), 255, every), (4, 64))
        n = 301
        out["codes_above_levels_2"] = (
            nnadq_oracle.make_record(1.5, 0.25, 2, rng.integers(0, 256, n).astype(np.uint8)), (n,))
    return out


def overflow_record(dtype, scheme: str) -> tuple[np.ndarray, tuple[int, ...]]:
    """A product that overflows in the codec's dtype (fp32: norm 3e38 times slot 255): the oracle gives
    infinities there, and the decoder raises the input flag."""
    big = 3e38 if np.dtype(dtype) == np.float32 else 1.5e308
    n = 40
    values = np.arange(n, dtype=np.uint8)
    values[-1] = 255
    if scheme == "qsgd":
        return qsgd_oracle.make_record(big, 255, values, np.arange(n) % 3 == 0), (n,)
    return nnadq_oracle.make_record(0.0, big, 255, values), (n,)


def bad_header_record(scheme: str, level: int) -> tuple[np.ndarray, tuple[int, ...]]:
    """A header whose level / levels is ``level`` (0 or 256: outside [1, 255])."""
    n = 20
    values = np.ones(n, dtype=np.uint8)
    if scheme == "qsgd":
        return qsgd_oracle.make_record(1.0, level, values, np.ones(n)), (n,)
    return nnadq_oracle.make_record(0.0, 0.5, level, values), (n,)


def as_quantized(record: np.ndarray, shape: tuple[int, ...], dtype, scheme: str,
                 device: torch.device | str = "cpu") -> QuantizedTensor:
    return QuantizedTensor(torch.from_numpy(record.copy()).to(device), shape, codec_for(torch_dtype(dtype), scheme))


def quantized_dict(cases: dict[str, tuple[np.ndarray, tuple[int, ...]]], dtype, scheme: str,
                   device: torch.device | str = "cpu") -> dict[str, QuantizedTensor]:
    return {k: as_quantized(r, s, dtype, scheme, device) for k, (r, s) in cases.items()}


def assert_same_bits(got: torch.Tensor, record: np.ndarray, shape: tuple[int, ...], dtype, scheme: str,
                     what: str = "") -> None:
    n = int(np.prod(shape, dtype=np.int64))
    want = oracle_dequantize(record, n, dtype, scheme)
    assert want.dtype == np.dtype(dtype)
    assert tuple(got.shape) == tuple(shape) and got.dtype == torch_dtype(dtype), what
    g = got.detach().cpu().contiguous().numpy().reshape(-1)
    bits = np.uint64 if np.dtype(dtype) == np.float64 else np.uint32
    if not np.array_equal(g.view(bits), want.view(bits)):
        bad = np.flatnonzero(g.view(bits) != want.view(bits))
        raise AssertionError(f"{what}: {bad.size} of {n} elements differ, first at {bad[:6]}: got {g[bad[:6]]}, "
                             f"want {want[bad[:6]]}")


def guarded(shape: tuple[int, ...], dtype: torch.dtype, device,
            offset: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """(buffer, view): a byte buffer pre-filled with 0xA5 and a view of ``shape`` inside it with
    ``GUARD`` bytes before and after; ``offset``: the view starts one element past a 16-byte boundary."""
    n = int(np.prod(shape, dtype=np.int64))
    size = torch.empty((), dtype=dtype).element_size()
    lead = GUARD + (size if offset else 0)
    buf = torch.full((lead + n * size + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    assert buf.data_ptr() % 16 == 0
    view = buf[lead : lead + n * size].view(dtype).reshape(shape)
    assert view.data_ptr() % 16 == (size if offset else 0) and view.is_contiguous()
    return buf, view


def assert_guards_intact(buf: torch.Tensor, view: torch.Tensor, what: str = "") -> None:
    lead = view.data_ptr() - buf.data_ptr()
    end = lead + view.numel() * view.element_size()
    assert bool((buf[:lead] == 0xA5).all()) and bool((buf[end:] == 0xA5).all()), what

