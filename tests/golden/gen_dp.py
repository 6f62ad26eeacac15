"""Generate the golden fixtures of the differential-privacy layer from the REFERENCE's own code.

The reference's ``simulation_lib/dp.py`` is loaded unmodified behind the stubs of
``gen_golden._load_reference``; nothing of it is copied. Its one source of randomness,
``torch.randn_like``, is replaced in that module by the defined normal stream
(``distributed_learning_simulation_lib_amd.dp.normal_stream``: tensor ``k`` of a parameter dict takes
stream id ``k``), so the recorded outputs are the reference's arithmetic on this project's noise. All
tensors are fp64 and all inputs are ``k * 2**-8`` with small integer ``k``: their sum of squares is
exact in any order, so the reference's ``vector_norm`` and the pinned order agree to the bit. The
cases cover a norm below, at and above ``C``, an all-zero tensor and ``sigma = 0``. A no-op where
the reference is absent.

Output: tests/golden/dp_golden.npz (data only): ``sigma/in`` [n, 2] (epsilon, delta) and
``sigma/out`` [n]; per parameter case ``p<i>/meta`` = (C, sigma, seed, draw), ``p<i>/names``,
``p<i>/in/<name>``, ``p<i>/out/<name>``; per tensor case ``t<i>/meta`` = (C, sigma, seed, draw,
tensor id), ``t<i>/in``, ``t<i>/out``. Re-run: `python tests/golden/gen_dp.py`.
"""

from __future__ import annotations

import importlib
import sys
from pathlib import Path

import numpy as np
import torch

OUT_DIR = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT_DIR))
import gen_golden  # noqa: E402  (the loader of the reference and its stubs)

from distributed_learning_simulation_lib_amd.dp import normal_stream  # noqa: E402

SEED = 20240611


class TorchWithStream:
    """``torch`` with ``randn_like`` answering from the defined stream: ``plan`` lists (tensor id,
    element count) of what the next call covers, in order."""

    def __init__(self) -> None:
        self.plan: list[tuple[int, int]] = []
        self.draw = 0

    def __getattr__(self, name: str):
        return getattr(torch, name)

    def randn_like(self, t: torch.Tensor) -> torch.Tensor:
        z = np.concatenate([normal_stream(SEED, self.draw, tid, n) for tid, n in self.plan])
        assert z.size == t.numel() and t.dtype == torch.float64
        return torch.from_numpy(z).reshape(t.shape)


def q8(values) -> torch.Tensor:
    return torch.tensor(values, dtype=torch.float64) * 2.0**-8


def parameter_cases():
    rng = np.random.default_rng(5)

    def model(scale=1):
        return {"a": q8(rng.integers(-40, 41, 5) * scale), "b": q8(rng.integers(-40, 41, (3, 4)) * scale),
                "s": q8(int(rng.integers(1, 9)) * scale), "c": q8(rng.integers(-40, 41, 9) * scale)}

    exact = {"a": q8([0, 3, 0, 0, 0]), "b": q8(np.zeros((3, 4))), "s": q8(-4), "c": q8(np.zeros(9))}  # norm 5/256
    zero = {k: torch.zeros_like(v) for k, v in exact.items()}
    sigma = 1.2
    return [("below", model(), 100.0, sigma, 0), ("at", exact, 5 * 2.0**-8, sigma, 1), ("above", model(), 2.0**-6, sigma, 2),
            ("zero", zero, 1.0, sigma, 3), ("sigma0_above", model(), 2.0**-6, 0.0, 4), ("sigma0_below", model(), 64.0, 0.0, 5)]


def tensor_cases():
    rng = np.random.default_rng(6)
    rows = q8(rng.integers(-40, 41, (5, 6)))
    rows[0] = 0
    rows[1] = q8([0, 3, 0, 0, -4, 0])   # norm 5/256 = C
    rows[2] = q8([1, 0, -1, 0, 1, 0])   # below
    cube = q8(rng.integers(-40, 41, (3, 2, 5)))
    vec = q8(rng.integers(-40, 41, 11))
    return [("rows", rows, 5 * 2.0**-8, 1.2, 0, 0), ("cube", cube, 0.125, 0.8, 1, 3), ("vector", vec, 0.125, 1.2, 2, 1),
            ("vector_below", vec, 8.0, 1.2, 3, 1), ("rows_sigma0", rows, 5 * 2.0**-8, 0.0, 4, 2),
            ("zeros", torch.zeros(4, 3, dtype=torch.float64), 1.0, 1.2, 5, 0)]


def main() -> int:
    if not gen_golden.REF.exists():
        print("reference not present: nothing to generate")
        return 0
    gen_golden._load_reference()
    ref_dp = importlib.import_module("simulation_lib.dp")
    patched = ref_dp.torch = TorchWithStream()
    out: dict[str, np.ndarray] = {}

    pairs = [(4.0, 1e-5), (1.0, 1e-5), (8.0, 1e-3), (0.5, 0.5)]
    out["sigma/in"] = np.array(pairs, dtype=np.float64)
    out["sigma/out"] = np.array([ref_dp.compute_dp_sigma(epsilon=e, delta=d) for e, d in pairs], dtype=np.float64)
    assert ref_dp.compute_dp_sigma() == out["sigma/out"][0]

    for i, (name, parameter, C, sigma, draw) in enumerate(parameter_cases()):
        patched.plan, patched.draw = [(k, v.numel()) for k, v in enumerate(parameter.values())], draw
        result = ref_dp.add_dp_noise_to_parameter(parameter, C=C, sigma=sigma)
        out[f"p{i}/meta"] = np.array([C, sigma, SEED, draw], dtype=np.float64)
        out[f"p{i}/names"] = np.array(list(parameter))
        for k, v in parameter.items():
            assert result[k].dtype == torch.float64 and result[k].shape == v.shape
            out[f"p{i}/in/{k}"], out[f"p{i}/out/{k}"] = v.numpy(), result[k].numpy()
        print(f"parameter {name}: ok")

    for i, (name, tensor, C, sigma, draw, tid) in enumerate(tensor_cases()):
        patched.plan, patched.draw = [(tid, tensor.numel())], draw
        result = ref_dp.add_dp_noise(tensor=tensor, C=C, sigma=sigma)
        assert result.dtype == torch.float64 and result.shape == tensor.shape
        out[f"t{i}/meta"] = np.array([C, sigma, SEED, draw, tid], dtype=np.float64)
        out[f"t{i}/in"], out[f"t{i}/out"] = tensor.numpy(), result.numpy()
        print(f"tensor {name}: ok")

    np.savez_compressed(OUT_DIR / "dp_golden.npz", **out)
    print(f"wrote {(OUT_DIR / 'dp_golden.npz').stat().st_size / 1e3:.1f} kB")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
