"""``FedAvgContext``'s side-kernel wrappers without a GPU or a library: the real methods run on a
CPU context over a stand-in that records what would have reached ``fedavg_*``.

Two things are pinned. Every refusal of ``tests/context_refusal_cases.py`` raises its exception
type with its full text, in its order, and nothing reaches the library. And one accepted call per
wrapper reaches it with exactly the argument tuple written out below: pointer arrays, codes, counts,
scalars, and ``None`` where a table is optional. In those tuples an address is shown as the name of
the tensor it belongs to (``Env.names``; the two wrappers that allocate their result name it
``"result"``), a client table's entry as the made-up address ``client_ptr`` gave it, an array as the
list of its elements, and a ``byref`` out-parameter as ``"byref"``.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import _native, fedavg
from distributed_learning_simulation_lib_amd.fedavg import FedAvgContext, SparseTable
from tests import context_refusal_cases as cases
from tests.context_refusal_cases import F16, F32, F64, NNADQ, NNADQ64, QSGD, QSGD64

HANDLE, STREAM = 1, 0x5EED
# the layout-free calls pass their tables as raw addresses: argument index -> (element type, index
# of the argument that holds the count)
RAW_TABLES = {
    "fedavg_quant_encode": {2: (np.uint64, 5), 3: (np.int64, 5), 4: (np.uint32, 5), 6: (np.uint64, 5)},
    "fedavg_quant_decode": {2: (np.uint64, 4), 3: (np.int64, 4), 5: (np.uint64, 4), 6: (np.uint64, 4)},
    "fedavg_dp_noise": {2: (np.uint64, 5), 3: (np.int64, 5), 4: (np.uint32, 5), 6: (np.uint64, 5)},
    "fedavg_topk_sparsify": {2: (np.uint64, 6), 3: (np.uint64, 6), 4: (np.int64, 6), 5: (np.int64, 6),
                             7: (np.uint64, 6), 8: (np.uint64, 6), 9: (np.uint64, 6)},
}


def client_ptr(k: int, t: int) -> int:
    return 0x1000 * (k + 1) + 0x100 * t


class Recorder:
    """Answers every ``fedavg_*`` call with 0 and keeps its name and its arguments as plain values
    (arrays are read out during the call, while what they point at is alive)."""

    def __init__(self) -> None:
        self.calls: list[tuple[str, tuple]] = []

    def __getattr__(self, name: str):
        if not name.startswith("fedavg_"):
            raise AttributeError(name)

        def call(*args):
            raw = RAW_TABLES.get(name, {})
            plain = []
            for i, a in enumerate(args):
                if i in raw and a is not None:
                    dtype, count = raw[i]
                    size = args[count] * np.dtype(dtype).itemsize
                    a = np.frombuffer(ctypes.string_at(a, size), dtype=dtype).tolist()
                plain.append(self._plain(a))
            self.calls.append((name, tuple(plain)))
            return 0

        return call

    @staticmethod
    def _plain(a):
        if isinstance(a, ctypes.c_void_p):
            return a.value
        if isinstance(a, ctypes.Array):
            return list(a)
        if isinstance(a, ctypes._Pointer):
            return a._arr.tolist()  # numpy's data_as keeps its array on the pointer
        if isinstance(a, np.ndarray):
            return a.tolist()
        if type(a).__name__ == "CArgObject":
            return "byref"
        return a

    def named(self, names: dict[int, str]) -> list[tuple[str, tuple]]:
        """The calls with every address that belongs to a named tensor shown as the name."""
        def name(a):
            if isinstance(a, list):
                return [name(x) for x in a]
            return names.get(a, a) if isinstance(a, int) and not isinstance(a, bool) and a > 0xFFFF else a
        return [(fn, tuple(name(a) for a in args)) for fn, args in self.calls]


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setattr(fedavg, "_stream_handle", lambda device: ctypes.c_void_p(STREAM))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    ctx = FedAvgContext.borrowed(lib=Recorder(), handle=HANDLE, layout=cases.LAYOUT, device=torch.device("cpu"),
                                 accumulator=torch.zeros(64, dtype=torch.float64))
    return cases.Env(ctx, client_ptr, 0)


@pytest.mark.parametrize("case", cases.REFUSALS, ids=[c.id for c in cases.REFUSALS])
def test_refusal(env, case):
    cases.check_refusal(env, case)
    assert env.ctx._lib.calls == []


CLIENTS = [0x1000, 0x1100, 0x2000, 0x2100]
OUT = ["out0", "out1"]
POINT = ["point0", "point1"]


def _moments_origin(e):
    return cases.moments(e, centre=None)


def _opt_avgm(e):
    return cases.opt(e, mode="avgm", v_in=None, v_out=None, out_dtype=F32, tau=0.0)


def _sparse_table(e):
    return cases.sparse_fold(e, SparseTable(e.rows(2, F16), cases.LAYOUT, e.device), out_dtype=F32)


def _sparse_unchecked(e):
    return e.ctx.sparse_aggregate_delta(e.rows(), (1.0, 3.0), 4.0, e.segs("base"), e.segs("out"), check_indices=False)


def _topk_partial_errors(e):
    return cases.topk(e, errors=[None, e.flat("err1", 7, F32), None], keeps=(0, 3, 17), sizes=(0, 7, 17),
                      indices=e.segs("idx", torch.int32, (0, 3, 17)), values=e.segs("val", F32, (0, 3, 17)))


SPARSE_ARGS = (["d00.i", 0, "d10.i", 0], ["d00.v", 0, "d10.v", 0], [2, 0, 2, 0])
# id -> (call, [(function, arguments)])
ACCEPTED = {
    "robust-median": (lambda e: cases.robust(e, e.table(3, holes=((1, 1),))), [
        ("fedavg_robust_aggregate", (HANDLE, [0x1000, 0x1100, 0x2000, 0, 0x3000, 0x3100], _native.F32, 3,
                                     _native.ROBUST_MEDIAN, [1, 0], OUT, _native.F64, STREAM))]),
    "robust-trimmed-mean": (lambda e: cases.robust(e, e.table(5), mode="trimmed_mean", trim=0.25, out_dtype=F32), [
        ("fedavg_robust_aggregate", (HANDLE, [client_ptr(k, t) for k in range(5) for t in range(2)], _native.F32, 5,
                                     _native.ROBUST_TRIMMED_MEAN, [1, 1], OUT, _native.F32, STREAM))]),
    "mam": (lambda e: cases.mam(e, e.table(2, holes=((1, 1),)), keep=[2, 1]), [
        ("fedavg_mean_around_median", (HANDLE, [0x1000, 0x1100, 0x2000, 0], _native.F32, 2, [2, 1], OUT, _native.F64,
                                       STREAM))]),
    "mam-one-keep": (lambda e: cases.mam(e, keep=2, out_dtype=F32), [
        ("fedavg_mean_around_median", (HANDLE, CLIENTS, _native.F32, 2, [2, 2], OUT, _native.F32, STREAM))]),
    "pairwise": (cases.pairwise, [("fedavg_pairwise_sqdist", (HANDLE, CLIENTS, _native.F32, 2, "result", STREAM))]),
    "sqdist": (cases.sqdist, [("fedavg_sqdist_to_point", (HANDLE, CLIENTS, _native.F32, 2, POINT, "result", STREAM))]),
    "sqdist-origin": (lambda e: cases.sqdist(e, point=None), [
        ("fedavg_sqdist_to_point", (HANDLE, CLIENTS, _native.F32, 2, None, "result", STREAM))]),
    "moments": (cases.moments, [
        ("fedavg_moments_about_point", (HANDLE, CLIENTS, _native.F32, 2, ["centre0", "centre1"],
                                        ["direction0", "direction1"], "result", STREAM))]),
    "moments-origin": (_moments_origin, [
        ("fedavg_moments_about_point", (HANDLE, CLIENTS, _native.F32, 2, None, ["direction0", "direction1"], "result",
                                        STREAM))]),
    "fold": (cases.fold, [
        ("fedavg_fold_about_point", (HANDLE, CLIENTS, _native.F32, [1.0, 2.0], 2, 2.0, POINT, OUT, _native.F64,
                                     STREAM))]),
    "fold-f32": (lambda e: cases.fold(e, coef=[0, -3], divisor=7, out_dtype=F32), [
        ("fedavg_fold_about_point", (HANDLE, CLIENTS, _native.F32, [0.0, -3.0], 2, 7.0, POINT, OUT, _native.F32,
                                     STREAM))]),
    "opt-adam": (cases.opt, [
        ("fedavg_server_opt_step", (HANDLE, CLIENTS, _native.F32, [1.0, 2.0], 2, 2.0, POINT, ["m_in0", "m_in1"],
                                    ["v_in0", "v_in1"], ["m_out0", "m_out1"], ["v_out0", "v_out1"], _native.OPT_ADAM,
                                    0.5, 0.9, 1.0 - 0.9, 0.99, 1.0 - 0.99, 0.001, OUT, _native.F64, STREAM))]),
    "opt-avgm": (_opt_avgm, [
        ("fedavg_server_opt_step", (HANDLE, CLIENTS, _native.F32, [1.0, 2.0], 2, 2.0, POINT, ["m_in0", "m_in1"], None,
                                    ["m_out0", "m_out1"], None, _native.OPT_AVGM, 0.5, 0.9, 1.0 - 0.9, 0.99,
                                    1.0 - 0.99, 0.0, OUT, _native.F32, STREAM))]),
    "opt-avgm-ignores-v": (lambda e: cases.opt(e, mode="avgm"), [
        ("fedavg_server_opt_step", (HANDLE, CLIENTS, _native.F32, [1.0, 2.0], 2, 2.0, POINT, ["m_in0", "m_in1"], None,
                                    ["m_out0", "m_out1"], None, _native.OPT_AVGM, 0.5, 0.9, 1.0 - 0.9, 0.99,
                                    1.0 - 0.99, 0.001, OUT, _native.F64, STREAM))]),
    "sparse": (cases.sparse_fold, [
        ("fedavg_sparse_aggregate_delta", (HANDLE, *SPARSE_ARGS, _native.F32, [1.0, 3.0], 2, 4.0, ["base0", "base1"],
                                           OUT, _native.F64, STREAM)),
        ("fedavg_sparse_index_errors", (HANDLE, STREAM, "byref"))]),
    "sparse-table-f16": (_sparse_table, [
        ("fedavg_sparse_aggregate_delta", (HANDLE, *SPARSE_ARGS, _native.F16, [1.0, 3.0], 2, 4.0, ["base0", "base1"],
                                           OUT, _native.F32, STREAM)),
        ("fedavg_sparse_index_errors", (HANDLE, STREAM, "byref"))]),
    "sparse-unchecked": (_sparse_unchecked, [
        ("fedavg_sparse_aggregate_delta", (HANDLE, *SPARSE_ARGS, _native.F32, [1.0, 3.0], 2, 4.0, ["base0", "base1"],
                                           OUT, _native.F64, STREAM))]),
    # tensors of 0, 7 and 17 elements: an empty tensor's address is passed as 0, its record's is not
    "encode-qsgd": (lambda e: cases.encode(e, QSGD, sizes=(0, 7, 17), need=(16, 48, 64)), [
        ("fedavg_quant_encode", (HANDLE, QSGD, [0, "x1", "x2"], [0, 7, 17], [0, 1, 2], 3, ["rec0", "rec1", "rec2"],
                                 255, 0.01, 0, 0, STREAM))]),
    "encode-nnadq-f64": (lambda e: cases.encode(e, NNADQ64, sizes=(17, 0, 7), need=(64, 32, 48), dtype=F64, level=16,
                                                weight=0.5, seed=(1 << 64) - 1, draw=(1 << 32) - 1,
                                                tensor_ids=[9, 8, 7]), [
        ("fedavg_quant_encode", (HANDLE, NNADQ64, ["x0", 0, "x2"], [17, 0, 7], [9, 8, 7], 3, ["rec0", "rec1", "rec2"],
                                 16, 0.5, (1 << 64) - 1, (1 << 32) - 1, STREAM))]),
    "decode-qsgd": (lambda e: cases.decode(e, QSGD, sizes=(0, 7, 17), need=(16, 48, 64)), [
        ("fedavg_quant_decode", (HANDLE, QSGD, ["rec0", "rec1", "rec2"], [0, 7, 17], 3, [0, "out1", "out2"], None,
                                 STREAM))]),
    "decode-nnadq-wide": (lambda e: cases.decode(e, NNADQ, sizes=(7, 17, 0), need=(48, 64, 32),
                                                 outs64=e.segs("wide", F64, (7, 17, 0))), [
        ("fedavg_quant_decode", (HANDLE, NNADQ, ["rec0", "rec1", "rec2"], [7, 17, 0], 3, ["out0", "out1", 0],
                                 ["wide0", "wide1", 0], STREAM))]),
    "decode-qsgd-f64": (lambda e: cases.decode(e, QSGD64, dtype=F64), [
        ("fedavg_quant_decode", (HANDLE, QSGD64, ["rec0", "rec1"], [7, 17], 2, ["out0", "out1"], None, STREAM))]),
    "noise": (lambda e: cases.noise(e, sizes=(0, 7, 17)), [
        ("fedavg_dp_noise", (HANDLE, _native.F32, [0, "x1", "x2"], [0, 7, 17], [0, 1, 2], 3, [0, "out1", "out2"], 0,
                             1.0, 0.5, 0, 0, STREAM))]),
    "noise-rows-bf16": (lambda e: cases.noise(e, sizes=(17,), dtype=torch.bfloat16, seed=3, draw=4, tensor_ids=[6],
                                              row_len=1), [
        ("fedavg_dp_noise", (HANDLE, _native.BF16, ["x0"], [17], [6], 1, ["out0"], 1, 1.0, 0.5, 3, 4, STREAM))]),
    "topk": (lambda e: cases.topk(e), [
        ("fedavg_topk_sparsify", (HANDLE, _native.F32, ["delta0", "delta1"], ["err0", "err1"], [7, 17], [3, 0],
                                  2, ["idx0", 0], ["val0", 0], ["res0", "res1"], STREAM))]),
    "topk-no-errors": (lambda e: cases.topk(e, errors=None, dtype=F64), [
        ("fedavg_topk_sparsify", (HANDLE, _native.F64, ["delta0", "delta1"], None, [7, 17], [3, 0], 2, ["idx0", 0],
                                  ["val0", 0], ["res0", "res1"], STREAM))]),
    "topk-some-errors": (_topk_partial_errors, [
        ("fedavg_topk_sparsify", (HANDLE, _native.F32, [0, "delta1", "delta2"], [0, "err1", 0], [0, 7, 17], [0, 3, 17],
                                  3, [0, "idx1", "idx2"], [0, "val1", "val2"], [0, "res1", "res2"], STREAM))]),
}


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_accepted_call(env, name):
    call, expected = ACCEPTED[name]
    result = call(env)
    if isinstance(result, tuple):  # (dots, sqnorms): two rows of one allocation
        assert result[1].data_ptr() == result[0].data_ptr() + 2 * 8
        result = result[0]
    if isinstance(result, torch.Tensor):
        env.names[result.data_ptr()] = "result"
    assert env.ctx._lib.named(env.names) == expected


def test_results_are_allocated_for_the_table(env):
    """The wrappers that allocate their result size it by the client count."""
    table = env.table(3)
    assert env.ctx.pairwise_sqdist(table, F32).shape == (3, 3)
    assert env.ctx.sqdist_to_point(table, F32).shape == (3,)
    dots, sqnorms = env.ctx.moments_about_point(table, F32, None, env.segs("direction"))
    assert dots.shape == sqnorms.shape == (3,)
    assert {r.dtype for r in (dots, sqnorms)} == {F64}


def test_index_violation_is_reported(env, monkeypatch):
    """``sparse_aggregate_delta`` raises after the launch when the library reports an index error."""
    lib = env.ctx._lib

    def errors(h, stream, out):
        out._obj.value = 1
        return 0

    monkeypatch.setattr(lib, "fedavg_sparse_index_errors", errors, raising=False)
    with pytest.raises(ValueError) as err:
        cases.sparse_fold(env)
    assert str(err.value) == fedavg.SPARSE_INDEX_MESSAGE
    assert [fn for fn, _ in lib.calls] == ["fedavg_sparse_aggregate_delta"]
