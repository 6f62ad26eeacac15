"""The routed row gather (csrc/route_kernels.hip, ``fedavg_route_rows``) against DESIGN.md §5o,
through the C ABI itself, at the smallest shapes where the kernels can go wrong: every row width
class (element path, 16-byte path, a row longer than one workgroup pass), a misaligned source, list
lengths around the chunk (``route_chunk`` from the build) under four hit patterns, ids at the edges
of the node space, the source-table edges, the surroundings of all three outputs, the error bits and
the table's return to empty, reuse of one handle, and the refusals before any launch.

Every pointer handed over is a whole torch tensor or a view that ends inside its buffer; the
ill-formed inputs (a duplicate id, a list out of order) are well-formed buffers whose *contents*
break a rule, which the kernels are specified to survive inside the buffers.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from distributed_learning_simulation_lib_amd import _native

pytestmark = pytest.mark.gpu

GUARD = 64          # guard bytes (rows), guard elements (ids, counts) on both sides of an output
ROW_FILL = 0xA5
ID_FILL = -7777
COUNT_FILL = -3333


def chunk() -> int:
    return _native.kernel_constant("route_chunk")


class Route:
    """A routing handle driven through the raw ABI."""

    def __init__(self, device) -> None:
        self.lib = _native.load()
        self.device = device
        self.h = ctypes.c_void_p()
        assert self.lib.fedavg_route_create(ctypes.byref(self.h), device.index) == _native.OK

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def rows(self, src_ptrs, src_rows, S, row_bytes, elem, src_ids, want_ids, want_off, N, node_space, out_rows,
             out_ids, out_count) -> int:
        return self.lib.fedavg_route_rows(self.h, src_ptrs, src_rows, S, row_bytes, elem, src_ids, want_ids, want_off,
                                          N, node_space, out_rows, out_ids, out_count, self.stream())

    def errors(self) -> int:
        out = ctypes.c_int32(-1)
        assert self.lib.fedavg_route_errors(self.h, self.stream(), ctypes.byref(out)) == _native.OK
        return out.value

    def close(self) -> None:
        assert self.lib.fedavg_route_destroy(self.h) == _native.OK


@pytest.fixture()
def route(hip_device):
    r = Route(hip_device)
    yield r
    r.close()


class Call:
    """One call's device buffers. ``sources`` = [(id list, uint8 array [n, row_bytes])], ``lists`` =
    [id list]. The outputs sit between guards; ``lead`` shifts every source block by that many bytes
    off its 16-byte-aligned allocation."""

    def __init__(self, device, sources, lists, row_bytes, elem, node_space, lead=0) -> None:
        self.sources, self.lists, self.row_bytes, self.elem, self.node_space = sources, lists, row_bytes, elem, node_space
        self.blocks = []
        for _, rows in sources:
            assert rows.dtype == np.uint8 and rows.shape[1:] == (row_bytes,)
            buf = torch.empty(rows.size + lead + 16, dtype=torch.uint8, device=device)
            view = buf[lead: lead + rows.size]
            view.copy_(torch.from_numpy(rows.reshape(-1)))
            assert rows.size == 0 or view.data_ptr() % 16 == lead % 16
            self.blocks.append(view)
        self.S, self.N = len(sources), len(lists)
        self.ptrs = np.array([b.data_ptr() for b in self.blocks], dtype=np.uint64)
        self.nrows = np.array([len(ids) for ids, _ in sources], dtype=np.int64)
        self.want_off = np.zeros(self.N + 1, dtype=np.int64)
        np.cumsum([len(x) for x in lists], out=self.want_off[1:])
        self.B = int(self.want_off[-1])
        flat = lambda xs: torch.tensor([i for x in xs for i in x], dtype=torch.int64, device=device)  # noqa: E731
        self.src_ids = flat([ids for ids, _ in sources])
        self.want_ids = flat(lists)
        self.out_rows = torch.full((GUARD + self.B * row_bytes + GUARD,), ROW_FILL, dtype=torch.uint8, device=device)
        self.out_ids = torch.full((GUARD + self.B + GUARD,), ID_FILL, dtype=torch.int64, device=device)
        self.out_count = torch.full((GUARD + self.N + GUARD,), COUNT_FILL, dtype=torch.int32, device=device)

    def args(self):
        return (self.ptrs.ctypes.data if self.S else None, self.nrows.ctypes.data if self.S else None, self.S,
                self.row_bytes, self.elem, self.src_ids.data_ptr(), self.want_ids.data_ptr(), self.want_off.ctypes.data,
                self.N, self.node_space, self.out_rows.data_ptr() + GUARD, self.out_ids.data_ptr() + 8 * GUARD,
                self.out_count.data_ptr() + 4 * GUARD)

    def run(self, route: Route) -> None:
        status = route.rows(*self.args())
        assert status == _native.OK, _native.last_error()

    def untouched(self) -> bool:
        return (bool((self.out_rows == ROW_FILL).all()) and bool((self.out_ids == ID_FILL).all())
                and bool((self.out_count == COUNT_FILL).all()))

    def check(self) -> None:
        """The contract, from dicts: counts, ids and rows of every list's packed prefix; everything
        else of the three buffers as it was (this implementation leaves the slots past a count
        alone, so a write into another list's slot shows)."""
        where = {}
        for ids, rows in self.sources:
            for i, node in enumerate(ids):
                where[node] = rows[i]
        rows = self.out_rows.cpu().numpy()
        ids = self.out_ids.cpu().numpy()
        counts = self.out_count.cpu().numpy()
        want_rows = np.full_like(rows, ROW_FILL)
        want_ids = np.full_like(ids, ID_FILL)
        want_counts = np.full_like(counts, COUNT_FILL)
        for j, wanted in enumerate(self.lists):
            hits = [n for n in wanted if n in where]
            want_counts[GUARD + j] = len(hits)
            at = int(self.want_off[j])
            for k, n in enumerate(hits):
                want_ids[GUARD + at + k] = n
                o = GUARD + (at + k) * self.row_bytes
                want_rows[o: o + self.row_bytes] = where[n]
        assert np.array_equal(counts, want_counts), (counts[GUARD:GUARD + self.N], want_counts[GUARD:GUARD + self.N])
        assert np.array_equal(ids, want_ids)
        assert np.array_equal(rows, want_rows)


def make_rows(rng, n, row_bytes) -> np.ndarray:
    rows = rng.integers(0, 255, size=(n, row_bytes), dtype=np.uint8)
    rows[rows == ROW_FILL] = 1  # a copied byte never looks like an untouched one
    return rows


def elem_of(row_bytes: int) -> int:
    return 8 if row_bytes % 8 == 0 else 4 if row_bytes % 4 == 0 else 2


@pytest.mark.parametrize("lead", [0, 8], ids=["aligned", "misaligned_source"])
@pytest.mark.parametrize("row_bytes", [2, 6, 8, 16, 24, 256, 20000])
def test_row_widths_and_source_alignment(route, hip_device, row_bytes, lead):
    rng = np.random.default_rng(row_bytes)
    elem = elem_of(row_bytes)
    ids = rng.permutation(200)[:20].tolist()
    sources = [(ids[:7], make_rows(rng, 7, row_bytes)), ([], make_rows(rng, 0, row_bytes)),
               (ids[7:8], make_rows(rng, 1, row_bytes)), (ids[8:20], make_rows(rng, 12, row_bytes))]
    lists = [sorted(ids[3:15] + [250, 251]), [], sorted(rng.permutation(260)[:90].tolist()), sorted(ids)]
    call = Call(hip_device, sources, lists, row_bytes, elem, 200, lead=lead)
    call.run(route)
    assert route.errors() == 0
    call.check()


def patterns(n: int, C: int) -> dict[str, list[int]]:
    """Positions of a list of n wanted ids that hit."""
    return {"all": list(range(n)), "none": [], "alternating": list(range(0, n, 2)),
            "last_of_each_chunk": sorted({p for p in range(n) if p % C == C - 1} | ({n - 1} if n else set()))}


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "last_of_each_chunk"])
@pytest.mark.parametrize("length", ["0", "1", "C-1", "C", "C+1", "3C+5"])
def test_list_lengths_around_the_chunk(route, hip_device, length, pattern):
    C = chunk()
    n = {"0": 0, "1": 1, "C-1": C - 1, "C": C, "C+1": C + 1, "3C+5": 3 * C + 5}[length]
    rng = np.random.default_rng(n)
    wanted = (np.arange(n) * 3 + 1).tolist()
    hits = [wanted[p] for p in patterns(n, C)[pattern]]
    extra = [0, 3 * n + 3, 3 * n + 6]  # sent, wanted by the neighbour lists only
    sent = rng.permutation(hits + extra).tolist()
    half = len(sent) // 2
    row_bytes = 16 if n % 2 else 8
    sources = [(sent[:half], make_rows(rng, half, row_bytes)), (sent[half:], make_rows(rng, len(sent) - half, row_bytes))]
    lists = [[0, 2, 3 * n + 6], wanted, [3 * n + 3, 3 * n + 4]]
    call = Call(hip_device, sources, lists, row_bytes, 8, 3 * n + 7)
    call.run(route)
    assert route.errors() == 0
    call.check()


def test_ids_at_the_edges_of_the_node_space_miss(route, hip_device):
    rng = np.random.default_rng(1)
    K = 1000
    sources = [([K - 1, 0, 5], make_rows(rng, 3, 24))]
    lists = [[-(1 << 40), -1, 0, K - 1, K, K + 1, 1 << 40], [-1], [K], [1 << 40], [K - 1]]
    call = Call(hip_device, sources, lists, 24, 8, K)
    call.run(route)
    assert route.errors() == 0
    call.check()
    assert call.out_count[GUARD: GUARD + 5].tolist() == [2, 0, 0, 0, 1]


def test_no_source_an_empty_source_and_1024_sources(route, hip_device):
    rng = np.random.default_rng(2)
    call = Call(hip_device, [], [[1, 2, 3], [], [7]], 8, 8, 100)  # S = 0: every list misses everything
    call.run(route)
    assert route.errors() == 0
    call.check()
    call = Call(hip_device, [([], make_rows(rng, 0, 8))], [[1, 2, 3]], 8, 8, 0)  # one source, no row
    call.run(route)
    assert route.errors() == 0
    call.check()
    ids = rng.permutation(5000)[:1024].tolist()
    sources = [([i], make_rows(rng, 1, 48)) for i in ids]
    call = Call(hip_device, sources, [sorted(ids), sorted(ids[::3] + [5000, 6000]), sorted(ids[1000:])], 48, 4, 5000)
    call.run(route)
    assert route.errors() == 0
    call.check()
    # one more than the limit is refused
    sources.append(([5001], make_rows(rng, 1, 48)))
    call = Call(hip_device, sources, [[1]], 48, 4, 6000)
    assert route.rows(*call.args()) == _native.ERR_INVALID


def clean_call(device, seed=3):
    rng = np.random.default_rng(seed)
    ids = rng.permutation(400)[:60].tolist()
    return Call(device, [(ids[:25], make_rows(rng, 25, 32)), (ids[25:], make_rows(rng, 35, 32))],
                [sorted(rng.permutation(400)[:150].tolist()), sorted(ids)], 32, 4, 400)


def test_error_bits_and_the_table_restored_after_them(route, hip_device):
    rng = np.random.default_rng(4)
    # a node id sent twice (across sources, and inside one)
    dup = Call(hip_device, [([5, 9, 300], make_rows(rng, 3, 16)), ([9, 11, 11], make_rows(rng, 3, 16))],
               [[5, 9, 11, 300]], 16, 4, 400)
    dup.run(route)
    assert route.errors() == _native.ROUTE_ERR_DUPLICATE
    assert route.errors() == 0  # reported once
    # guards intact, counts inside the slot
    assert bool((dup.out_rows[:GUARD] == ROW_FILL).all()) and bool((dup.out_rows[-GUARD:] == ROW_FILL).all())
    assert bool((dup.out_ids[:GUARD] == ID_FILL).all()) and bool((dup.out_ids[-GUARD:] == ID_FILL).all())
    assert 0 <= int(dup.out_count[GUARD]) <= 4
    call = clean_call(hip_device)  # wants 5, 9, 11, 300 among others: the table must be empty again
    call.run(route)
    assert route.errors() == 0
    call.check()
    # a want list that is not strictly increasing (equal neighbours; a descent across a chunk edge)
    C = chunk()
    for bad in ([3, 7, 7, 9], list(range(C)) + [C - 1, C + 5]):
        order = Call(hip_device, [([3, 7, 9], make_rows(rng, 3, 16))], [[1, 2], bad, [9]], 16, 4, 400)
        order.run(route)
        assert route.errors() == _native.ROUTE_ERR_ORDER
        assert bool((order.out_rows[:GUARD] == ROW_FILL).all()) and bool((order.out_rows[-GUARD:] == ROW_FILL).all())
        call = clean_call(hip_device, seed=5)
        call.run(route)
        assert route.errors() == 0
        call.check()
    # a sent id outside the node space is nobody's row
    out = Call(hip_device, [([3, 400, 9], make_rows(rng, 3, 16))], [[3, 9, 400]], 16, 4, 400)
    out.run(route)
    assert route.errors() == _native.ROUTE_ERR_RANGE
    assert int(out.out_count[GUARD]) == 2


def test_two_rounds_back_to_back_on_one_handle(route, hip_device):
    """No wait between the calls: the second sees an empty table, a grown node space and its own
    tables (the staging slots alternate); a third call shrinks the node space again."""
    rng = np.random.default_rng(6)
    a_ids = rng.permutation(300)[:80].tolist()
    a = Call(hip_device, [(a_ids, make_rows(rng, 80, 64))], [sorted(a_ids[:50] + [301]), sorted(a_ids[40:])], 64, 4, 300)
    b_ids = (rng.permutation(20000)[:90] + 300).tolist()  # none of round one's nodes
    b = Call(hip_device, [(b_ids[:30], make_rows(rng, 30, 6)), (b_ids[30:], make_rows(rng, 60, 6))],
             [sorted(a_ids), sorted(b_ids + a_ids[:10]), sorted(b_ids[::2])], 6, 2, 20300)
    c = Call(hip_device, [(a_ids[:5], make_rows(rng, 5, 64))], [sorted(a_ids + b_ids[:3])], 64, 8, 300)
    a.run(route)
    b.run(route)
    c.run(route)
    assert route.errors() == 0
    a.check()
    b.check()
    c.check()


def test_refusals_before_any_launch(route, hip_device):
    call = clean_call(hip_device)
    good = list(call.args())
    (PTRS, NROWS, S, ROW_BYTES, ELEM, SRC_IDS, WANT_IDS, WANT_OFF, N, NODE_SPACE, OUT_ROWS, OUT_IDS, OUT_COUNT) = range(13)

    def refused(**changes) -> None:
        args = list(good)
        for k, v in changes.items():
            args[globals_index[k]] = v
        assert route.rows(*args) == _native.ERR_INVALID, changes
        assert _native.last_error()

    globals_index = dict(ptrs=PTRS, nrows=NROWS, S=S, row_bytes=ROW_BYTES, elem=ELEM, src_ids=SRC_IDS, want_ids=WANT_IDS,
                         want_off=WANT_OFF, N=N, node_space=NODE_SPACE, out_rows=OUT_ROWS, out_ids=OUT_IDS,
                         out_count=OUT_COUNT)
    for name in ("ptrs", "nrows", "want_off", "out_count", "src_ids", "want_ids", "out_rows", "out_ids"):
        refused(**{name: None})  # NULL tables
    refused(S=-1)
    refused(S=1025)
    refused(N=0)
    refused(N=-1)
    refused(row_bytes=0)
    refused(row_bytes=-4)
    refused(row_bytes=30)  # not a multiple of the 4-byte element
    refused(elem=3)
    refused(elem=16)
    refused(node_space=-1)
    refused(node_space=(1 << 28) + 1)
    refused(out_rows=good[OUT_ROWS] + 2)  # not aligned to the element
    refused(src_ids=good[SRC_IDS] + 4)
    refused(want_ids=good[WANT_IDS] + 4)
    refused(out_ids=good[OUT_IDS] + 4)
    refused(out_count=good[OUT_COUNT] + 2)
    ptrs = call.ptrs.copy()
    ptrs[1] += 2
    refused(ptrs=ptrs.ctypes.data)
    nrows = call.nrows.copy()
    nrows[0] = -1
    refused(nrows=nrows.ctypes.data)
    nrows[0] = 1 << 31  # R >= 2^31
    refused(nrows=nrows.ctypes.data)
    for off in ([1, 150, 210], [0, 160, 150], [0, 150, 1 << 31]):  # not from 0, decreasing, B >= 2^31
        refused(want_off=np.array(off, dtype=np.int64).ctypes.data)
    assert route.lib.fedavg_route_rows(None, *good, route.stream()) == _native.ERR_INVALID
    assert route.errors() == 0
    assert call.untouched()  # nothing was launched
    call.run(route)  # and the handle still works
    assert route.errors() == 0
    call.check()
