"""The table ring of the side modules (csrc/call_tables.h, ``TableRing``) restated: how many bytes
of tables a call of each entry point uploads, and what ``TableRing::acquire`` does with its two
slots over a sequence of calls. tests/test_gpu_table_ring.py chooses its client counts from these.
"""

from __future__ import annotations

SLOTS = 2
FIRST_SLOT = 64 * 1024       # a slot's least capacity; one that is too small regrows to twice the need


def table_bytes(entry: str, n: int, T: int) -> int:
    """The bytes one call uploads for ``n`` clients of ``T`` segments, from the entry points' own
    arithmetic: [n][T] client pointers, then what the entry point adds."""
    clients = 8 * n * T
    return {
        "krum": clients,                       # fedavg_pairwise_sqdist
        "point": clients + 8 * T,              # fedavg_sqdist_to_point: the point's pointers
        "clip": clients + 16 * T + 8 * n,      # fedavg_fold_about_point: point, outs, coefficients
        "trust": clients + 16 * T,             # fedavg_moments_about_point: direction, centre
        "opt": clients + 48 * T + 8 * n,       # fedavg_server_opt_step: six segment tables, coefficients
    }[entry]


def slot_events(needs) -> list[str]:
    """Per call of a fresh state what ``acquire`` does with the slot it takes (call i takes slot
    i % 2): ``"first"`` allocates it, ``"regrow"`` frees and reallocates it, ``"fit"`` reuses it."""
    caps, out = [0] * SLOTS, []
    for i, b in enumerate(needs):
        s = i % SLOTS
        if caps[s] >= b:
            out.append("fit")
            continue
        out.append("regrow" if caps[s] else "first")
        caps[s] = max(2 * b, FIRST_SLOT)
    return out
