"""Reference of the seeded sweep (``include/mythgpu.h``, "seeded sweep"): the C port's generated
coordinates (``cport.gen_soa``), the seed overrides restated here from the documented rule, and the
C port's verdicts of the composed SoA (``cport.eval_soa``).  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from mythril_amd import ssa
from oracle import cport
from tests.gen3_ref import fmix64, lane_key, rnd_at as rnd  # noqa: F401

M64 = (1 << 64) - 1
M32 = 0xFFFFFFFF
GEN_LAZY = 6
NONE = 0xFFFFFFFF


def lazy_coords(gen_blob) -> set:
    n = int(gen_blob[1])
    return {c for c in range(n) if (int(gen_blob[4 + 8 * c]) & 0xFF) == GEN_LAZY}


def seeded_soa(P: ssa.Program, gen_blob, seeds, seed: int, start: int, n: int) -> np.ndarray:
    """The coordinates of seeded candidates [start, start + n) as SoA rows (mg_eval layout).
    ``seeds``: a ``native.SeedSet``."""
    soa = cport.gen_soa(P.to_bytes(), gen_blob, seed, start, n, P.coord_words)
    ns = seeds.n_seeds
    if ns == 0:
        return soa
    lazy = lazy_coords(gen_blob)
    offs = P.coord_row_offsets()
    for q in range(n):
        i = start + q
        g, lane = i >> 6, i & 63
        m, rnd_ = g % ns, g // ns
        for c in P.coords:
            ci = c.index
            row = int(seeds.coord_row[ci])
            if row == NONE or not (int(seeds.coord_has[ci]) >> m) & 1 or ci in lazy:
                continue
            if not ((lane == 0 and rnd_ == 0) or (rnd(seed, i, ci, 0xFFFD) >> 16) < seeds.keep16):
                continue
            L = ssa.limbs(c.width)
            v = ssa.limbs_to_int([int(seeds.rows[row + j, m]) for j in range(L)]) & ((1 << c.width) - 1)
            for j in range(L):
                soa[offs[ci] + j, q] = (v >> (32 * j)) & M32
    return soa


def seeded_verdicts(P: ssa.Program, gen_blob, seeds, seed: int, start: int, n: int):
    """(verdicts uint8[n], the composed SoA)."""
    soa = seeded_soa(P, gen_blob, seeds, seed, start, n)
    return cport.eval_soa(P.to_bytes(), soa, n), soa


def seeded_search(P: ssa.Program, gen_blob, seeds, seed: int, start: int, count: int):
    """(first hit or None, hit count) of the full seeded sweep."""
    ver, _ = seeded_verdicts(P, gen_blob, seeds, seed, start, count)
    hits = np.flatnonzero(ver)
    return (start + int(hits[0]) if hits.size else None), int(hits.size)


def seed_set(P: ssa.Program, models, keep16: int = 65536, never=()):
    """A ``native.SeedSet`` from ``models``: one {coord index: value} dict per seed.  Coordinates in
    ``never`` (and those no model mentions) get ``coord_row = MG_NONE``."""
    from mythril_amd import native

    ns = len(models)
    coord_row = np.full(len(P.coords), NONE, dtype=np.uint32)
    coord_has = np.zeros(len(P.coords), dtype=np.uint32)
    rows = []
    for c in P.coords:
        if c.index in never or not any(c.index in m for m in models):
            continue
        coord_row[c.index] = len(rows)
        L = ssa.limbs(c.width)
        for j in range(L):
            rows.append([(int(m.get(c.index, 0)) >> (32 * j)) & M32 for m in models])
        for k, m in enumerate(models):
            if c.index in m:
                coord_has[c.index] |= 1 << k
    arr = np.array(rows, dtype=np.uint32).reshape(len(rows), ns) if rows else np.zeros((0, ns), dtype=np.uint32)
    return native.SeedSet(arr, coord_row, coord_has, keep16=keep16)
