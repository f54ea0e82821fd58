"""Host side of the warm start (``search.ModelCache``, ``search.search(warm=...)``, the
``MYTHGPU_WARM`` switch of the hook): no GPU, no native library.

Reference anchor: LASER's successor queries are the parent's constraints plus one condition
(``mythril/laser/ethereum/svm.py:252-257``), and the independence solver's buckets merge when a
new constraint joins their variables (``independence_solver.py:119-140``).
"""
import numpy as np

from mythril_amd import partition, plugin, search, ssa
from mythril_amd.smt import Array, Function, UGT, ULT, symbol_factory
from tests.test_search_host import FakeEngine

BVV = symbol_factory.BitVecVal
BVS = symbol_factory.BitVecSym


def _mixed_query():
    """Scalars, a calldata byte (an AUX word and a site sliced from it), a storage site and an
    inverse-UF site whose default is lazy."""
    x, y = BVS("wh_x", 256), BVS("wh_y", 40)
    calldata = Array("7_calldata", 256, 8)
    storage = Array("Storage", 256, 256)
    h, hinv = Function("keccak256_256", 256, 256), Function("keccak256_256-1", 256, 256)
    return [ULT(x, BVV(77, 256)).raw, (y == BVV(5, 40)).raw, (calldata[BVV(5, 256)] == BVV(9, 8)).raw,
            UGT(storage[x], BVV(3, 256)).raw, (hinv(h(x)) == x).raw]


def test_coords_from_assignment_round_trips_through_the_soa():
    P, _ = search.prepare(_mixed_query())
    entries, widths = search.model_watch(P)
    kinds = {c.kind for c in P.coords}
    assert {ssa.COORD_SCALAR, ssa.COORD_AUX, ssa.COORD_ARRAY_SITE, ssa.COORD_UF_SITE} <= kinds
    # watch rows as a search writes them: one value per entry, limbs little-endian
    vals = [(0x1111111111111111111111111111111111111111111111111111111111111111 * (i + 1)) & ((1 << w) - 1)
            for i, w in enumerate(widths)]
    assign = np.array([limb for v, w in zip(vals, widths) for limb in ssa.int_to_limbs(v, w)], dtype=np.uint32)
    assert assign.size == P.watch_words
    coords = search.coords_from_assignment(P, assign)
    by_entry = {}
    for e, v in zip(entries, vals):  # a node may be watched twice (a scalar that is also a site's key):
        by_entry.setdefault(e, v)    # the scalars come first
    lazy = {c.index for c in P.coords if search._is_lazy(P, c)}
    assert lazy and P.aux_slice
    for c in P.coords:
        if c.kind in (ssa.COORD_SCALAR, ssa.COORD_AUX):
            assert coords[c.index] == by_entry[c.node], c
        elif c.index in lazy or c.index in P.aux_slice:
            assert c.index not in coords, c
        else:
            assert coords[c.index] == by_entry[0x80000000 | c.index], c
    # ... and through soa_from_assignments: the rows of every recovered coordinate hold its limbs
    soa = ssa.soa_from_assignments(P, [[coords.get(c.index, 0) for c in P.coords]])
    offs = P.coord_row_offsets()
    for ci, v in coords.items():
        L = ssa.limbs(P.coords[ci].width)
        assert ssa.limbs_to_int(soa[offs[ci]:offs[ci] + L, 0]) == v
    # the cache hands the same limbs to the engine, by key
    cache = search.ModelCache()
    cache.store(P, _mixed_query(), coords)
    s = cache.lookup(P, _mixed_query())
    assert s.n_seeds == 1 and s.n_rows == s.rows.shape[0]
    for c in P.coords:
        row = int(s.coord_row[c.index])
        if c.index in coords:
            L = ssa.limbs(c.width)
            assert ssa.limbs_to_int(s.rows[row:row + L, 0]) == coords[c.index] and int(s.coord_has[c.index]) == 1
        else:
            assert row == ssa.MG_NONE and int(s.coord_has[c.index]) == 0


def _two_buckets():
    a, b, c, d = (BVS(f"wm_{n}", 256) for n in "abcd")
    left = [ULT(a, b).raw, UGT(a, BVV(5, 256)).raw]
    right = [ULT(c, d).raw]
    join = (b + c == BVV(99, 256)).raw
    return left, right, join


def test_cache_keys_survive_a_bucket_merge():
    """Two buckets solved on their own, then a root that joins them: the merged bucket's program
    has other coordinate positions, and still finds both models' values."""
    left, right, join = _two_buckets()
    assert len(partition.partition(left + right)) == 2
    merged = partition.partition(left + right + [join])
    assert len(merged) == 1
    cache = search.ModelCache()
    Pl, _ = search.prepare(left)
    Pr, _ = search.prepare(right)
    vl = {c.index: 1000 + c.index for c in Pl.coords}
    vr = {c.index: 2000 + c.index for c in Pr.coords}
    cache.store(Pl, left, vl)
    cache.store(Pr, right, vr)
    # the merged bucket in an order that moves the coordinates (the right bucket's roots first)
    roots = right + [join] + left
    P, _ = search.prepare(roots)
    name = {c.name: c for c in P.coords}
    assert [c.name for c in P.coords][:2] == ["wm_c", "wm_d"] and [c.name for c in Pl.coords][0] == "wm_a"
    s = cache.lookup(P, roots)
    assert s.n_seeds == 2  # [left (two shared roots), right (one)]
    want = {"wm_a": (0, vl), "wm_b": (0, vl), "wm_c": (1, vr), "wm_d": (1, vr)}
    for n, (m, vals) in want.items():
        c = name[n]
        src = next(x for x in (Pl if m == 0 else Pr).coords if x.name == n)
        row = int(s.coord_row[c.index])
        assert int(s.coord_has[c.index]) == 1 << m, n
        assert ssa.limbs_to_int(s.rows[row:row + 8, m]) == vals[src.index], n
    # a query that shares no root finds nothing
    assert cache.lookup(P, [join]) is None


def _q(i):
    return [ULT(BVS("wl_x", 256), BVV(10 + i, 256)).raw]


def test_lru_bound():
    cache = search.ModelCache()
    assert cache.capacity == search.ModelCache.CAPACITY == 256
    P, _ = search.prepare(_q(0))
    for i in range(300):
        cache.store(P, _q(i), {0: i})
    assert len(cache) == 256
    assert cache.lookup(P, _q(43)) is None            # the 44 oldest are gone
    assert int(cache.lookup(P, _q(44)).rows[0, 0]) == 44
    # a used entry is the most recent again: 45 more stores push out 45.., not 44
    for i in range(300, 345):
        cache.store(P, _q(i), {0: i})
    assert cache.lookup(P, _q(44)) is not None and cache.lookup(P, _q(46)) is None
    # storing a query again replaces its model and does not grow the cache
    cache.store(P, _q(44), {0: 7})
    assert len(cache) == 256 and int(cache.lookup(P, _q(44)).rows[0, 0]) == 7


def test_lookup_ranking():
    """Up to four entries: most shared roots first, then the most recent; at least one shared root."""
    x = BVS("wr_x", 256)
    r = [ULT(x, BVV(100 + i, 256)).raw for i in range(6)]
    other = [UGT(BVS("wr_y", 256), BVV(1, 256)).raw]
    P, _ = search.prepare(r)
    cache = search.ModelCache()
    stored = [(r[:1], 10), (r[:3], 11), (r[1:2], 12), (other, 13), (r[:2], 14), (r[3:5], 15), (r[5:], 16)]
    for roots, v in stored:
        cache.store(P if roots is not other else search.prepare(other)[0], roots, {0: v})
    s = cache.lookup(P, r[:3] + [r[5]])
    assert s.n_seeds == 4 == search.ModelCache.MAX_SEEDS
    # shared roots: 11 -> 3, 14 -> 2, then one each: 16 (newest), 12, 10; `other` and 15 share none
    assert [int(v) for v in s.rows[0]] == [11, 14, 16, 12]
    assert cache.lookup(P, other + [r[0]]) is not None
    assert cache.lookup(P, [UGT(x, BVV(7, 256)).raw]) is None
    assert search.warm_keep16(1) == search.warm_keep16(4) == 32768 and search.warm_keep16(16) == 65536 - 8192


class SeededFake(FakeEngine):
    def __init__(self, answer):
        super().__init__()
        self.answer = answer
        self.seeded_calls = []

    def search_seeded(self, prog, gh, seeds, seed, start, n, early_exit=True, assign=None):
        self.seeded_calls.append((seeds.n_seeds, seeds.keep16, start, n))
        return self.answer


def test_search_takes_a_seeded_hit_and_falls_through_a_miss():
    roots = _q(0) + [UGT(BVS("wl_x", 256), BVV(2, 256)).raw]
    P, _ = search.prepare(roots)
    cache = search.ModelCache()
    cache.store(P, _q(0), {0: 4})
    eng = SeededFake((0, 3))
    res = search.search(eng, roots, timeout_s=0.05, warm=cache)
    assert eng.seeded_calls == [(1, 32768, 0, 1 << 12)] and eng.launches["interp"] == 0
    assert (res.index, res.hits, res.engine, res.seeded, res.replay) == (0, 3, "seeded", True, True)
    assert res.timing["seeded_ms"] >= 0 and len(cache) == 2  # the hit's model is stored
    eng = SeededFake((128, 1))  # group 2 of the two seeds now cached: round 1, not a replay lane
    res = search.search(eng, roots, timeout_s=0.05, warm=cache, want_model=False)
    assert res.seeded and not res.replay
    eng = SeededFake((None, 0))
    res = search.search(eng, roots, timeout_s=0.03, max_candidates=1 << 40, warm=cache, jit="never")
    assert len(eng.seeded_calls) == 1 and eng.launches["interp"] > 0
    assert res.index is None and not res.seeded and res.engine == "interp" and "seeded_ms" in res.timing
    # without a cache, or with one that has nothing for the query, the engine is never asked
    for warm in (None, search.ModelCache()):
        eng = SeededFake((0, 1))
        search.search(eng, roots, timeout_s=0.02, max_candidates=1 << 40, warm=warm, jit="never")
        assert eng.seeded_calls == []


def test_warm_switch_is_off_by_default(monkeypatch):
    calls = []

    def fake_partitioned(engine, terms, **kw):
        calls.append(kw)
        return search.SearchResult(None, 0, 0, 0.0)

    monkeypatch.setattr(search, "search_partitioned", fake_partitioned)
    monkeypatch.setattr("mythril_amd.native.Engine.get", classmethod(lambda cls: FakeEngine()))
    monkeypatch.delenv("MYTHGPU_WARM", raising=False)
    monkeypatch.setattr(plugin, "_WARM", None)
    plugin._gpu_search(_q(0), 0.01, None)
    assert calls[-1] == {"timeout_s": 0.01, "max_candidates": 1 << 40, "cancel": None,
                         "max_launch_s": plugin.RACE_LAUNCH_S}
    assert plugin._WARM is None
    monkeypatch.setenv("MYTHGPU_WARM", "1")
    plugin._gpu_search(_q(0), 0.01, None)
    plugin._gpu_search(_q(0), 0.01, None)
    assert isinstance(calls[-1]["warm"], search.ModelCache) and calls[-1]["warm"] is calls[-2]["warm"]
    assert {k: v for k, v in calls[-1].items() if k != "warm"} == calls[0]


def test_unset_switch_runs_the_same_engine_calls(monkeypatch):
    """``_gpu_search`` against the stand-in engine with the switch unset: ordinary launches only
    (the stand-in has no seeded entry point, so a seeded call would raise)."""
    eng = FakeEngine()
    monkeypatch.setattr("mythril_amd.native.Engine.get", classmethod(lambda cls: eng))
    monkeypatch.delenv("MYTHGPU_WARM", raising=False)
    before = (plugin.STATS.warm_tried, plugin.STATS.warm_hits, plugin.STATS.warm_replay_hits)
    res = plugin._gpu_search(_q(0), 0.03, None)
    assert res.index is None and eng.launches["interp"] > 0
    assert (plugin.STATS.warm_tried, plugin.STATS.warm_hits, plugin.STATS.warm_replay_hits) == before
