"""The climb on the device (``mg_search_climb``: kernels ``k_run_climb`` and ``k_climb_select``,
``search.climb(ClimbConfig(device=True))``) against the host climb on the same engine and, for the
star and chain queries, against ``tests/scored_ref.py`` (the C port's sweeps and the restated loop).
Every comparison is exact: the same candidates, the same population, the same trajectory."""
import numpy as np
import pytest

from mythril_amd import native, search, ssa, workloads
from mythril_amd.smt import terms as T
from oracle.bv import OracleModel, evaluate
from tests import scored_ref, seeded_ref
from tests.climb_device_ref import assert_same

pytestmark = pytest.mark.gpu

SEED0 = 0x6D797468
A = 0x1F3A9C5B27D4EB4F00C0FFEE5EED12349E3779B97F4A7C15F39CC0605CEDC835

# name: (query, chunk, ClimbConfig arguments, what the CPU reference measured: stop, rounds, best)
CONFIGS = {
    "star8": ("star", 4096, {}, ("hit", 8, 0)),
    "star8-rounds3": ("star", 4096, {"rounds": 3}, ("rounds", 3, 3)),
    "star8-beam1": ("star", 4096, {"beam": 1}, ("hit", None, 0)),
    "star8-beam5": ("star", 4096, {"beam": 5}, ("hit", None, 0)),
    "star8-beam32": ("star", 4096, {"beam": 32}, ("patience", 13, 1)),
    "star8-chunk192": ("star", 192, {"rounds": 6}, ("rounds", 6, None)),
    # an unaligned window.  (The C-port reference and the host climb both end this one on a hit in
    # round 10, at index 2984; the rounds limit is covered by star8-rounds3 and star8-chunk192.)
    "star8-unaligned": ("star", 64 * 5 + 7, {"beam": 3}, ("hit", 10, 0)),
    "chain8": ("chain", 4096, {}, ("patience", 9, 2)),
}


class Query:
    def __init__(self, engine, roots):
        self.roots = roots
        self.P, self.blob = search.prepare(roots, None)
        self.prog = engine.load(self.P.to_bytes())
        self.gen = engine.load_gen(self.prog, self.blob)


def _site_roots(n_star):
    """Star roots plus a site read at the shared variable and coordinates of 40, 8 and 1 bits."""
    y, e = T.BitVecVar("cs_y", 256), T.BitVecVar("cs_e", 256)
    c40, d8, f = T.BitVecVar("cs_c", 40), T.BitVecVar("cs_d", 8), T.BoolVar("cs_f")
    site = T.select(T.ArrayVar("cs_mem", 256, 256), y)
    return workloads.climb_star(n_star, tag="cs") + [
        T.eq(T.extract(5, 0, T.bvbin("bvadd", site, e)), T.BitVecVal(33, 6)),
        T.eq(T.extract(39, 35, c40), T.BitVecVal(9, 5)),
        T.and_(T.bvcmp("bvult", d8, T.BitVecVal(0x10, 8)), f)]


@pytest.fixture(scope="module")
def queries(engine):
    out = {"star": Query(engine, workloads.climb_star(8)), "chain": Query(engine, workloads.climb_chain(8)),
           "site": Query(engine, _site_roots(6))}
    yield out
    for q in out.values():
        engine.free_gen(q.gen)
        engine.free(q.prog)


class Recorder:
    """The engine, remembering what every scored sweep returned."""

    def __init__(self, engine):
        self.engine, self.sweeps = engine, []
        self.stats = engine.stats

    def search_scored(self, *a, **kw):
        first, nh, slots, assigns = self.engine.search_scored(*a, **kw)
        self.sweeps.append((first, list(slots), assigns.copy()))
        return first, nh, slots, assigns


def _host(engine, q, chunk, kw, **more):
    return search.climb(engine, q.P, q.prog, q.gen, SEED0, chunk, search.ClimbConfig(**kw), **more)


def _device(engine, q, chunk, kw, burst=8, **more):
    return search.climb(engine, q.P, q.prog, q.gen, SEED0, chunk, search.ClimbConfig(device=True, burst=burst, **kw), **more)


_HOST = {}


def _host_run(engine, queries, name):
    """The host climb of a configuration on the GPU engine (once), with its sweeps."""
    if name not in _HOST:
        qn, chunk, kw, _ = CONFIGS[name]
        rec = Recorder(engine)
        _HOST[name] = (_host(rec, queries[qn], chunk, kw), rec.sweeps)
    return _HOST[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_device_climb_equals_host_climb_and_reference(engine, queries, name):
    qn, chunk, kw, (stop, rounds, best) = CONFIGS[name]
    q = queries[qn]
    want, _ = _host_run(engine, queries, name)
    before = engine.stats()
    got = _device(engine, q, chunk, kw)
    after = engine.stats()
    print(name, "stop", got.stop, "rounds", got.rounds, "best", got.best, "index", got.index, "population",
          [(v, i) for v, i, _ in got.population], "burst kernel ms", got.kernel_ms)
    assert_same(got, want, name)
    assert got.candidates == got.rounds * chunk
    assert after.launches - before.launches == got.rounds and after.candidates - before.candidates == got.candidates
    assert len(got.kernel_ms) == (got.rounds + 7) // 8 and all(ms > 0 for ms in got.kernel_ms)
    # what the CPU reference measured for this configuration
    assert want.stop == stop and (rounds is None or want.rounds == rounds) and (best is None or want.best == best)
    c = search.ClimbConfig(**kw)
    first, n_rounds, traj, ref_best = scored_ref.climb_ref(q.P, q.blob, SEED0, chunk, c.rounds, c.beam, c.patience)
    assert (got.index, got.rounds, got.best) == (first, n_rounds, ref_best)
    assert got.trajectory == traj
    if got.index is not None:
        scalars, arrays, funcs = search.model_from_assignment(q.P, got.assign)
        assert all(evaluate(t, OracleModel(scalars, arrays, funcs)) == 1 for t in q.roots)
        assert engine.search(q.prog, q.gen, SEED0, 0, got.candidates, early_exit=False) == (None, 0)


def _key(m):
    return tuple(sorted(m.items()))


def _edge_cases(P, sweeps, chunk, beam):
    """Rounds of a host run in which (a) a winner's assignment repeats another winner's or a previous
    member's and (b) the last place of the population is decided between a newcomer and a previous
    member with the same violations."""
    pop, dup_rounds, tie_rounds, dups = [], 0, 0, 0
    for r, (first, slots, assigns) in enumerate(sweeps):
        if first is not None:
            break
        winners = [(sl[1], sl[0], search.coords_from_assignment(P, assigns[s])) for s, sl in enumerate(slots) if sl is not None]
        keys = [_key(m) for _, _, m in winners]
        d = len(keys) - len(set(keys)) + len(set(keys) & {_key(m) for _, _, m in pop})
        dups += d
        dup_rounds += d > 0
        ranked = search.next_population(pop, winners, 64)
        if len(ranked) > beam and ranked[beam - 1][0] == ranked[beam][0]:
            # the cut falls inside a run of equal violations: a tie between a newcomer and a member
            # when the run holds both (the newcomers go first, so that rule decides who stays)
            new = {i >= r * chunk for v, i, _ in ranked if v == ranked[beam][0]}
            tie_rounds += new == {True, False}
        pop = ranked[:beam]
    return dup_rounds, tie_rounds, dups


def test_the_star_exercises_duplicates_and_ties(engine, queries):
    want, sweeps = _host_run(engine, queries, "star8")
    dup_rounds, tie_rounds, dups = _edge_cases(queries["star"].P, sweeps, 4096, 8)
    print("star8: rounds with a repeated assignment", dup_rounds, "repeats", dups, "rounds with a tie at the beam's edge",
          tie_rounds)
    assert (want.stop, want.rounds, want.index) == ("hit", 8, 28905)
    assert dup_rounds >= 1 and tie_rounds >= 1
    _, chain_sweeps = _host_run(engine, queries, "chain8")
    assert _edge_cases(queries["chain"].P, chain_sweeps, 4096, 8)[0] >= 1
    stops = {_host_run(engine, queries, n)[0].stop for n in CONFIGS}
    assert stops == {"hit", "rounds", "patience"}


def test_seed_count_changes_between_rounds(engine, queries):
    q = queries["star"]
    sizes = []
    for k in range(1, 7):
        want, got = _host(engine, q, 192, {"rounds": k}), _device(engine, q, 192, {"rounds": k})
        assert_same(got, want, k)
        sizes.append(len(got.population))
        assert sum(sl is not None for sl in got.trajectory[-1]) == 3  # most slots are empty
    assert sizes == [3, 6, 8, 8, 8, 8]


@pytest.mark.parametrize("burst", [1, 3, 16])
def test_burst_size_changes_nothing(engine, queries, burst):
    want, _ = _host_run(engine, queries, "star8")
    got = _device(engine, queries["star"], 4096, {}, burst=burst)
    assert_same(got, want, burst)
    assert len(got.kernel_ms) == (got.rounds + burst - 1) // burst


def test_site_and_narrow_coordinates(engine, queries):
    """Coordinates of 256, 40, 8 and 1 bits and an array site in the seed rows; the reference is the
    host climb on the same engine (the C port reads back node watches only)."""
    q = queries["site"]
    cmap = search.climb_map(q.P)
    seeded = {q.P.coords[c].width for c in range(len(q.P.coords)) if cmap.coord_row[c] != native.MG_NONE}
    assert {256, 40, 8, 1} <= seeded and any(cmap.coord_row[c.index] != native.MG_NONE for c in q.P.sites)
    for kw in ({}, {"beam": 5, "rounds": 12}):
        want = _host(engine, q, 4096, kw)
        got = _device(engine, q, 4096, kw)
        print("site query", kw, want.stop, want.rounds, want.best, want.index)
        assert want.rounds >= 4 and not (want.stop == "hit" and want.rounds == 1)
        assert_same(got, want, kw)


def test_round_zero_seed_set_with_its_own_layout(engine, queries):
    q = queries["star"]
    P = q.P
    m = (1 << 256) - 1
    some = [c.index for c in P.coords][::2]  # every other coordinate, and not the same ones per model
    models = [{ci: (A * (3 * k + ci + 1)) & m for ci in some[k:]} for k in range(3)]
    seeds = seeded_ref.seed_set(P, models, keep16=0x8000)
    assert seeds.n_rows < search.climb_map(P).n_rows and len({len(mo) for mo in models}) == 3
    plain, _ = _host_run(engine, queries, "star8")
    want = _host(engine, q, 4096, {}, seeds=seeds)
    got = _device(engine, q, 4096, {}, seeds=seeds)
    assert want.trajectory[0] != plain.trajectory[0]  # the set changed round 0
    assert_same(got, want, "round-0 seeds")


def _accepted(roots, model):
    ver, scalars, arrays, funcs = model[0:4]
    return ver == 1 and all(evaluate(r, OracleModel(scalars, arrays, funcs)) == 1 for r in roots)


def test_through_search(engine, queries):
    roots = queries["star"].roots
    kw = {"seed": SEED0, "chunk": 4096, "max_candidates": 1 << 16, "timeout_s": 60, "jit": "never"}
    a = search.search(engine, roots, climb=search.ClimbConfig(), **kw)
    b = search.search(engine, roots, climb=search.ClimbConfig(device=True), **kw)
    assert a.engine == b.engine == "climb" and b.climbed and a.index == b.index == 28905
    assert a.model[0:4] == b.model[0:4] and _accepted(roots, b.model)
    assert a.timing["climb_rounds"] == b.timing["climb_rounds"] == 8 and a.scanned == b.scanned


class _Set:
    def is_set(self):
        return True


def test_cancel_and_deadline(engine, queries):
    q = queries["star"]
    before = engine.stats().launches
    rc = _device(engine, q, 4096, {}, cancel=_Set())
    assert (rc.stop, rc.rounds, rc.candidates, rc.index, rc.population) == ("cancel", 0, 0, None, [])
    rb = _device(engine, q, 4096, {}, deadline=0.0)
    assert (rb.stop, rb.rounds, rb.trajectory) == ("budget", 0, [])
    assert engine.stats().launches == before
    # a word the caller owns, read before every burst
    word = np.zeros(1, dtype=np.uint32)
    cmap = search.climb_map(q.P)
    r0 = engine.search_climb(q.prog, q.gen, cmap, SEED0, 4096, cancel=word)
    assert (r0.stop, r0.rounds) == ("hit", 8)
    word[0] = 1
    r1 = engine.search_climb(q.prog, q.gen, cmap, SEED0, 4096, cancel=word)
    assert (r1.stop, r1.rounds) == ("cancel", 0)


def test_invalid_arguments_launch_nothing(engine, queries):
    q, other = queries["star"], queries["chain"]
    cmap = search.climb_map(q.P)
    ww = engine.info(q.prog).watch_words
    ok = {"rounds": 16, "beam": 8, "patience": 4, "burst": 8}
    past_ww = native.ClimbMap(cmap.coord_row, np.r_[cmap.watch_row[:-1], ww], cmap.keep16)
    past_rows = cmap.coord_row.copy()
    past_rows[int(np.argmax(cmap.coord_row))] = cmap.n_rows - 7  # eight limbs from there: one row past the end
    calls = [(name, q.prog, q.gen, cmap, 4096, dict(ok, **kw)) for name, kw in (
        ("rounds = 0", {"rounds": 0}), ("beam = 0", {"beam": 0}), ("beam = 33", {"beam": 33}),
        ("patience = 0", {"patience": 0}), ("burst = 0", {"burst": 0}))]
    calls += [
        ("chunk = 0", q.prog, q.gen, cmap, 0, ok),
        ("rounds * chunk above 2^48", q.prog, q.gen, cmap, (1 << 47) + 1, dict(ok, rounds=2)),
        ("watch_row past watch_words", q.prog, q.gen, past_ww, 4096, ok),
        ("coordinate rows past n_rows", q.prog, q.gen, native.ClimbMap(past_rows, cmap.watch_row, cmap.keep16), 4096, ok),
        ("no rows", q.prog, q.gen, native.ClimbMap(cmap.coord_row, [], cmap.keep16), 4096, ok),
        ("keep16", q.prog, q.gen, native.ClimbMap(cmap.coord_row, cmap.watch_row, 65537), 4096, ok),
        ("bad program", 0xDEAD0000, q.gen, cmap, 4096, ok),
        ("bad generator", q.prog, 0xDEAD0000, cmap, 4096, ok),
        ("generator of another program", q.prog, other.gen, cmap, 4096, ok),
        ("round-0 set with 33 seeds", q.prog, q.gen, cmap, 4096,
         dict(ok, seeds=native.SeedSet(np.zeros((8, 33), np.uint32), cmap.coord_row, cmap.coord_row))),
    ]
    before = engine.stats().launches
    for name, prog, gen, cm, chunk, kw in calls:
        with pytest.raises(native.EngineError) as ei:
            engine.search_climb(prog, gen, cm, SEED0, chunk, **kw)
        assert ei.value.code == native.MG_E_INVALID, name
    # a program without watch rows
    bare = ssa.flatten(q.roots)
    prog = engine.load(bare.to_bytes())
    gen = engine.load_gen(prog, q.blob)
    try:
        assert engine.info(prog).watch_words == 0
        with pytest.raises(native.EngineUnsupported):
            engine.search_climb(prog, gen, cmap, SEED0, 4096)
    finally:
        engine.free_gen(gen)
        engine.free(prog)
    assert engine.stats().launches == before
    assert_same(_device(engine, q, 4096, {}), _host_run(engine, queries, "star8")[0], "after the refused calls")


def test_a_scored_sweep_after_a_climb(engine, queries):
    q = queries["star"]
    start, count = 37, 64 * 70 + 11
    want = scored_ref.Scored(q.P, q.blob, None, SEED0, start, count)
    for kw in ({}, {"rounds": 3}):  # a climb that ended on a hit inside a burst, and one that ran out of rounds
        _device(engine, q, 4096, kw)
        first, hits, slots, _ = engine.search_scored(q.prog, q.gen, None, SEED0, start, count)
        assert slots == want.slots and (first, hits) == (want.first, want.hits), kw
    # ... and an ordinary search: the hit buffer is armed again
    _device(engine, q, 4096, {})
    assert engine.search(q.prog, q.gen, SEED0, 0, 1 << 14, early_exit=False) == (None, 0)
