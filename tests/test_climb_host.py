"""The climbing search's host loop (``search.climb``, ``search.next_population``,
``search.search(climb=...)``) without a GPU: the engine is a stand-in whose ``search_scored`` is the
reference sweep of ``tests/scored_ref.py`` and whose ``search`` is the C port.

The star query (``workloads.climb_star``): 8 roots of probability 2^-6 that share one variable, so
plain sampling needs about 2^48 candidates; the climb needs a few rounds of 4,096."""
import numpy as np
import pytest

from mythril_amd import search, workloads
from oracle import cport
from oracle.bv import OracleModel, evaluate
from tests import scored_ref

SEEDS = (0x6D797468, 12345, 987654321, 555)
CHUNK = 4096


class StandIn(scored_ref.RefEngine):
    """Enough of ``native.Engine`` for ``search.search(jit="never")``: the ordinary stream is the
    C port's search of the same program and generator."""

    def __init__(self, P, blob):
        super().__init__(P, blob)
        self.searches = []

    def load(self, pb):
        assert pb == self.P.to_bytes()
        return 1

    def load_gen(self, prog, blob):
        assert np.array_equal(blob, self.blob)
        return 2

    def free(self, prog):
        pass

    def free_gen(self, gh):
        pass

    def search(self, prog, gh, seed, start, n, early_exit=True, assign=None):
        self.searches.append((start, n))
        return cport.search(self.P.to_bytes(), self.blob, seed, start, n, threads=4)[:2]


@pytest.fixture(scope="module")
def star():
    roots = workloads.climb_star(8)
    P, blob = search.prepare(roots, None)
    return roots, P, blob


@pytest.fixture(scope="module")
def runs(star):
    """One ``search.climb`` per seed on the reference engine, shared by the tests below."""
    _, P, blob = star
    out = {}
    for seed in SEEDS:
        eng = scored_ref.RefEngine(P, blob)
        out[seed] = (search.climb(eng, P, 1, 2, seed, CHUNK, search.ClimbConfig()), eng)
    return out


def _m(**kw):
    return dict(kw)


def test_population_rule_orders_by_violations_then_round_then_index():
    prev = [(2, 10, _m(a=1)), (3, 11, _m(a=2))]
    win = [(3, 500, _m(a=3)), (2, 400, _m(a=4)), (1, 450, _m(a=5)), (2, 300, _m(a=6))]
    got = search.next_population(prev, win, beam=8)
    # violations first; at 2 this round's winners (by index) come before the previous entry although
    # its index is lower (the sideways preference); at 3 the same
    assert [(v, i) for v, i, _ in got] == [(1, 450), (2, 300), (2, 400), (2, 10), (3, 500), (3, 11)]


def test_population_rule_beam_and_sideways_replacement():
    prev = [(2, 10, _m(a=1)), (2, 11, _m(a=2))]
    win = [(2, 400, _m(a=4)), (2, 300, _m(a=6)), (5, 200, _m(a=7))]
    got = search.next_population(prev, win, beam=2)
    assert [(v, i) for v, i, _ in got] == [(2, 300), (2, 400)]  # equal violations: the newcomers stay
    got = search.next_population(prev, win[2:], beam=2)
    assert [(v, i) for v, i, _ in got] == [(2, 10), (2, 11)]  # a worse newcomer replaces nobody


def test_population_rule_keeps_distinct_assignments():
    same = _m(a=1, b=2)
    prev = [(2, 10, dict(same))]
    win = [(2, 400, dict(same)), (2, 300, _m(a=1, b=3)), (2, 350, dict(same))]
    got = search.next_population(prev, win, beam=8)
    # one copy of the repeated assignment: the best-ranked one (this round, lowest index)
    assert [(v, i) for v, i, _ in got] == [(2, 300), (2, 350)]
    assert search.next_population([], [], beam=8) == []


def test_config_is_checked():
    c = search.ClimbConfig()
    assert (c.rounds, c.beam, c.patience) == (16, 8, 4)
    for bad in ({"rounds": 0}, {"beam": 0}, {"beam": 33}, {"patience": 0}):
        with pytest.raises(ValueError):
            search.ClimbConfig(**bad)


@pytest.mark.parametrize("seed", SEEDS)
def test_star_is_solved_within_16_rounds(star, runs, seed):
    roots, P, blob = star
    res, eng = runs[seed]
    print(hex(seed), "rounds", res.rounds, "candidates", res.candidates, "index", res.index)
    assert res.stop == "hit" and res.index is not None and res.rounds <= 16 and res.best == 0
    assert res.candidates == res.rounds * CHUNK
    assert (res.rounds - 1) * CHUNK <= res.index < res.rounds * CHUNK
    # round r sweeps [r chunk, (r + 1) chunk); round 0 unseeded, later rounds from at most `beam` seeds
    for r, (seeds, s, start, count) in enumerate(eng.calls):
        assert (s, start, count) == (seed, r * CHUNK, CHUNK)
        assert (seeds is None) == (r == 0)
        if r:
            assert 1 <= seeds.n_seeds <= 8 and seeds.keep16 == search.warm_keep16(len(P.coords))
    scalars, arrays, funcs = search.model_from_assignment(P, res.assign)
    assert all(evaluate(t, OracleModel(scalars, arrays, funcs)) == 1 for t in roots)
    # plain sampling over the same number of candidates finds nothing
    assert cport.search(P.to_bytes(), blob, seed, 0, res.candidates, threads=4)[:2] == (None, 0)


def test_the_climb_starts_far_from_a_hit(runs):
    for res, _ in runs.values():
        best = [min(sl[1] for sl in slots if sl is not None) for slots in res.trajectory]
        assert best[0] >= 5 and best[-1] == 0  # no hit near the start: the climb does the work


def test_climb_is_deterministic_and_follows_the_restated_loop(star, runs):
    _, P, blob = star
    seed = SEEDS[0]
    res, _ = runs[seed]
    again = search.climb(scored_ref.RefEngine(P, blob), P, 1, 2, seed, CHUNK, search.ClimbConfig())
    assert again.trajectory == res.trajectory and again.index == res.index and again.rounds == res.rounds
    first, rounds, traj, best = scored_ref.climb_ref(P, blob, seed, CHUNK)
    assert (first, rounds, best) == (res.index, res.rounds, 0)
    assert traj == res.trajectory


def test_limits_stop_the_climb(star):
    _, P, blob = star
    seed = SEEDS[1]
    r2 = search.climb(scored_ref.RefEngine(P, blob), P, 1, 2, seed, 256, search.ClimbConfig(rounds=2))
    assert (r2.index, r2.rounds, r2.stop, r2.candidates) == (None, 2, "rounds", 512)
    assert len(r2.population) <= 8 and r2.best == r2.population[0][0] > 0

    class Set:
        def is_set(self):
            return True

    rc = search.climb(scored_ref.RefEngine(P, blob), P, 1, 2, seed, 256, search.ClimbConfig(), cancel=Set())
    assert (rc.rounds, rc.stop) == (0, "cancel")
    rb = search.climb(scored_ref.RefEngine(P, blob), P, 1, 2, seed, 256, search.ClimbConfig(), deadline=0.0)
    assert (rb.rounds, rb.stop) == (0, "budget")
    # beam 1, one slot per round (64 candidates): no lower best for `patience` rounds in a row
    rp = search.climb(scored_ref.RefEngine(P, blob), P, 1, 2, seed, 64, search.ClimbConfig(rounds=16, beam=1, patience=1))
    assert rp.stop in ("patience", "rounds") and rp.index is None
    if rp.stop == "patience":
        assert rp.rounds < 16


def test_search_runs_the_climb_after_the_first_miss(star):
    roots, P, blob = star
    seed = SEEDS[0]
    eng = StandIn(P, blob)
    res = search.search(eng, roots, seed=seed, chunk=CHUNK, max_candidates=1 << 14, timeout_s=600, jit="never",
                        climb=search.ClimbConfig())
    assert eng.searches == [(0, CHUNK)]  # the first ordinary launch, then the climb
    assert res.engine == "climb" and res.climbed and res.scanned == CHUNK
    assert res.timing["climb_rounds"] == len(eng.calls) and res.timing["climb_best"] == 0
    ver, scalars, arrays, funcs = res.model[0:4]
    assert ver == 1 and all(evaluate(t, OracleModel(scalars, arrays, funcs)) == 1 for t in roots)
    # without it: the same stream, no scored sweep, no model within the budget
    off = StandIn(P, blob)
    r0 = search.search(off, roots, seed=seed, chunk=CHUNK, max_candidates=1 << 14, timeout_s=600, jit="never")
    assert r0.index is None and not r0.climbed and off.calls == [] and "climb_ms" not in r0.timing


def test_a_climb_miss_leaves_the_ordinary_stream_as_it_was(star):
    roots, P, blob = star
    a, b = StandIn(P, blob), StandIn(P, blob)
    kw = {"seed": SEEDS[2], "chunk": 256, "max_candidates": 1 << 13, "timeout_s": 600, "jit": "never"}
    ra = search.search(a, roots, **kw)
    rb = search.search(b, roots, climb=search.ClimbConfig(rounds=2), **kw)
    assert len(b.calls) == 2 and rb.timing["climb_candidates"] == 512 and not rb.climbed
    assert a.searches == b.searches and (ra.index, ra.scanned) == (rb.index, rb.scanned) == (None, 1 << 13)


def test_climb_switch_is_off_by_default(monkeypatch):
    from mythril_amd import plugin

    calls = []

    def fake_partitioned(engine, terms, **kw):
        calls.append(kw)
        return search.SearchResult(None, 0, 0, 0.0)

    monkeypatch.setattr(search, "search_partitioned", fake_partitioned)
    monkeypatch.setattr("mythril_amd.native.Engine.get", classmethod(lambda cls: object()))
    monkeypatch.delenv("MYTHGPU_WARM", raising=False)
    monkeypatch.delenv("MYTHGPU_CLIMB", raising=False)
    plugin._gpu_search([], 0.01, None)
    assert "climb" not in calls[-1]
    monkeypatch.setenv("MYTHGPU_CLIMB", "1")
    before = plugin.STATS.climb_hits
    plugin._gpu_search([], 0.01, None)
    cfg = calls[-1]["climb"]
    assert isinstance(cfg, search.ClimbConfig) and (cfg.rounds, cfg.beam, cfg.patience) == (16, 8, 4)
    assert {k: v for k, v in calls[-1].items() if k != "climb"} == calls[0]
    assert plugin.STATS.climb_hits == before  # nothing was answered
