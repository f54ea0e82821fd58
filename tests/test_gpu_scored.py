"""Scored sweeps (``mg_search_scored``, kernel ``k_run_scored``) against the reference of
``tests/scored_ref.py`` (the C port's per-root values under the seeded candidates, numpy for the
violation counts and slot minima), and the climbing search built on them (``search.climb``,
``search.search(climb=...)``) end to end.

The parity programs are those of ``tests/test_gpu_seeded.py`` (three interpreter tiers, both
value-file policies) plus the 8-root star query of ``workloads.climb_star``."""
import ctypes as C
import random

import numpy as np
import pytest

from mythril_amd import native, search, ssa, workloads
from mythril_amd.smt import terms as T
from oracle import cport
from oracle.bv import OracleModel, evaluate
from tests import scored_ref, seeded_ref
from tests.test_gpu_search_batch import _needles
from tests.test_gpu_seeded import A, CASES, SEED0, SENTINEL, _parity_roots

pytestmark = pytest.mark.gpu

START, COUNT = 37, 64 * 70 + 11  # unaligned, a partial first and last group, two groups or more per slot
BIG_START = (1 << 62) | random.Random(0x5C02ED).getrandbits(62)  # a fixed draw; bit 62 set: all 63 bits
BIG_COUNT = 64 * 34 + 11  # every slot, the first two twice
PROGRAMS = CASES + ("star",)
SLOTS = native.MG_SCORED_SLOTS


class Prog:
    """One parity program: loaded, with its generator, the three-model seed set of
    ``test_gpu_seeded`` at keep16 = 0x8000, and the reference sweeps of its windows (computed once,
    on first use, and shared)."""

    def __init__(self, engine, name):
        self.name = name
        if name == "star":
            self.roots = workloads.climb_star(8)
            self.P, self.blob = search.prepare(self.roots, None)
            P = self.P
            self.watched = [c.index for c in P.coords]
            m = (1 << 256) - 1
            models = [{c.index: (A * (3 * k + c.index + 1)) & m for c in P.coords} for k in range(3)]
            self.seeds = seeded_ref.seed_set(P, models, keep16=0x8000)
        else:
            self.roots = _parity_roots(name)
            self.P = P = ssa.flatten(self.roots)
            ci = {c.name: c.index for c in P.coords}
            site = P.sites[0].index
            P.set_watch([c.node for c in P.scalar_coords()] + [0x80000000 | site])
            self.watched = [x.index for x in P.scalar_coords()] + [site]
            g = search.GenBuilder(P)
            g.mixed(ci["sp_b"], [1, 2, 3], p_dict=0.2, copy_from=ci["sp_a"], p_copy=0.5, p_delta=0.25, small_bits=8,
                    p_small=0.1)
            self.blob = g.blob()
            m = (1 << 256) - 1
            models = []
            for k in range(3):
                mod = {ci["sp_a"]: (A * (k + 3)) & m, ci["sp_b"]: (A * (k + 3) + 5 - 4 * k) & m,
                       ci["sp_d"]: 0x70 + 0x10 * k, ci["sp_f"]: k & 1, site: (A >> (8 * k)) & m, ci["sp_e"]: 7}
                if k != 1:
                    mod[ci["sp_c"]] = 0x12345678AB | ((1 << 45) if k == 2 else 0)
                models.append(mod)
            self.seeds = seeded_ref.seed_set(P, models, keep16=0x8000, never={ci["sp_e"]})
        self.pb = self.P.to_bytes()
        self.prog = self.gen = None
        if engine is not None:
            self.prog = engine.load(self.pb)
            self.gen = engine.load_gen(self.prog, self.blob)
            self.info = engine.info(self.prog)
        self._ref = {}

    def ref(self, seeded, start=START, count=COUNT, seed=SEED0):
        key = (seeded, start, count, seed)
        if key not in self._ref:
            self._ref[key] = scored_ref.Scored(self.P, self.blob, self.seeds if seeded else None, seed, start, count)
        return self._ref[key]


@pytest.fixture(scope="module")
def progs(engine):
    out = {}

    def get(name):
        if name not in out:
            out[name] = Prog(engine, name)
        return out[name]

    yield get
    for p in out.values():
        engine.free_gen(p.gen)
        engine.free(p.prog)


def _sweep(engine, p, seeded, start=START, count=COUNT, early=False, assigns=None, want_assigns=True):
    return engine.search_scored(p.prog, p.gen, p.seeds if seeded else None, SEED0, start, count, early_exit=early,
                                assigns=assigns, want_assigns=want_assigns)


def _assert_equal(got, want, what):
    first, hits, slots, _ = got
    print(what, "first", first, want.first, "hits", hits, want.hits, "violations", sorted(set(want.viol.tolist())))
    assert slots == want.slots, what
    assert (first, hits) == (want.first, want.hits), what


def test_programs_cover_tiers_and_value_files(engine, progs):
    ops = {c: {int(i[0]) for i in native.specialized_program(progs(c).pb, None, interp=True)["code"]} for c in CASES}
    K_MUL, K_UDIV = 4, 5
    assert K_MUL not in ops["light"] and K_UDIV not in ops["light"]
    assert K_MUL in ops["mid"] and K_UDIV not in ops["mid"]
    assert K_UDIV in ops["heavy"]
    assert progs("global").info.value_words > 255 and not progs("global").info.uses_lds
    assert progs("light").info.value_words <= 160 and progs("star").info.value_words <= 160


def _teeth(want):
    """What makes a window a test of the slot rule: three violation counts or more, a slot whose
    winner is not its first candidate, and a slot whose minimum is shared (the lowest index decides)."""
    first_of, tie = {}, False
    late = False
    for q in range(want.count):
        first_of.setdefault(int(want.slot_of[q]), want.start + q)
    for s, sl in enumerate(want.slots):
        if sl is None:
            continue
        late = late or sl[0] != first_of[s]
        tie = tie or int(((want.slot_of == s) & (want.viol == sl[1])).sum()) > 1
    return len(set(want.viol.tolist())) >= 3, late, tie


@pytest.mark.parametrize("name", PROGRAMS)
@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "plain"])
def test_slot_parity(engine, progs, name, seeded):
    p = progs(name)
    want = p.ref(seeded)
    assert _teeth(want) == (True, True, True), (name, seeded)
    assert sum(sl is not None for sl in want.slots) == SLOTS
    _assert_equal(_sweep(engine, p, seeded, want_assigns=False), want, f"{name} seeded={seeded}")


@pytest.mark.parametrize("name", PROGRAMS)
def test_slot_parity_at_a_63_bit_start(engine, progs, name):
    p = progs(name)
    assert BIG_START >> 62 == 1
    want = p.ref(True, BIG_START, BIG_COUNT)
    _assert_equal(_sweep(engine, p, True, BIG_START, BIG_COUNT, want_assigns=False), want, f"{name} at {BIG_START:#x}")


@pytest.mark.parametrize("name", PROGRAMS)
def test_assign_rows_are_the_winners_models(engine, progs, name):
    p = progs(name)
    want = p.ref(True)
    ww = p.info.watch_words
    assigns = np.full((SLOTS, ww), SENTINEL, dtype=np.uint32)
    got = _sweep(engine, p, True, assigns=assigns)
    assert got[2] == want.slots and got[3] is assigns
    offs = p.P.coord_row_offsets()
    for s, (index, _) in enumerate(want.slots):
        _, watch = engine.eval_seeded(p.prog, p.gen, p.seeds, SEED0, index, 1, watch_words=ww)
        assert np.array_equal(assigns[s], watch[:ww, 0]), (name, s)
        col, r = want.column(index), 0
        for ci in p.watched:  # watch-list order, against the composed SoA limb for limb
            L = ssa.limbs(p.P.coords[ci].width)
            assert np.array_equal(assigns[s, r:r + L], col[offs[ci]:offs[ci] + L]), (name, s, p.P.coords[ci].name)
            r += L
        assert r == ww


@pytest.mark.parametrize("name", ["light", "global"])
def test_empty_slots(engine, progs, name):
    p = progs(name)
    ww = p.info.watch_words
    want = p.ref(True, 0, 64 * 5)
    assigns = np.full((SLOTS, ww), SENTINEL, dtype=np.uint32)
    first, hits, slots, _ = _sweep(engine, p, True, 0, 64 * 5, assigns=assigns)
    assert slots == want.slots and (first, hits) == (want.first, want.hits)
    assert [s for s in range(SLOTS) if slots[s] is None] == list(range(5, SLOTS))
    assert (assigns[5:] == SENTINEL).all() and not (assigns[:5] == SENTINEL).all(axis=1).any()
    # count = 0: nothing in any slot, nothing written
    assigns[:] = SENTINEL
    assert _sweep(engine, p, True, 123, 0, assigns=assigns)[:3] == (None, 0, [None] * SLOTS)
    assert (assigns == SENTINEL).all()


def test_duplicate_and_trivial_roots_count_once(engine):
    a, b = T.BitVecVar("sd_a", 256), T.BitVecVar("sd_b", 8)
    r0 = T.eq(T.extract(2, 0, a), T.BitVecVal(5, 3))
    r1 = T.bvcmp("bvult", b, T.BitVecVal(64, 8))
    P = ssa.flatten([r0, r0, T.BoolVal(True), r1])
    P.set_watch(search.model_watch(P)[0])
    blob = search.GenBuilder(P).blob()
    prog = engine.load(P.to_bytes())
    gen = engine.load_gen(prog, blob)
    try:
        want = scored_ref.Scored(P, blob, None, SEED0, START, 64 * 40)
        assert sorted(set(want.viol.tolist())) == [0, 1, 2]  # two roots, however often they are listed
        got = engine.search_scored(prog, gen, None, SEED0, START, 64 * 40)
        _assert_equal(got, want, "duplicate roots")
        assert max(sl[1] for sl in got[2]) <= 2
    finally:
        engine.free_gen(gen)
        engine.free(prog)


def test_early_exit(engine, progs):
    for name in CASES:  # windows with hits: the first hit is exact
        p = progs(name)
        want = p.ref(True)
        assert want.hits > 0
        assert _sweep(engine, p, True, early=True, want_assigns=False)[0] == want.first, name
    star = progs("star")
    want = star.ref(False)
    assert want.hits == 0
    _assert_equal(_sweep(engine, star, False, early=True, want_assigns=False), want, "star, early exit")


def test_invalid_arguments_launch_nothing(engine, progs):
    c, other = progs("light"), progs("mid")
    s = c.seeds
    ci = {x.name: x.index for x in c.P.coords}
    past = s.coord_row.copy()
    past[ci["sp_a"]] = s.n_rows - 7  # eight limbs from there run one row past the end
    bad_sets = {
        "n_seeds > 32": native.SeedSet(np.zeros((s.n_rows, 33), np.uint32), s.coord_row, s.coord_has),
        "rows past n_rows": native.SeedSet(s.rows, past, s.coord_has),
        "null rows": native.SeedSet(None, s.coord_row, s.coord_has, n_seeds=3, n_rows=s.n_rows),
        "null coord_row": native.SeedSet(s.rows, None, s.coord_has),
        "null coord_has": native.SeedSet(s.rows, s.coord_row, None),
        "keep16": native.SeedSet(s.rows, s.coord_row, s.coord_has, keep16=65537),
        "keep16, no seeds": native.SeedSet(keep16=65537),
    }
    calls = [(name, c.prog, c.gen, bad, COUNT) for name, bad in bad_sets.items()]
    calls += [("bad program", 0xDEAD0000, c.gen, s, COUNT), ("bad generator", c.prog, 0xDEAD0000, s, COUNT),
              ("generator of another program", c.prog, other.gen, s, COUNT),
              ("count above 2^48", c.prog, c.gen, s, (1 << 48) + 1), ("count above 2^48, no seeds", c.prog, c.gen, None, 1 << 63)]
    before = engine.stats().launches
    for name, prog, gen, seeds, count in calls:
        with pytest.raises(native.EngineError) as ei:
            engine.search_scored(prog, gen, seeds, SEED0, START, count)
        assert ei.value.code == native.MG_E_INVALID, name
    sc = s.as_c()
    rows = np.full((SLOTS, c.info.watch_words), SENTINEL, dtype=np.uint32)
    rc = engine.lib.mg_search_scored(c.prog, c.gen, C.byref(sc), SEED0, START, COUNT, 0, None,
                                     rows.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == native.MG_E_INVALID and (rows == SENTINEL).all()  # a null res
    assert engine.stats().launches == before
    got = _sweep(engine, c, True, want_assigns=False)
    assert got[2] == c.ref(True).slots
    s1 = engine.stats()
    assert s1.launches == before + 1 and s1.last_candidates == COUNT


def _accepted(roots, model):
    ver, scalars, arrays, funcs = model[0:4]
    om = OracleModel(scalars, arrays, funcs)
    return ver == 1 and all(evaluate(r, om) == 1 for r in roots)


def test_climb_solves_the_star_on_the_reference_trajectory(engine, progs):
    p = progs("star")
    chunk = 4096
    res = search.climb(engine, p.P, p.prog, p.gen, SEED0, chunk, search.ClimbConfig())
    print("rounds", res.rounds, "index", res.index, "kernel ms per round", res.kernel_ms)
    assert res.stop == "hit" and res.rounds <= 16
    scalars, arrays, funcs = search.model_from_assignment(p.P, res.assign)
    assert all(evaluate(t, OracleModel(scalars, arrays, funcs)) == 1 for t in p.roots)
    first, rounds, traj, _ = scored_ref.climb_ref(p.P, p.blob, SEED0, chunk)
    assert (res.index, res.rounds) == (first, rounds)
    assert res.trajectory == traj  # every round's 32 (index, violations), exactly
    assert engine.search(p.prog, p.gen, SEED0, 0, res.candidates, early_exit=False) == (None, 0)
    # through search(): the first ordinary launch misses, the climb answers
    r = search.search(engine, p.roots, seed=SEED0, chunk=chunk, max_candidates=1 << 16, timeout_s=60, jit="never",
                      climb=search.ClimbConfig())
    assert r.engine == "climb" and r.climbed and r.index == first and r.scanned == chunk
    assert _accepted(p.roots, r.model) and r.timing["climb_rounds"] == rounds


def test_a_climb_miss_keeps_the_first_hit(engine):
    """One 2^-16 needle: a violation count of 0 or 1 gives the climb nothing to follow."""
    roots = _needles()[:1]
    kw = {"max_candidates": 1 << 24, "timeout_s": 60, "jit": "never"}
    a = search.search(engine, roots, climb=None, **kw)
    b = search.search(engine, roots, climb=search.ClimbConfig(rounds=2), **kw)
    print("needle", a.index, b.index, b.timing)
    assert a.index == b.index == 205095 and a.scanned == b.scanned
    assert not b.climbed and b.engine == "interp" and b.timing["climb_rounds"] == 2
    assert a.model[0:4] == b.model[0:4] and "climb_ms" not in a.timing
