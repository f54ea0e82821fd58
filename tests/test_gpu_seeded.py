"""Seeded sweeps (``mg_search_seeded`` / ``mg_eval_seeded``, kernel ``k_run_seeded``) against the C
port composed with the documented seed rule (``tests/seeded_ref.py``), and the host path that
feeds them (``search.search(warm=ModelCache)``).

Reference anchor: LASER asks for a state's constraints plus one JUMPI condition
(``mythril/laser/ethereum/svm.py:252-257``, ``instructions.py:1543-1616``); the parent's model
satisfies one of the two successor queries as it is.
"""
import numpy as np
import pytest

from mythril_amd import native, partition, search, ssa, workloads
from mythril_amd.smt import Extract, Not, UGT, ULT, symbol_factory
from mythril_amd.smt import terms as T
from oracle import cport
from oracle.bv import OracleModel, evaluate
from tests import seeded_ref

pytestmark = pytest.mark.gpu
BVV = symbol_factory.BitVecVal
BVS = symbol_factory.BitVecSym

SEED0 = 0x6D797468
SENTINEL = 0xA5A5A5A5
A = 0x1F3A9C5B27D4EB4F00C0FFEE5EED12349E3779B97F4A7C15F39CC0605CEDC835
START, COUNT = 37, 64 * 7 + 11  # unaligned, replay groups, later rounds, a partial last group
CASES = ("light", "mid", "heavy", "global")


def _ult(a, b):
    return T.bvcmp("bvult", a, b)


def _parity_roots(case):
    """Coordinates of 256, 40, 8 and 1 bits, an array site and (by the generator below) a MIXED
    coordinate copying a seeded one; ORs, so verdicts carry information.  ``mid`` adds a MUL,
    ``heavy`` a UDIV, ``global`` forty 256-bit products that are all live at once (a value file
    of more than 255 words per lane)."""
    a, b, e = (T.BitVecVar(f"sp_{n}", 256) for n in "abe")
    c, d, f = T.BitVecVar("sp_c", 40), T.BitVecVar("sp_d", 8), T.BoolVar("sp_f")
    site = T.select(T.ArrayVar("sp_store", 256, 256), a)
    roots = [T.or_(_ult(a, b), T.eq(c, T.BitVecVal(0x12345678AB, 40)), f),
             T.or_(_ult(d, T.BitVecVal(0x80, 8)), T.eq(site, e), _ult(e, a))]
    if case in ("mid", "global"):
        roots.append(T.or_(_ult(T.bvbin("bvmul", a, e), b), f))
    if case == "heavy":
        q = T.bvbin("bvudiv", b, T.bvbin("bvor", T.zero_extend(248, d), T.BitVecVal(1, 256)))
        roots.append(T.or_(T.eq(T.extract(0, 0, q), T.BitVecVal(1, 1)), f))
    if case == "global":
        acc = None
        prods = [T.bvbin("bvmul", a, T.BitVecVal(0x9E3779B97F4A7C15 + 2 * i, 256)) for i in range(40)]
        for p in reversed(prods):
            acc = p if acc is None else T.bvbin("bvxor", p, acc)
        roots.append(T.or_(_ult(acc, b), T.not_(f)))
    return roots


class Case:
    def __init__(self, engine, case):
        self.P = ssa.flatten(_parity_roots(case))
        P = self.P
        ci = {c.name: c.index for c in P.coords}
        self.ci = ci
        site = P.sites[0].index
        P.set_watch([c.node for c in P.scalar_coords()] + [0x80000000 | site])
        g = search.GenBuilder(P)
        assert ci["sp_a"] < ci["sp_b"]
        g.mixed(ci["sp_b"], [1, 2, 3], p_dict=0.2, copy_from=ci["sp_a"], p_copy=0.5, p_delta=0.25, small_bits=8,
                p_small=0.1)
        self.blob = g.blob()
        self.pb = P.to_bytes()
        self.prog = engine.load(self.pb)
        self.gen = engine.load_gen(self.prog, self.blob)
        self.info = engine.info(self.prog)
        m = (1 << 256) - 1
        models = []
        for k in range(3):
            mod = {ci["sp_a"]: (A * (k + 3)) & m, ci["sp_b"]: (A * (k + 3) + 5 - 4 * k) & m,
                   ci["sp_d"]: 0x70 + 0x10 * k, ci["sp_f"]: k & 1, site: (A >> (8 * k)) & m,
                   ci["sp_e"]: 7}
            if k != 1:  # missing from seed 1 only; seed 2's value is wider than the coordinate
                mod[ci["sp_c"]] = 0x12345678AB | ((1 << 45) if k == 2 else 0)
            models.append(mod)
        # sp_e is in every model but never seeded (coord_row = MG_NONE)
        self.seeds = seeded_ref.seed_set(P, models, keep16=0x8000, never={ci["sp_e"]})
        self.want_ver, self.want_soa = seeded_ref.seeded_verdicts(P, self.blob, self.seeds, SEED0, START, COUNT)


@pytest.fixture(scope="module")
def cases(engine):
    out = {c: Case(engine, c) for c in CASES}
    yield out
    for c in out.values():
        engine.free_gen(c.gen)
        engine.free(c.prog)


def test_cases_cover_tiers_and_value_files(engine, cases):
    """What the parity cases rely on: the three interpreter tiers, both value-file policies, a seed
    set with a never-seeded coordinate and one missing from seed 1 only, and windows whose
    reference verdicts hold both values."""
    ops = {c: {int(i[0]) for i in native.specialized_program(cases[c].pb, None, interp=True)["code"]} for c in CASES}
    K_MUL, K_UDIV = 4, 5
    assert K_MUL not in ops["light"] and K_UDIV not in ops["light"]
    assert K_MUL in ops["mid"] and K_UDIV not in ops["mid"]
    assert K_UDIV in ops["heavy"]
    assert cases["global"].info.value_words > 255 and not cases["global"].info.uses_lds
    assert cases["light"].info.value_words <= 160
    c = cases["light"]
    assert int(c.seeds.coord_row[c.ci["sp_e"]]) == native.MG_NONE
    assert int(c.seeds.coord_has[c.ci["sp_c"]]) == 0b101 and int(c.seeds.coord_has[c.ci["sp_a"]]) == 0b111
    for k in CASES:
        assert 0 < int(cases[k].want_ver.sum()) < COUNT, k


@pytest.mark.parametrize("case", CASES)
def test_per_candidate_parity(engine, cases, case):
    c = cases[case]
    ver, watch = engine.eval_seeded(c.prog, c.gen, c.seeds, SEED0, START, COUNT, watch_words=c.info.watch_words)
    print(case, "verdict ones", int(ver.sum()), "reference", int(c.want_ver.sum()))
    assert np.array_equal(ver, c.want_ver)
    offs = c.P.coord_row_offsets()
    r = 0
    watched = [x.index for x in c.P.scalar_coords()] + [c.P.sites[0].index]
    for ci in watched:  # watch rows, in watch-list order, against the composed SoA limb for limb
        L = ssa.limbs(c.P.coords[ci].width)
        assert np.array_equal(watch[r:r + L], c.want_soa[offs[ci]:offs[ci] + L]), (case, c.P.coords[ci].name)
        r += L
    assert r == c.info.watch_words
    # the seeds matter: the window differs from the unseeded candidates
    plain = cport.gen_soa(c.pb, c.blob, SEED0, START, COUNT, c.P.coord_words)
    assert not np.array_equal(plain, c.want_soa)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("early", [False, True])
def test_search_over_the_parity_windows(engine, cases, case, early):
    """First hit exact in both modes; the hit count of the full sweep."""
    c = cases[case]
    hits = np.flatnonzero(c.want_ver)
    got = engine.search_seeded(c.prog, c.gen, c.seeds, SEED0, START, COUNT, early_exit=early)
    assert got[0] == START + int(hits[0])
    if not early:
        assert got[1] == hits.size


def _xy(engine, extra=None):
    x, y = BVS("sr_x", 256), BVS("sr_y", 256)
    roots = [(x == BVV(A, 256)).raw, (y == x + BVV(1, 256)).raw] if extra is None else extra(x)
    P = ssa.flatten(roots)
    P.set_watch(search.model_watch(P)[0])
    blob = search.GenBuilder(P).blob()  # UNIFORM everywhere
    prog = engine.load(P.to_bytes())
    return roots, P, blob, prog, engine.load_gen(prog, blob)


def test_replay_lane_finds_the_cached_model(engine):
    roots, P, blob, prog, gen = _xy(engine)
    try:
        ci = {c.name: c.index for c in P.coords}
        models = [{ci["sr_x"]: 1, ci["sr_y"]: 1}, {ci["sr_x"]: A, ci["sr_y"]: A + 1}]
        seeds = seeded_ref.seed_set(P, models, keep16=0x8000)
        ww = engine.info(prog).watch_words
        for early in (True, False):
            assign = np.full(ww, SENTINEL, dtype=np.uint32)
            first, n = engine.search_seeded(prog, gen, seeds, SEED0, 0, 128, early_exit=early, assign=assign)
            assert first == 64 and n >= 1
            scalars, arrays, funcs = search.model_from_assignment(P, assign)
            assert scalars == {"sr_x": A, "sr_y": A + 1}
            assert all(evaluate(r, OracleModel(scalars, arrays, funcs)) == 1 for r in roots)
        assert (first, n) == seeded_ref.seeded_search(P, blob, seeds, SEED0, 0, 128)
        assert engine.search(prog, gen, SEED0, 0, 128, early_exit=False) == (None, 0)
        # a miss: only the wrong model, kept whole on every lane
        wrong = seeded_ref.seed_set(P, models[:1], keep16=65536)
        assign = np.full(ww, SENTINEL, dtype=np.uint32)
        assert engine.search_seeded(prog, gen, wrong, SEED0, 0, 128, assign=assign) == (None, 0)
        assert (assign == SENTINEL).all()
        assert engine.search_seeded(prog, gen, seeds, SEED0, 0, 0) == (None, 0)  # count = 0
    finally:
        engine.free_gen(gen)
        engine.free(prog)


def test_neighbourhood_of_a_seed(engine):
    """x == A from the seed on every lane, z < 16 from the generator (z is not in the seed)."""
    def extra(x):
        return [(x == BVV(A, 256)).raw, ULT(BVS("sr_z", 8), BVV(16, 8)).raw]

    roots, P, blob, prog, gen = _xy(engine, extra)
    try:
        ci = {c.name: c.index for c in P.coords}
        seeds = seeded_ref.seed_set(P, [{ci["sr_x"]: A}], keep16=65536)
        want = seeded_ref.seeded_search(P, blob, seeds, SEED0, 0, 256)
        assert want[0] is not None  # the reference itself finds one (miss chance (15/16)^255)
        assert engine.search_seeded(prog, gen, seeds, SEED0, 0, 256, early_exit=False) == want
        assert engine.search_seeded(prog, gen, seeds, SEED0, 0, 256, early_exit=True)[0] == want[0]
        assert engine.search(prog, gen, SEED0, 0, 256, early_exit=False) == (None, 0)
    finally:
        engine.free_gen(gen)
        engine.free(prog)


@pytest.mark.parametrize("w", list(workloads.WORKLOADS))
def test_no_seeds_is_the_plain_stream(engine, w):
    """n_seeds = 0 on the workload's largest bucket: the generator-independent lowering under the
    plain GEN3 candidates, equal to the C port's search of the same program and generator."""
    roots = max(partition.partition([c.raw for c in workloads.WORKLOADS[w]()]), key=len)
    P, blob = search.prepare(roots)
    pb = P.to_bytes()
    prog = engine.load(pb)
    gen = engine.load_gen(prog, blob)
    try:
        for start, count in ((0, 4096), (12345, 1000)):
            want = cport.search(pb, blob, SEED0, start, count, threads=16)[:2]
            assert engine.search_seeded(prog, gen, native.SeedSet(), SEED0, start, count, early_exit=False) == want
            assert engine.search_seeded(prog, gen, native.SeedSet(), SEED0, start, count)[0] == want[0]
    finally:
        engine.free_gen(gen)
        engine.free(prog)


def test_invalid_arguments_launch_nothing(engine, cases):
    c, other = cases["light"], cases["mid"]
    s = c.seeds
    nc = len(c.P.coords)
    past = s.coord_row.copy()
    past[c.ci["sp_a"]] = s.n_rows - 7  # eight limbs from there run one row past the end
    bad_sets = {
        "n_seeds > 32": native.SeedSet(np.zeros((s.n_rows, 33), np.uint32), s.coord_row, s.coord_has),
        "rows past n_rows": native.SeedSet(s.rows, past, s.coord_has),
        "null rows": native.SeedSet(None, s.coord_row, s.coord_has, n_seeds=3, n_rows=s.n_rows),
        "null coord_row": native.SeedSet(s.rows, None, s.coord_has),
        "null coord_has": native.SeedSet(s.rows, s.coord_row, None),
        "keep16": native.SeedSet(s.rows, s.coord_row, s.coord_has, keep16=65537),
        "keep16, no seeds": native.SeedSet(keep16=65537),
    }
    assert len(s.coord_row) == nc
    calls = [(name, c.prog, c.gen, bad) for name, bad in bad_sets.items()]
    calls += [("bad program", 0xDEAD0000, c.gen, s), ("bad generator", c.prog, 0xDEAD0000, s),
              ("generator of another program", c.prog, other.gen, s)]
    before = engine.stats().launches
    for name, prog, gen, seeds in calls:
        for call in (lambda: engine.search_seeded(prog, gen, seeds, SEED0, START, COUNT),
                     lambda: engine.eval_seeded(prog, gen, seeds, SEED0, START, COUNT)):
            with pytest.raises(native.EngineError) as ei:
                call()
            assert ei.value.code == native.MG_E_INVALID, name
    assert engine.stats().launches == before
    ver, _ = engine.eval_seeded(c.prog, c.gen, s, SEED0, START, COUNT)
    assert np.array_equal(ver, c.want_ver)
    s1 = engine.stats()
    assert s1.launches == before + 1 and s1.last_candidates == COUNT


def _accepted(roots, model):
    ver, scalars, arrays, funcs = model[0:4]
    om = OracleModel(scalars, arrays, funcs)
    return ver == 1 and all(evaluate(r, om) == 1 for r in roots)


def test_host_path_parent_child_sibling(engine):
    """The parent's model answers the child it satisfies from the replay lane; the negated
    sibling is answered too (by either engine)."""
    x, y = BVS("sh_x", 256), BVS("sh_y", 256)
    parent = [ULT(x, BVV(1000, 256)).raw, UGT(y, x).raw]
    cache = search.ModelCache()
    kw = {"max_candidates": 1 << 24, "timeout_s": 30, "warm": cache}
    rp = search.search(engine, parent, **kw)
    assert rp.index is not None and not rp.seeded and "seeded_ms" not in rp.timing
    assert _accepted(parent, rp.model) and len(cache) == 1
    sc = rp.model[1]
    bit = (sc["sh_x"] + sc["sh_y"]) & 1
    cond = Extract(0, 0, x + y) == BVV(bit, 1)
    child = parent + [cond.raw]
    rc = search.search(engine, child, **kw)
    print("child", rc.index, rc.engine, rc.timing)
    assert rc.engine == "seeded" and rc.seeded and rc.replay and rc.index == 0
    assert rc.timing["seeded_ms"] > 0 and rc.model[1] == sc
    assert _accepted(child, rc.model)
    sibling = parent + [Not(cond).raw]
    rs = search.search(engine, sibling, **kw)
    print("sibling", rs.index, rs.engine, rs.timing)
    assert rs.index is not None and "seeded_ms" in rs.timing
    assert _accepted(sibling, rs.model)
    assert len(cache) == 3


def test_host_path_needles_unchanged_by_an_empty_cache(engine):
    """A miss (here: nothing to seed from) continues exactly as without a cache."""
    from tests.test_gpu_search_batch import _needles

    kw = {"max_candidates": 1 << 24, "timeout_s": 30, "batch": False}
    a = search.search_partitioned(engine, _needles(), warm=None, **kw)
    b = search.search_partitioned(engine, _needles(), warm=search.ModelCache(), **kw)
    assert a.index == b.index == (205095, 390657)
    assert a.model[0:4] == b.model[0:4]
    assert not b.seeded and "seeded_ms" not in b.timing
