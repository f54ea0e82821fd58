"""GEN3 at its edge parameters on the GPU, every engine: the case table of
``tests/gen3_edge_cases.py`` (span / count 0, sums that wrap the width, shifts beyond the
coordinate's limbs, borrowing deltas, narrow and odd widths, clamps at the top of the range, a COPY
chain of depth 64, a fix record on a COPY source, a 65,535-entry dictionary).

* the interpreter's generated VALUES, read directly as watch rows of the coordinate VAR nodes,
  against the header's restatement (``tests/gen3_ref.py``) limb for limb;
* per-candidate VERDICTS of a probe root that depends on every bit of every coordinate —
  interpreter, O3 kernel and first tier — against the C port, and every search entry point's
  ``(first_hit, n_hits)`` and read-back rows;
* the batch path, the seeded and scored sweeps on the MIXED program and the chain;
* the window rule (``include/mythgpu.h``, WINDOWS): every sweeping entry point refuses a window
  that reaches 2^64 before anything is queued, and accepts the last usable one.

Windows of 2,048 candidates: from 0, ending at the last usable index 2^64 - 2, and a random 63-bit
start with bit 31 of the low word set.  Only generators ``mg_gen_load`` accepts reach the GPU."""
import random

import numpy as np
import pytest

from mythril_amd import native
from oracle import cport
from tests import gen3_edge_cases as E
from tests import gen3_ref as R
from tests import seeded_ref

pytestmark = pytest.mark.gpu
SEED = E.SEED0
N = E.WINDOW
TOP = 1 << 64


class Loaded:
    def __init__(self, engine, c):
        self.c = c
        self.prog = engine.load(c.prog)
        self.gen = engine.load_gen(self.prog, c.blob)
        self.ww = engine.info(self.prog).watch_words
        assert self.ww == c.P.coord_words == engine.gen_info(self.gen).watch_words
        # the references, once: the C port's verdicts and the restatement's rows per window
        self.ver = {s: cport.search(c.prog, c.blob, SEED, s, N, verdicts=True) for s in E.STARTS}
        self._rows = {}
        self.jit = {}

    def rows(self, start):
        if start not in self._rows:
            self._rows[start] = np.array(self.c.ref_rows(SEED, start, N), dtype=np.uint32)
        return self._rows[start]

    def kernel(self, engine, asm):
        """The O3 kernel or the first tier's, compiled once with mgj_gen.  A refusal fails the test."""
        if asm not in self.jit:
            self.jit[asm] = engine.jit_compile(self.prog, self.gen, gen_verdicts=True, asm=asm)
            flags = engine.jit_layout(self.jit[asm])[0]
            assert bool(flags & native.MG_JIT_ASM) == asm
            print(self.c.name, "first tier" if asm else "O3 kernel", "compile ms", round(engine.jit_info(self.jit[asm])[0], 1))
        return self.jit[asm]


@pytest.fixture(scope="module")
def loaded(engine):
    out = {c.name: Loaded(engine, c) for c in E.cases()}
    yield out
    for ld in out.values():
        for j in ld.jit.values():
            engine.jit_free(j)
        engine.free_gen(ld.gen)
        engine.free(ld.prog)


def _check_hit_rows(ld, first, assign):
    want = R.soa_rows(R.gen_values(ld.c.specs, ld.c.consts, ld.c.widths, SEED, first), ld.c.widths)
    assert assign.tolist() == want, (ld.c.name, hex(first))


@pytest.mark.parametrize("name", E.NAMES)
def test_interpreter_values_and_verdicts(engine, loaded, name):
    """Generated limbs read on the GPU against the restatement; verdicts against the C port."""
    ld = loaded[name]
    for start in E.STARTS:
        ver, watch = engine.eval_generated(ld.prog, ld.gen, SEED, start, N, watch_words=ld.ww)
        bad = np.argwhere(watch != ld.rows(start))
        assert bad.size == 0, (name, hex(start), "row, candidate:", bad[:4].tolist())
        assert np.array_equal(ver, ld.ver[start][2]), (name, hex(start), np.flatnonzero(ver != ld.ver[start][2])[:4])


@pytest.mark.parametrize("name", E.NAMES)
def test_interpreter_search(engine, loaded, name):
    ld = loaded[name]
    for start in E.STARTS:
        first, n, _ = ld.ver[start]
        assign = np.zeros(ld.ww, dtype=np.uint32)
        assert engine.search(ld.prog, ld.gen, SEED, start, N, early_exit=False, assign=assign) == (first, n)
        assert first is not None
        _check_hit_rows(ld, first, assign)
        assert engine.search(ld.prog, ld.gen, SEED, start, N, early_exit=True)[0] == first


@pytest.mark.parametrize("asm", [False, True], ids=["o3", "first_tier"])
@pytest.mark.parametrize("name", E.NAMES)
def test_compiled_kernels(engine, loaded, name, asm):
    """mgj_gen's per-candidate verdicts and mgj_search's result and read-back, both tiers."""
    ld = loaded[name]
    jh = ld.kernel(engine, asm)
    for start in E.STARTS:
        first, n, want = ld.ver[start]
        ver = engine.jit_verdicts(jh, SEED, start, N)
        assert np.array_equal(ver, want), (name, asm, hex(start), np.flatnonzero(ver != want)[:4])
        assign = np.zeros(ld.ww, dtype=np.uint32)
        assert engine.jit_search(jh, SEED, start, N, early_exit=False, assign=assign) == (first, n)
        _check_hit_rows(ld, first, assign)
        assert engine.jit_search(jh, SEED, start, N, early_exit=True)[0] == first


def test_batch_path(engine, loaded):
    """Every table program in one mg_search_batch call equals mg_search (and the C port) entry for entry."""
    reqs, want, ref = [], [], []
    for q, name in enumerate(E.NAMES):
        ld = loaded[name]
        start = E.STARTS[q % len(E.STARTS)]
        reqs.append((ld.prog, ld.gen, SEED, start, 1000, np.zeros(ld.ww, dtype=np.uint32)))
        want.append(engine.search(ld.prog, ld.gen, SEED, start, 1000, early_exit=False))
        ref.append(cport.search(ld.c.prog, ld.c.blob, SEED, start, 1000)[:2])
    got = engine.search_batch(reqs, early_exit=False)
    assert got == want == ref
    for (first, _), req, name in zip(got, reqs, E.NAMES):
        _check_hit_rows(loaded[name], first, req[5])


@pytest.mark.parametrize("name", ["mixed", "chain"])
def test_seeded_and_scored_sweeps(engine, loaded, name):
    """Every second coordinate seeded, keep16 = 1/2: a COPY copies the GENERATED final value of its
    source, seeded or not, along chains."""
    ld = loaded[name]
    P = ld.c.P
    rng = random.Random("seeded-" + name)
    models = [{c.index: rng.getrandbits(c.width) for c in P.coords if c.index % 2 == 0} for _ in range(3)]
    seeds = seeded_ref.seed_set(P, models, keep16=32768)
    start = E.STARTS[2]
    want, soa = seeded_ref.seeded_verdicts(P, ld.c.blob, seeds, SEED, start, N)
    assert not np.array_equal(soa, ld.rows(start))  # the seeds matter
    assert 0 < int(want.sum()) < N
    ver, watch = engine.eval_seeded(ld.prog, ld.gen, seeds, SEED, start, N, watch_words=ld.ww)
    bad = np.argwhere(watch != soa)
    assert bad.size == 0, (name, "row, candidate:", bad[:4].tolist())
    assert np.array_equal(ver, want)
    hits = np.flatnonzero(want)
    ref = (start + int(hits[0]), int(hits.size))
    assert engine.search_seeded(ld.prog, ld.gen, seeds, SEED, start, N, early_exit=False) == ref
    assert engine.search_scored(ld.prog, ld.gen, seeds, SEED, start, N, want_assigns=False)[:2] == ref


# ---- the window rule ---------------------------------------------------------------------------

BAD = [(TOP - 64, 64), (TOP - 1, 1)]
LAST = (TOP - 65, 64)  # ends at index 2^64 - 2, the last usable one


def _entry_points(engine, ld, jits):
    """name -> f(start, count) for every sweeping entry point of the shim."""
    empty = native.SeedSet()
    ok = (ld.prog, ld.gen, SEED, 0, 64, None)
    return {
        "mg_search": lambda s, n: engine.search(ld.prog, ld.gen, SEED, s, n, early_exit=False),
        "mg_search_batch": lambda s, n: engine.search_batch([ok, (ld.prog, ld.gen, SEED, s, n, None), ok],
                                                            early_exit=False)[1],
        "mg_eval_generated": lambda s, n: engine.eval_generated(ld.prog, ld.gen, SEED, s, n)[0],
        "mg_search_seeded": lambda s, n: engine.search_seeded(ld.prog, ld.gen, empty, SEED, s, n, early_exit=False),
        "mg_eval_seeded": lambda s, n: engine.eval_seeded(ld.prog, ld.gen, empty, SEED, s, n)[0],
        "mg_search_scored": lambda s, n: engine.search_scored(ld.prog, ld.gen, None, SEED, s, n, want_assigns=False)[:2],
        "mg_jit_search": lambda s, n: engine.jit_search(jits[0], SEED, s, n, early_exit=False),
        "mg_jit_search(first tier)": lambda s, n: engine.jit_search(jits[1], SEED, s, n, early_exit=False),
        "mg_jit_search_many": lambda s, n: engine.jit_search_many(jits[0], [SEED] * 3, [0, s, 64], [64, n, 64])[1],
        "mg_jit_verdicts": lambda s, n: engine.jit_verdicts(jits[0], SEED, s, n),
        "mg_jit_verdicts(first tier)": lambda s, n: engine.jit_verdicts(jits[1], SEED, s, n),
    }


def test_windows_that_reach_2_64_are_refused(engine, loaded):
    """MG_E_INVALID with a message and no launch, from every entry point; mg_split_range likewise."""
    ld = loaded["range"]
    fs = _entry_points(engine, ld, [ld.kernel(engine, False), ld.kernel(engine, True)])
    for name, f in fs.items():
        for start, count in BAD:
            before = engine.stats().launches
            with pytest.raises(native.EngineError, match="window reaches 2\\^64") as ei:
                f(start, count)
            assert ei.value.code == native.MG_E_INVALID, (name, ei.value)
            assert engine.stats().launches == before, name
    for start, count in BAD:
        with pytest.raises(native.EngineError, match="window reaches 2\\^64"):
            native.split_range(start, count, 2)


def test_last_usable_window_is_swept(engine, loaded):
    """[2^64 - 65, 2^64 - 1) is accepted everywhere and gives the C port's answer."""
    ld = loaded["range"]
    fs = _entry_points(engine, ld, [ld.kernel(engine, False), ld.kernel(engine, True)])
    start, count = LAST
    first, n, ver = cport.search(ld.c.prog, ld.c.blob, SEED, start, count, verdicts=True)
    assert first is not None and 0 < n < count
    for name, f in fs.items():
        got = f(start, count)
        if isinstance(got, np.ndarray):
            assert np.array_equal(got, ver), name
        else:
            assert tuple(got) == (first, n), (name, got)
    assert sum(c for _, c in native.split_range(start, count, 2)) == count
