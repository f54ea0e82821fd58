"""``mg_search_batch``: several different (program, generator, seed, window) searches in one
interpreter launch (``k_run_batch``), against the C port and against single ``mg_search`` calls.

The entries are the real buckets the independence solver produces
(``mythril/laser/smt/solver/independence_solver.py:119-140``): every bucket of the six workloads,
the two independent 2^-16 needles of ``test_gpu_solver.py`` and a variable-free bucket.  Expected
values come from the C port (``oracle/bveval.c``) for windows of at most 4096 candidates and from
``Engine.search`` beyond.  First hits are exact in every mode; hit counts are compared for full
sweeps only (with early exit they depend on when the waves above the hit saw it).
"""
import numpy as np
import pytest

from mythril_amd import native, partition, search, workloads
from mythril_amd.smt import ULT, Extract, symbol_factory
from oracle import cport
from oracle.bv import OracleModel, evaluate

pytestmark = pytest.mark.gpu
BVV = symbol_factory.BitVecVal
BVS = symbol_factory.BitVecSym

SEED0 = 0x6D797468
SEEDS = (SEED0, 0x1F3A9C5B27D4EB4F, 0x00C0FFEE5EED1234)  # the default and two random ones
STARTS = (0, 12345, (1 << 40) | 1)
COUNTS = (0, 1, 63, 64, 65, 1000, 4096, (1 << 20) + 17)  # the last one is not batchable
SENTINEL = 0xA5A5A5A5

# device ops of mythril_amd/csrc/program.hpp that put a program into the mid / heavy interpreter tier
_MID_OPS = {4, 15, 16, 17, 28}    # MUL, SHL, LSHR, ASHR, UMUL_NOOVF
_HEAVY_OPS = {5, 6, 7, 8, 9, 29}  # UDIV, UREM, SDIV, SREM, SMOD, EXP
_K_KECCAK = 31


def _needles():
    x, y = BVS("x", 256), BVS("y", 256)
    k1, k2 = BVV(0x9E3779B97F4A7C15F39CC0605CEDC835, 256), BVV(0xC2B2AE3D27D4EB4F165667B19E3779F9, 256)
    return [(Extract(15, 0, x * k1) == BVV(0x1234, 16)).raw, (Extract(15, 0, y * k2) == BVV(0xBEEF, 16)).raw]


def _queries():
    qs = {w: [c.raw for c in f()] for w, f in workloads.WORKLOADS.items()}
    qs["needles"] = _needles()
    qs["ground"] = [ULT(BVV(3, 256), BVV(5, 256)).raw]
    return qs


def _tier(pb, blob):
    t = 0
    for ins in native.specialized_program(pb, blob, interp=True)["code"]:
        op = int(ins[0])
        if op in _MID_OPS:
            t = max(t, 1)
        if op in _HEAVY_OPS or (op == _K_KECCAK and int(ins[3]) != 0xFFFFFFFF):
            t = 2
    return t


def _watch_value_words(e):
    """Value-file words of the entry's watch-list variant (what a capturing launch runs)."""
    return native.check_program_gen(e.pb, e.blob).value_words


class Entry:
    def __init__(self, engine, name, roots):
        self.name, self.roots = name, roots
        self.P, self.blob = search.prepare(roots)
        self.pb = self.P.to_bytes()
        self.prog = engine.load(self.pb)
        self.gen = engine.load_gen(self.prog, self.blob)
        self.ww = max(self.P.watch_words, 1)


@pytest.fixture(scope="module")
def entries(engine):
    out = []
    for w, roots in _queries().items():
        for i, b in enumerate(partition.partition(roots)):
            out.append(Entry(engine, f"{w}[{i}]", b))
    yield out
    for e in out:
        engine.free_gen(e.gen)
        engine.free(e.prog)


def _expect(engine, e, seed, start, count):
    """(first hit or None, hits) of a full sweep: the C port up to 4096 candidates, else the engine."""
    if count <= 4096:
        return cport.search(e.pb, e.blob, seed, start, count, threads=16)[:2]
    return engine.search(e.prog, e.gen, seed, start, count, early_exit=False)


@pytest.fixture(scope="module")
def sweep(engine, entries):
    """The requests of the sweep cases and their expected results, computed once: every entry over
    [0, 4096) at the default seed, then every entry under each seed with the starts rotating and
    the counts cycling."""
    reqs = [(e, SEED0, 0, 4096) for e in entries]
    j = 0
    for k, seed in enumerate(SEEDS):
        for i, e in enumerate(entries):
            reqs.append((e, seed, STARTS[(i + k) % len(STARTS)], COUNTS[j % len(COUNTS)]))
            j += 1
    want = [_expect(engine, e, seed, start, count) for e, seed, start, count in reqs]
    return reqs, want


def _batch(engine, reqs, early_exit, assigns=None):
    assigns = assigns or [None] * len(reqs)
    return engine.search_batch([(e.prog, e.gen, seed, start, count, a)
                                for (e, seed, start, count), a in zip(reqs, assigns)], early_exit=early_exit)


def test_entries_cover_the_tiers_and_both_outcomes(engine, entries, sweep):
    """What the other cases rely on: the light, mid and heavy interpreter tiers are all in the
    batch; every search program fits one block's LDS (so only the window decides the routing) while
    one watch-list variant does not (a batched entry whose model is read back after the launch);
    and at the default seed [0, 4096) holds hits and misses (the needles' first hits are at 205095
    and 390657)."""
    assert {_tier(e.pb, e.blob) for e in entries} == {0, 1, 2}
    assert all(engine.gen_info(e.gen).value_words <= 255 for e in entries)
    watch_words = [_watch_value_words(e) for e in entries]
    assert max(watch_words) > 255 and min(watch_words) <= 255
    first = {e.name: w[0] for (e, _, _, _), w in zip(sweep[0][:len(entries)], sweep[1])}
    assert first["suicide_kill[0]"] == 2594 and first["bectoken_batch_overflow[0]"] == 1412
    assert first["token_transfer_underflow[0]"] == 5 and first["ground[0]"] == 0
    assert first["needles[0]"] is None and first["needles[1]"] is None


def test_full_sweep_first_hits_and_counts(engine, sweep):
    reqs, want = sweep
    got = _batch(engine, reqs, early_exit=False)
    for (e, seed, start, count), g, w in zip(reqs, got, want):
        print(e.name, hex(seed), start, count, g, w)
        assert g == w, (e.name, hex(seed), start, count)


def test_early_exit_first_hits(engine, sweep):
    reqs, want = sweep
    got = _batch(engine, reqs, early_exit=True)
    for (e, seed, start, count), g, w in zip(reqs, got, want):
        assert g[0] == w[0], (e.name, hex(seed), start, count)


@pytest.mark.parametrize("w", list(workloads.WORKLOADS))
def test_per_candidate_verdicts(engine, entries, w):
    """64 entries of one candidate each: an aligned group that holds both verdicts, then the 64
    candidates that straddle its upper boundary."""
    mine = sorted((e for e in entries if e.name.startswith(w + "[")), key=lambda e: -len(e.roots))
    for e in mine:  # the largest bucket with such a group
        ver = cport.search(e.pb, e.blob, SEED0, 0, 4096, threads=16, verdicts=True)[2]
        groups = [g for g in range(0, 4096 - 128, 64) if 0 < int(ver[g:g + 64].sum()) < 64]
        if groups:
            break
    else:
        pytest.fail(f"{w}: no aligned group with both verdicts in [0, 4096)")
    for base in (groups[0], groups[0] + 32):
        got = _batch(engine, [(e, SEED0, base + q, 1) for q in range(64)], early_exit=False)
        assert [h for _, h in got] == [int(v) for v in ver[base:base + 64]], (e.name, base)
        assert [f for f, _ in got] == [base + q if ver[base + q] else None for q in range(64)], (e.name, base)


def test_models_captured_and_read_back(engine, entries):
    """A hit's watch rows equal ``Engine.search``'s for the same arguments: for captured entries
    (4096 from 0, one group per block) and for the non-batchable count, whose model comes from
    the single-query path.  A miss leaves its buffer untouched."""
    reqs = [(e, SEED0, 0, 4096) for e in entries] + [(e, SEEDS[1], 12345, COUNTS[-1]) for e in entries[:6]]
    assigns = [np.full(e.ww, SENTINEL, dtype=np.uint32) for e, _, _, _ in reqs]
    got = _batch(engine, reqs, early_exit=True, assigns=assigns)
    hit = miss = 0
    for (e, seed, start, count), a, g in zip(reqs, assigns, got):
        ref = np.full(e.ww, SENTINEL, dtype=np.uint32)
        r = engine.search(e.prog, e.gen, seed, start, count, early_exit=True, assign=ref)
        assert g[0] == r[0], (e.name, count)
        assert np.array_equal(a, ref), (e.name, count)
        if g[0] is None:
            miss += 1
            assert (a == SENTINEL).all(), e.name
        else:
            hit += 1
    assert hit and miss


def test_model_of_a_batched_entry_without_capture(engine, entries):
    """Entries that ask for a model after the capture buffer (64 MiB) is used up: enough copies of
    the widest capturable watch list, 4096 candidates each, that the last ones do not fit.  They
    still return ``Engine.search``'s model: the engine reads it back after the launch."""
    e = max((x for x in entries if _watch_value_words(x) <= 255), key=lambda x: x.ww)
    per_entry = 64 * e.ww * 64 * 4  # blocks x rows x lanes x bytes
    n = min(64, (64 << 20) // per_entry + 2)
    if (n - 1) * per_entry <= (64 << 20):
        pytest.fail(f"{e.name}: {n} entries of {per_entry} bytes do not exceed the capture buffer")
    reqs = [(e, 100 + q, 0, 4096) for q in range(n)]
    assigns = [np.full(e.ww, SENTINEL, dtype=np.uint32) for _ in reqs]
    got = _batch(engine, reqs, early_exit=True, assigns=assigns)
    for (_, seed, start, count), a, g in zip(reqs, assigns, got):
        ref = np.full(e.ww, SENTINEL, dtype=np.uint32)
        assert g[0] == engine.search(e.prog, e.gen, seed, start, count, early_exit=True, assign=ref)[0]
        assert np.array_equal(a, ref), seed


def test_more_entries_than_one_launch_holds(engine, entries):
    """70 entries (64 per launch), one (program, generator) under 70 seeds."""
    e = next(x for x in entries if x.name == "token_transfer_underflow[0]")
    reqs = [(e, 1000 + q, 64 * q, 1000) for q in range(70)]
    got = _batch(engine, reqs, early_exit=False)
    want = [engine.search(e.prog, e.gen, seed, start, count, early_exit=False) for _, seed, start, count in reqs]
    assert got == want
    assert len({g for g in got}) > 1  # the seeds matter


def test_bad_handle_fails_the_whole_call(engine, entries):
    good = [(e, SEED0, 0, 4096) for e in entries[:5]]
    raw = [(e.prog, e.gen, seed, start, count, None) for e, seed, start, count in good]
    bad = list(raw)
    bad[3] = (bad[3][0], 0xDEAD0000, SEED0, 0, 4096, None)
    before = engine.stats().launches
    with pytest.raises(native.EngineError) as ei:
        engine.search_batch(bad, early_exit=False)
    assert ei.value.code == native.MG_E_INVALID
    assert engine.stats().launches == before
    got = engine.search_batch(raw, early_exit=False)
    assert got == [_expect(engine, e, seed, start, count) for e, seed, start, count in good]


def test_empty_batch_and_stats(engine, entries):
    assert engine.search_batch([]) == []
    reqs = [(e, SEED0, 0, 4096) for e in entries]
    s0 = engine.stats()
    _batch(engine, reqs, early_exit=False)
    s1 = engine.stats()
    assert s1.launches - s0.launches == 1  # every entry in one interpreter launch
    assert s1.candidates - s0.candidates == 4096 * len(reqs)
    assert s1.last_candidates == 4096 * len(reqs) and s1.last_kernel_ms > 0


@pytest.mark.parametrize("jit", ["never", None])
@pytest.mark.parametrize("w", list(workloads.WORKLOADS) + ["needles"])
def test_search_partitioned_batched_equals_serial(engine, w, jit):
    """Same index tuple, model and bucket count with the buckets' first launches batched; in the
    needle query both buckets miss the first launch and continue."""
    roots = _queries()[w]
    kw = {"max_candidates": 1 << 24, "timeout_s": 30}
    if jit is not None:
        kw["jit"] = jit
    a = search.search_partitioned(engine, roots, batch=False, **kw)
    b = search.search_partitioned(engine, roots, batch=True, **kw)
    assert b.index == a.index
    assert b.buckets == a.buckets == len(partition.partition(roots))
    assert a.index is not None and isinstance(a.index, tuple), "the serial search gave up"
    assert b.model[0:4] == a.model[0:4]
    ver, scalars, arrays, funcs = b.model[0:4]
    om = OracleModel(scalars, arrays, funcs)
    assert ver == 1 and all(evaluate(c, om) == 1 for c in roots)
    if w == "needles":
        assert a.index == (205095, 390657)
