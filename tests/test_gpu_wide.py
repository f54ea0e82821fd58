"""Every engine above 1024 bits: wide values and multi-block Keccak on the GPU, bit-exact.

The engine takes values up to ``MG_MAX_WIDTH`` = 32768 bits; above 256 bits it lowers ADD / SUB /
AND / OR / XOR / NOT / NEG, CONCAT / EXTRACT / ZEXT / SEXT, ITE, EQ / ULT / ULE / SLT / SLE, wide
coordinates, UF tables with wide keys and Keccak-256 of any byte length.  LASER builds such
values: SHA3 over a memory region is a ``Concat`` of bytes of any concrete length
(``mythril/laser/ethereum/keccak_function_manager.py:59-72``).

References: explicit inputs (the Keccak length sweep, the operators, the UF keys, MG_MAX_WIDTH)
against the Python oracle (``oracle/bv.py``, ``oracle/keccak.py``, itself pinned against hashlib in
``tests/test_wide_cpu.py``); generator-mode verdicts against the wide C port
(``oracle/libbveval_wide.so``, ``cport.*(wide=True)``); wide UNIFORM coordinates against the
documented recurrence (``uniform_raw`` of ``tests/test_gen3_spec.py``).

Engines: the interpreter (``k_run``), the first tier (``jit_asm.cpp``, values up to 2048 bits: above
that its refusal is asserted) and the O3 kernels (``jit.cpp``).  Shapes are small: at most a few
hundred candidates per launch.
"""
import random

import numpy as np
import pytest

from mythril_amd import native, search, ssa
from mythril_amd.smt import terms as T
from oracle import cport
from oracle.bv import OracleModel, evaluate_many
from tests.helpers import (LENS, gpu_eval_terms, keccak_sweep_inputs, memory_region_queries, wide_edge_values,
                           wide_operator_terms)
from tests.test_gen3_spec import keys, uniform_raw

pytestmark = pytest.mark.gpu

SEED = 0x6D797468
KINDS = ("interp", "asm", "o3")
# Keccak lengths per program, sized from host compile times of the O3 eval kernel
# (native.jit_source(compile=True)): 0.6 .. 3.0 s per group, the first tier's in milliseconds
KECCAK_GROUPS = ((1, 2, 3, 4, 5, 7, 8, 9), (20, 31, 32, 33, 55, 63), (64, 65, 100, 127), (128, 129, 134, 135),
                 (136, 137, 200), (255, 256), (257, 271, 272, 273), (408, 500, 512))
assert tuple(n for g in KECCAK_GROUPS for n in g) == LENS
ASM_MAX_BITS = 2048  # the first tier's widest value (jit_asm.cpp: kMaxLimbs)


def _watched_program(terms):
    P = ssa.flatten([T.BoolVal(True)], extra=list(terms))
    P.set_watch([P.term_node[t.id] for t in terms])
    return P


def _run(engine, P, terms, assigns, kind, tiled=False):
    """Explicit candidates through one engine: (ProgramInfo, verdicts, [values of ``terms``] per row).
    ``assigns``: per candidate a row in P's coordinate order, or a {coordinate name: value} dict."""
    assert all(c.kind == ssa.COORD_SCALAR for c in P.coords)
    assigns = [[a.get(c.name, 0) for c in P.coords] if isinstance(a, dict) else a for a in assigns]
    soa = ssa.soa_from_assignments(P, assigns)
    n = len(assigns)
    prog = engine.load(P.to_bytes())
    try:
        info = engine.info(prog)
        assert info.watch_words == sum(ssa.limbs(t.width) for t in terms)
        if kind == "interp":
            ver, watch = engine.eval(prog, soa, n, watch_words=info.watch_words)
        else:
            jh = engine.jit_compile(prog, 0, asm=kind == "asm", tiled=tiled, o3=kind == "o3")
            try:
                flags = engine.jit_layout(jh)[0]
                assert bool(flags & native.MG_JIT_ASM) == (kind == "asm")  # the tier that was asked for
                ver, watch = engine.jit_eval(jh, native.tile_soa(soa) if tiled else soa, n,
                                             watch_words=info.watch_words)
            finally:
                engine.jit_free(jh)
    finally:
        engine.free(prog)
    widths = [t.width for t in terms]
    return info, ver, [search.read_rows(watch, widths, i) for i in range(n)]


def _inside_asm(t):
    return all(s.sort[0] != "bv" or s.width <= ASM_MAX_BITS for s in T.postorder([t]))


# ---------------------------------------------------------------------------
# Keccak length sweep on explicit inputs
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keccak_cases():
    """Per group: (digest terms, program, input rows, reference digests per row), the reference
    from ``oracle.keccak`` through ``evaluate_many``, computed once for all engines."""
    rng = random.Random(0xC0DE)
    out = {}
    for g in KECCAK_GROUPS:
        xs = [T.BitVecVar(f"kx{n}", 8 * n) for n in g]
        hs = [T.keccak256(x) for x in xs]
        P = _watched_program(hs)
        ci = {c.name: c.index for c in P.coords}
        cols = {x.params[0]: keccak_sweep_inputs(n, rng) for x, n in zip(xs, g)}
        rows = []
        for i in range(16):
            row = [0] * len(P.coords)
            for name, vals in cols.items():
                row[ci[name]] = vals[i]
            rows.append(row)
        want = [evaluate_many(hs, OracleModel({name: vals[i] for name, vals in cols.items()})) for i in range(16)]
        out[g] = (hs, P, rows, want)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("group", KECCAK_GROUPS, ids=lambda g: f"{g[0]}-{g[-1]}")
def test_keccak_length_sweep(engine, keccak_cases, group, kind):
    """Keccak-256 of 1 .. 512 bytes (one to four sponge blocks; every partial-word remainder; 135 /
    136 / 137 and 271 / 272 / 273 at the block edges) on zero, all ones, only the first byte 0x01,
    only the last byte 0x80 and 12 random inputs: every digest equals the oracle's.  The first tier
    runs row-major and tiled up to 256 bytes and refuses a 257-byte input."""
    hs, P, rows, want = keccak_cases[group]
    if kind == "asm" and 8 * group[-1] > ASM_MAX_BITS:
        prog = engine.load(P.to_bytes())
        try:
            with pytest.raises(native.EngineUnsupported, match="wider than 2048 bits"):
                engine.jit_compile(prog, 0, asm=True)
        finally:
            engine.free(prog)
        return
    for tiled in ((False, True) if kind == "asm" else (False,)):
        _, ver, got = _run(engine, P, hs, rows, kind, tiled=tiled)
        assert ver.all()
        for i in range(len(rows)):
            for n, g, w in zip(group, got[i], want[i]):
                assert g == w, f"{kind}: keccak of {n} bytes, row {i}: {g:064x} != {w:064x}"


# ---------------------------------------------------------------------------
# memory-region queries in generator mode
# ---------------------------------------------------------------------------
WINDOWS = ((37, 512), ((0x5A17 << 32) | 0x80000000 | 0x3FD, 512))  # unaligned; bit 31 of the low word set


@pytest.mark.parametrize("name", sorted(memory_region_queries()))
def test_memory_region_queries_generated(engine, name):
    """SHA3 over a memory region (literals and symbols mixed, 135 .. 200 bytes) under the default
    generator: per-candidate verdicts of the interpreter (``eval_generated``), the O3 kernel and the
    first tier (``jit_verdicts``) equal the wide C port's on two unaligned 512-candidate windows;
    ``search`` / ``jit_search`` report its first hit and hit count, and its first hit with early exit."""
    roots, _ = memory_region_queries()[name]
    P, blob = search.prepare(roots)
    pb = P.to_bytes()
    prog = engine.load(pb)
    gh = engine.load_gen(prog, blob)
    jits = {}
    try:
        jits["o3"] = engine.jit_compile(prog, gh, gen_verdicts=True)
        jits["asm"] = engine.jit_compile(prog, gh, gen_verdicts=True, asm=True)
        assert engine.jit_layout(jits["asm"])[0] & native.MG_JIT_ASM
        assert not engine.jit_layout(jits["o3"])[0] & native.MG_JIT_ASM
        for start, n in WINDOWS:
            cf, ch, want = cport.search(pb, blob, SEED, start, n, threads=8, verdicts=True, wide=True)
            assert 0 < int(want.sum()) < n, (name, int(want.sum()))
            got = {"interp": engine.eval_generated(prog, gh, SEED, start, n)[0]}
            for k, jh in jits.items():
                got[k] = engine.jit_verdicts(jh, SEED, start, n)
            for k, v in got.items():
                bad = np.flatnonzero(v != want)
                assert bad.size == 0, f"{name} {k}: {bad.size} verdicts differ, first at index {start + int(bad[0])}"
            assert engine.search(prog, gh, SEED, start, n, early_exit=False) == (cf, ch)
            assert engine.search(prog, gh, SEED, start, n, early_exit=True)[0] == cf
            for k, jh in jits.items():
                assert engine.jit_search(jh, SEED, start, n, early_exit=False) == (cf, ch), k
                assert engine.jit_search(jh, SEED, start, n, early_exit=True)[0] == cf, k
    finally:
        for jh in jits.values():
            engine.jit_free(jh)
        engine.free_gen(gh)
        engine.free(prog)


# ---------------------------------------------------------------------------
# wide operators
# ---------------------------------------------------------------------------
WIDTHS = (1025, 1056, 1088, 2047, 2048, 2049, 4096)


@pytest.fixture(scope="module")
def operator_cases():
    """Per width: (terms, program, coordinate rows, reference values per row) — the reference from
    ``oracle/bv.py``, computed once for all engines."""
    out = {}
    for w in WIDTHS:
        a, b, c, terms = wide_operator_terms(w)
        P = _watched_program(terms)
        rows, want = [], []  # rows by coordinate name: the chunks' programs have their own coordinate order
        for k, (x, y) in enumerate(wide_edge_values(w, random.Random(w))):
            rows.append({a.params[0]: x, b.params[0]: y, c.params[0]: k & 1})
            want.append(evaluate_many(terms, OracleModel(rows[-1])))
        out[w] = (terms, P, rows, want)
    return out


def _compare(kind, w, terms, got, want):
    for i in range(len(want)):
        for t, g, v in zip(terms, got[i], want[i]):
            assert g == v, f"{kind} at {w} bits, row {i}: {T.to_sexpr(t, 2)} = {g:#x}, oracle {v:#x}"


O3_PARTS = 6  # O3 kernels of 128-limb values take up to 3 s of host compile time each: a sixth of the terms per case
OPERATOR_CASES = [(w, kind, part) for w in WIDTHS for kind in KINDS
                  for part in (range(O3_PARTS) if kind == "o3" else (0,))]


@pytest.mark.parametrize("w,kind,part", OPERATOR_CASES, ids=lambda v: str(v))
def test_wide_operators_bit_exact(engine, operator_cases, w, kind, part):
    """Every operator the lowering admits above 256 bits, at 1025 .. 4096 bits, on the edge operands
    (0, 1, 2^W-1, 2^(W-1), 2^(W-1)-1, 2^1024, 2^1024-1, pairs differing only in limb 0 or only in
    the top limb, 2^W-1 + 1: a carry through every limb) and random ones; extracts at offsets 0, 1,
    31, 32, 33, W-33, 1023 and 1024.  The interpreter runs all terms in one program (from 2047 bits
    on a value file of more than 255 words per lane, in global memory); the O3 tier one kernel per
    term, a sixth of the terms per case; the first tier what stays within 2048 bits (a few watched values per kernel),
    and it refuses the rest."""
    terms, P, rows, want = operator_cases[w]
    if kind == "interp":
        info, ver, got = _run(engine, P, terms, rows, kind)
        assert ver.all()
        if w >= 2047:
            assert info.value_words > 255 and not info.uses_lds
        _compare(kind, w, terms, got, want)
        return
    if kind == "o3":
        # one term per kernel: several 128-limb values live at once multiply hipRTC's compile time
        for k in range(part, len(terms), O3_PARTS):
            _, ver, got = _run(engine, _watched_program([terms[k]]), [terms[k]], rows, kind)
            assert ver.all()
            _compare(kind, w, [terms[k]], got, [[r[k]] for r in want])
        return
    inside = [k for k, t in enumerate(terms) if _inside_asm(t)]
    outside = [k for k in range(len(terms)) if k not in inside]
    assert bool(outside) == (w + 8 > ASM_MAX_BITS)  # the terms that widen their operand (ZEXT / SEXT / CONCAT)
    assert inside if w <= 2048 else not inside
    for lo in range(0, len(inside), 4):
        idx = inside[lo:lo + 4]
        chunk = [terms[k] for k in idx]
        _, ver, got = _run(engine, _watched_program(chunk), chunk, rows, "asm", tiled=bool(lo & 4))
        assert ver.all()
        _compare("asm", w, chunk, got, [[r[k] for k in idx] for r in want])
    if outside:
        chunk = [terms[k] for k in outside]
        prog = engine.load(_watched_program(chunk).to_bytes())
        try:
            with pytest.raises(native.EngineUnsupported, match="wider than 2048 bits"):
                engine.jit_compile(prog, 0, asm=True)
        finally:
            engine.free(prog)


def test_wide_operators_lds_value_file(engine, operator_cases):
    """The other value-file placement: a few wide terms at a time keep the interpreter's file at no
    more than 255 words per lane, in LDS (``engine.info``: ``uses_lds``, or the small-launch rule of
    ``launch_async``), where ``test_wide_operators_bit_exact`` runs it in global memory."""
    n_lds = 0
    for w in (1025, 1088):
        terms, _, rows, want = operator_cases[w]
        for k in range(0, len(terms), 2):
            chunk = terms[k:k + 2]
            info, ver, got = _run(engine, _watched_program(chunk), chunk, rows, "interp")
            assert info.value_words <= 255, (w, k, info.value_words)
            n_lds += bool(info.uses_lds)
            _compare("interp (LDS)", w, chunk, got, [r[k:k + 2] for r in want])
    assert n_lds > 0


# ---------------------------------------------------------------------------
# UF tables with wide keys
# ---------------------------------------------------------------------------
def _wide_uf_query():
    """LASER's Keccak bookkeeping (``keccak_model.KeccakFunctionManager``) over 1088-bit symbolic
    inputs: x and y at two sites with unequal keys, and x again under a structurally different term
    of equal value (an equal key: the sites share one table entry)."""
    from mythril_amd.keccak_model import KeccakFunctionManager
    from mythril_amd.smt import Concat, Extract, Not, symbol_factory
    from oracle.keccak import keccak256

    km = KeccakFunctionManager(hasher=lambda msgs: [keccak256(m) for m in msgs])
    x, y = symbol_factory.BitVecSym("uf_x", 1088), symbol_factory.BitVecSym("uf_y", 1088)
    x2 = Concat(Extract(1087, 256, x), Extract(255, 0, x))
    (hx, cx), (hy, cy), (hx2, cx2) = km.create_keccak(x), km.create_keccak(y), km.create_keccak(x2)
    cs = [cx, cy, cx2, hx == hx2, Not(hx == hy)]
    return [c.raw for c in cs], [hx.raw, hy.raw, hx2.raw, x2.raw]


def test_wide_uf_keys_search_finds_an_accepted_model(engine):
    """The search over 1088-bit UF keys finds a model — the interpreter, the first tier and the O3
    kernel at the same index — and the oracle accepts it."""
    from oracle.bv import evaluate

    roots, _ = _wide_uf_query()
    P, blob = search.prepare(roots)
    prog = engine.load(P.to_bytes())
    gh = engine.load_gen(prog, blob)
    jits = []
    try:
        assign = np.zeros(engine.info(prog).watch_words, dtype=np.uint32)
        first, _ = engine.search(prog, gh, SEED, 0, 1 << 14, early_exit=True, assign=assign)
        assert first is not None, "no model among 2^14 candidates"
        scalars, arrays, funcs = search.model_from_assignment(P, assign)
        m = OracleModel(scalars, arrays, funcs)
        assert all(evaluate(r, m) == 1 for r in roots), "the oracle rejects the model"
        assert len(funcs["keccak256_1088"][0]) == 2  # x and x2 share an entry, y has its own
        for asm in (True, False):
            jits.append(engine.jit_compile(prog, gh, asm=asm))
            a2 = np.zeros_like(assign)
            assert engine.jit_search(jits[-1], SEED, 0, 1 << 14, early_exit=True, assign=a2)[0] == first
            assert (a2 == assign).all()
    finally:
        for jh in jits:
            engine.jit_free(jh)
        engine.free_gen(gh)
        engine.free(prog)


@pytest.mark.parametrize("kind", KINDS)
def test_wide_uf_keys_values_under_read_back_models(engine, kind):
    """Per candidate, every hash term and the verdict equal the oracle's under the model the GPU
    read back (as ``test_random_dags_bit_exact``); rows where x == y make the two sites' keys
    collide at run time."""
    roots, watch = _wide_uf_query()
    P0 = ssa.flatten(list(roots), extra=list(watch))  # gpu_eval_terms flattens the same way: same coordinates
    cx, cy = ([c.index for c in P0.coords if c.name == n][0] for n in ("uf_x", "uf_y"))
    rng = random.Random(0x0F)
    assigns = []
    for i in range(48):
        row = [rng.getrandbits(c.width) for c in P0.coords]
        if i % 8 == 1:
            row[cx] = (1 << 1088) - 1 if i & 8 else 1 << 1024
        if i % 3 == 0:  # y == x: one key for every site
            row[cy] = row[cx]
        assigns.append(row)
    P, _, ver, vals, models = gpu_eval_terms(engine, roots, watch, assigns=assigns, jit=kind != "interp",
                                             asm=kind == "asm", o3=kind == "o3")
    shared = 0
    for i in range(len(assigns)):
        mdl = models[i]
        for c in P.scalar_coords():
            assert mdl.scalars[c.name] == assigns[i][c.index] & ((1 << c.width) - 1)
        want = evaluate_many(list(watch) + list(roots), mdl)
        for t, w in zip(watch, want):
            assert vals[i][t.id] == w, (kind, i, T.to_sexpr(t, 2))
        assert ver[i] == int(all(want[len(watch):])), (kind, i)
        shared += len(mdl.funcs["keccak256_1088"][0]) == 1
    assert shared == len(assigns[::3])


# ---------------------------------------------------------------------------
# wide UNIFORM coordinates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1088, 4096])
def test_wide_uniform_coordinates(engine, w):
    """GEN-mode watch rows of a UNIFORM coordinate of 1088 / 4096 bits across a 64-index group
    boundary equal the documented recurrence limb for limb, and the searches of ``x == v`` (the
    interpreter, the O3 kernel, the first tier up to 2048 bits) hit exactly the index that draws v."""
    x = T.BitVecVar("g3w", w)
    L = ssa.limbs(w)
    start, n, pick = (1 << 40) | 0x800000BD, 70, 41  # low word: bit 31 set, 61 mod 64

    def program(v):
        P = ssa.flatten([T.eq(x, T.BitVecVal(v, w))])
        (c,) = [co for co in P.coords if co.name == "g3w"]
        P.set_watch([c.node])
        gb = search.GenBuilder(P)
        gb.uniform(c.index)
        return P, gb.blob(), c.index

    _, _, c = program(0)
    want = [uniform_raw(keys(start + i, SEED), c, L) for i in range(n)]
    v = ssa.limbs_to_int(want[pick])
    P, blob, _ = program(v)
    prog = engine.load(P.to_bytes())
    gh = engine.load_gen(prog, blob)
    jits = []
    try:
        ver, watch = engine.eval_generated(prog, gh, SEED, start, n, watch_words=L)
        for i in range(n):
            assert [int(u) for u in watch[:, i]] == want[i], (w, start + i)
        assert [int(u) for u in np.flatnonzero(ver)] == [pick]
        assert engine.search(prog, gh, SEED, start, n, early_exit=False) == (start + pick, 1)
        jits.append(engine.jit_compile(prog, gh))
        if w <= ASM_MAX_BITS:
            jits.append(engine.jit_compile(prog, gh, asm=True))
        else:
            with pytest.raises(native.EngineUnsupported, match="wider than 2048 bits"):
                engine.jit_compile(prog, gh, asm=True)
        for jh in jits:
            assert engine.jit_search(jh, SEED, start, n, early_exit=False) == (start + pick, 1)
    finally:
        for jh in jits:
            engine.jit_free(jh)
        engine.free_gen(gh)
        engine.free(prog)


# ---------------------------------------------------------------------------
# MG_MAX_WIDTH (interpreter only)
# ---------------------------------------------------------------------------
def test_max_width_interpreter(engine):
    """32768 bits, the widest value the engine takes, on the interpreter (compiled tiers are not
    launched at this width): an ADD whose carry crosses all 1024 limbs, EQ on operands that differ
    only in the top limb / only in limb 0, and Keccak-256 of 4096 bytes (31 sponge blocks), n = 8."""
    w = 32768
    a, b = T.BitVecVar("mw_a", w), T.BitVecVar("mw_b", w)
    terms = [T.bvbin("bvadd", a, b), T.eq(a, b), T.eq(T.bvbin("bvadd", a, b), T.BitVecVal(0, w)), T.keccak256(a),
             T.bvcmp("bvult", a, b)]
    P = _watched_program(terms)
    rng = random.Random(0x8000)
    m = (1 << w) - 1
    r = rng.getrandbits(w)
    pairs = [(m, 1), (m, m), (r, r), (r, r ^ (1 << (w - 1))), (r, r ^ 1), (0, 0),
             (rng.getrandbits(w), rng.getrandbits(w)), ((1 << (w - 1)) | 1, (1 << (w - 1)) - 1)]
    rows = [{"mw_a": x, "mw_b": y} for x, y in pairs]
    info, ver, got = _run(engine, P, terms, rows, "interp")
    assert ver.all() and info.value_words > 2 * 1024 and not info.uses_lds
    for i, (x, y) in enumerate(pairs):
        want = evaluate_many(terms, OracleModel({"mw_a": x, "mw_b": y}))
        for t, g, v in zip(terms, got[i], want):
            assert g == v, (i, T.to_sexpr(t, 2))
