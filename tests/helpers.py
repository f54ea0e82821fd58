"""Shared test infrastructure: golden-vector loaders, a random term-DAG
generator and the GPU-vs-oracle comparison used by the parity tests."""
from __future__ import annotations

import json
import random
from pathlib import Path
from typing import Dict, List, Sequence

import numpy as np

from mythril_amd import ssa
from mythril_amd.replay import ExceptionalHalt, ReplayUnsupported, replay, replay_assignment
from mythril_amd.smt import terms as T
from oracle.bv import OracleModel, evaluate_many

GOLDEN = Path(__file__).resolve().parent / "golden"


def load_json(name):
    return json.loads((GOLDEN / name).read_text())


# VMTests vectors with a post-state that the replay refuses, by name: none since round 4
# (CALLDATACOPY, CODECOPY, SELFDESTRUCT and the input-dependent jumps of DynamicJump_value* and
# TestNameRegistrator, followed along the concrete path).  A regression that refuses more shows up
# as a failed assertion in vmtest_cases, not as a silently shorter list.
VMTEST_REFUSED: Dict[str, str] = {}


def vmtest_cases(follow: bool = True):
    """(name, vector, ReplayResult) for every VMTests vector whose outcome is a post-state (not
    ignored by the reference: ``tests/laser/evm_testsuite/evm_test.py:109-188``).  Input-dependent
    jumps are followed along the vector's concrete path (the oracle evaluates the decision; the
    replay keeps it as a path constraint, ``ReplayResult.path``)."""
    out, refused = [], {}
    for name, v in sorted(load_json("vmtests.json").items()):
        if v["reference_ignored"] or v["post_storage"] is None:
            continue
        pre = {int(k, 16): int(x, 16) for k, x in v["pre_storage"].items()}
        fol = None
        if follow:
            scal, arrs = replay_assignment(v)
            m = OracleModel(scal, arrs)
            fol = lambda t, m=m: evaluate_many([t], m)[0]  # noqa: E731
        try:
            r = replay(v["code"], bytes.fromhex(v["data"]), pre, follow=fol)
        except (ReplayUnsupported, ExceptionalHalt) as e:
            refused[name] = str(e)
            continue
        out.append((name, v, r))
    if follow:
        assert refused == VMTEST_REFUSED, f"replay refuses VMTests vectors: {refused}"
    return out


# ---------------------------------------------------------------------------
# random programs
# ---------------------------------------------------------------------------
EDGE_256 = [0, 1, 2, 3, 31, 32, 255, 256, 257, (1 << 255), (1 << 255) - 1, (1 << 256) - 1, (1 << 256) - 2,
            (1 << 128), (1 << 160) - 1, (1 << 64) + 1]

BIN_OPS = ["bvadd", "bvsub", "bvmul", "bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod", "bvand", "bvor",
           "bvxor", "bvshl", "bvlshr", "bvashr"]
CMP_OPS = ["bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge", "bvumul_noovfl"]


def edge_value(rng: random.Random, w: int) -> int:
    m = (1 << w) - 1
    r = rng.random()
    if r < 0.35:
        return rng.choice(EDGE_256) & m
    if r < 0.5:
        return rng.choice([0, 1, m, m - 1, 1 << (w - 1), (1 << (w - 1)) - 1]) & m
    if r < 0.65:
        return rng.getrandbits(min(w, rng.choice([4, 8, 16, 64])))
    return rng.getrandbits(w)


class RandomProgram:
    """A random constraint DAG over scalars, one array and one UF, with a list of
    'interesting' terms to compare value-by-value."""

    def __init__(self, seed: int, n_ops: int = 40, widths=(256, 256, 256, 160, 64, 32, 8, 1 + 7, 257, 512)):
        rng = random.Random(seed)
        self.rng = rng
        self.vars: Dict[int, List[T.Term]] = {}
        pool: Dict[int, List[T.Term]] = {}

        def add(t):
            pool.setdefault(t.width, []).append(t)
            return t

        for i, w in enumerate(widths):
            v = T.BitVecVar(f"v{i}_{w}", w)
            self.vars.setdefault(w, []).append(v)
            add(v)
            add(T.BitVecVal(edge_value(rng, w), w))
        bools: List[T.Term] = [T.BoolVar("flag")]
        arr = T.ArrayVar("Storage", 256, 256)
        fn = T.FuncDecl("keccak256_512", 512, 256)
        terms: List[T.Term] = []
        for _ in range(n_ops):
            kind = rng.random()
            w = rng.choice([256, 256, 256, 64, 160, 8, 32])
            src = pool.get(w) or [T.BitVecVal(0, w)]
            a, b = rng.choice(src), rng.choice(src)
            if kind < 0.45:
                op = rng.choice(BIN_OPS)
                if op in ("bvmul", "bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod", "bvshl", "bvlshr", "bvashr") and w > 256:
                    op = "bvadd"
                t = T.bvbin(op, a, b)
            elif kind < 0.55:
                t = T.bvun(rng.choice(["bvnot", "bvneg"]), a)
            elif kind < 0.65:
                c = T.bvcmp(rng.choice(CMP_OPS), a, b) if w <= 256 else T.eq(a, b)
                bools.append(c)
                terms.append(c)
                continue
            elif kind < 0.72:
                c = rng.choice(bools)
                t = T.ite(c, a, b)
            elif kind < 0.80:
                hi = rng.randrange(w)
                lo = rng.randrange(hi + 1)
                t = T.extract(hi, lo, a)
            elif kind < 0.86:
                w2 = rng.choice([8, 32, 96, 160, 256])
                b2 = rng.choice(pool.get(w2) or [T.BitVecVal(1, w2)])
                t = T.concat(a, b2) if a.width + w2 <= 1024 else a
            elif kind < 0.90:
                k = rng.choice([1, 8, 96, 256])
                t = T.zero_extend(k, a) if rng.random() < 0.5 else T.sign_extend(k, a)
            elif kind < 0.95:
                idx = rng.choice(pool.get(256) or [T.BitVecVal(0, 256)])
                if rng.random() < 0.5:
                    st = T.store(arr, rng.choice(pool[256]), rng.choice(pool[256]))
                    t = T.select(st, idx)
                else:
                    t = T.select(arr, idx)
            else:
                x = rng.choice(pool.get(256))
                y = rng.choice(pool.get(256))
                t = T.app(fn, T.concat(x, y))
            add(t)
            terms.append(t)
        # logical glue
        for _ in range(4):
            x, y = rng.choice(bools), rng.choice(bools)
            c = rng.choice([T.and_(x, y), T.or_(x, y), T.not_(x), T.xor_(x, y), T.eq(x, y)])
            bools.append(c)
            terms.append(c)
        self.terms = terms
        self.bools = bools
        self.root = T.or_(*bools[-3:]) if len(bools) >= 3 else T.BoolVal(True)


def random_assignments(P: ssa.Program, n: int, seed: int):
    rng = random.Random(seed)
    return [[edge_value(rng, c.width) for c in P.coords] for _ in range(n)]


def lift_literals(terms: Sequence[T.Term], min_width: int = 8):
    """Replace every bit-vector literal (width >= min_width) by a fresh variable ``lit<k>``.
    Returns (new terms, {name: value}).  Evaluated with those values as runtime inputs, the
    JIT cannot constant-fold the arithmetic (hipRTC folds literal operands at -O3)."""
    memo: Dict[int, T.Term] = {}
    vals: Dict[str, int] = {}
    for t in T.postorder(list(terms)):
        if t.op == "bvconst" and t.width >= min_width:
            name = f"lit{len(vals)}_{t.width}"
            vals[name] = t.params[0]
            memo[t.id] = T.BitVecVar(name, t.width)
            continue
        args = tuple(memo[a.id] for a in t.args)
        memo[t.id] = t if args == t.args else T.mk(t.op, t.sort, args, t.params)
    return [memo[t.id] for t in terms], vals


def gpu_eval_terms(engine, roots: Sequence[T.Term], watch_terms: Sequence[T.Term], assigns=None, n=64, seed=0,
                   jit: bool = False, asm: bool = False, tiled: bool = False, o3: bool = False):
    """Evaluate on the GPU (the interpreter, or with ``jit`` the compiled eval kernel on the same
    runtime SoA inputs: with watch rows the first tier's by default, ``o3`` the O3 kernel); returns
    (P, assigns, verdicts, per-candidate dict term-id -> value, per-candidate oracle models)."""
    P = ssa.flatten(list(roots), extra=list(watch_terms))
    # watch every requested term that the program contains, plus the model read-back entries
    from mythril_amd.search import model_watch

    for t in watch_terms:
        if t.id not in P.term_node:
            raise KeyError("watch term not in program")
    term_entries = [P.term_node[t.id] for t in watch_terms]
    m_entries, m_widths = model_watch(P)
    entries = term_entries + m_entries
    widths = [P.node_width[e] for e in term_entries] + m_widths
    P.set_watch(entries)
    if assigns is None:
        assigns = random_assignments(P, n, seed)
    soa = ssa.soa_from_assignments(P, assigns)
    prog = engine.load(P.to_bytes())
    try:
        info = engine.info(prog)
        if jit or asm:
            jh = engine.jit_compile(prog, 0, asm=asm, tiled=tiled, o3=o3)
            try:
                from mythril_amd.native import tile_soa

                ver, watch = engine.jit_eval(jh, tile_soa(soa) if tiled else soa, len(assigns),
                                             watch_words=info.watch_words)
            finally:
                engine.jit_free(jh)
        else:
            ver, watch = engine.eval(prog, soa, len(assigns), watch_words=info.watch_words)
    finally:
        engine.free(prog)
    from mythril_amd.search import decode_model, read_rows

    results, models = [], []
    for i in range(len(assigns)):
        vals = read_rows(watch, widths, i)
        tv = {t.id: vals[j] for j, t in enumerate(watch_terms)}
        s, a, f = decode_model(P, vals[len(watch_terms):])
        results.append(tv)
        models.append(OracleModel(s, a, f))
    return P, assigns, ver, results, models


def literal_tail_query():
    """Mapping keys ``Concat(key, slot)`` with literal slots, as LASER addresses storage through
    ``keccak(Concat(key, slot))``: an EQ of an ITE over such keys, two keccak sites with slot 5 and
    one with slot 6 (different literal tails never compare equal)."""
    from mythril_amd.smt import Array, Concat, Function, If, Not, ULT, symbol_factory

    BVV, S = symbol_factory.BitVecVal, symbol_factory.BitVecSym
    a, b, d, e = S("nk_a", 256), S("nk_b", 256), S("nk_d", 256), S("nk_e", 256)
    slot, other = BVV(5, 256), BVV(6, 256)
    k1, k2, k3 = Concat(a, slot), Concat(b, slot), Concat(d, slot)
    h = Function("keccak256_512", 512, 256)
    storage = Array("Storage", 256, 256)
    return [If(ULT(a, b), k1, k2) == k3, Not(a == b),
            ULT(storage[h(k1)], storage[h(k3)] + BVV(3, 256)),
            Not(storage[h(Concat(e, other))] == BVV(0, 256))]


# operators of the first tier (random_tier_program)
_BIN = ["bvadd", "bvsub", "bvmul", "bvand", "bvor", "bvxor"]
_FULL_BIN = ["bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod", "bvshl", "bvlshr", "bvashr"]
_CMP = ["bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge", "bvumul_noovfl"]


def random_tier_program(seed: int, n_ops: int = 36, full: bool = False):
    """Random programs over the first tier's operators (``full``: also symbolic division, remainders,
    shifts, EXP and concrete Keccak): two ORs of random Bools, so verdicts carry information."""
    rng = random.Random(seed)
    pool = {}

    def add(t):
        pool.setdefault(t.width, []).append(t)
        return t

    for i, w in enumerate((256, 256, 160, 64, 32, 8, 1 + 7, 257, 512, 1)):
        if w == 1:
            continue
        add(T.BitVecVar(f"a{seed}_{i}_{w}", w))
        add(T.BitVecVal(edge_value(rng, w), w))
    bools = [T.BoolVar(f"f{seed}")]
    arr = T.ArrayVar("Storage", 256, 256)
    fn = T.FuncDecl("keccak256_512", 512, 256)
    for _ in range(n_ops):
        kind = rng.random()
        w = rng.choice([256, 256, 64, 160, 8, 32, 512])
        src = pool.get(w) or [T.BitVecVal(0, w)]
        a, b = rng.choice(src), rng.choice(src)
        if full and kind < 0.12:
            op = rng.choice(_FULL_BIN)
            t = T.bvbin(op, a, b) if w <= 256 else T.bvbin("bvadd", a, b)  # the lowering's bound
            if w <= 256 and op in ("bvshl", "bvlshr", "bvashr") and rng.random() < 0.6:  # amounts that matter
                t = T.bvbin(op, a, T.bvbin("bvand", b, T.BitVecVal(rng.choice([7, 63, 255, 511]), w)))
        elif full and kind < 0.16:
            t = T.bvexp(a, T.bvbin("bvand", b, T.BitVecVal(rng.choice([3, 15, 255]), w))) if w == 256 else a
        elif full and kind < 0.18 and w in (256, 512):
            t = T.keccak256(a)
        elif kind < 0.35:
            op = rng.choice(_BIN)
            t = T.bvbin(op if not (op == "bvmul" and w > 256) else "bvadd", a, b)
        elif kind < 0.45:
            t = T.bvun(rng.choice(["bvnot", "bvneg"]), a)
        elif kind < 0.60:
            c = T.bvcmp(rng.choice(_CMP), a, b) if w <= 256 else T.eq(a, b)
            bools.append(c)
            continue
        elif kind < 0.68:
            t = T.ite(rng.choice(bools), a, b)
        elif kind < 0.76:
            hi = rng.randrange(w)
            t = T.extract(hi, rng.randrange(hi + 1), a)
        elif kind < 0.82:
            w2 = rng.choice([8, 32, 96, 160, 256])
            b2 = rng.choice(pool.get(w2) or [T.BitVecVal(1, w2)])
            t = T.concat(a, b2) if a.width + w2 <= 1024 else a
        elif kind < 0.88:
            k = rng.choice([1, 8, 96, 256])
            t = T.zero_extend(k, a) if rng.random() < 0.5 else T.sign_extend(k, a)
        elif kind < 0.95:
            idx = rng.choice(pool[256])
            st = T.store(arr, rng.choice(pool[256]), rng.choice(pool[256])) if rng.random() < 0.5 else arr
            t = T.select(st, idx)
        else:
            t = T.app(fn, T.concat(rng.choice(pool[256]), rng.choice(pool[256])))
        add(t)
        if t.width <= 256 and rng.random() < 0.3:
            bools.append(T.eq(t, rng.choice(pool.get(t.width) or [t])))
    for _ in range(3):
        x, y = rng.choice(bools), rng.choice(bools)
        bools.append(rng.choice([T.and_(x, y), T.or_(x, y), T.not_(x), T.xor_(x, y), T.eq(x, y)]))
    # an OR of a few of them: satisfiable by many candidates, so verdicts carry information
    return [T.or_(*rng.sample(bools, min(3, len(bools)))), T.or_(*rng.sample(bools, min(3, len(bools))))]


# ---------------------------------------------------------------------------
# values above 1024 bits and multi-block Keccak (tests/test_wide_cpu.py, tests/test_gpu_wide.py,
# the wide records of tests/test_asm_sim.py)
# ---------------------------------------------------------------------------
# Keccak input lengths in bytes: every partial-word remainder, the word and lane edges, the
# block edge of the rate (135 / 136 / 137, 271 / 272 / 273, 408 = 3 x 136) and several blocks
LENS = (1, 2, 3, 4, 5, 7, 8, 9, 20, 31, 32, 33, 55, 63, 64, 65, 100, 127, 128, 129, 134, 135, 136, 137, 200, 255,
        256, 257, 271, 272, 273, 408, 500, 512)


def lit_bytes(n: int, salt: int = 0) -> T.Term:
    """An ``n``-byte literal with no zero and no repeated neighbouring bytes (a byte read from the
    wrong place changes the digest)."""
    data = bytes(((i * 37 + 11 * salt + 1) % 255) + 1 for i in range(n))
    return T.BitVecVal(int.from_bytes(data, "big"), 8 * n)


def memory_region_queries():
    """SHA3 over a memory region as LASER builds it: a ``Concat`` of literal bytes and symbols of any
    concrete length (``keccak_function_manager.py:59-72``).  {name: (roots, region bytes)}; each root
    is ``ULT(keccak(region), 2^255) OR z == 7`` over the 256-bit symbols x, y and the 8-bit z."""
    from oracle.keccak import keccak256_int

    x, y, z = T.BitVecVar("mr_x", 256), T.BitVecVar("mr_y", 256), T.BitVecVar("mr_z", 8)
    byte = lambda v, i: T.extract(8 * i + 7, 8 * i, v)  # noqa: E731
    # fully constant: a literal whose digest is >= 2^255, so the verdict is z == 7 alone
    salt = next(s for s in range(64) if keccak256_int(lit_bytes(200, s).params[0].to_bytes(200, "big")) >> 255)
    regions = {
        "literal_across_block_edge": T.concat(lit_bytes(4), x, lit_bytes(100, 1), y, lit_bytes(3, 2)),  # 171
        "both_pad_bits_in_one_byte": T.concat(x, lit_bytes(103)),  # 135
        "block0_all_literal": T.concat(lit_bytes(135), z),  # 136
        "one_byte_into_block1": T.concat(z, lit_bytes(136)),  # 137
        "interleaved_bytes": T.concat(byte(x, 0), lit_bytes(1, 3), byte(y, 31), lit_bytes(2, 4), x, lit_bytes(130, 5),
                                      byte(y, 0), lit_bytes(1, 6), byte(x, 1)),  # 170
        "fully_constant": lit_bytes(200, salt),
    }
    out = {}
    for name, region in regions.items():
        root = T.or_(T.bvcmp("bvult", T.keccak256(region), T.BitVecVal(1 << 255, 256)),
                     T.eq(z, T.BitVecVal(7, 8)))
        out[name] = ([root], region.width // 8)
    assert [n for _, n in out.values()] == [171, 135, 136, 137, 170, 200]
    return out


def wide_edge_values(w: int, rng: random.Random, n_random: int = 6):
    """Operand pairs (a, b) at width ``w`` > 1024: the extremes, 2^1024 and its predecessor (the C
    port's old limit), pairs that differ only in limb 0 or only in the top limb, and
    ``2^w - 1, 1`` (a carry through every limb)."""
    m = (1 << w) - 1
    top = 32 * ((w - 1) // 32)  # bit 0 of the top limb
    r = rng.getrandbits(w)
    singles = [0, 1, m, 1 << (w - 1), (1 << (w - 1)) - 1, 1 << 1024, (1 << 1024) - 1]
    pairs = [(a, b) for a in singles for b in (0, 1, m, 1 << (w - 1), (1 << 1024) - 1)]
    pairs += [(r, r ^ 1), (r ^ 1, r), (r, r ^ (1 << top)), (r ^ (1 << top), r), (r, r), (m, 1), (1, m),
              (m - 1, 1), (1 << top, (1 << top) - 1)]
    pairs += [(rng.getrandbits(w), rng.getrandbits(w)) for _ in range(n_random)]
    return pairs


def wide_operator_terms(w: int, a: T.Term = None, b: T.Term = None):
    """Every operator the lowering admits above 256 bits, at width ``w`` over the variables a and b
    (a Bool c for ITE): ADD / SUB / AND / OR / XOR / NOT / NEG, CONCAT / EXTRACT / ZEXT / SEXT, ITE,
    EQ / ULT / ULE / SLT / SLE (and their mirrored forms).  Returns (a, b, c, [terms])."""
    a = a or T.BitVecVar(f"wa{w}", w)
    b = b or T.BitVecVar(f"wb{w}", w)
    c = T.BoolVar(f"wc{w}")
    terms = [T.bvbin(op, a, b) for op in ("bvadd", "bvsub", "bvand", "bvor", "bvxor")]
    terms += [T.bvun("bvnot", a), T.bvun("bvneg", a), T.bvun("bvneg", b)]
    terms += [T.bvcmp(op, a, b) for op in ("bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge")]
    terms += [T.eq(a, b), T.ite(c, a, b)]
    # extracts: 32 bits at the offsets where limbs split (0, 1, 31, 32, 33, W-33, around bit 1024),
    # one bit, and slices that are themselves wider than 1024 bits
    for lo in (0, 1, 31, 32, 33, w - 33, 1023, 1024):
        hi = min(lo + 31, w - 1)
        terms.append(T.extract(hi, lo, a))
    terms += [T.extract(w - 1, w - 1, a), T.extract(1024, 1023, a), T.extract(w - 1, 1, a), T.extract(w - 2, 0, b),
              T.extract(w - 1, 33, T.bvbin("bvadd", a, b))]
    lo_half = T.extract(w // 2 - 1, 0, a)
    hi_half = T.extract(w - 1, w // 2, b)
    terms += [T.concat(hi_half, lo_half), T.eq(T.concat(T.extract(w - 1, w // 2, a), lo_half), a)]
    if w + 64 <= 4096:
        terms += [T.zero_extend(33, a), T.sign_extend(33, a), T.sign_extend(64, T.extract(w - 2, 0, b)),
                  T.concat(a, T.BitVecVal(0xA5, 8)), T.concat(T.BitVecVal(0x5A, 8), b)]
    terms += [T.zero_extend(w - 8, T.extract(7, 0, a)), T.sign_extend(w - 8, T.extract(7, 0, b)),
              T.sign_extend(w - 1025, T.extract(1024, 0, a))]
    return a, b, c, terms


class WideRandomProgram:
    """``RandomProgram`` above 1024 bits: a random DAG over variables of ``widths`` (two of each)
    with the operators the lowering admits there, slices of any width, concatenations up to
    ``max_width``, a UF and concrete Keccak over wide keys.  ``terms`` are compared value by value;
    ``roots`` are two ORs of its Bools."""

    def __init__(self, seed: int, n_ops: int = 40, widths=(1025, 1088, 2048, 4096), max_width: int = 4096):
        rng = random.Random(seed)
        pool: Dict[int, List[T.Term]] = {}

        def add(t):
            pool.setdefault(t.width, []).append(t)
            return t

        for w in widths:
            add(T.BitVecVar(f"w{seed}_a{w}", w))
            add(T.BitVecVar(f"w{seed}_b{w}", w))
            add(T.BitVecVal(rng.choice([1, (1 << w) - 1, 1 << 1024, (1 << 1024) - 1, rng.getrandbits(w)]), w))
        bools: List[T.Term] = [T.BoolVar(f"w{seed}_flag")]
        fns = {w: T.FuncDecl(f"keccak256_{w}", w, 256) for w in widths}
        terms: List[T.Term] = []
        for _ in range(n_ops):
            kind = rng.random()
            w = rng.choice(widths)
            a, b = rng.choice(pool[w]), rng.choice(pool[w])
            if kind < 0.25:
                t = T.bvbin(rng.choice(["bvadd", "bvsub", "bvand", "bvor", "bvxor"]), a, b)
            elif kind < 0.35:
                t = T.bvun(rng.choice(["bvnot", "bvneg"]), a)
            elif kind < 0.55:
                op = rng.choice(["eq", "bvult", "bvule", "bvugt", "bvuge", "bvslt", "bvsle", "bvsgt", "bvsge"])
                c = T.eq(a, b) if op == "eq" else T.bvcmp(op, a, b)
                bools.append(c)
                terms.append(c)
                continue
            elif kind < 0.63:
                t = T.ite(rng.choice(bools), a, b)
            elif kind < 0.75:
                lo = rng.choice([0, 1, 31, 32, 33, 1023, 1024, rng.randrange(w)])
                lo = min(lo, w - 1)
                hi = rng.choice([w - 1, min(w - 1, lo + 31), rng.randrange(lo, w)])
                t = T.extract(hi, lo, a)
            elif kind < 0.83:
                other = rng.choice(pool[rng.choice(sorted(pool))])
                t = T.concat(a, other) if a.width + other.width <= max_width else T.bvbin("bvxor", a, b)
            elif kind < 0.90:
                src_w = rng.choice([x for x in sorted(pool) if x <= w])
                src = rng.choice(pool[src_w])
                t = (T.zero_extend if rng.random() < 0.5 else T.sign_extend)(w - src_w, src)
            elif kind < 0.95:
                t = T.app(fns[w], a)
            else:
                t = T.keccak256(a) if w % 8 == 0 else T.app(fns[w], b)
            add(t)
            terms.append(t)
            if rng.random() < 0.3:
                c = T.eq(t, rng.choice(pool[t.width]))
                bools.append(c)
                terms.append(c)
        self.terms = terms
        self.bools = bools
        self.roots = [T.or_(*rng.sample(bools, min(3, len(bools)))), T.or_(*rng.sample(bools, min(3, len(bools))))]


def keccak_sweep_inputs(nbytes: int, rng: random.Random, n_random: int = 12):
    """Inputs of a Keccak length sweep as integers (big-endian messages): zero, all ones, only the
    first byte 0x01, only the last byte 0x80 (the pad bits' mirror images), and random values."""
    w = 8 * nbytes
    return [0, (1 << w) - 1, 1 << (w - 8), 0x80] + [rng.getrandbits(w) for _ in range(n_random)]


def wide_literal_tail_query():
    """``literal_tail_query`` above 1024 bits: keys ``Concat(key, literal)`` of 1088 bits (a 256-bit
    symbol over an 832-bit literal tail, the shape of a hashed memory region with a symbolic head)
    in an EQ of an ITE, in UF keys with equal and with different tails, and ORs so that verdicts
    carry information."""
    a, b, d, e = (T.BitVecVar(f"wk_{n}", 256) for n in "abde")
    f = T.BoolVar("wk_f")
    tail, other = lit_bytes(104, 7), lit_bytes(104, 8)
    k1, k2, k3 = T.concat(a, tail), T.concat(b, tail), T.concat(d, tail)
    h = T.FuncDecl("keccak256_1088", 1088, 256)
    ult = lambda x, y: T.bvcmp("bvult", x, y)  # noqa: E731
    return [T.or_(T.eq(T.ite(ult(a, b), k1, k2), k3), ult(d, a)),
            T.or_(ult(T.app(h, k1), T.bvbin("bvadd", T.app(h, k3), T.BitVecVal(3, 256))), f),
            T.or_(T.not_(T.eq(T.app(h, T.concat(e, other)), T.app(h, k2))), T.eq(k1, T.concat(e, other)), f)]
