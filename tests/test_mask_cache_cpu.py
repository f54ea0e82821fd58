"""Value numbering of the specialised programs and the first tier's mask cache (CPU, no GPU).

``program.cpp: value_number`` merges the pure instructions of a specialised program that compute
the same value; ``jit_asm.cpp``'s mask cache hands a compare's lane mask (an SGPR pair) out again
instead of issuing the ``v_cmp`` a second time.  Both are exact, so everything here is a comparison
with the C port (``oracle/bveval.c``) on the unspecialised program:

* the specialised programs of the six workloads hold no two pure instructions with one canonical
  key, and keep every verdict on generated candidates of aligned and unaligned 63-bit windows;
* hand-built programs at the shapes where a mask cache can go wrong (``cases``) run through the
  emitter, comgr's assembler and the instruction-level simulator (``tests/asmsim``): ``mgj_gen``
  verdicts per candidate, ``mgj_search`` first hit and hit count with early exit off and on, over
  four 64-candidate groups entered and left mid-group, under the emitter's lifetime checker
  (``MYTHGPU_JIT_ASM_CHECK``), with the cache on, with it off, and with the cache alone merging
  (``MYTHGPU_GVN=0``);
* the LASER-shaped fuzz of ``tests/test_asm_sim.py`` once more with the cache off, and the spill
  configuration (the artificial 72-register file) with the cache on and off.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``).
"""
import json
import multiprocessing as mp
import os
import pickle
import random
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

from mythril_amd import native, search, workloads
from mythril_amd.smt import terms as T
from oracle import cport, kops
from tests.test_asm_sim import (WORKERS, _cached, _fuzz_records, record, run_sim)

ROOT = Path(__file__).resolve().parent.parent
K_LOOKUP = 30
COMMUTATIVE = {kops.K_EQ, kops.K_AND, kops.K_OR, kops.K_XOR, kops.K_ADD, kops.K_MUL}
IMPURE = {kops.K_CONST, kops.K_COORD, kops.K_ASSERT, kops.K_WATCH}


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _cached(tmp_path_factory, sanitize=False)


# ---------------------------------------------------------------------------------------------
# the specialiser
# ---------------------------------------------------------------------------------------------
def canonical_keys(spec):
    """[(key, dst)] of the pure instructions of a specialised program: (op, width, a, b, c, p0, p1)
    with commutative operands in ascending order and a LOOKUP's prior list in place of its offset."""
    out = []
    for r in spec["code"]:
        op, wd, dst, a, b, c, p0, p1 = (int(x) for x in r)
        if op in IMPURE:
            continue
        if op in COMMUTATIVE and a > b:
            a, b = b, a
        if op == K_LOOKUP:
            key = (op, wd, a, b, c, p0, 0) + tuple(int(x) for x in spec["aux"][p1:p1 + 2 * c])
        else:
            key = (op, wd, a, b, c, p0, p1)
        out.append((key, dst))
    return out


VARIANTS = {"search": dict(keep_watch=False, interp=False), "watch": dict(keep_watch=True, interp=False),
            "interp": dict(keep_watch=False, interp=True), "interp_watch": dict(keep_watch=True, interp=True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(workloads.WORKLOADS), ids=workloads.test_id)
def test_value_numbered_program_has_no_repeat_and_keeps_verdicts(name, variant):
    """No two pure instructions of the specialised program share a canonical key, no value is
    asserted twice, and the program gives the C port's verdicts (on the unspecialised program) for
    the generator's own candidates at an aligned and an unaligned 63-bit window."""
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
    pb = P.to_bytes()
    spec = native.specialized_program(pb, blob, **VARIANTS[variant])
    keys = [k for k, _ in canonical_keys(spec)]
    assert len(set(keys)) == len(keys), f"{name}: {len(keys) - len(set(keys))} repeated pure instructions"
    asserted = [int(r[3]) for r in spec["code"] if int(r[0]) == kops.K_ASSERT]
    assert len(set(asserted)) == len(asserted)
    rng = random.Random(zlib.crc32(name.encode()) ^ 0x6A5C)
    widths = [c.width for c in P.coords]
    words = sum((w + 31) // 32 for w in widths)
    n = 256 if name != "sha3_keyed_mapping" else 64
    for start in ((rng.getrandbits(63) & ~63) | (1 << 62), rng.getrandbits(63) | (1 << 62) | 1):
        seed = rng.getrandbits(32)
        soa = cport.gen_soa(pb, blob, seed, start, n, words)
        want = cport.search(pb, blob, seed, start, n, threads=4, verdicts=True)[2]
        got = kops.verdicts(spec, soa, widths, n)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}/{variant}: verdict differs at index {start + int(bad[0])} (seed {seed})"


def _in_child(code: str, payload, env: dict) -> str:
    """Run ``code`` (reads the pickled payload on stdin) in a fresh interpreter: the native library
    reads its switches once per process."""
    r = subprocess.run([sys.executable, "-c", code], input=pickle.dumps(payload), capture_output=True,
                       env=dict(os.environ, **env), cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode()


_SPEC_COUNTS = """
import pickle, sys, json
from mythril_amd import native
out = {}
for name, (pb, blob) in pickle.loads(sys.stdin.buffer.read()).items():
    out[name] = [len(native.specialized_program(pb, blob, interp=i)["code"]) for i in (False, True)]
print(json.dumps(out))
"""


def test_value_numbering_fires_and_has_a_switch():
    """C2's compiled program holds one EQ twice and C4's nine repeated instructions (the compare
    pushdown's EQ(v_q, x) per prior, LASER's injectivity conditions per site): with MYTHGPU_GVN=0
    the programs are that much longer, and never shorter."""
    progs = {}
    for name in sorted(workloads.WORKLOADS):
        P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
        progs[name] = (P.to_bytes(), blob)
    on = json.loads(_in_child(_SPEC_COUNTS, progs, {"MYTHGPU_GVN": "1"}))
    off = json.loads(_in_child(_SPEC_COUNTS, progs, {"MYTHGPU_GVN": "0"}))
    for name in progs:
        assert all(a <= b for a, b in zip(on[name], off[name])), (name, on[name], off[name])
    assert off["token_transfer_underflow"][0] - on["token_transfer_underflow"][0] >= 1
    assert off["walletlibrary_kill"][0] - on["walletlibrary_kill"][0] >= 9


# ---------------------------------------------------------------------------------------------
# the mask cache: hand-built programs
# ---------------------------------------------------------------------------------------------
W = 256
A1, A2, A3 = search.ACTORS
VALS = [A1, A2, A3]


def _v(name, w=W):
    return T.BitVecVar(name, w)


def _k(v, w=W):
    return T.BitVecVal(v % (1 << w), w)


def _ult(a, b):
    return T.bvcmp("bvult", a, b)


def _coin(name):
    """True for about half the candidates: keeps the conjunction of a case's roots satisfiable
    for a fair share of them, so a wrong mask shows as a wrong verdict."""
    return _ult(_v(name, 32), _k(0xC0000000, 32))


def _prepare(roots, shape):
    """(P, generator blob): ``shape(g, coord index by name)`` replaces the propagated generator
    specs of the coordinates the case is about."""
    P, _ = search.prepare(roots)
    g = search.default_generator(P, roots=roots)
    shape(g, {c.name: c.index for c in P.coords})
    return P, g.blob()


def case_eq_two_asserts_mixed_between():
    """(1) One EQ read by two ASSERTs and by a UF's key test, with a MIXED coordinate of all four
    alternatives (COPY, DICT, SMALL, UNIFORM) and a delta generated between them."""
    a, b, m = _v("mc1_a"), _v("mc1_b"), _v("mc1_m")
    f = T.FuncDecl("mc1_f", W, W)
    e = T.eq(a, b)
    roots = [T.or_(e, _coin("mc1_x")),
             T.or_(T.eq(m, a), _ult(m, _k(1 << 255)), _coin("mc1_y")),
             T.or_(e, _coin("mc1_z")),
             T.or_(_ult(T.app(f, b), T.app(f, a)), e, _coin("mc1_u"))]

    def shape(g, ix):
        g.dict(ix["mc1_a"], VALS)
        g.dict(ix["mc1_b"], VALS)
        lo, hi = sorted((ix["mc1_a"], ix["mc1_m"]))
        assert hi == ix["mc1_m"], "the MIXED coordinate copies an earlier one"
        g.mixed(ix["mc1_m"], VALS, p_dict=0.25, copy_from=ix["mc1_a"], p_copy=0.25, p_delta=0.5, small_bits=8,
                p_small=0.25)

    return _prepare(roots, shape)


def case_compare_in_conditional_region():
    """(2) Compares first emitted inside conditional regions — the body of a division by a
    dictionary-drawn divisor (its high limbs against zero), a MIXED alternative's clamp, an EXP —
    and needed again after the join."""
    x, d, m, s = _v("mc2_x"), _v("mc2_d"), _v("mc2_m"), _v("mc2_s", 8)
    hi = T.extract(255, 32, d)
    zero_hi = T.eq(hi, _k(0, 224))
    p = T.bvexp(_k(3), T.zero_extend(248, s))
    roots = [T.or_(_ult(T.bvbin("bvudiv", x, d), _k(1 << 200)), _coin("mc2_c0")),
             T.or_(zero_hi, _coin("mc2_c1")),
             T.or_(T.eq(m, _k(5)), _ult(_k(40), m), _coin("mc2_c2")),
             T.or_(T.eq(m, _k(5)), zero_hi, _coin("mc2_c3")),
             T.or_(_ult(p, _k(1 << 100)), T.eq(d, _k(7)), _coin("mc2_c4")),
             T.or_(T.eq(d, _k(7)), _coin("mc2_c5"))]

    def shape(g, ix):
        g.dict(ix["mc2_d"], [0, 7, 1 << 200, (1 << 64) + 3])
        g.mixed(ix["mc2_m"], [5, 9, 70], p_dict=0.5, p_delta=0.5, small_bits=6, p_small=0.25, clamp=(3, 60))

    return _prepare(roots, shape)


def case_operand_dies_register_reused():
    """(3) a and b compared, a dies, a new value takes a's registers and is compared with b: not the
    cached mask.  The same for a dictionary index register that is reused."""
    a, b, c = _v("mc3_a"), _v("mc3_b"), _v("mc3_c")
    a2, c2 = _v("mc3_a2"), _v("mc3_c2")
    roots = [T.or_(T.eq(a, b), _coin("mc3_x")),
             T.or_(T.eq(c, b), _coin("mc3_y")),
             T.or_(T.eq(a2, _k(A2)), _coin("mc3_z")),
             T.or_(T.eq(c2, _k(A2)), _coin("mc3_u")),
             T.or_(T.eq(c2, _k(A2)), T.eq(c, b), _coin("mc3_v"))]

    def shape(g, ix):
        for n in ("mc3_a", "mc3_c"):
            g.mixed(ix[n], VALS, p_dict=0.7, small_bits=2, p_small=0.2)
        g.dict(ix["mc3_b"], VALS)
        for n in ("mc3_a2", "mc3_c2"):
            g.dict(ix[n], VALS)

    return _prepare(roots, shape)


def case_more_bools_than_sgpr_pairs(n=36):
    """(4) More live Bools than SGPR pairs (28): an array read at n symbolic keys — canonicalising
    LOOKUPs of up to n - 1 priors, each key compared with every earlier one, the VMTests
    ``calldataload*`` read-backs' shape cut down — between the first and the last use of n Bools.
    The cache fills with the key tests' masks, which are evicted when the pairs run out, and then
    live Bools move to their VGPR form."""
    arr = T.ArrayVar("mc4_cd", 64, 8)
    keys = [_v(f"mc4_k{i}", 64) for i in range(n)]
    bools = [_ult(k, _k(3 + i % 2, 64)) for i, k in enumerate(keys)]
    rng = random.Random(4)
    acc = _k(0, 32)
    for k in keys:
        acc = T.bvbin("bvadd", acc, T.bvbin("bvmul", T.zero_extend(24, T.select(arr, k)), _k(rng.getrandbits(32), 32)))
    last = [T.xor_(bools[i], bools[(i + 7) % n]) for i in range(n)]
    roots = [T.or_(*bools),
             T.or_(T.eq(keys[0], keys[1]), _coin("mc4_c0")),
             T.or_(T.eq(T.extract(1, 0, acc), _k(1, 2)), T.eq(keys[0], keys[1]), _coin("mc4_c1")),
             T.or_(T.and_(*last[:n // 2]), T.and_(*last[n // 2:]), T.eq(keys[2], keys[1]), _coin("mc4_c2"))]

    def shape(g, ix):
        for i in range(n):
            g.dict(ix[f"mc4_k{i}"], [1 + i % 3, 7, 1 << 40])

    return _prepare(roots, shape)


def case_cached_mask_consumers():
    """(5) A cached mask consumed by NOT, by a Bool ITE's else side, by a Bool lookup with a literal
    default (LASER's keccak bookkeeping of two mapping slots keyed by a and b, whose key test is the
    compare of a and b again) and by ASSERT, then read again.  The consumers read EQ(b, a), the
    first root EQ(a, b): one value when the specialiser merges them, a cache hit each with
    MYTHGPU_GVN=0."""
    from mythril_amd.keccak_model import KeccakFunctionManager
    from mythril_amd.smt import Array, symbol_factory

    km = KeccakFunctionManager()
    storage = Array("mc5_storage", 256, 256)
    A, B = symbol_factory.BitVecSym("mc5_a", 256), symbol_factory.BitVecSym("mc5_b", 256)
    conds = []
    ka = workloads.mapping_slot(km, A, 1, conds)
    kb = workloads.mapping_slot(km, B, 1, conds)
    a, b = A.raw, B.raw
    e, e2 = T.eq(a, b), T.eq(b, a)
    q = _coin("mc5_q")
    roots = [T.or_(e, _coin("mc5_c0")),
             T.or_(T.not_(e2), _coin("mc5_c1")),
             T.or_(T.ite(q, _coin("mc5_c2"), e2), _coin("mc5_c3")),
             T.or_(_ult(storage[ka].raw, storage[kb].raw), e2, _coin("mc5_c4"))]
    roots += [c.raw for c in conds]
    roots += [e2, T.or_(T.xor_(e2, q), _coin("mc5_c5")), T.or_(e, T.eq(b, _k(A3)))]

    def shape(g, ix):
        g.dict(ix["mc5_a"], VALS)
        g.dict(ix["mc5_b"], VALS)

    return _prepare(roots, shape)


def case_same_eq_twice():
    """(6) The same EQ twice in the program (operands swapped; one more behind a UF's key test): with
    MYTHGPU_GVN=0 the cache alone merges them."""
    a, b = _v("mc6_a"), _v("mc6_b")
    one = T.eq(a, b)
    two = T.eq(b, a)
    roots = [T.or_(one, _coin("mc6_x")), T.or_(T.not_(two), _coin("mc6_y")), T.or_(two, one, _coin("mc6_z"))]

    def shape(g, ix):
        g.mixed(ix["mc6_a"], VALS, p_dict=0.8, p_delta=0.3)
        g.mixed(ix["mc6_b"], VALS, p_dict=0.8, p_delta=0.3)

    return _prepare(roots, shape)


def cases():
    return {"eq_two_asserts_mixed_between": case_eq_two_asserts_mixed_between(),
            "compare_in_conditional_region": case_compare_in_conditional_region(),
            "operand_dies_register_reused": case_operand_dies_register_reused(),
            "more_bools_than_sgpr_pairs": case_more_bools_than_sgpr_pairs(),
            "cached_mask_consumers": case_cached_mask_consumers(),
            "same_eq_twice": case_same_eq_twice()}


CASE_ENVS = {"cache": {}, "no_cache": {"MYTHGPU_JIT_ASM_NO_MASK_CACHE": "1"}, "no_gvn": {"MYTHGPU_GVN": "0"},
             "neither": {"MYTHGPU_JIT_ASM_NO_MASK_CACHE": "1", "MYTHGPU_GVN": "0"}}
START, COUNT = (1 << 40) + 5, 200  # four 64-candidate groups, entered and left mid-group


@pytest.mark.parametrize("env", sorted(CASE_ENVS))
def test_mask_cache_cases_on_the_simulator(sim, env):
    """Every case, assembled by comgr and simulated: per-candidate verdicts, first hit and hit count
    (early exit off and on) equal the C port's, under the lifetime checker; each case has both
    verdicts among its candidates."""
    rng = random.Random(0xCAC4E)
    recs, names = [], []
    for name, (P, blob) in cases().items():
        pb = P.to_bytes()
        for seed in (rng.getrandbits(32), rng.getrandbits(32)):
            want = cport.search(pb, blob, seed, START, COUNT, threads=2, verdicts=True)[2]
            assert 0 < int(want.sum()) < COUNT, (name, int(want.sum()))
            recs.append(record(0, pb, blob, seed, START, COUNT, flags=1))
            names.append(name)
    rc, summary, bad, err = run_sim(sim, b"".join(recs), dict(CASE_ENVS[env], MYTHGPU_JIT_ASM_CHECK="1"))
    assert rc == 0 and summary, f"{summary}\n" + "\n".join(bad[:8]) + "\n" + err[-3000:]
    assert int(summary["ok"]) == len(recs), (summary, bad[:8])


_ASM = """
import pickle, sys, json, re
from mythril_amd import native
out = {}
for name, (pb, blob) in pickle.loads(sys.stdin.buffer.read()).items():
    src = native.jit_asm(pb, blob)
    note = re.findall(r"; mask cache: (\\d+) hits, (\\d+) evictions, (\\d+) mask spills", src)
    out[name] = {"notes": [[int(x) for x in n] for n in note], "v_cmp": src.count("v_cmp_")}
print(json.dumps(out))
"""


def test_mask_cache_counters():
    """The emitter's counters (the comment after each kernel's last instruction): the cases built
    around a repeated compare hit; (4) evicts cache entries and then spills masks; with the cache
    off nothing hits and no case issues fewer compares than with it on; (6) with MYTHGPU_GVN=0
    hits, so the cache alone merges the repeated EQ."""
    progs = {name: (P.to_bytes(), blob) for name, (P, blob) in cases().items()}
    on = json.loads(_in_child(_ASM, progs, {"MYTHGPU_JIT_ASM_CHECK": "1"}))
    off = json.loads(_in_child(_ASM, progs, {"MYTHGPU_JIT_ASM_CHECK": "1", "MYTHGPU_JIT_ASM_NO_MASK_CACHE": "1"}))
    nogvn = json.loads(_in_child(_ASM, progs, {"MYTHGPU_JIT_ASM_CHECK": "1", "MYTHGPU_GVN": "0"}))
    hits = lambda d, name: sum(n[0] for n in d[name]["notes"])  # noqa: E731
    for name in progs:
        assert on[name]["notes"] and hits(off, name) == 0, name
        assert on[name]["v_cmp"] <= off[name]["v_cmp"], name
    for name in ("eq_two_asserts_mixed_between", "cached_mask_consumers"):
        assert hits(on, name) > 0 and on[name]["v_cmp"] < off[name]["v_cmp"], (name, on[name], off[name])
    assert hits(nogvn, "same_eq_twice") > 0 and hits(nogvn, "cached_mask_consumers") > hits(on, "cached_mask_consumers")
    big = on["more_bools_than_sgpr_pairs"]["notes"]
    assert sum(n[1] for n in big) > 0 and sum(n[2] for n in big) > 0, big


# ---------------------------------------------------------------------------------------------
# the fuzz of tests/test_asm_sim.py, cache off; the spill configuration
# ---------------------------------------------------------------------------------------------
FUZZ_ENVS = {"no_cache": {"MYTHGPU_JIT_ASM_NO_MASK_CACHE": "1"}, "small_file": {"MYTHGPU_JIT_ASM_SPILL_TEST": "72"}}


def _fuzz_worker(args):
    exe, lo, hi, env = args
    rc, summary, bad, err = run_sim(Path(exe), _fuzz_records(lo, hi), dict(FUZZ_ENVS[env], MYTHGPU_JIT_ASM_CHECK="1"))
    return rc, summary, bad[:5], err[-3000:]


@pytest.mark.parametrize("env", sorted(FUZZ_ENVS))
def test_laser_fuzz_once_more(sim, env):
    """The 10,000 LASER-shaped queries of ``test_asm_tier_laser_fuzz_under_asan`` (which runs them
    with the cache on) once more with MYTHGPU_JIT_ASM_NO_MASK_CACHE=1 — the switch leaves a correct
    emitter behind — and with the cache on under the artificial 72-register file, where a kernel
    that does not fit is refused (outside the tier) and every other one is right."""
    n = int(os.environ.get("MYTHGPU_SIMFUZZ_N", "10000"))
    step = max(1, n // (WORKERS * 4))
    tasks = [(str(sim), lo, min(n, lo + step), env) for lo in range(0, n, step)]
    with mp.get_context("fork").Pool(WORKERS) as pool:
        results = pool.map(_fuzz_worker, tasks, chunksize=1)
    total = {"records": 0, "ok": 0, "outside": 0}
    for rc, summary, bad, err in results:
        assert summary and rc == 0, f"{summary}\n" + "\n".join(bad) + "\n" + err
        for k in total:
            total[k] += int(summary[k])
    assert total["records"] == n, total
    if env == "no_cache":
        assert total["ok"] == n, total
    else:
        assert total["ok"] + total["outside"] == n and total["ok"] >= n // 2, total


@pytest.mark.parametrize("cache", ["cache", "no_cache"])
def test_search_and_eval_under_the_small_register_file(sim, cache):
    """The spill configuration of ``test_asm_eval_spills_sim`` (an artificial 72-register file, so
    values go to LDS and come back while masks sit in the cache) on eval and search kernels: the
    workloads, the hand-built cases and random tier programs; a kernel the spiller cannot fit is
    refused, never wrong."""
    from tests.helpers import random_tier_program

    rng = random.Random(9)
    recs = []
    for name in ("walletlibrary_kill", "token_transfer_underflow", "etherstore_reentrancy"):
        P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
        recs.append(record(0, P.to_bytes(), blob, rng.getrandbits(32), START, COUNT))
        prev = P.watch
        P.set_watch([])
        pe = P.to_bytes()
        P.set_watch(prev)
        recs += [record(kind, pe, None, rng.getrandbits(32), 0, 64 * 2 + 9) for kind in (1, 2)]
    for name, (P, blob) in cases().items():
        recs.append(record(0, P.to_bytes(), blob, rng.getrandbits(32), START, COUNT))
    for s_ in range(24):
        P, blob = search.prepare(random_tier_program(41_000 + s_, full=bool(s_ & 1)))
        recs.append(record(0, P.to_bytes(), blob, rng.getrandbits(32), rng.getrandbits(63), 192))
        prev = P.watch
        P.set_watch([])
        recs.append(record(1 + (s_ & 1), P.to_bytes(), None, rng.getrandbits(32), 0, 64 * 2 + 5))
        P.set_watch(prev)
    env = dict(CASE_ENVS[cache], MYTHGPU_JIT_ASM_CHECK="1", MYTHGPU_JIT_ASM_SPILL_TEST="72")
    rc, summary, bad, err = run_sim(sim, b"".join(recs), env)
    assert rc == 0 and summary, err[-3000:]
    assert summary["mismatch"] == "0" and summary["simerror"] == "0" and summary["asmerror"] == "0", (summary, bad[:5])
    assert int(summary["ok"]) >= len(recs) // 2, summary
