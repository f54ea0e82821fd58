"""Generator representations crossed with the operators that read them, on the CPU: the table and
the fuzz of ``tests/gen_repr_cases.py``.

Layer by layer, so that a failure names the layer: the C port's generated limbs against the
big-integer restatement (``tests/gen3_ref.py``); the specialised program (both lowerings) in the
oracle's evaluator of device ops against the C port on the unspecialised program; the first tier
in the instruction-level simulator (``mgj_gen`` verdicts, ``mgj_search`` first hit and hit count,
early exit off and on) under the emitter's lifetime checker, the table under every configuration of
``test_asm_sim.CONFIGS`` and with the LDS staging and the guarded regions off; the O3 tier's host
compile.  The corpus conditions (hits and misses in every window; all-false, mixed and all-true
groups of every guarded condition) are asserted from the C port alone before a tier is looked at.

Teeth: an emitter with the packed 32-bit dictionary put back (``v_bfe_u32`` with a field width of 32
reads as 0: every lane got 0) fails on the table's (32, 1) shapes and on the fuzz; one whose else-arm
select has its operands flipped fails on the fuzz; one whose region leaks a register is an
assembly error under the checker, not a silent retry without regions.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``)."""
import multiprocessing as mp
import re
from pathlib import Path

import numpy as np
import pytest

from mythril_amd import native
from oracle import cport, kops
from tests import gen3_ref as R
from tests import gen_repr_cases as G
from tests.test_asm_sim import CONFIGS, WORKERS, _mutants, record, run_sim, sim  # noqa: F401  (sim: fixture)

WINDOWS = [(G.ALIGNED, G.SIM_COUNT), (G.ODD, G.SIM_COUNT)]
TABLE_ENVS = CONFIGS + [{"MYTHGPU_JIT_ASM_NO_LDS": "1"}, {"MYTHGPU_JIT_ASM_NO_LAZY": "1"}]
CHECK = {"MYTHGPU_JIT_ASM_CHECK": "1"}
# The pools here start fresh interpreters ("spawn"): their workers call into the native library and
# the C port, and a fork of a test process whose earlier tests left threads behind can inherit a held lock.
PACKED32 = {"mythril_amd/csrc/jit_asm.cpp": ("if (w < 32 && n && (uint64_t)n * w <= 32) {",
                                             "if (w <= 32 && n && (uint64_t)n * w <= 32) {")}
ELSE_FLIP = {"mythril_amd/csrc/jit_asm.cpp": (
    "const std::string f = rg.true_arm ? VL(rg.r[j]) : src(a), t = rg.true_arm ? src(a) : VL(rg.r[j]);",
    "const std::string f = VL(rg.r[j]), t = src(a);")}
LEAK = {"mythril_amd/csrc/jit_asm.cpp": ("SP(m.s), {m.s, m.s + 1});\n      drop(a);\n    }\n  }\n  void region_close",
                                         "SP(m.s), {m.s, m.s + 1});\n    }\n  }\n  void region_close")}


def _records(case, n_done=None, assemble=True):
    """The case's two windows as search records after the corpus conditions; through comgr's
    assembler as well: every table record, every 25th of a fuzz run (``n_done``); never for a mutant
    driver, built without the assembler."""
    seed = G.seed_of(case)
    recs = []
    for k, (start, count) in enumerate(WINDOWS):
        assert G.window_ok(case, seed, start, count), (case.name, seed, hex(start))
        recs.append(record(0, case.pb, case.blob, seed, start, count, flags=int(assemble and (n_done is None or (n_done + k) % 25 == 0))))
    return recs


# ---- the reference itself, and the specialiser ---------------------------------------------------


@pytest.mark.parametrize("wc", sorted(G.WIDTH_CLASSES))
def test_c_port_generates_the_restatements_limbs(wc):
    """Every limb of every coordinate of the compare programs (x, its twin, the COPY sources): the C
    port against the big-integer restatement, two groups from each start."""
    for name in G.program_names():
        if not name.startswith(wc + "_cmp_"):
            continue
        c = G.program(name)
        specs, consts = R.split_blob(c.blob)
        widths = [co.width for co in c.P.coords]
        for start in (G.ALIGNED, G.ODD):
            got = cport.gen_soa(c.pb, c.blob, G.seed_of(c), start, 128, c.words()).astype(np.uint64)
            want = np.array([R.soa_rows(R.gen_values(specs, consts, widths, G.seed_of(c), start + q), widths)
                             for q in range(128)], dtype=np.uint64).T
            bad = np.argwhere(got != want)
            assert bad.size == 0, (name, hex(start), "row, candidate:", bad[:4].tolist())


def _spec_worker(name):
    c = G.program(name)
    native.check_program_gen(c.pb, c.blob)
    widths = [co.width for co in c.P.coords]
    progs = {interp: native.specialized_program(c.pb, c.blob, interp=interp) for interp in (False, True)}
    same = all(np.array_equal(progs[False][k], progs[True][k]) for k in ("code", "consts", "aux"))
    seed = G.seed_of(c)
    out = []
    for start, count in WINDOWS:
        soa = cport.gen_soa(c.pb, c.blob, seed, start, count, c.words())
        want = cport.search(c.pb, c.blob, seed, start, count, verdicts=True)[2]
        for interp, spec in progs.items():
            if interp and same:
                continue
            bad = np.flatnonzero(kops.verdicts(spec, soa, widths, count) != want)
            if bad.size:
                out.append((name, interp, hex(start), int(bad.size), bad[:4].tolist()))
    return out


def test_specialised_programs_keep_every_verdict():
    """kops on the specialised program (both lowerings) == the C port on the unspecialised one, every
    table program, both windows: the layer above the emitters is sound on these generators."""
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        bad = sum(pool.map(_spec_worker, G.program_names(), chunksize=1), [])
    assert not bad, bad[:8]


# ---- the first tier on the simulator -------------------------------------------------------------


def _table_worker(args):
    exe, names, env, assemble = args
    recs = []
    for name in names:
        recs += _records(G.program(name), assemble=assemble)
    rc, summary, bad, err = run_sim(Path(exe), b"".join(recs), dict(env, **CHECK))
    return rc, summary, bad[:6], err[-2000:], len(recs), env


def _run_table(exe, envs, names=None, assemble=True):
    names = names or G.program_names()
    step = (len(names) + WORKERS - 1) // WORKERS
    tasks = [(str(exe), names[lo:lo + step], env, assemble) for env in envs for lo in range(0, len(names), step)]
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        return pool.map(_table_worker, tasks, chunksize=1)


def _all_ok(results):
    for rc, summary, bad, err, n, env in results:
        assert summary, (rc, env, err)
        assert rc == 0 and int(summary["ok"]) == n == int(summary["records"]), (env, summary, bad, err)


@pytest.mark.parametrize("env", range(len(TABLE_ENVS)), ids=["config0", "config1", "config2", "config3", "no_lds", "no_lazy"])
def test_table_on_the_simulator(sim, env):  # noqa: F811
    """Every table program, both windows: all ``ok`` (inside the tier, no mismatch, no simulator rule
    broken, no lifetime violation)."""
    _all_ok(_run_table(sim, [TABLE_ENVS[env]]))


def _fuzz_worker(args):
    exe, lo, hi, env, assemble = args
    recs = []
    for s in range(lo, hi):
        recs += _records(G.fuzz_case(s), len(recs), assemble)
    rc, summary, bad, err = run_sim(Path(exe), b"".join(recs), dict(env, **CHECK))
    return rc, summary, bad[:6], err[-2000:], len(recs), env


def _run_fuzz(exe, n, envs=CONFIGS, assemble=True):
    step = max(1, n // (WORKERS * 4))
    tasks = [(str(exe), lo, min(n, lo + step), envs[(lo // step) % len(envs)], assemble) for lo in range(0, n, step)]
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        return pool.map(_fuzz_worker, tasks, chunksize=1)


def test_fuzz_on_the_simulator(sim):  # noqa: F811
    """1,000 fuzz programs spread over the four configurations, both windows each."""
    _all_ok(_run_fuzz(sim, G.N_FUZZ_SIM))


def _regions_worker(args):
    lo, hi = args
    out = []
    for s in range(lo, hi):
        c = G.fuzz_case(s)
        src = native.jit_asm(c.pb, c.blob)
        out.append(sum(int(x) for x in re.findall(r"; lazy arms: (\d+) guarded regions", src)) > 0)
    return out


def test_fuzz_exercises_the_guarded_regions():
    """At least three quarters of the fuzz programs emit a guarded region (the ``lazy arms`` comment
    of the emitted text), at the default threshold."""
    n = G.N_FUZZ_SIM
    step = (n + WORKERS - 1) // WORKERS
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        got = sum(pool.map(_regions_worker, [(lo, min(n, lo + step)) for lo in range(0, n, step)]), [])
    print("fuzz programs with a guarded region:", sum(got), "of", n)
    assert sum(got) >= 0.75 * n, (sum(got), n)


# ---- the O3 tier: host compile ---------------------------------------------------------------------


def _o3_worker(name):
    c = G.program(name)
    return name, "mgj_search" in native.jit_source(c.pb, c.blob, compile=True)


def test_o3_tier_compiles_every_table_program_on_the_host():
    """No refusal to meet on the GPU (its verdicts are the GPU tests' matter)."""
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        got = pool.map(_o3_worker, G.program_names(), chunksize=1)
    assert all(ok for _, ok in got), [n for n, ok in got if not ok]


def test_table_covers_the_thresholds():
    """What the table promises, from the shapes alone."""
    pairs = {(s.w, len(s.values)) for s in G.shapes() if s.how == "dict"}
    assert pairs >= set(G.DICT_PAIRS)
    for how in ("dict", "mixed", "copy"):
        assert {(s.w, len(s.values)) for s in G.shapes() if s.how == how} == pairs
    assert {s.w for s in G.shapes() if s.how == "fixall"} == set(G.CONST_WIDTHS)
    for s in G.shapes():
        if s.how == "dict":
            assert s.values[0] >> (s.w - 1) == 1  # the top bit of the width
    used = [s.name for n in G.program_names() for s in G.shapes_of(n)]
    assert sorted(used) == sorted([s.name for s in G.shapes()] * len(G.FAMILIES))


# ---- teeth -----------------------------------------------------------------------------------------


def test_the_table_and_the_fuzz_have_teeth(sim, tmp_path):  # noqa: F811
    """The packed 32-bit dictionary put back fails on every w32 program (they hold the (32, 1)
    shapes) and on the fuzz; flipped else-arm select operands fail on the fuzz; a register leaked
    inside a region is an assembly error under the checker.  The unedited driver passes the same
    records (``test_table_on_the_simulator``, ``test_fuzz_on_the_simulator`` and here)."""
    exes = _mutants(tmp_path, {"packed32": PACKED32, "else_flip": ELSE_FLIP, "leak": LEAK})
    w32 = [n for n in G.program_names() if n.startswith("w32_")]
    assert all(any(s.w == 32 and len(s.values) == 1 and s.how == "dict" for s in G.shapes_of(n)) for n in w32)
    _all_ok(_run_table(sim, [{}], w32))
    failed = 0
    for rc, summary, bad, err, n, env in _run_table(exes["packed32"], [{}], w32, assemble=False):
        assert summary and rc != 0, (summary, err)
        failed += int(summary["mismatch"])
    print("packed32 mutant: table records with wrong verdicts:", failed, "of", 2 * len(w32))
    assert failed == 2 * len(w32), failed
    n = 200
    _all_ok(_run_fuzz(sim, n))
    for name in ("packed32", "else_flip"):
        wrong = sum(int(r[1]["mismatch"]) + int(r[1]["simerror"]) for r in _run_fuzz(exes[name], n, assemble=False) if r[1])
        print(name, "mutant: fuzz records that fail:", wrong, "of", 2 * n)
        assert wrong > 0, name
    leaks = _run_fuzz(exes["leak"], 40, envs=[{}], assemble=False)
    errors = sum(int(r[1]["asmerror"]) for r in leaks)
    print("leak mutant: fuzz records refused as emitter errors:", errors, "of", 80)
    assert errors >= 40, [(r[1], r[2]) for r in leaks]  # (920 of 1,000 fuzz programs hold a region)
    assert any("internal: VGPR" in line or "internal: v" in line for r in leaks for line in r[2]), leaks[0][2]
