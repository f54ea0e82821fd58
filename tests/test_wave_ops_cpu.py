"""The wave table of ``tests/wave_op_cases.py`` on the CPU.

* Its self-check, per width: every decision value the table promises is reached, from the Python
  restatements alone.
* The C port (``oracle/bveval.c``, explicit assignments, watch rows) against the big-integer oracle
  (``oracle/bv.py``), value for value, on every wave of every width.
* Generator form (DICT coordinates that pin a profile): between 1/8 and 7/8 of each window satisfy
  the root under the C port; the first tier in the instruction-level simulator under the emitter's
  lifetime checker, and the O3 tier's compiled kernels in the same simulator, against the C port
  (``mgj_gen`` verdicts, ``mgj_search`` first hit and hit count), as ``tests/test_asm_sim.py`` and
  ``tests/test_o3_sim_cpu.py`` do (their driver takes generator-mode records only).
* Teeth: five planted bugs, applied to scratch copies of the sources by ``test_asm_sim._mutants``,
  each fail named cases (the docstrings of the two ``test_planted_*`` tests): the second correction
  removed from ``div_one_limb`` and from ``udivrem8``, the ``c != 0`` term dropped from
  ``udivrem_nb``, ``& ~1u`` dropped from ``bv_exp``'s ``skip``, NB one class too small in the first
  tier's ``udivrem``.  The ``bv_device.h`` ones reach the simulator through the O3 tier's prelude,
  which ``mythril_amd/build.py`` generates from that header.

Reference anchor: a term's value is ``Model.eval(term, model_completion=True)``
(``mythril/laser/smt/model.py:45-59``)."""
import pytest

from oracle import cport
from tests import wave_op_cases as W


@pytest.mark.parametrize("w", W.WIDTHS)
def test_table_reaches_every_decision(w):
    """EXP: every maximum exponent length as a uniform wave, a mixed wave and with the single long
    lane at lane 0 and at lane 63, each with the live limbs, m, skip and steps it implies.  Division:
    every divisor class alone, with one outlier and mixed with zero divisors; all three paths; NB = 2,
    4 and 8 (1, 2, 4 and all limbs in the first tier); every quotient length alone and mixed; the
    loop's carry at NB = 2 and 4 (none at the full width: module docstring); every combination of the
    2/1 step's corrections at every limb position but the second correction at the top one; a
    wrapping candidate sum; the literal divisors' multiples and neighbours; the signed edges; the
    shift amounts; the multiply edges."""
    s = W.check_width(w)
    print("width", w, "waves:", s["waves"], "correction combinations by limb position:", s.get("mg", {}).get(w))
    assert s["waves"] == len(W.waves(w)) >= 16


def test_restated_step_is_exact():
    """The restated 2/1 step divides exactly (every 6-bit step, 200,000 random 32-bit ones) and all
    four correction combinations occur among the random steps."""
    seen = W._steps_are_exact()
    print("random 2/1 steps by corrections:", seen)
    assert set(seen) == set(W.COMBOS)


def test_table_size():
    assert sum(len(W.waves(w)) for w in W.WIDTHS) >= 500


@pytest.mark.parametrize("w", W.WIDTHS)
def test_c_port_matches_the_oracle_on_every_wave(w):
    p = W.program(w)
    ver, watch = cport.eval_soa(p.pb, p.soa, p.n, watch_words=p.watch_words)
    assert ver.all()
    assert not p.mismatches(watch), (w, p.mismatches(watch))


# ---- generator form: the C port's share, the first tier on the simulator, planted bugs -----------------

import multiprocessing as mp  # noqa: E402
from pathlib import Path  # noqa: E402

from tests.test_asm_sim import WORKERS, _mutants, record, run_sim, sim  # noqa: E402,F401  (sim: fixture)

CHECK = {"MYTHGPU_JIT_ASM_CHECK": "1"}
# jit_asm.cpp mutants (tests/test_asm_sim._mutants, as tests/test_gen_repr_cpu.py pins its three)
NO_SECOND_CORRECTION = {"mythril_amd/csrc/jit_asm.cpp": (
    'VL(rr) + ", " + VL(dn));\n      vsel(q1, q1, t, M);\n      vsel(rr, rr, q0, M);\n      E.valu("v_mov_b32_e32 " + VL(quo[j])',
    'VL(rr) + ", " + VL(dn));\n      E.valu("v_mov_b32_e32 " + VL(quo[j])')}
NB_ONE_CLASS_SMALL = {"mythril_amd/csrc/jit_asm.cpp": (
    'E.salu("s_cmp_gt_u32 " + S(sNB) + ", " + imm(NB));', 'E.salu("s_cmp_gt_u32 " + S(sNB) + ", " + imm(widths[vi + 1]));')}


@pytest.mark.parametrize("name", W.gen_case_names())
def test_generator_form_share_under_the_c_port(name):
    """Between 1/8 and 7/8 of each window's candidates satisfy the root, so verdicts, first hit and
    hit count carry information."""
    c = W.gen_case(name)
    for start in W.GEN_STARTS:
        _, hits, ver = cport.search(c.pb, c.blob, c.seed, start, W.GEN_COUNT, verdicts=True)
        assert hits == int(ver.sum()) and W.GEN_COUNT // 8 <= hits <= 7 * W.GEN_COUNT // 8, (name, hex(start), hits)


def _sim_worker(args):
    exe, names, env = args
    recs = [record(0, W.gen_case(n).pb, W.gen_case(n).blob, W.gen_case(n).seed, start, W.SIM_COUNT)
            for n in names for start in W.GEN_STARTS]
    rc, summary, lines, err = run_sim(Path(exe), b"".join(recs), env)
    return names, rc, summary, lines[:8], err[-1500:], len(recs)


def _simulate(exe, names, env):
    step = max(1, (len(names) + WORKERS - 1) // WORKERS)
    tasks = [(str(exe), names[lo:lo + step], env) for lo in range(0, len(names), step)]
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        return pool.map(_sim_worker, tasks, chunksize=1)


def test_first_tier_on_the_simulator(sim):  # noqa: F811
    """Every generator-form case, both windows: ``mgj_gen`` verdicts, ``mgj_search`` first hit and hit
    count equal the C port's, no simulator rule broken, under the emitter's lifetime checker."""
    for names, rc, summary, lines, err, n in _simulate(sim, W.gen_case_names(), CHECK):
        assert summary, (names, rc, err)
        assert rc == 0 and int(summary["ok"]) == n == int(summary["records"]), (names, summary, lines, err)


def test_planted_first_tier_bugs_fail_named_cases(sim, tmp_path):  # noqa: F811
    """``div_one_limb`` without its second correction fails w256_div_mg_01 and w256_div_mg_11 (the
    waves whose every lane takes it) and w64_div_mg_01; ``udivrem`` with NB one class too small
    (a wave whose widest divisor has 2 limbs served by the 1-limb loop, 4 by 2, all by 4) fails
    w256_div_all_c2, w256_div_all_c3 and w256_div_all_c4.  The unedited driver passes the same
    records (``test_first_tier_on_the_simulator``)."""
    exes = _mutants(tmp_path, {"no_c2": NO_SECOND_CORRECTION, "nb_small": NB_ONE_CLASS_SMALL})
    want = {"no_c2": ["w256_div_mg_01", "w256_div_mg_11", "w64_div_mg_01"],
            "nb_small": ["w256_div_all_c2", "w256_div_all_c3", "w256_div_all_c4"]}
    for mutant, names in want.items():
        for name in names:
            (_, rc, summary, lines, err, n), = _simulate(exes[mutant], [name], {})
            assert summary, (mutant, name, rc, err)
            print(mutant, name, summary)
            assert rc != 0 and int(summary["mismatch"]) > 0, (mutant, name, summary, lines)


# ---- the O3 tier on the simulator, and planted bugs in bv_device.h --------------------------------------
# mythril_amd/build.py write_prelude() generates csrc/jit_prelude.inc, the text jit.cpp puts in front
# of every O3 kernel, from bv_device.h (and the keccak, generator and jit device headers): an edit of
# bv_device.h reaches the O3 tier's kernels, and the simulator runs them.  A mutant driver is jit.cpp
# with its #include pointed at a prelude generated from the edited header.

import re  # noqa: E402
import shutil  # noqa: E402
import sys  # noqa: E402
import tempfile  # noqa: E402

from tests.test_asm_sim import ROOT  # noqa: E402

DEVICE_MUTANTS = {
    "dev_no_c2": ("      q1 = ge ? q1 + 1u : q1;\n      r1 = ge ? r1 - dn : r1;\n", ""),
    "dev_no_carry": ("const bool ge = (c != 0) | (br == 0);", "const bool ge = (br == 0);"),
    "dev_odd_skip": ("const u32 skip = (32u - m) & ~1u;", "const u32 skip = (32u - m);"),
}


def _o3_worker(args):
    """Compile the cases' search kernels with the driver's jit.cpp, convert the code objects to text,
    run both windows in the simulator against the C port.  (names, compile, run, private, windows)"""
    exe, names, env = args
    sys.path.insert(0, str(ROOT))
    from tools.o3dis import convert

    cases = [W.gen_case(n) for n in names]
    tmp = Path(tempfile.mkdtemp(prefix="waveo3"))
    try:
        recs = b"".join(record(0, c.pb, c.blob, c.seed, W.GEN_STARTS[0], W.SIM_COUNT) for c in cases)
        rc, summary, lines, err = run_sim(Path(exe), recs, dict(env, ASMSIM_O3_DUMP=str(tmp)))
        comp = (rc, summary, lines[:6], err[-1500:])
        if rc or not summary or int(summary["ok"]) != len(cases):
            return names, comp, None, {}, 0
        priv = {int(m.group(1)): int(m.group(2)) for m in (re.match(r"o3 record (\d+): kernels \d+ private (\d+)", ln)
                                                            for ln in lines) if m}
        run_dir = tmp / "run"
        run_dir.mkdir()
        run, private = [], {}
        for i, c in enumerate(cases):
            if priv[i]:
                private[c.name] = priv[i]
                continue
            text = convert(str(tmp / f"{i}.co"))
            for start in W.GEN_STARTS:
                (run_dir / f"{len(run)}.s").write_text(text)
                run.append(record(0, c.pb, c.blob, c.seed, start, W.SIM_COUNT))
        rc, summary, lines, err = run_sim(Path(exe), b"".join(run), dict(env, ASMSIM_SEARCH_SOURCE_DIR=str(run_dir)))
        return names, comp, (rc, summary, lines[:6], err[-1500:]), private, len(run)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _o3_simulate(exe, names, chunk=3):
    tasks = [(str(exe), names[lo:lo + chunk], {}) for lo in range(0, len(names), chunk)]
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        return pool.map(_o3_worker, tasks, chunksize=1)


# generator-form cases whose O3 code object has a private segment (the simulator has no scratch): left out
O3_SCRATCH = {}


def test_o3_tier_on_the_simulator(sim):  # noqa: F811
    """Every generator-form case, both windows, compiled by this tree's jit.cpp: verdicts, first hit and
    hit count equal the C port's."""
    private = {}
    for names, comp, run, priv, n in _o3_simulate(sim, W.gen_case_names()):
        assert run is not None, (names, comp)
        rc, summary, lines, err = run
        assert summary, (names, rc, err)
        assert rc == 0 and int(summary["ok"]) == n == int(summary["records"]), (names, summary, lines, err)
        private.update(priv)
    assert private == O3_SCRATCH, private


def test_planted_bv_device_bugs_fail_named_cases(sim, tmp_path):  # noqa: F811
    """Through the O3 tier's prelude: ``udivrem8``'s one-limb step without its second correction fails
    w256_div_mg_01 and w256_div_mg_11; ``udivrem_nb`` without the ``c != 0`` term fails
    w256_div_carry_nb2 and w256_div_carry_nb4; ``bv_exp`` with ``& ~1u`` dropped from ``skip`` fails
    w256_exp_mixed_L33_lane0 and w256_exp_uniform_L129 (m = 1: an odd skip of 31)."""
    from mythril_amd import build

    edits = {}
    for name, (old, new) in DEVICE_MUTANTS.items():
        body = []
        for p in build.PRELUDE_PARTS:
            text = p.read_text()
            if p.name == "bv_device.h":
                assert text.count(old) == 1, (name, old)
                text = text.replace(old, new)
            body += [ln for ln in text.splitlines() if not ln.strip().startswith("#include") and ln.strip() != "#pragma once"]
        inc = tmp_path / f"{name}_prelude.inc"
        inc.write_text("R\"MGJ(\n" + "\n".join(body) + "\n)MGJ\"\n")
        edits[name] = {"mythril_amd/csrc/jit.cpp": ('#include "jit_prelude.inc"', f'#include "{inc}"')}
    exes = _mutants(tmp_path, edits, o3=True)
    want = {"dev_no_c2": ["w256_div_mg_01", "w256_div_mg_11"], "dev_no_carry": ["w256_div_carry_nb2", "w256_div_carry_nb4"],
            "dev_odd_skip": ["w256_exp_mixed_L33_lane0", "w256_exp_uniform_L129"]}
    for mutant, names in want.items():
        for names_, comp, run, priv, n in _o3_simulate(exes[mutant], names, chunk=1):
            assert run is not None and run[1] and not priv, (mutant, names_, comp, run)
            print(mutant, names_, run[1])
            assert run[0] != 0 and int(run[1]["mismatch"]) > 0, (mutant, names_, run)
