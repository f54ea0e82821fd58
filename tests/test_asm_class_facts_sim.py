"""The first tier's MIXED alternatives (``jit_asm.cpp: gen_value``) on the CPU simulator: the
threshold cascade ordered by the alternatives' shares, the kernel-lifetime scalar literals, and
COPY sources generated into the copier's registers.

Every case of ``tests/class_fact_cases.py`` runs through the emitter, comgr's assembler and the
instruction-level simulator (``tests/asmsim``) over 96 groups, on two seeds, aligned and from an
odd index: ``mgj_gen`` verdicts per candidate and ``mgj_search`` first hit and hit count equal the
C port's (``oracle/bveval.c``).  Configurations: default, MYTHGPU_JIT_ASM_NO_CLASS_FACTS=1, the
emitter's lifetime checker, b32 LDS reads, and the spill-test register file.  Two mutants of
``jit_asm.cpp`` each fail the table.  With the switch the emitted text of every workload is the
parent's (``tests/golden/class_facts_parent_sha.json``).

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``).
"""
import json
from pathlib import Path

import pytest

from mythril_amd import search, workloads
from oracle import cport
from tests import class_fact_cases as CF
from tests.test_asm_lazy_sim import _texts
from tests.test_asm_sim import _cached, _mutants, record, run_sim

ROOT = Path(__file__).resolve().parent.parent
OFF = {"MYTHGPU_JIT_ASM_NO_CLASS_FACTS": "1"}
ENVS = {
    "default": {},
    "off": OFF,
    "check": {"MYTHGPU_JIT_ASM_CHECK": "1"},
    "lds_b32": {"MYTHGPU_JIT_ASM_LDS_B32": "1", "MYTHGPU_JIT_ASM_CHECK": "1"},
    "spill": {"MYTHGPU_JIT_ASM_SPILL_TEST": "64", "MYTHGPU_JIT_ASM_CHECK": "1"},
}
WINDOWS = [(CF.ALIGNED, CF.SIM_COUNT), (CF.ODD, CF.SIM_COUNT)]

# the cascade testing the next alternative's threshold
CASCADE_BUG = {"mythril_amd/csrc/jit_asm.cpp": ('hexs(alts[k].T << 16));', 'hexs(alts[k + 1].T << 16));')}
# a region's code (the delta's test of the choice word) taking a pinned literal's SGPR as its scratch
PIN_BUG = {"mythril_amd/csrc/jit_asm.cpp": (
    '''    E.salu("s_and_b32 s40, " + S(ws) + ", 0xffff", {40});
    E.salu("s_cmp_lt_u32 s40, " + imm(pdelta));''',
    '''    const int sx = spin1.empty() ? 40 : spin1.begin()->second;
    E.salu("s_and_b32 " + S(sx) + ", " + S(ws) + ", 0xffff", {sx});
    E.salu("s_cmp_lt_u32 " + S(sx) + ", " + imm(pdelta));''')}


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _cached(tmp_path_factory, sanitize=False)


@pytest.fixture(scope="module")
def cases():
    return {name: build() for name, build in CF.BUILDERS.items()}


_RECS = {}


def _records(cases, name, flags=1):
    """The case's records (search with verdicts, per seed and window), checked informative once.
    (flags=0: for the mutant drivers, which are built without the assembler)"""
    if flags != 1:
        return [r[:-4] + flags.to_bytes(4, "little") for r in _records(cases, name)]
    if name not in _RECS:
        case, recs = cases[name], []
        for seed in CF.SEEDS:
            for start, count in WINDOWS:
                want = cport.search(case.pb, case.blob, seed, start, count, threads=2, verdicts=True)[2]
                assert 0 < int(want.sum()) < count, (name, seed, start, int(want.sum()))
                recs.append(record(0, case.pb, case.blob, seed, start, count, flags=1))
        _RECS[name] = recs
    return _RECS[name]


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("name", sorted(CF.BUILDERS))
def test_cases_on_the_simulator(sim, cases, name, env):
    recs = _records(cases, name)
    rc, summary, bad, err = run_sim(sim, b"".join(recs), ENVS[env])
    assert rc == 0 and summary, f"{summary}\n" + "\n".join(bad[:8]) + "\n" + err[-3000:]
    assert int(summary["ok"]) == len(recs), (summary, bad[:8])


def test_the_changes_are_in_the_text(cases):
    """Four like alternatives test the middle threshold first; the scalars case keeps its ALIGNED
    base and spans in SGPRs loaded before the group loop; neither with the switch."""
    progs = {n: (cases[n].pb, cases[n].blob) for n in ("four_alts", "scalars", "two_alts")}
    on, off = _sources(progs, {}), _sources(progs, OFF)
    c = CF.BUILDERS["four_alts"]()
    spec = [s for s in c.blob[4:4 + 8 * int(c.blob[1])].reshape(-1, 8) if (s[0] & 0xFF) == search.GEN_MIXED and s[4] != search.NONE][0]
    pc, pd, ps = int(spec[3]) & 0xFFFF, int(spec[3]) >> 16, int(spec[5]) & 0xFFFF
    first = lambda src: [ln for ln in src.splitlines() if "s_cmp_lt_u32" in ln and ln.strip().endswith("0000")]  # noqa: E731
    assert first(on["four_alts"])[0].endswith(", 0x%x" % ((pc + pd) << 16)), first(on["four_alts"])[:3]
    assert first(off["four_alts"])[0].endswith(", 0x%x" % (pc << 16)), first(off["four_alts"])[:3]
    assert first(on["two_alts"]) == first(off["two_alts"])  # one threshold: nothing to order
    base = "v_mad_u64_u32"
    assert any(base in ln and "s[40:41]" in ln for ln in off["scalars"].splitlines())
    assert not any(base in ln and "s[40:41]" in ln for ln in on["scalars"].splitlines())
    assert on["scalars"].count("0xfff00000") < off["scalars"].count("0xfff00000")


_SRC = """
import pickle, sys, json
from mythril_amd import native
print(json.dumps({n: native.jit_asm(pb, blob) for n, (pb, blob) in pickle.loads(sys.stdin.buffer.read()).items()}))
"""


def _sources(progs, env):
    import os
    import pickle
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-c", _SRC], input=pickle.dumps(progs), capture_output=True,
                       env=dict(os.environ, **env), cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads(r.stdout.decode())


@pytest.mark.parametrize("env", ["check", "default", "off"])
def test_workloads_with_regenerated_copy_sources(sim, env):
    """C1 and C2 hold COPY alternatives whose MIXED source no code has read where the copier is
    generated: it is generated again, into the copier's registers (as in the table's ``regen_*``
    cases).  64 x 32 candidates from an odd index."""
    recs = []
    for name in ("suicide_kill", "token_transfer_underflow"):
        P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
        recs.append(record(0, P.to_bytes(), blob, 7, CF.ODD, 64 * 32, flags=1))
    rc, summary, bad, err = run_sim(sim, b"".join(recs), ENVS[env])
    assert rc == 0 and summary and int(summary["ok"]) == len(recs), f"{summary}\n" + "\n".join(bad[:8]) + "\n" + err[-3000:]


def test_copy_sources_are_generated_in_place(cases):
    """The ``regen_*`` cases (a source that is generated again: plain, with a fix record that sets
    limbs whole, clamped, narrow) and C1 hold fewer register-to-register moves with the COPY item
    than without it; a source a root reads whole stays live, and keeps its moves."""
    names = ["regen_mixed", "regen_fix", "regen_clamped", "regen_w8", "copy_live", "copy_dead_mixed"]
    tprogs = {n: (cases[n].pb, cases[n].blob) for n in names}
    ton, trest = _texts(tprogs, {}), _texts(tprogs, {"MYTHGPU_JIT_ASM_CLASS_FACTS": "6"})
    for n in names:
        if n.startswith("regen"):
            assert ton[n]["moves"] < trest[n]["moves"], (n, ton[n], trest[n])
        else:
            assert ton[n]["moves"] == trest[n]["moves"] > 0, (n, ton[n], trest[n])
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS["suicide_kill"]()])
    progs = {"c1": (P.to_bytes(), blob)}
    on = _texts(progs, {})["c1"]
    rest = _texts(progs, {"MYTHGPU_JIT_ASM_CLASS_FACTS": "6"})["c1"]  # everything but the COPY item
    assert on["moves"] < rest["moves"], (on, rest)


def test_the_table_has_teeth(cases, tmp_path):
    """Each mutant of the emitter fails records of the table (wrong verdicts or counts)."""
    exes = _mutants(tmp_path, {"cascade": CASCADE_BUG, "pin": PIN_BUG})
    for mutant, names in (("cascade", ["four_alts", "three_alts_low", "edge_delta_clamp"]),
                          ("pin", ["scalars", "edge_delta_clamp", "copy_live"])):
        recs = [r for n in names for r in _records(cases, n, flags=0)]
        rc, summary, bad, _ = run_sim(exes[mutant], b"".join(recs))
        print(mutant, "mutant:", summary)
        assert rc != 0 and int(summary["mismatch"]) > 0, (mutant, summary, bad[:4])


def test_switch_restores_the_parent_text():
    """MYTHGPU_JIT_ASM_NO_CLASS_FACTS=1: every workload's emitted text is byte-identical to the text
    before these changes (its SHA); without the switch C2's differs."""
    want = json.loads((ROOT / "tests/golden/class_facts_parent_sha.json").read_text())
    progs = {}
    for name in sorted(workloads.WORKLOADS):
        P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
        progs[name] = (P.to_bytes(), blob)
    assert sorted(progs) == sorted(want)
    off = _texts(progs, OFF)
    assert {n: off[n]["sha"] for n in progs} == want
    on = _texts(progs, {})
    assert on["token_transfer_underflow"]["sha"] != want["token_transfer_underflow"]
