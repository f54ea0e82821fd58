"""The first tier's guarded select arms (``jit_asm.cpp: plan_lazy``) on the CPU simulator.

A wide ITE whose condition holds in no lane of a 64-candidate group skips the true arm's
exclusive cone and its selects (the else arm likewise when every lane holds; a LOOKUP's select
chain when no key test matches).  That is exact, so everything here is a comparison with the C
port (``oracle/bveval.c``) on the unspecialised program, through the emitter, comgr's assembler and
the instruction-level simulator (``tests/asmsim``): ``mgj_gen`` verdicts per candidate and
``mgj_search`` first hit and hit count with early exit off and on.

The probes (``tests/lazy_cases.py``) control the lane masks from the generator: every window holds
all-false, mixed and all-true groups of each guarded condition, which each test first checks from
the C port's generated coordinates alone.  Every case also runs with MYTHGPU_JIT_ASM_NO_LAZY=1;
with the switch the emitted text of C2 is what it was before the pass existed.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``).
"""
import json
import os
import pickle
import subprocess
import sys
from pathlib import Path

import pytest

from mythril_amd import search, workloads
from oracle import cport
from tests import lazy_cases as LC
from tests.test_asm_sim import _cached, record, run_sim

ROOT = Path(__file__).resolve().parent.parent
ENVS = {"lazy": {}, "off": {"MYTHGPU_JIT_ASM_NO_LAZY": "1"}}
C2_PARENT_SHA = "20bd10fe49b8e846"  # C2's first-tier text before the pass


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return _cached(tmp_path_factory, sanitize=False)


@pytest.fixture(scope="module")
def cases():
    return {name: build() for name, build in LC.BUILDERS.items()}


def _window_records(case, name, seed, windows):
    recs = []
    for start, count in windows:
        for c in range(len(case.conds)):
            none, mixed, every = case.group_classes(seed, start, count, c)
            assert none > 0 and mixed > 0 and every > 0, (name, start, c, (none, mixed, every))
        want = cport.search(case.pb, case.blob, seed, start, count, threads=2, verdicts=True)[2]
        assert 0 < int(want.sum()) < count, (name, start, int(want.sum()))
        recs.append(record(0, case.pb, case.blob, seed, start, count, flags=1))
    return recs


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("name", sorted(LC.BUILDERS))
def test_lazy_cases_on_the_simulator(sim, cases, name, env):
    """Each probe over 64 x 8 candidates, aligned and from an odd index (a partial first and last
    group), with the guards and with the switch: verdicts, first hit and hit count equal the C
    port's, under the emitter's lifetime checker."""
    case = cases[name]
    recs = _window_records(case, name, LC.SEEDS[name], [(LC.ALIGNED, LC.COUNT), (LC.ODD, LC.COUNT)])
    rc, summary, bad, err = run_sim(sim, b"".join(recs), dict(ENVS[env], MYTHGPU_JIT_ASM_CHECK="1", **case.env))
    assert rc == 0 and summary, f"{summary}\n" + "\n".join(bad[:8]) + "\n" + err[-3000:]
    assert int(summary["ok"]) == len(recs), (summary, bad[:8])


@pytest.mark.parametrize("env", sorted(ENVS))
def test_single_lane_groups(sim, cases, env):
    """A group whose condition holds in lane 0 alone, and one in lane 63 alone: the region runs for
    one lane's sake and the select changes that lane only."""
    case = cases["true_arm"]
    recs = []
    for lane, (seed, base) in sorted(LC.SINGLE_LANE.items()):
        t = case.lanes_true(seed, base, 64)
        assert int(t.sum()) == 1 and bool(t[lane]), (lane, t.nonzero())
        recs.append(record(0, case.pb, case.blob, seed, base, 64, flags=1))
    rc, summary, bad, err = run_sim(sim, b"".join(recs), dict(ENVS[env], MYTHGPU_JIT_ASM_CHECK="1"))
    assert rc == 0 and summary, f"{summary}\n" + "\n".join(bad[:8]) + "\n" + err[-3000:]
    assert int(summary["ok"]) == len(recs) == 2, (summary, bad[:8])


_ASM = """
import pickle, sys, json, re, hashlib
from mythril_amd import native
out = {}
for name, (pb, blob) in pickle.loads(sys.stdin.buffer.read()).items():
    src = native.jit_asm(pb, blob)
    out[name] = {"sha": hashlib.sha256(src.encode()).hexdigest()[:16],
                 "regions": [int(x) for x in re.findall(r"; lazy arms: (\\d+) guarded regions", src)],
                 "else_guards": len(re.findall(r"s_cmp_eq_u64 s\\[\\d+:\\d+\\], -1\\n", src)),
                 "guards": len(re.findall(r"s_cmp_eq_u64 s\\[\\d+:\\d+\\], 0\\n", src)),
                 "moves": len(re.findall(r"v_mov_b32_e32 v\\d+, v\\d+\\n", src)),
                 "mask_spills": [int(x) for x in re.findall(r"(\\d+) mask spills", src)]}
print(json.dumps(out))
"""


def _texts(progs, env):
    r = subprocess.run([sys.executable, "-c", _ASM], input=pickle.dumps(progs), capture_output=True,
                       env=dict(os.environ, **env), cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads(r.stdout.decode())


def test_emitted_text_has_the_expected_guards(cases):
    """The regions each probe's two kernels (mgj_search, mgj_gen) hold: a guard where the arm has an
    exclusive cone, none where the arm is shared, and none around a coordinate that another
    coordinate copies (the unlinked twin of that probe is guarded); the else arm's guard compares
    with -1; the copy path moves the unguarded operand into fresh registers; the Bools live across
    a region move to their VGPR form before its branch.  With the switch no region is emitted."""
    by_env = {}
    for name, case in cases.items():
        by_env.setdefault(json.dumps(case.env, sort_keys=True), {})[name] = (case.pb, case.blob)
    on, off = {}, {}
    for env, progs in by_env.items():
        on.update(_texts(progs, json.loads(env)))
        off.update(_texts(progs, dict(json.loads(env), MYTHGPU_JIT_ASM_NO_LAZY="1")))
    for name, case in cases.items():
        assert on[name]["regions"] == [case.regions, case.regions], (name, on[name])
        assert off[name]["regions"] == [], (name, off[name])
        added = {k: on[name][k] - off[name][k] for k in ("guards", "else_guards")}  # (the kernel's own compares aside)
        assert added["guards"] + added["else_guards"] == 2 * case.regions, (name, on[name], off[name])
    assert on["copy_source"]["regions"] == [0, 0] and on["copy_source_unlinked"]["regions"] == [1, 1]
    assert on["shared_arm"]["regions"] == [0, 0]
    assert on["else_arm"]["else_guards"] - off["else_arm"]["else_guards"] == 2
    assert on["true_arm"]["else_guards"] == off["true_arm"]["else_guards"]
    assert on["copy_path"]["moves"] - off["copy_path"]["moves"] >= 2 * 8, (on["copy_path"], off["copy_path"])
    assert on["true_arm"]["moves"] == off["true_arm"]["moves"], (on["true_arm"], off["true_arm"])
    assert sum(on["many_bools"]["mask_spills"]) > 0, on["many_bools"]


def test_switch_restores_the_parent_text_of_c2():
    """MYTHGPU_JIT_ASM_NO_LAZY=1: C2's emitted text is byte-identical to the text before the pass
    (its SHA); without the switch the kernels hold a guarded region."""
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS["token_transfer_underflow"]()])
    progs = {"c2": (P.to_bytes(), blob)}
    off = _texts(progs, {"MYTHGPU_JIT_ASM_NO_LAZY": "1"})["c2"]
    on = _texts(progs, {})["c2"]
    assert off["sha"] == C2_PARENT_SHA, off
    assert on["sha"] != C2_PARENT_SHA and on["regions"] and min(on["regions"]) >= 1, on
