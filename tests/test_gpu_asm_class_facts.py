"""The first tier's MIXED alternatives on the GPU: the share-ordered threshold cascade, the
kernel-lifetime scalar literals and COPY sources generated into the copier's registers
(``jit_asm.cpp: gen_value``, ``pinned_kernel``).

The table of ``tests/class_fact_cases.py`` at 4,096 candidates from an odd index: ``mgj_gen``
verdicts equal the C port's (``oracle/bveval.c``) byte for byte, ``mgj_search`` first hit and hit
count equal ``cport.search`` with early exit off and on; the six workloads over 2^16 candidates.
The switch is read once per process, so the default and MYTHGPU_JIT_ASM_NO_CLASS_FACTS=1 run in
a child process each; both are compared with the C port.  No timing is asserted.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``) over the GEN3 candidate stream.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from mythril_amd import search, workloads
from tests import class_fact_cases as CF
from tests.test_gpu_asm_lazy import _want

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SEED = CF.SEEDS[0]
WSTART, WN, WSEED = 1 << 40, 1 << 16, 0x6D797468
VARIANTS = {"facts": {}, "off": {"MYTHGPU_JIT_ASM_NO_CLASS_FACTS": "1"}}

SCRIPT = r"""
import json, sys, zlib
from mythril_amd import native, search, workloads
from tests import class_fact_cases as CF
eng = native.Engine.get()
spec = json.loads(sys.argv[1])
out = {}
def run(pb, blob, seed, start, n):
    prog = eng.load(pb)
    gh = eng.load_gen(prog, blob)
    jh = eng.jit_compile(prog, gh, gen_verdicts=True, asm=True)
    assert eng.jit_layout(jh)[0] & native.MG_JIT_ASM, "not the first tier"
    v = eng.jit_verdicts(jh, seed, start, n)
    full = eng.jit_search(jh, seed, start, n, early_exit=False)
    early = eng.jit_search(jh, seed, start, n, early_exit=True)
    eng.jit_free(jh)
    eng.free_gen(gh)
    eng.free(prog)
    return [[start, n, zlib.crc32(v.tobytes()), int(v.sum()), list(full), early[0]]]
for name in sorted(CF.BUILDERS):
    c = CF.BUILDERS[name]()
    out[name] = run(c.pb, c.blob, spec["seed"], CF.ODD, CF.GPU_COUNT)
for w in sorted(workloads.WORKLOADS):
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[w]()])
    out[w] = run(P.to_bytes(), blob, spec["wseed"], spec["wstart"], spec["wn"])
print(json.dumps(out))
"""

_RUNS = {}


def _compare(name, rows, pb, blob, seed, informative=True):
    for start, n, crc, total, full, early in rows:
        wcrc, wsum, wfull = _want(name, pb, blob, seed, start, n)
        assert not informative or 0 < wsum < n, (name, start, wsum)
        assert (crc, total) == (wcrc, wsum), (name, start, "verdicts differ from the C port", total, wsum)
        assert full == wfull, (name, start, full, wfull)
        assert early == wfull[0], (name, start, early, wfull[0])


def _runs(variant):
    if variant not in _RUNS:
        spec = {"seed": SEED, "wseed": WSEED, "wstart": WSTART, "wn": WN}
        env = dict(os.environ, PYTHONPATH=str(ROOT), MYTHGPU_JIT_DISK_CACHE="0")
        env.update(VARIANTS[variant])
        r = subprocess.run([sys.executable, "-c", SCRIPT, json.dumps(spec)], env=env, capture_output=True, text=True,
                           timeout=300, cwd=str(ROOT))
        assert r.returncode == 0, r.stderr[-3000:]
        _RUNS[variant] = json.loads(r.stdout.strip().splitlines()[-1])
    return _RUNS[variant]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(CF.BUILDERS))
def test_case_matches_c_port(engine, name, variant):
    case = CF.BUILDERS[name]()
    _compare("cf_" + name, _runs(variant)[name], case.pb, case.blob, SEED)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", sorted(workloads.WORKLOADS), ids=workloads.test_id)
def test_workloads_match_c_port(engine, name, variant):
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
    # (a workload's window may hold no hit: the verdict bytes and counts are compared all the same)
    _compare(name, _runs(variant)[name], P.to_bytes(), blob, WSEED, informative=False)
