"""The first tier's guarded select arms (``jit_asm.cpp: plan_lazy``) on the GPU: the probes of
``tests/lazy_cases.py`` (all-false, mixed and all-true groups of every guarded condition in each
window, checked from the C port's generated coordinates first) and the two workloads full of
store-chain selects, C2 and C4.

``mgj_gen`` verdicts over 4,096 candidates from an aligned and from an odd index equal the C
port's (``oracle/bveval.c``) byte for byte; ``mgj_search`` first hit and hit count, full sweep and
early exit, equal ``cport.search``.  The switches are read once per process, so each variant
(guards on, MYTHGPU_JIT_ASM_NO_LAZY=1, and MYTHGPU_JIT_ASM_LAZY_PRIORS=3 for the three-prior
lookup) runs in a child process of its own; every variant is compared with the C port, so the
results with the switch on and off are the same because both are right.  The O3 tier is not
changed by the pass and is not run here.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``) over the GEN3 candidate stream.
"""
import json
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

from mythril_amd import search, workloads
from oracle import cport
from tests import lazy_cases as LC

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
N = 4096
WORKLOADS = ("token_transfer_underflow", "walletlibrary_kill")
WSTART, WN, WSEED = 1 << 40, 1 << 16, 0x6D797468
VARIANTS = {"lazy": {}, "off": {"MYTHGPU_JIT_ASM_NO_LAZY": "1"}, "priors3": {"MYTHGPU_JIT_ASM_LAZY_PRIORS": "3"}}

SCRIPT = r"""
import json, sys, zlib
from mythril_amd import native, search, workloads
from tests import lazy_cases as LC
eng = native.Engine.get()
spec = json.loads(sys.argv[1])
out = {}
def run(pb, blob, seed, windows):
    prog = eng.load(pb)
    gh = eng.load_gen(prog, blob)
    jh = eng.jit_compile(prog, gh, gen_verdicts=True, asm=True)
    assert eng.jit_layout(jh)[0] & native.MG_JIT_ASM, "not the first tier"
    rows = []
    for start, n in windows:
        v = eng.jit_verdicts(jh, seed, start, n)
        full = eng.jit_search(jh, seed, start, n, early_exit=False)
        early = eng.jit_search(jh, seed, start, n, early_exit=True)
        rows.append([start, n, zlib.crc32(v.tobytes()), int(v.sum()), list(full), early[0]])
    eng.jit_free(jh)
    eng.free_gen(gh)
    eng.free(prog)
    return rows
for name in spec["cases"]:
    c = LC.BUILDERS[name]()
    out[name] = run(c.pb, c.blob, LC.SEEDS[name], [(LC.ALIGNED, spec["n"]), (LC.ODD, spec["n"])])
for w in spec["workloads"]:
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[w]()])
    out[w] = run(P.to_bytes(), blob, spec["wseed"], [(spec["wstart"], spec["wn"])])
print(json.dumps(out))
"""


def _child(variant):
    cases = ["lookup_3"] if variant == "priors3" else sorted(LC.BUILDERS)
    spec = {"cases": cases, "workloads": [] if variant == "priors3" else list(WORKLOADS), "n": N,
            "wseed": WSEED, "wstart": WSTART, "wn": WN}
    env = dict(os.environ, PYTHONPATH=str(ROOT), MYTHGPU_JIT_DISK_CACHE="0")
    env.update(VARIANTS[variant])
    r = subprocess.run([sys.executable, "-c", SCRIPT, json.dumps(spec)], env=env, capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


_RUNS, _WANT = {}, {}


def _runs(variant):
    if variant not in _RUNS:
        _RUNS[variant] = _child(variant)
    return _RUNS[variant]


def _want(key, pb, blob, seed, start, n):
    """The C port's (verdict crc, verdict sum, [first hit, hits]) of one window, computed once."""
    k = (key, start, n)
    if k not in _WANT:
        first, hits, v = cport.search(pb, blob, seed, start, n, threads=16, verdicts=True)
        _WANT[k] = (zlib.crc32(np.asarray(v, dtype=np.uint8).tobytes()), int(v.sum()), [first, hits])
    return _WANT[k]


def _compare(name, rows, pb, blob, seed):
    for start, n, crc, total, full, early in rows:
        wcrc, wsum, wfull = _want(name, pb, blob, seed, start, n)
        assert 0 < wsum < n, (name, start, wsum)
        assert (crc, total) == (wcrc, wsum), (name, start, "verdicts differ from the C port", total, wsum)
        assert full == wfull, (name, start, full, wfull)
        assert early == wfull[0], (name, start, early, wfull[0])


@pytest.mark.parametrize("variant", ["lazy", "off"])
@pytest.mark.parametrize("name", sorted(LC.BUILDERS))
def test_probe_matches_c_port(engine, name, variant):
    case = LC.BUILDERS[name]()
    for start in (LC.ALIGNED, LC.ODD):
        for c in range(len(case.conds)):
            assert min(case.group_classes(LC.SEEDS[name], start, N, c)) > 0, (name, start, c)
    _compare(name, _runs(variant)[name], case.pb, case.blob, LC.SEEDS[name])


def test_three_prior_lookup_guarded_matches_c_port(engine):
    case = LC.BUILDERS["lookup_3"]()
    assert case.env == VARIANTS["priors3"]
    _compare("lookup_3", _runs("priors3")["lookup_3"], case.pb, case.blob, LC.SEEDS["lookup_3"])


@pytest.mark.parametrize("variant", ["lazy", "off"])
@pytest.mark.parametrize("name", WORKLOADS, ids=workloads.test_id)
def test_store_chain_workloads_match_c_port(engine, name, variant):
    """C2 and C4 over 2^16 candidates from 2^40 with the bench's seed."""
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
    _compare(name, _runs(variant)[name], P.to_bytes(), blob, WSEED)
