"""The first tier's mask cache and the specialiser's value numbering on the GPU.

Each configuration runs in its own process (the switches are read once): the six hand-built
programs of ``tests/test_mask_cache_cpu.py`` and C2, C4 and etherstore through the first tier's
``mgj_gen`` (per-candidate verdicts of 2^12 candidates from an unaligned 63-bit start) and
``mgj_search`` (first hit and hit count of a 2^16 full sweep), with the cache on and off, and the
same sweep on the interpreter.  Every verdict, first hit and hit count equals the C port's
(``oracle/bveval.c``), so each configuration is checked, not only compared with the others.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``) over the GEN3 candidate stream."""
import json
import os
import pickle
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
WORKLOADS = ("token_transfer_underflow", "walletlibrary_kill", "etherstore_reentrancy")
SEED = 11
V_START, V_N = (1 << 62) + (1 << 33) + 37, 1 << 12
S_START, S_N = (1 << 62) + 12345, 1 << 16

SCRIPT = r"""
import json, pickle, sys
from mythril_amd import native
eng = native.Engine.get()
progs, seed, v_start, v_n, s_start, s_n = pickle.loads(sys.stdin.buffer.read())
out = {}
for name, (pb, blob) in progs.items():
    prog = eng.load(pb)
    gh = eng.load_gen(prog, blob)
    jh = eng.jit_compile(prog, gh, gen_verdicts=True, asm=True)
    assert eng.jit_layout(jh)[0] & native.MG_JIT_ASM, "not the first tier"
    ver = eng.jit_verdicts(jh, seed, v_start, v_n)
    out[name] = {"verdicts": ver.tobytes().hex(), "asm": list(eng.jit_search(jh, seed, s_start, s_n, early_exit=False)),
                 "interp": list(eng.search(prog, gh, seed, s_start, s_n, early_exit=False))}
    eng.jit_free(jh)
    eng.free_gen(gh)
    eng.free(prog)
print(json.dumps(out))
"""


def _programs():
    from mythril_amd import search, workloads
    from tests.test_mask_cache_cpu import cases

    progs = {name: (P.to_bytes(), blob) for name, (P, blob) in cases().items()}
    for w in WORKLOADS:
        P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[w]()])
        progs[w] = (P.to_bytes(), blob)
    return progs


@pytest.fixture(scope="module")
def reference():
    """The C port's verdicts, first hit and hit count per program (computed once)."""
    from oracle import cport

    ref = {}
    for name, (pb, blob) in _programs().items():
        ver = cport.search(pb, blob, SEED, V_START, V_N, threads=16, verdicts=True)[2]
        first, hits = cport.search(pb, blob, SEED, S_START, S_N, threads=16)[:2]
        ref[name] = (np.asarray(ver, dtype=np.uint8), first, hits)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [
    {},
    {"MYTHGPU_JIT_ASM_NO_MASK_CACHE": "1"},
    {"MYTHGPU_GVN": "0"},
    {"MYTHGPU_JIT_ASM_NO_MASK_CACHE": "1", "MYTHGPU_GVN": "0"},
], ids=["default", "no_mask_cache", "no_gvn", "neither"])
def test_mask_cache_variant_matches_c_port(variant, reference):
    payload = (_programs(), SEED, V_START, V_N, S_START, S_N)
    env = dict(os.environ, PYTHONPATH=str(ROOT), MYTHGPU_JIT_DISK_CACHE="0")
    env.update(variant)
    r = subprocess.run([sys.executable, "-c", SCRIPT], input=pickle.dumps(payload), env=env, capture_output=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    got = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert set(got) == set(reference)
    for name, (ver, first, hits) in reference.items():
        g = got[name]
        gv = np.frombuffer(bytes.fromhex(g["verdicts"]), dtype=np.uint8)
        bad = np.flatnonzero(gv != ver)
        assert bad.size == 0, f"{name} {variant}: mgj_gen verdict differs at index {V_START + int(bad[0])}"
        assert 0 < int(ver.sum()) < V_N or name in WORKLOADS, (name, int(ver.sum()))
        assert tuple(g["asm"]) == (first, hits), (name, variant, g["asm"], (first, hits))
        assert tuple(g["interp"]) == (first, hits), (name, variant, g["interp"], (first, hits))
