"""``bench.py`` as the driver runs it: a plain run stops after the timed steps (every leg measured
beside the headline figure is null without ``--full``), ``--steps`` sets the number of timed steps,
and ``--dump-outputs`` writes what the last timed step returned — checked against the C port
(``oracle/bveval.c``) on the same window of the GEN3 candidate stream.

The launch is small and odd-sized (2^16 + 77 candidates: several blocks, a ragged last wave) so the
C port's sweep of the same window takes a fraction of a second.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
C = (1 << 16) + 77
STEPS, WARMUP = 3, 1
FULL_ONLY = ("cpu_baseline", "roofline_eval", "dropin_stream", "jit_asm_tier", "time_to_first_model_ms",
             "time_to_first_model_cold_ms", "time_to_first_model_hard", "time_to_first_model_sharded_ms",
             "first_model_index")


def test_plain_run_dumps_the_last_step(engine, tmp_path):
    from mythril_amd import search, workloads
    from mythril_amd.distributed import chunk_start
    from oracle import cport

    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
                        str(WARMUP), "--candidates", str(C), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["config"]["candidates_per_gpu_step"] == C
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(C / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert all(d[k] is None for k in FULL_ONLY), {k: d[k] for k in FULL_ONLY if d[k] is not None}

    first = np.load(tmp_path / "out" / "first_hit_index.npy")
    hits = np.load(tmp_path / "out" / "hit_count.npy")
    assert first.dtype == np.float64 and hits.dtype == np.float64 and first.shape == hits.shape == (1,)

    # the same windows through the C port: the last timed step's and all timed steps' together
    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS["token_transfer_underflow"]()])
    seed = 0x6D797468  # bench.py's default --seed
    want = [cport.search(P.to_bytes(), blob, seed, chunk_start(s, 0, 1, C), C, threads=16)[:2]
            for s in range(WARMUP, WARMUP + STEPS)]
    wf, wh = want[-1]
    assert int(hits[0]) == wh and int(first[0]) == (-1 if wf is None else wf)
    assert d["hits_in_timed_region"] == sum(h for _, h in want)
