"""Warm start on the simulated LASER query stream: ``search_partitioned`` with and without a
``search.ModelCache`` (``warm=``), query by query in LASER order (``stream_bench.stream_queries``:
every prefix of a workload's constraint list, the negated siblings, one infeasible sibling).

Per workload stream and mode it records the queries and sat answers, the queries answered by the
seeded first launch and by one of its replay lanes, p50 / p99 of the time to first model over the
sat queries, and the mean time of the seeded launches of queries that the seeded launch did not
answer (what a miss adds; for a query of several buckets the buckets' seeded launches are summed).
Every query is bounded by ``--max-candidates`` under a generous timeout, not by wall time, and
stays on the interpreter (``jit="never"``), so the answers do not depend on the clock.  The cache
is fresh per stream and repeat; the modes alternate within a repeat, after one untimed pass of
both (code objects loaded, flatten and generator caches filled as in a running analysis).

What must hold (exit status 1 otherwise): every query answered sat with warm off is answered sat
with warm on.  No threshold is set on the times.

usage: python tools/warm_bench.py [--repeats 5] [--workloads a,b] [--out profiles/warm_stream.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from mythril_amd import native, search, workloads  # noqa: E402
from tools.stream_bench import stream_queries  # noqa: E402


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p * (len(xs) - 1))))] if xs else None


def run_stream(eng, queries, warm, max_candidates, timeout_s):
    """One pass over a stream: per query (sat, seeded, replay, ms, seeded_ms or None)."""
    out = []
    for _, q in queries:
        roots = [c.raw for c in q]
        t = time.perf_counter()
        r = search.search_partitioned(eng, roots, batch=False, timeout_s=timeout_s, max_candidates=max_candidates,
                                      jit="never", warm=warm)
        ms = (time.perf_counter() - t) * 1e3
        out.append((r.index is not None, bool(r.seeded), bool(r.replay), ms, r.timing.get("seeded_ms")))
    return out


def summarize(passes):
    """``passes``: the repeats of one (stream, mode).  Counts are of the first pass (they are the
    same in every pass: nothing depends on time); times are pooled over the passes."""
    first = passes[0]
    sat_ms = [ms for p in passes for sat, _, _, ms, _ in p if sat]
    miss_ms = [s for p in passes for _, seeded, _, _, s in p if s is not None and not seeded]
    r3 = lambda x: None if x is None else round(x, 3)
    return {"queries": len(first), "sat": sum(q[0] for q in first), "seeded_answers": sum(q[1] for q in first),
            "replay_answers": sum(q[2] for q in first), "seeded_launches": sum(q[4] is not None for q in first),
            "first_model_ms_p50": r3(pct(sat_ms, 0.5)), "first_model_ms_p99": r3(pct(sat_ms, 0.99)),
            "seeded_miss_extra_ms_mean": r3(sum(miss_ms) / len(miss_ms)) if miss_ms else None,
            "counts_stable": all([q[:3] for q in p] == [q[:3] for q in first] for p in passes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(workloads.WORKLOADS))
    ap.add_argument("--max-candidates", type=int, default=1 << 22)
    ap.add_argument("--timeout-s", type=float, default=30.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "warm_stream.json"))
    a = ap.parse_args()
    eng = native.Engine.get()
    rows, lost = [], []
    for name in [w for w in a.workloads.split(",") if w]:
        qs = stream_queries(name)
        run = lambda warm: run_stream(eng, qs, warm, a.max_candidates, a.timeout_s)
        run(None), run(search.ModelCache())  # untimed
        off, on = [], []
        for _ in range(a.repeats):
            off.append(run(None))
            on.append(run(search.ModelCache()))
        for (label, _), x, y in zip(qs, off[0], on[0]):
            if x[0] and not y[0]:
                lost.append(f"{name}/{label}")
        row = {"workload": name, "max_candidates": a.max_candidates, "repeats": a.repeats,
               "off": summarize(off), "on": summarize(on)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    doc = {"tool": "tools/warm_bench.py", "device": f"gfx950 ({eng.stats().cu_count} CUs)", "streams": rows,
           "sat_lost_with_warm_on": lost}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    if lost:
        print("answered sat with warm off but not with warm on:", ", ".join(lost), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
