"""Batched against serial first launches (GPU box): what ``mg_search_batch`` buys a partitioned query.

Three comparisons, each with the serial and the batched variant alternating inside this process
(caches warm, profiler off), ``--reps`` timed repetitions per variant, median and 10th / 90th
percentile in microseconds:

* per workload, ``search_partitioned`` serial against ``batch=True`` (``jit="never"``): the time to
  first model and the engine's launches per query (``mg_stats``);
* k copies of the one-constraint probe query of ``tools/latency_probe.py`` as k ``mg_search`` calls
  against one ``mg_search_batch``, k in 1, 2, 4, 16, 64;
* a batch of light-tier entries alone against the same entries plus one heavy-tier entry (the
  cost of launching at the highest tier among the entries).

usage: python tools/batch_latency.py [--reps 50] [--out profiles/batch_latency.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402

from mythril_amd import native, partition, search, workloads  # noqa: E402
from mythril_amd.smt import symbol_factory as sf  # noqa: E402


def stat(ts):
    a = 1e6 * np.asarray(ts)
    return {"median_us": round(float(np.median(a)), 1), "p10_us": round(float(np.percentile(a, 10)), 1),
            "p90_us": round(float(np.percentile(a, 90)), 1)}


def alternate(fa, fb, reps):
    """Timings of fa and fb, alternating, after two warm-up rounds."""
    for _ in range(2):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fa()
        t1 = time.perf_counter()
        fb()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    return ta, tb


def verdict(serial, batched):
    """'faster' / 'slower' only when the medians differ by more than either spread (p90 - p10)."""
    spread = max(serial["p90_us"] - serial["p10_us"], batched["p90_us"] - batched["p10_us"])
    d = serial["median_us"] - batched["median_us"]
    return "batched faster" if d > spread else "batched slower" if -d > spread else "within spread"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="profiles/batch_latency.json")
    args = ap.parse_args()
    eng = native.Engine.get()
    out = {"reps": args.reps, "device": "measured on the GPU this ran on", "workloads": {}, "probe": {}, "tier": {}}

    def launches(fn):
        n0 = eng.stats().launches
        r = fn()
        return eng.stats().launches - n0, r

    for w, f in workloads.WORKLOADS.items():
        roots = [c.raw for c in f()]
        kw = dict(jit="never", timeout_s=10)
        ls, rs = launches(lambda: search.search_partitioned(eng, roots, batch=False, **kw))
        lb, rb = launches(lambda: search.search_partitioned(eng, roots, batch=True, **kw))
        assert rs.index == rb.index and rs.model[0:4] == rb.model[0:4], w
        ts, tb = alternate(lambda: search.search_partitioned(eng, roots, batch=False, **kw),
                           lambda: search.search_partitioned(eng, roots, batch=True, **kw), args.reps)
        s, b = stat(ts), stat(tb)
        out["workloads"][w] = {"buckets": len(partition.partition(roots)), "index": list(rs.index),
                               "serial": dict(s, launches=ls), "batched": dict(b, launches=lb), "result": verdict(s, b)}
        print(w, json.dumps(out["workloads"][w]), flush=True)

    # the fixed cost of a call: a one-constraint program, 64 candidates, no hit in the window
    x = sf.BitVecSym("probe_x", 8)
    P1, blob1 = search.prepare([(x == sf.BitVecVal(5, 8)).raw])
    prog1 = eng.load(P1.to_bytes())
    gh1 = eng.load_gen(prog1, blob1)
    for k in (1, 2, 4, 16, 64):
        reqs = [(prog1, gh1, 7 + q, 1 << 40, 64, None) for q in range(k)]
        one = [eng.search(*r[:5], early_exit=True)[0] for r in reqs]
        assert [r[0] for r in eng.search_batch(reqs)] == one
        ts, tb = alternate(lambda: [eng.search(*r[:5], early_exit=True) for r in reqs],
                           lambda: eng.search_batch(reqs), args.reps)
        eng.search_batch(reqs)
        s, b = stat(ts), stat(tb)
        out["probe"][str(k)] = {"serial": s, "batched": dict(b, kernel_us=round(1e3 * eng.stats().last_kernel_ms, 1)),
                                "result": verdict(s, b)}
        print("probe", k, json.dumps(out["probe"][str(k)]), flush=True)

    # the max-tier rule: eight light entries alone, then with one heavy entry (sha3's first bucket)
    light = [(prog1, gh1, 7 + q, 0, 4096, None) for q in range(8)]
    hb = partition.partition([c.raw for c in workloads.WORKLOADS["sha3_keyed_mapping"]()])[0]
    Ph, blobh = search.prepare(hb)
    progh = eng.load(Ph.to_bytes())
    ghh = eng.load_gen(progh, blobh)
    heavy = (progh, ghh, 7, 0, 4096, None)
    ta, tb = alternate(lambda: eng.search_batch(light), lambda: eng.search_batch(light + [heavy]), args.reps)
    th, _ = alternate(lambda: eng.search_batch([heavy]), lambda: None, args.reps)
    eng.search_batch(light)
    k_light = eng.stats().last_kernel_ms
    eng.search_batch(light + [heavy])
    k_mixed = eng.stats().last_kernel_ms
    eng.search_batch([heavy])
    k_heavy = eng.stats().last_kernel_ms
    out["tier"] = {"light_x8": dict(stat(ta), kernel_us=round(1e3 * k_light, 1)),
                   "light_x8_plus_heavy": dict(stat(tb), kernel_us=round(1e3 * k_mixed, 1)),
                   "heavy_alone": dict(stat(th), kernel_us=round(1e3 * k_heavy, 1))}
    print("tier", json.dumps(out["tier"]), flush=True)
    for h, g in ((ghh, progh), (gh1, prog1)):
        eng.free_gen(h)
        eng.free(g)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"wrote": args.out}))


if __name__ == "__main__":
    main()
