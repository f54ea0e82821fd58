"""The climbing search (``search.search(climb=ClimbConfig())``, ``mg_search_scored``) measured.

Part 1, the simulated LASER query streams of ``tools/stream_bench.py``: ``search_partitioned`` with
climb off and on, query by query, the modes alternating within a repeat after one untimed pass of
both (as ``tools/warm_bench.py`` does).  Per stream and mode: queries, sat answers, queries the
climb ran on and answered, p50 / p99 of the candidates and of the time to first model over the sat
queries, rounds used and the kernel time per round.  Every query is bounded by
``--max-candidates`` under a generous timeout and stays on the interpreter (``jit="never"``), so
the answers do not depend on the clock.

Part 2, the conjunctions that need a consistent assignment (``workloads.climb_star`` with 4, 6, 8
and 10 roots of probability 2^-6, ``workloads.climb_chain`` with 8): per seed, plain sampling
against the climb, candidates and time to first model; for the chain the best violation count of
every round of a long climb (its stall).

What must hold (exit status 1 otherwise): every stream query answered sat with climb off is
answered sat with climb on, with the same counts in every repeat.  No threshold is set on the
times or on the families.

``--device``: the same streams and conjunctions (and the chain's long climb) with the host climb
against the device climb (``ClimbConfig(device=True)``, ``mg_search_climb``), alternating in one
process: wall time per climb round, time to first model and kernel time per round for each path,
to ``profiles/climb_device.json``.  Exit status 1 when the two paths do not run the same search.

usage: python tools/climb_bench.py [--repeats 5] [--workloads a,b] [--out profiles/climb_stream.json] [--device]
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

SEEDS = (0x6D797468, 12345, 987654321, 555, 20240229)


def pct(xs, p):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(round(p * (len(xs) - 1))))] if xs else None


def r3(x):
    return None if x is None else round(x, 3)


def run_stream(eng, queries, cfg, max_candidates, timeout_s):
    """One pass over a stream: per query (sat, climb ran, climb answered, candidates, ms, rounds,
    kernel ms of its rounds)."""
    out = []
    for _, q in queries:
        roots = [c.raw for c in q]
        t = time.perf_counter()
        r = search.search_partitioned(eng, roots, batch=False, timeout_s=timeout_s, max_candidates=max_candidates,
                                      jit="never", climb=cfg)
        ms = (time.perf_counter() - t) * 1e3
        # a query of several buckets: search_partitioned keeps no per-bucket timing, the engine's
        # record of the last search does
        last = search.LAST_RESULT.timing if search.LAST_RESULT is not None else {}
        tm = r.timing if "climb_rounds" in r.timing else last
        rounds = tm.get("climb_rounds", 0)
        out.append((r.index is not None, rounds > 0, "climb" in str(getattr(r, "engine", "")),
                    r.scanned + tm.get("climb_candidates", 0), ms, rounds, list(tm.get("climb_kernel_ms", [])),
                    tm.get("climb_ms", 0.0)))
    return out


def summarize(passes):
    first = passes[0]
    sat_ms = [q[4] for p in passes for q in p if q[0]]
    sat_cand = [q[3] for q in first if q[0]]
    kms = [k for p in passes for q in p for k in q[6]]
    return {"queries": len(first), "sat": sum(q[0] for q in first), "climb_ran": sum(q[1] for q in first),
            "climb_answers": sum(q[2] for q in first), "climb_rounds": sum(q[5] for q in first),
            "first_model_candidates_p50": pct(sat_cand, 0.5), "first_model_candidates_p99": pct(sat_cand, 0.99),
            "first_model_ms_p50": r3(pct(sat_ms, 0.5)), "first_model_ms_p99": r3(pct(sat_ms, 0.99)),
            "round_kernel_ms_p50": r3(pct(kms, 0.5)), "round_kernel_ms_p99": r3(pct(kms, 0.99)),
            "counts_stable": all([q[:4] + (q[5],) for q in p] == [q[:4] + (q[5],) for q in first] for p in passes)}


def family(eng, label, roots, plain_candidates, cfg, timeout_s):
    """Plain sampling against the climb on one query, per seed."""
    runs = []
    for seed in SEEDS:
        row = {"seed": seed}
        for mode, c in (("plain", None), ("climb", cfg)):
            t = time.perf_counter()
            r = search.search(eng, roots, seed=seed, max_candidates=plain_candidates, timeout_s=timeout_s, jit="never",
                              climb=c)
            ms = (time.perf_counter() - t) * 1e3
            row[mode] = {"sat": r.index is not None, "engine": r.engine,
                         "candidates": r.scanned + r.timing.get("climb_candidates", 0), "ms": r3(ms),
                         "rounds": r.timing.get("climb_rounds"), "best_violations": r.timing.get("climb_best"),
                         "round_kernel_ms": [r3(k) for k in r.timing.get("climb_kernel_ms", [])]}
        runs.append(row)
    out = {"query": label, "roots": len(roots), "plain_max_candidates": plain_candidates, "runs": runs}
    for mode in ("plain", "climb"):
        sat = [x[mode] for x in runs if x[mode]["sat"]]
        out[mode] = {"sat": len(sat), "of": len(runs), "candidates_p50": pct([x["candidates"] for x in sat], 0.5),
                     "ms_p50": r3(pct([x["ms"] for x in sat], 0.5))}
    return out


def chain_stall(eng, roots, rounds, chunk=4096):
    """A long climb on the chain: the best violation count after every round, per seed."""
    P, blob = search.prepare(roots, None)
    prog = eng.load(P.to_bytes())
    gh = eng.load_gen(prog, blob)
    out = []
    try:
        for seed in SEEDS:
            r = search.climb(eng, P, prog, gh, seed, chunk, search.ClimbConfig(rounds=rounds, beam=8, patience=rounds))
            best = [min(sl[1] for sl in slots if sl is not None) for slots in r.trajectory]
            out.append({"seed": seed, "solved": r.index is not None, "rounds": r.rounds, "candidates": r.candidates,
                        "best_violations_by_round": best})
    finally:
        eng.free_gen(gh)
        eng.free(prog)
    return out


PATHS = (("host", False), ("device", True))


def per_round(passes):
    """Wall and kernel time per climb round over the queries on which the climb ran: the climb's
    time (``timing["climb_ms"]``) and its kernels' (per round on the host path, per burst on the
    device path) over its rounds."""
    ran = [q for p in passes for q in p if q[5]]
    rounds = sum(q[5] for q in ran)
    return {"round_wall_ms": r3(sum(q[7] for q in ran) / rounds) if rounds else None,
            "round_kernel_ms": r3(sum(sum(q[6]) for q in ran) / rounds) if rounds else None,
            "climb_ms_p50": r3(pct([q[7] for q in ran], 0.5))}


def device_streams(eng, names, a):
    rows = []
    for name in names:
        qs = stream_queries(name)
        cfgs = {p: search.ClimbConfig(device=d) for p, d in PATHS}
        run = lambda c: run_stream(eng, qs, c, a.max_candidates, a.timeout_s)
        for c in cfgs.values():
            run(c)  # untimed
        passes = {p: [] for p in cfgs}
        for _ in range(a.repeats):
            for p, c in cfgs.items():
                passes[p].append(run(c))
        row = {"workload": name, "max_candidates": a.max_candidates, "repeats": a.repeats}
        for p in cfgs:
            row[p] = dict(summarize(passes[p]), **per_round(passes[p]))
        # the same search: the same answers, rounds and candidates query by query
        row["same_counts"] = [q[:4] + (q[5],) for q in passes["host"][0]] == [q[:4] + (q[5],) for q in passes["device"][0]]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def device_family(eng, label, roots, cfg_kw, a, repeats=3, chunk=4096):
    """Host climb against device climb on one query through ``search.search``, per seed: time to the
    first model (the ordinary first launch included), the climb's wall time per round and its kernel
    time per round; the paths alternate, after one untimed run of each."""
    runs = []
    for seed in SEEDS:
        row = {"seed": seed}
        for p, d in PATHS:
            row[p] = {"ms": [], "climb_ms": [], "kernel_ms": []}
        for rep in range(repeats + 1):
            for p, d in PATHS:
                cfg = search.ClimbConfig(device=d, **cfg_kw)
                t = time.perf_counter()
                # one ordinary launch, the climb, and after a climb that missed one ordinary launch more
                r = search.search(eng, roots, seed=seed, chunk=chunk, max_candidates=2 * chunk, timeout_s=a.timeout_s,
                                  jit="never", climb=cfg)
                ms = (time.perf_counter() - t) * 1e3
                x = row[p]
                x.update({"sat": r.index is not None, "index": r.index, "rounds": r.timing.get("climb_rounds"),
                          "best_violations": r.timing.get("climb_best")})
                if rep:
                    x["ms"].append(ms)
                    x["climb_ms"].append(r.timing.get("climb_ms", 0.0))
                    x["kernel_ms"].append(sum(r.timing.get("climb_kernel_ms", [])))
        for p, _ in PATHS:
            x = row[p]
            x["ms"], x["climb_ms"], x["kernel_ms"] = (r3(pct(x[k], 0.5)) for k in ("ms", "climb_ms", "kernel_ms"))
        row["same_search"] = all(row["host"][k] == row["device"][k] for k in ("sat", "index", "rounds", "best_violations"))
        runs.append(row)
    out = {"query": label, "roots": len(roots), "config": cfg_kw or "default", "chunk": chunk, "runs": runs,
           "same_search": all(x["same_search"] for x in runs)}
    for p, _ in PATHS:
        xs = [x[p] for x in runs]
        sat = [x for x in xs if x["sat"]]
        rounds = sum(x["rounds"] or 0 for x in xs)
        out[p] = {"sat": len(sat), "of": len(xs), "rounds_min": min(x["rounds"] for x in xs), "rounds_max": max(x["rounds"] for x in xs),
                  "first_model_ms_p50": r3(pct([x["ms"] for x in sat], 0.5)), "ms_p50": r3(pct([x["ms"] for x in xs], 0.5)),
                  "round_wall_ms": r3(sum(x["climb_ms"] for x in xs) / rounds) if rounds else None,
                  "round_kernel_ms": r3(sum(x["kernel_ms"] for x in xs) / rounds) if rounds else None}
    print(json.dumps({k: v for k, v in out.items() if k != "runs"}), flush=True)
    return out


def main_device(a, eng):
    """``--device``: everything above again, host climb against device climb in one process."""
    names = [w for w in a.workloads.split(",") if w]
    doc = {"tool": "tools/climb_bench.py --device", "device": f"gfx950 ({eng.stats().cu_count} CUs)",
           "config": {"rounds": 16, "beam": 8, "patience": 4, "chunk": 4096, "burst": 8},
           "streams": device_streams(eng, names, a), "families": [], "chain_long": None}
    for n in (4, 6, 8, 10):
        doc["families"].append(device_family(eng, f"star{n}", workloads.climb_star(n, f"st{n}"), {}, a))
    chain = workloads.climb_chain(8)
    doc["families"].append(device_family(eng, "chain8", chain, {}, a))
    doc["chain_long"] = device_family(eng, "chain8", chain, {"rounds": a.chain_rounds, "patience": a.chain_rounds}, a)
    out = a.out if a.out != str(ROOT / "profiles" / "climb_stream.json") else str(ROOT / "profiles" / "climb_device.json")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(doc, indent=1) + "\n")
    differ = [r["workload"] for r in doc["streams"] if not r["same_counts"]]
    differ += [f["query"] for f in doc["families"] + [doc["chain_long"]] if not f["same_search"]]
    if differ:
        print("host and device climb differ on:", ", ".join(differ), file=sys.stderr)
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true",
                    help="host climb against device climb (ClimbConfig(device=True)); writes profiles/climb_device.json")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default=",".join(workloads.WORKLOADS))
    ap.add_argument("--max-candidates", type=int, default=1 << 22)
    ap.add_argument("--family-candidates", type=int, default=1 << 24)
    ap.add_argument("--chain-rounds", type=int, default=48)
    ap.add_argument("--timeout-s", type=float, default=30.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "climb_stream.json"))
    a = ap.parse_args()
    eng = native.Engine.get()
    if a.device:
        return main_device(a, eng)
    cfg = search.ClimbConfig()
    rows, lost, unstable = [], [], []
    t0 = time.perf_counter()
    for name in [w for w in a.workloads.split(",") if w]:
        qs = stream_queries(name)
        run = lambda c: run_stream(eng, qs, c, a.max_candidates, a.timeout_s)
        run(None), run(cfg)  # untimed
        off, on = [], []
        for _ in range(a.repeats):
            off.append(run(None))
            on.append(run(cfg))
        for (label, _), x, y in zip(qs, off[0], on[0]):
            if x[0] and not y[0]:
                lost.append(f"{name}/{label}")
        row = {"workload": name, "max_candidates": a.max_candidates, "repeats": a.repeats,
               "off": summarize(off), "on": summarize(on)}
        if not (row["off"]["counts_stable"] and row["on"]["counts_stable"]):
            unstable.append(name)
        rows.append(row)
        print(json.dumps(row), f"[{time.perf_counter() - t0:.0f} s]", flush=True)
    fams = []
    for n in (4, 6, 8, 10):
        fams.append(family(eng, f"star{n}", workloads.climb_star(n, f"st{n}"), a.family_candidates, cfg, a.timeout_s))
        print(json.dumps({k: v for k, v in fams[-1].items() if k != "runs"}), flush=True)
    chain = workloads.climb_chain(8)
    fams.append(family(eng, "chain8", chain, a.family_candidates, cfg, a.timeout_s))
    print(json.dumps({k: v for k, v in fams[-1].items() if k != "runs"}), flush=True)
    stall = chain_stall(eng, chain, a.chain_rounds)
    print(json.dumps(stall), flush=True)
    doc = {"tool": "tools/climb_bench.py", "device": f"gfx950 ({eng.stats().cu_count} CUs)",
           "config": {"rounds": cfg.rounds, "beam": cfg.beam, "patience": cfg.patience, "chunk": 4096},
           "streams": rows, "sat_lost_with_climb_on": lost, "streams_with_unstable_counts": unstable,
           "families": fams, "chain_stall": {"rounds": a.chain_rounds, "chunk": 4096, "runs": stall}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    if lost:
        print("answered sat with climb off but not with climb on:", ", ".join(lost), file=sys.stderr)
    if unstable:
        print("counts differ between repeats:", ", ".join(unstable), file=sys.stderr)
    return 1 if lost or unstable else 0


if __name__ == "__main__":
    sys.exit(main())
