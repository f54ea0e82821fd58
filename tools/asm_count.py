"""Instructions per candidate of the first tier's search kernel on the CPU simulator (tests/asmsim):
every workload, a full-evaluation launch (no early exit) over a window of 64-candidate groups, VALU
and SALU lane-instructions per candidate (the PMC's SQ_INSTS_VALU x 64 / candidates, without a GPU).

  python tools/asm_count.py [workload ...] [--env K=V ...]   (ASMSIM_SEED / ASMSIM_START / ASMSIM_GROUPS: the window;
   ASMSIM_JSONL=file ASMSIM_LABEL=name: append each workload's counts to a JSON-lines file)"""
import json
import os
import random
import re
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    from mythril_amd import search, workloads
    from tests.test_asm_sim import _cached, record
    import pytest  # noqa: F401  (the builder's skip path)

    class TPF:  # the fixture's tmp_path_factory, outside pytest
        def mktemp(self, name):
            import tempfile
            return Path(tempfile.mkdtemp(prefix=name))

    names = [a for a in sys.argv[1:] if "=" not in a] or sorted(workloads.WORKLOADS)
    env = dict(os.environ, ASMSIM_COUNT="1")
    for a in sys.argv[1:]:
        if "=" in a:
            k, v = a.split("=", 1)
            env[k.lstrip("-")] = v
    exe = _cached(TPF(), sanitize=False)
    for name in names:
        P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
        # ASMSIM_SEED / ASMSIM_START / ASMSIM_GROUPS: the window (default seed 7, 64 groups from 2^40)
        rec = record(0, P.to_bytes(), blob, int(env.get("ASMSIM_SEED", "7"), 0), int(env.get("ASMSIM_START", str(1 << 40)), 0),
                     64 * int(env.get("ASMSIM_GROUPS", "64"), 0))
        r = subprocess.run([str(exe)], input=rec, capture_output=True, env=env)
        line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("count record")]
        summ = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("records=")]
        ok = bool(summ) and " ok=1 " in summ[0]
        print(name, line[0].split(":", 1)[1].strip() if line else r.stdout.decode()[-300:] + r.stderr.decode()[-300:],
              "" if ok else "(DIFFERS from the C port: %s)" % (r.stdout.decode()[-400:]))
        # MYTHGPU_JIT_ASM_ANNOTATE=1: the program instructions costing the most VALU per candidate
        tags = []
        for ln in r.stdout.decode().splitlines():
            if ln.startswith("count tag "):
                t, v = ln[len("count tag "):].rsplit(":", 1)
                va, _, sa = v.strip().partition(" salu ")
                tags.append((float(va), float(sa or 0), t.strip()))
        # guarded select arms (jit_asm.cpp: plan_lazy): a region's select tag names its selects, so their
        # simulated count over that number is the share of all groups that took the region
        for v, sv, t in tags:
            m = re.match(r"vcode (\d+) lazy:select x(\d+)$", t)
            if m and int(m.group(2)):
                print(f"  guard closing at vcode {m.group(1)}: region taken by {v / int(m.group(2)):.3f} of the groups")
        # the MIXED generator's phases over all coordinates and emission sites: VALU and SALU per group
        # (a phase emitted in several alternatives, or per limb, is one tag per site above)
        mixed = {}
        for v, sv, t in tags:
            m = re.match(r"vcode \d+ (mixed:\w+)$", t)
            if m:
                a = mixed.setdefault(m.group(1), [0.0, 0.0])
                a[0] += v
                a[1] += sv
        if mixed:
            print("  MIXED phases (VALU, SALU per group): " +
                  "  ".join(f"{k[6:]} {a[0]:.2f}/{a[1]:.2f}" for k, a in sorted(mixed.items())))
        if env.get("ASMSIM_JSONL") and line:
            words = line[0].split(":", 1)[1].split()
            rec = {"workload": name, "label": env.get("ASMSIM_LABEL", ""), "seed": int(env.get("ASMSIM_SEED", "7"), 0),
                   "start": int(env.get("ASMSIM_START", str(1 << 40)), 0), "groups": int(env.get("ASMSIM_GROUPS", "64"), 0),
                   "equals_c_port": ok,
                   "per_group": {words[i]: float(words[i + 1]) for i in range(0, len(words) - 2, 2)},
                   "mixed_phases": {k[6:]: {"valu": round(a[0], 2), "salu": round(a[1], 2)} for k, a in sorted(mixed.items())}}
            with open(env["ASMSIM_JSONL"], "a") as f:
                f.write(json.dumps(rec) + "\n")
        key = (lambda x: x[1]) if env.get("ASMSIM_SORT") == "salu" else (lambda x: x[0])
        for v, sv, t in sorted(tags, key=key, reverse=True)[:int(env.get("ASMSIM_TOP", "40"))]:
            print(f"  {v:8.2f} {sv:8.2f}  {t}")


if __name__ == "__main__":
    main()
