"""Instructions per candidate of the O3 tier's search kernel on the CPU simulator (tests/asmsim):
the simulator's driver compiles the kernel as the engine does (this tree's jit.cpp through comgr, no
GPU: ASMSIM_O3_DUMP), tools/o3dis.py disassembles it, and the driver runs it over a window of
64-candidate groups with full evaluation (ASMSIM_SEARCH_SOURCE_DIR), its verdicts and hits checked
against the C port.  Exits 1 when a kernel's hits differ from the C port's or the simulator refuses it.
VALU / SALU lane-instructions per candidate (SQ_INSTS_VALU x 64 / candidates) and LDS bank-conflict
cycles (SQ_LDS_BANK_CONFLICT) per 64 candidates, without a GPU.

  python tools/o3_count.py [workload ...] [--lines] [--top N] [K=V ...]

--lines: compile with line tables and print the source statements costing the most VALU."""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def o3_kernel(exe, rec, env, lines=False, tmp=None):
    """(sim text, O3 source) of the search record's kernels, compiled by the driver `exe`"""
    tmp = tmp or tempfile.mkdtemp(prefix="o3count")
    e = dict(env, ASMSIM_O3_DUMP=tmp)
    if lines:
        e["MYTHGPU_JIT_EXTRA"] = (e.get("MYTHGPU_JIT_EXTRA", "") + " -gline-tables-only").strip()
    r = subprocess.run([str(exe)], input=rec, capture_output=True, env=e)
    if r.returncode:
        raise RuntimeError("O3 compile failed: " + r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:])
    from tools.o3dis import convert
    return convert(os.path.join(tmp, "0.co"), lines=lines), Path(tmp, "0.hip").read_text()


def main():
    from mythril_amd import search, workloads
    from tests.test_asm_sim import _cached, record

    class TPF:
        def mktemp(self, name):
            return Path(tempfile.mkdtemp(prefix=name))

    args = sys.argv[1:]
    lines = "--lines" in args
    top = 30
    if "--top" in args:
        top = int(args[args.index("--top") + 1])
    env = dict(os.environ)
    names = []
    skip = False
    for i, a in enumerate(args):
        if skip:
            skip = False
            continue
        if a == "--top":
            skip = True
        elif a.startswith("--"):
            continue
        elif "=" in a:
            k, v = a.split("=", 1)
            env[k] = v
        else:
            names.append(a)
    names = names or sorted(workloads.WORKLOADS)
    exe = _cached(TPF(), sanitize=False)
    differ = 0
    for name in names:
        tmp = tempfile.mkdtemp(prefix="o3count")
        P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[name]()])
        rec = record(0, P.to_bytes(), blob, 7, 1 << 40, 64 * 64)
        text, src = o3_kernel(exe, rec, env, lines, tmp)
        Path(tmp, "0.s").write_text(text)
        r = subprocess.run([str(exe)], input=rec, capture_output=True,
                           env=dict(env, ASMSIM_COUNT="1", ASMSIM_SEARCH_SOURCE_DIR=tmp))
        out = r.stdout.decode()
        cnt = [ln for ln in out.splitlines() if ln.startswith("count record")]
        summ = [ln for ln in out.splitlines() if ln.startswith("records=")]
        ok = bool(summ) and " ok=1 " in summ[0]
        differ += not ok
        print(name, cnt[0].split(":", 1)[1].strip() if cnt else out[-300:] + r.stderr.decode()[-300:],
              "" if ok else "HITS DIFFER from the C port: %s %s" % (summ[0] if summ else "?", out[:300]))
        if lines:
            srcl = src.splitlines()
            # the comgr shim's lines come first: the kernel's signature line locates the offset
            sig = next(i for i, l in enumerate(srcl, 1) if "mgj_search(" in l)
            first = int(re.search(r"; vcode line (\d+)", text).group(1))
            off = first - sig
            rows = []
            for ln in out.splitlines():
                if ln.startswith("count tag vcode line "):
                    a, v = ln[len("count tag vcode line "):].rsplit(":", 1)
                    v = v.split(" salu ")[0]
                    n = int(a) - off
                    rows.append((float(v), n, srcl[n - 1][:140] if 0 < n <= len(srcl) else "?"))
            for v, n, t in sorted(rows, reverse=True)[:top]:
                print("  %7.2f %5d %s" % (v, n, t))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
