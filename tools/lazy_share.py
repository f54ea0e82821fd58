"""How often the conditions of a workload's wide selects are uniform over a 64-candidate group, from
the C port alone (no GPU, no emitter): for every wide ITE and every prior of every wide LOOKUP of
the specialised program, the share of lanes in which the condition / key test holds and the share
of aligned groups in which it holds in no lane and in every lane.  These are the groups the first
tier's guarded select arms skip (jit_asm.cpp: plan_lazy).

The candidates are the generator's own (``cport.gen_soa``); a condition's value is the verdict of
the specialised program cut after the condition's definition with the condition asserted alone,
evaluated by ``oracle/kops.run``.

  python tools/lazy_share.py [workload] [--groups 512] [--start 0] [--seed 0x6D797468]"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="token_transfer_underflow")
    ap.add_argument("--groups", type=int, default=512)
    ap.add_argument("--start", type=lambda x: int(x, 0), default=0)
    ap.add_argument("--seed", type=lambda x: int(x, 0), default=0x6D797468)
    a = ap.parse_args()
    from mythril_amd import native, search, workloads
    from oracle import cport, kops

    P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[a.workload]()])
    pb = P.to_bytes()
    spec = native.specialized_program(pb, blob)
    code = np.asarray(spec["code"]).tolist()
    aux = np.asarray(spec["aux"]).tolist()
    widths = [c.width for c in P.coords]
    words = sum((w + 31) // 32 for w in widths)
    start = a.start & ~63
    n = 64 * a.groups
    soa = cport.gen_soa(pb, blob, a.seed, start, n, words)
    free_id = 1 + max(int(r[2]) for r in code if int(r[2]) != kops.NONE)

    # (label, rows of the program that compute the condition, the condition's value id)
    probes = []
    for k, r in enumerate(code):
        op, W, d, x, y, c, p0, p1 = r
        if W <= 1:
            continue
        body = [q for q in code[:k] if q[0] not in (kops.K_ASSERT, kops.K_WATCH)]
        if op == kops.K_ITE:
            probes.append((f"row {k} ITE w {W}: condition value {x}", body, x))
        elif op == kops.K_LOOKUP:
            for p in range(c):
                kv = aux[p1 + 2 * p]
                eq = [kops.K_EQ, 1, free_id, x, kv, kops.NONE, 0, y]
                probes.append((f"row {k} LOOKUP w {W}, {c} prior(s): key test of prior {p}", body + [eq], free_id))
    cols = np.asarray(soa).T.tolist()
    cands = []
    for col in cols:
        coords, row = [], 0
        for w in widths:
            L = (w + 31) // 32
            coords.append(kops._limbs_to_int(col[row:row + L]))
            row += L
        cands.append(coords)
    print(f"{a.workload}: {a.groups} groups of 64 from {start}, seed {a.seed:#x}")
    for label, body, v in probes:
        cut = dict(spec, code=body + [[kops.K_ASSERT, 1, kops.NONE, v, kops.NONE, kops.NONE, 0, 0]],
                   consts=np.asarray(spec["consts"]).tolist(), aux=aux)
        t = np.array([kops.run(cut, c) for c in cands], dtype=np.uint8).reshape(-1, 64).sum(axis=1)
        print(f"  {label}: lanes true {t.sum() / n:.4f}, groups all-false {np.mean(t == 0):.3f}, "
              f"all-true {np.mean(t == 64):.3f}")


if __name__ == "__main__":
    main()
