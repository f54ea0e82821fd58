"""Reference of the scored sweep (``include/mythgpu.h``, "scored sweep") and of the climbing
search built on it (``search.climb``): the seeded candidates of ``tests/seeded_ref.py``, the C
port's value of every distinct root node under each candidate (the roots as the watch list), and
numpy for violations, slot minima, hits and the climb loop, restated here from the documented
rules.  Test infrastructure only."""
from __future__ import annotations

import copy

import numpy as np

from mythril_amd import native, search, ssa
from oracle import cport
from tests import seeded_ref

SLOTS = 32


def root_values(P: ssa.Program, soa: np.ndarray, n: int) -> np.ndarray:
    """[distinct root][candidate] 0/1: the C port's value of every distinct root node."""
    Q = copy.copy(P)
    Q.set_watch(dict.fromkeys(P.roots))
    assert all(Q.watch_width(r) == 1 for r in Q.watch)
    _, rows = cport.eval_soa(Q.to_bytes(), soa, n, watch_words=Q.watch_words)
    return rows & 1


class Scored:
    """The scored sweep of ``[start, start + count)``: ``viol[q]`` of candidate ``start + q``,
    ``first`` / ``hits`` as a search reports them, ``slots[s]`` = ``(index, violations)`` or None,
    and ``soa``, the candidates' coordinates."""

    def __init__(self, P, gen_blob, seeds, seed, start, count):
        seeds = seeds if seeds is not None else native.SeedSet()
        self.start, self.count = start, count
        self.soa = seeded_ref.seeded_soa(P, gen_blob, seeds, seed, start, count)
        self.viol = (root_values(P, self.soa, count) == 0).sum(axis=0).astype(np.int64)
        hit = np.flatnonzero(self.viol == 0)
        self.first = start + int(hit[0]) if hit.size else None
        self.hits = int(hit.size)
        idx = start + np.arange(count, dtype=object)
        slot = np.array([(int(i) >> 6) % SLOTS for i in idx])
        self.slot_of = slot
        self.slots = []
        for s in range(SLOTS):
            q = np.flatnonzero(slot == s)
            if not q.size:
                self.slots.append(None)
                continue
            best = q[np.argmin(self.viol[q])]  # argmin: the first (lowest index) of the minima
            self.slots.append((start + int(best), int(self.viol[best])))

    def column(self, index: int) -> np.ndarray:
        return self.soa[:, index - self.start]


def watch_rows(P: ssa.Program, soa_cols: np.ndarray) -> np.ndarray:
    """The program's watch rows of the given candidates, [candidate][watch_words]."""
    n = soa_cols.shape[1]
    if P.watch_words == 0 or n == 0:
        return np.zeros((n, max(P.watch_words, 1)), dtype=np.uint32)
    _, rows = cport.eval_soa(P.to_bytes(), np.ascontiguousarray(soa_cols), n, watch_words=P.watch_words)
    return np.ascontiguousarray(rows.T)


class RefEngine:
    """A stand-in for ``native.Engine`` whose ``search_scored`` is the reference (one program and
    generator; the handles are ignored).  ``calls`` records every sweep's arguments."""

    def __init__(self, P: ssa.Program, gen_blob):
        self.P, self.blob = P, gen_blob
        self.calls = []

    def search_scored(self, prog, gen, seeds, seed, start, count, early_exit=False, assigns=None, want_assigns=True):
        self.calls.append((seeds, seed, start, count))
        sc = Scored(self.P, self.blob, seeds, seed, start, count)
        ww = self.P.watch_words
        out = np.zeros((SLOTS, max(ww, 1)), dtype=np.uint32)
        used = [s for s in range(SLOTS) if sc.slots[s] is not None]
        if used:
            cols = np.stack([sc.column(sc.slots[s][0]) for s in used], axis=1)
            out[used, :max(ww, 1)] = watch_rows(self.P, cols)[:, :max(ww, 1)]
        return sc.first, sc.hits, sc.slots, out


def climb_ref(P: ssa.Program, gen_blob, seed: int, chunk: int, rounds: int = 16, beam: int = 8, patience: int = 4):
    """The climb loop restated from its rule, on the reference sweep.  Returns ``(first hit or
    None, rounds run, [slots of every round], best violation count)``.

    Round r sweeps [r chunk, (r + 1) chunk); round 0 unseeded, later rounds seeded from the
    population with keep16 = warm_keep16(seeded coordinates).  New population: the best ``beam``
    distinct assignments among this round's slot winners and the previous population, ordered by
    violations, then this round before the previous population, then index."""
    eng = RefEngine(P, gen_blob)
    pop = []  # (viol, index, {coord: value})
    traj, best, stale = [], None, 0
    for r in range(rounds):
        seeds = None
        if r:
            models = [m for _, _, m in pop]
            cs = sorted({c for m in models for c in m})
            seeds = seeded_ref.seed_set(P, models, keep16=search.warm_keep16(len(cs)))
        first, _, slots, assigns = eng.search_scored(0, 0, seeds, seed, r * chunk, chunk)
        traj.append(slots)
        if first is not None:
            return first, r + 1, traj, 0
        entries = [(sl[1], 0, sl[0], search.coords_from_assignment(P, assigns[s]))
                   for s, sl in enumerate(slots) if sl is not None]
        entries += [(v, 1, i, m) for v, i, m in pop]
        entries.sort(key=lambda e: (e[0], e[1], e[2]))
        pop, seen = [], []
        for v, _, i, m in entries:
            if m in seen:
                continue
            seen.append(m)
            pop.append((v, i, m))
            if len(pop) == beam:
                break
        if best is None or pop[0][0] < best:
            best, stale = pop[0][0], 0
        else:
            stale += 1
            if stale >= patience:
                return None, r + 1, traj, best
    return None, rounds, traj, best
