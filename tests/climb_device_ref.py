"""Helpers of the device-climb tests: a stand-in engine whose ``search_climb`` is the reference sweep
(``tests/scored_ref.py``) and the Python population rule, and the comparison of two ``ClimbResult``.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from mythril_amd import native, search
from tests import scored_ref


def result_fields(res: search.ClimbResult):
    """Everything two runs of the same climb must agree on (not the times)."""
    return {
        "trajectory": res.trajectory, "rounds": res.rounds, "candidates": res.candidates, "best": res.best,
        "stop": res.stop, "index": res.index, "hits": res.hits,
        "assign": None if res.assign is None else np.asarray(res.assign).tolist(),
        "population": [(v, i, dict(m)) for v, i, m in res.population],
    }


def assert_same(got: search.ClimbResult, want: search.ClimbResult, what=""):
    g, w = result_fields(got), result_fields(want)
    for k in w:
        assert g[k] == w[k], (what, k)


class DeviceStandIn(scored_ref.RefEngine):
    """``RefEngine`` plus ``search_climb`` as ``native.Engine`` has it: the contract of
    ``mg_search_climb`` (include/mythgpu.h) restated in Python over the reference sweep."""

    def __init__(self, P, blob):
        super().__init__(P, blob)
        self.climbs = []

    def search_climb(self, prog, gen, cmap, seed, chunk, rounds=16, beam=8, patience=4, burst=8, seeds=None,
                     cancel=None, budget_s=None):
        P = self.P
        self.climbs.append({"rounds": rounds, "beam": beam, "patience": patience, "burst": burst})
        out = native.DeviceClimb()
        pop, stale, stop = [], 0, None
        rows = np.zeros((cmap.n_rows, 0), dtype=np.uint32)
        for r in range(rounds):
            if r % burst == 0:
                if cancel is not None and cancel.is_set():
                    stop = "cancel"
                    break
                if budget_s is not None and budget_s <= 0:
                    stop = "budget"
                    break
            if r:
                seeds = native.SeedSet(rows, cmap.coord_row, np.where(cmap.coord_row != native.MG_NONE, 0xFFFFFFFF, 0),
                                       keep16=cmap.keep16)
            first, nh, slots, assigns = self.search_scored(prog, gen, seeds, seed, r * chunk, chunk)
            out.rounds += 1
            out.trajectory.append(list(slots))
            if first is not None:
                out.index, out.hits, out.best, stop = first, nh, 0, "hit"
                out.assign = np.array(assigns[(first >> 6) & 31], dtype=np.uint32)
                break
            winners = [(sl[1], sl[0], search.coords_from_assignment(P, assigns[s]))
                       for s, sl in enumerate(slots) if sl is not None]
            pop = search.next_population(pop, winners, beam)
            if not pop:
                stop = "rounds"
                break
            s = search.population_seeds(P, [m for _, _, m in pop])
            # the row map is population_seeds' layout
            assert np.array_equal(s.coord_row, cmap.coord_row) and s.keep16 == cmap.keep16
            rows = s.rows
            if out.best is None or pop[0][0] < out.best:
                out.best, stale = pop[0][0], 0
            else:
                stale += 1
                if stale >= patience:
                    stop = "patience"
                    break
        out.stop = stop or "rounds"
        out.population = [(v, i) for v, i, _ in pop]
        out.pop_rows = rows
        out.kernel_ms = [0.0] * ((out.rounds + burst - 1) // burst)
        return out
