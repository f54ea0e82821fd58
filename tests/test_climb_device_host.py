"""The device climb's host side without a GPU: the row map (``search.climb_map``) against
``coords_from_assignment`` and ``population_seeds``, ``search.climb(device=True)`` on a stand-in
engine (``tests/climb_device_ref.py``) against the host loop, the configuration and the hook's
switch."""
import random

import numpy as np
import pytest

from mythril_amd import native, search, ssa, workloads
from mythril_amd.smt import terms as T
from tests import scored_ref
from tests.climb_device_ref import DeviceStandIn, assert_same
from tests.test_gpu_seeded import CASES, _parity_roots

SEED0 = 0x6D797468


def _prepared(roots):
    P = ssa.flatten(roots)
    P.set_watch(search.model_watch(P)[0])
    return P


def _programs():
    out = {"star": search.prepare(workloads.climb_star(8), None)[0], "chain": search.prepare(workloads.climb_chain(8), None)[0]}
    out.update({c: _prepared(_parity_roots(c)) for c in CASES})
    out.update({w: search.prepare([c.raw for c in fn()])[0] for w, fn in workloads.WORKLOADS.items()})
    return out


def _gather(P, cmap, assign):
    out = {}
    for c in P.coords:
        r = int(cmap.coord_row[c.index])
        if r != native.MG_NONE:
            out[c.index] = ssa.limbs_to_int(assign[cmap.watch_row[r:r + ssa.limbs(c.width)]])
    return out


def test_row_map_gathers_what_coords_from_assignment_reads():
    rng = random.Random(0xC0DE)
    kinds, skipped = set(), 0
    for name, P in _programs().items():
        cmap = search.climb_map(P)
        assert cmap is not None and search.climb_map(P) is cmap, name  # built once per program
        ww = sum(ssa.limbs(w) for w in search.model_watch(P)[1])  # the model watch rows, whatever P watches now
        assert cmap.n_rows >= 1 and (cmap.watch_row < ww).all() and len(set(cmap.watch_row.tolist())) == cmap.n_rows
        for _ in range(8):
            assign = np.array([rng.getrandbits(32) for _ in range(ww)], dtype=np.uint32)
            want = search.coords_from_assignment(P, assign)
            assert _gather(P, cmap, assign) == want, name
            # ... and laid out as population_seeds lays a population of such models out
            s = search.population_seeds(P, [want, want])
            assert np.array_equal(s.coord_row, cmap.coord_row) and s.keep16 == cmap.keep16, name
            assert np.array_equal(s.rows[:, 0], assign[cmap.watch_row]), name
        for c in P.coords:
            if cmap.coord_row[c.index] != native.MG_NONE:
                kinds.add((c.kind, c.width))
            else:  # LAZY sites and sites that are a slice of an AUX word
                skipped += 1
                assert search._is_lazy(P, c) or c.index in P.aux_slice, (name, c.name)
    widths = {w for _, w in kinds}
    assert {256, 40, 8, 1} <= widths and {k for k, _ in kinds} >= {ssa.COORD_SCALAR, ssa.COORD_ARRAY_SITE, ssa.COORD_AUX}
    assert skipped > 0


def test_no_row_map_when_widths_disagree_or_nothing_is_seeded(monkeypatch):
    P = _prepared(_parity_roots("light"))
    entries, widths, plan = search._model_layout(P)
    P._model_layout = (entries, [w + 1 if w == 40 else w for w in widths], plan)
    assert search.climb_map(P) is None
    # the host loop then runs, whatever the engine offers
    class NoClimb(scored_ref.RefEngine):
        def search_climb(self, *a, **kw):
            raise AssertionError("not the device path")

        def search_scored(self, *a, **kw):
            raise KeyError("the host loop")

    with pytest.raises(KeyError):
        search.climb(NoClimb(P, None), P, 1, 2, SEED0, 64, search.ClimbConfig(device=True))


@pytest.fixture(scope="module")
def star():
    return search.prepare(workloads.climb_star(8), None)


@pytest.mark.parametrize("kw", [{}, {"rounds": 3}, {"beam": 1, "rounds": 4}, {"beam": 5, "burst": 3, "rounds": 4},
                                {"patience": 1, "beam": 1, "rounds": 6}], ids=str)
def test_device_path_returns_the_host_loops_result(star, kw):
    P, blob = star
    chunk = 4096 if not kw else 256
    want = search.climb(scored_ref.RefEngine(P, blob), P, 1, 2, SEED0, chunk, search.ClimbConfig(**kw))
    eng = DeviceStandIn(P, blob)
    got = search.climb(eng, P, 1, 2, SEED0, chunk, search.ClimbConfig(device=True, **kw))
    assert len(eng.climbs) == 1 and eng.climbs[0]["burst"] == kw.get("burst", 8)
    assert_same(got, want, kw)
    assert len(got.kernel_ms) == (got.rounds + kw.get("burst", 8) - 1) // kw.get("burst", 8)
    if not kw:
        assert want.stop == "hit" and want.rounds == 8 and want.index == 28905


def test_device_path_cancel_and_deadline(star):
    P, blob = star

    class Set:
        def is_set(self):
            return True

    for kw, stop in (({"cancel": Set()}, "cancel"), ({"deadline": 0.0}, "budget")):
        want = search.climb(scored_ref.RefEngine(P, blob), P, 1, 2, SEED0, 256, search.ClimbConfig(), **kw)
        got = search.climb(DeviceStandIn(P, blob), P, 1, 2, SEED0, 256, search.ClimbConfig(device=True), **kw)
        assert (got.rounds, got.stop) == (0, stop)
        assert_same(got, want, stop)


def test_device_false_never_asks_the_engine_for_a_device_climb(star):
    P, blob = star
    eng = DeviceStandIn(P, blob)
    search.climb(eng, P, 1, 2, SEED0, 256, search.ClimbConfig(rounds=2))
    assert eng.climbs == [] and len(eng.calls) == 2


def test_config_is_checked():
    c = search.ClimbConfig()
    assert (c.rounds, c.beam, c.patience, c.device, c.burst) == (16, 8, 4, False, 8)
    c = search.ClimbConfig(device=True, burst=3)
    assert (c.device, c.burst) == (True, 3)
    for bad in ({"burst": 0}, {"burst": -1}, {"rounds": 0, "device": True}, {"beam": 33, "device": True}):
        with pytest.raises(ValueError):
            search.ClimbConfig(**bad)


def test_hook_switch(monkeypatch):
    from mythril_amd import plugin

    monkeypatch.delenv("MYTHGPU_CLIMB", raising=False)
    monkeypatch.setenv("MYTHGPU_CLIMB_DEVICE", "1")
    assert plugin._climb_kw() == {}  # only together with MYTHGPU_CLIMB
    monkeypatch.setenv("MYTHGPU_CLIMB", "1")
    cfg = plugin._climb_kw()["climb"]
    assert cfg.device and (cfg.rounds, cfg.beam, cfg.patience, cfg.burst) == (16, 8, 4, 8)
    monkeypatch.setenv("MYTHGPU_CLIMB_DEVICE", "0")
    assert not plugin._climb_kw()["climb"].device
    monkeypatch.delenv("MYTHGPU_CLIMB_DEVICE")
    assert not plugin._climb_kw()["climb"].device
