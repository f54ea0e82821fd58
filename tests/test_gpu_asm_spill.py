"""The first tier's spilling eval kernels at their thresholds, on the device: the boundary cases of
``tests/spill_cases.py`` — per key width the last four-wave kernel and the first solo kernel of
each layout, the four-wave kernel at the largest legal high-water mark (159), the program whose
four-wave attempt needs a 160th slot (solo since the cap bounds the stride) and the one past it —
row-major and tiled.  ``tests/test_asm_spill_sim.py`` checks the same kernels' text and runs them
in the simulator; here the hardware's LDS, wait counts and launch grid (four waves per workgroup
over a group loop, or one working wave and one 64-candidate group per workgroup) take its place.

Every kernel declares at most 163,840 B of LDS (asserted from its text before it is loaded).

Reference anchor: a candidate's verdict and a watched term's value are ``Model.eval(...,
model_completion=True)`` (``mythril/laser/smt/model.py:45-59``), here through the C port
(``oracle/bveval.c``), verdicts and watch rows limb for limb.
"""
import functools

import numpy as np
import pytest

from mythril_amd import native, ssa
from oracle import cport
from tests import spill_cases as sc
from tests.helpers import random_assignments

pytestmark = pytest.mark.gpu

SIZES = (1, 64, 64 * 2 + 5)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(SoA rows of edge-value assignments, C port verdicts, C port watch rows) at the largest size;
    the smaller sizes are its leading candidates (computed once per case, shared by the layouts)."""
    P, pb = sc.program(case)
    n = max(SIZES)
    soa = ssa.soa_from_assignments(P, random_assignments(P, n, seed=case.width * 1000 + case.keys))
    ww = sum(ssa.limbs(P.watch_width(e)) for e in P.watch)
    ver, watch = cport.eval_soa(pb, soa, n, watch_words=ww)
    for a in (soa, ver, watch):
        a.setflags(write=False)
    return soa, ver, watch


@pytest.mark.parametrize("tiled", [False, True], ids=["row", "tiled"])
@pytest.mark.parametrize("case", sc.BOUNDARY, ids=[c.name for c in sc.BOUNDARY])
def test_asm_spill_boundary_kernels(engine, case, tiled, monkeypatch):
    monkeypatch.delenv("MYTHGPU_JIT_ASM_SPILL_TEST", raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    P, pb = sc.program(case)
    f = sc.facts(native.jit_asm(pb, None, tiled=tiled))
    assert f.cls == case.cls(tiled) and f.lds <= sc.LDS_PER_CU, (case.name, tiled, f._replace(offsets=()))
    soa, want_v, want_w = _reference(case)
    prog = engine.load(pb)
    try:
        ww = int(engine.info(prog).watch_words)
        assert ww == want_w.shape[0]
        jh = engine.jit_compile(prog, 0, asm=True, tiled=tiled)  # must succeed on the first tier
        try:
            flags, _, kww = engine.jit_layout(jh)
            assert flags & native.MG_JIT_ASM and bool(flags & native.MG_JIT_SOA_TILED) == tiled and kww == ww
            for n in SIZES:
                rows = np.ascontiguousarray(soa[:, :n])
                ver, watch = engine.jit_eval(jh, native.tile_soa(rows) if tiled else rows, n, watch_words=ww)
                assert np.array_equal(ver[:n], want_v[:n]), (case.name, tiled, n)
                got = np.asarray(watch)[:ww, :n]
                bad = np.argwhere(got != want_w[:, :n])
                assert bad.size == 0, (case.name, tiled, n, "watch row, candidate:", bad[:4].tolist())
        finally:
            engine.jit_free(jh)
    finally:
        engine.free(prog)
