"""The first tier's LDS spiller at its three thresholds, on the CPU (``tests/spill_cases.py``):
whether an eval kernel spills at all, whether its slots fit four working waves per workgroup (159
per wave) and whether it runs solo (639), past which it is refused.

Per case and layout the emitted text must be of the declared class, declare exactly the LDS its
slots take, within the 160 KiB of a gfx950 CU, and pass the load gate or be refused as outside the
tier — never fail in the assembler.  Every kernel runs in the simulator (which refuses a kernel
that declares more LDS than a CU has, and a DS offset past 16 bits) against the C port, verdicts
and model read-back rows, row-major and tiled.  Two mutants show that the table bites: the slot
cap as it was before it bounded the stride (slot 159 accepted: 4 x 161 x 256 B = 164,864 B), and a
reload that reads limb j from limb j + 1's slot.
"""
import random

import pytest

from tests import spill_cases as sc
from tests.test_asm_sim import _mutants, record, run_sim, sim  # noqa: F401  (sim: the module's fixture)

LAYOUTS = (False, True)
IDS = [c.name for c in sc.CASES]


def _emit(case, tiled, monkeypatch, compile=False):
    from mythril_amd import native

    monkeypatch.delenv("MYTHGPU_JIT_ASM_SPILL_TEST", raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    return native.jit_asm(sc.program(case)[1], None, tiled=tiled, compile=compile)


def _check_text(case, tiled, src):
    """The emitted text against the case's declaration; returns its facts."""
    f = sc.facts(src)
    where = (case.name, "tiled" if tiled else "row-major", f._replace(offsets=()))
    assert f.cls == case.cls(tiled), where
    if case.hwm(tiled) is not None:
        assert f.hwm == case.hwm(tiled), where
    assert f.solo_marker == (f.cls == sc.SOLO), where
    if f.cls == sc.RESIDENT:
        assert f.hwm == 0, where
        return f
    waves = 1 if f.cls == sc.SOLO else 4
    assert 1 <= f.hwm <= (sc.SOLO_CAP if f.cls == sc.SOLO else sc.FOUR_WAVE_CAP), where
    stride = f.hwm | 1
    assert stride % 2 == 1
    # the stride the kernel computes its lane's slots with is the one the declaration is sized by
    assert f"v_mul_u32_u24_e32 " in src and f", {hex(stride)}, v1\n" in src, where
    assert f.lds == waves * stride * 256 <= sc.LDS_PER_CU, where
    assert all(o % 4 == 0 and o < 4 * stride and o < 65536 for o in f.offsets), where
    return f


@pytest.mark.parametrize("tiled", LAYOUTS, ids=["row", "tiled"])
@pytest.mark.parametrize("case", sc.CASES, ids=IDS)
def test_spill_table_text(case, tiled, monkeypatch):
    """Class, LDS declaration (waves x stride x 256 B, inside the CU's 163,840 B), odd stride, slot
    offsets below 4 x stride and below 2^16, and the solo marker exactly on solo kernels."""
    from mythril_amd import native

    if case.cls(tiled) == sc.REFUSED:
        with pytest.raises(native.EngineUnsupported, match="spill slots"):
            _emit(case, tiled, monkeypatch)
        return
    _check_text(case, tiled, _emit(case, tiled, monkeypatch))


@pytest.mark.parametrize("tiled", LAYOUTS, ids=["row", "tiled"])
@pytest.mark.parametrize("case", [c for c in sc.CASES if sc.REFUSED not in (c.row, c.tiled)],
                         ids=[c.name for c in sc.CASES if sc.REFUSED not in (c.row, c.tiled)])
def test_spill_table_load_gate(case, tiled, monkeypatch):
    """Assembled and linked by comgr and through the load gate: accepted, or refused as outside the
    tier (``EngineUnsupported``: the O3 kernel then) — any other ``EngineError`` (an emitted kernel
    that does not assemble fails the whole compile ticket) fails the test."""
    from mythril_amd import native

    try:
        _emit(case, tiled, monkeypatch, compile=True)
    except native.EngineUnsupported:
        pass


def test_spill_table_holds_the_thresholds(monkeypatch):
    """The table stands where it says (``spill_cases.CASES``' roles), read from the emitted text."""
    from mythril_amd import native

    def f(case, tiled):
        try:
            return sc.facts(_emit(case, tiled, monkeypatch))
        except native.EngineUnsupported:
            return None

    def find(width, keys, watch="model"):
        hit = [c for c in sc.CASES if (c.width, c.keys, c.regs, c.watch) == (width, keys, None, watch)]
        assert len(hit) == 1, (width, keys, watch)
        return hit[0]

    for w in sc.WIDTHS:
        last = [c for c in sc.by_role("last-resident") if c.width == w]
        assert len(last) == 1, w
        nxt = find(w, last[0].keys + 1)
        assert "first-spill" in nxt.roles
        for tiled in LAYOUTS:
            assert f(last[0], tiled).cls == sc.RESIDENT and f(nxt, tiled).cls == sc.FOUR_WAVE, (w, tiled)
        for tiled in LAYOUTS:
            lay = ":tiled" if tiled else ":row"
            last = [c for c in sc.by_role("last-four-wave" + lay) if c.width == w]
            assert len(last) == 1, (w, lay)
            nxt = find(w, last[0].keys + 1)
            assert "first-solo" + lay in nxt.roles
            assert f(last[0], tiled).cls == sc.FOUR_WAVE and f(nxt, tiled).cls == sc.SOLO, (w, lay)
    # the largest legal four-wave kernel, in both layouts
    top = sc.by_role("hwm-159")
    assert top and all(f(c, t).cls == sc.FOUR_WAVE and f(c, t).hwm == sc.FOUR_WAVE_CAP for c in top for t in LAYOUTS)
    # programs whose four-wave attempt needs a 160th slot run solo, and so does the next one
    need = sc.by_role("needs-160")
    assert len({c.width for c in need}) >= 4
    for c in need:
        lays = [t for t in LAYOUTS if c.hwm(t) == sc.FOUR_WAVE_CAP + 1]  # the layout(s) that need exactly 160
        assert lays, c.name
        nxt = find(c.width, c.keys + 1, c.watch)
        assert "past-160" in nxt.roles
        for t in lays:
            assert f(c, t).cls == sc.SOLO and f(c, t).hwm == sc.FOUR_WAVE_CAP + 1, (c.name, t)
            assert f(nxt, t).cls == sc.SOLO and f(nxt, t).hwm > sc.FOUR_WAVE_CAP + 1, (nxt.name, t)
    # the solo cap
    (cap,), (past,) = sc.by_role("hwm-639"), sc.by_role("past-639")
    assert (past.width, past.keys) == (cap.width, cap.keys + 1)
    assert all(f(cap, t).cls == sc.SOLO and f(cap, t).hwm == sc.SOLO_CAP and f(past, t) is None for t in LAYOUTS)
    a, b = sorted(sc.by_role("needs-640"), key=lambda c: c.keys)
    assert (a.width, b.width, b.keys) == (256, 256, a.keys + 1)
    # 256-bit keys spill eight slots at a time: 632 in use, the next key's eight end at slot 639
    assert all(f(a, t).hwm == sc.SOLO_CAP + 1 - 8 and f(b, t) is None for t in LAYOUTS)


def _records(cases, rng, assemble=True):
    """Every non-refused kernel of ``cases``, row-major and tiled, at n = 64 x 2 + 5 (a partial last
    group) and, solo, at n = 1; the boundary cases also through comgr (record flag 1; ``assemble``:
    the mutant drivers are built without the assembler)."""
    recs = []
    for c in cases:
        pb = sc.program(c)[1]
        for tiled in LAYOUTS:
            if c.cls(tiled) == sc.REFUSED:
                continue
            flags = int(assemble and "boundary" in c.roles)
            recs.append(record(2 if tiled else 1, pb, None, rng.getrandbits(32), 0, 64 * 2 + 5, flags=flags))
            if c.cls(tiled) == sc.SOLO:
                recs.append(record(2 if tiled else 1, pb, None, rng.getrandbits(32), 0, 1, flags=flags))
    return recs


def _sim_worker(args):
    exe, names, env = args
    cases = [c for c in sc.CASES if c.name in names]
    recs = _records(cases, random.Random(len(names)))
    rc, summary, bad, err = run_sim(exe, b"".join(recs), dict(env, MYTHGPU_JIT_ASM_CHECK="1"))
    return names, len(recs), rc, summary, bad[:5], err[-2000:]


def test_spill_table_in_the_simulator(sim):  # noqa: F811
    """Every kernel of the table against the C port in the simulator: verdicts and every model
    read-back row, with the simulator's LDS bounds, wait counts and lifetimes and the emitter's own
    checker (MYTHGPU_JIT_ASM_CHECK).  No case may be outside the tier, skipped or excused."""
    import multiprocessing as mp

    from tests.test_asm_sim import WORKERS

    live = [c for c in sc.CASES if (c.row, c.tiled) != (sc.REFUSED, sc.REFUSED)]
    tasks = [(sim, [c.name], c.env) for c in live if c.regs]
    plain = sorted((c for c in live if not c.regs), key=lambda c: -c.keys * c.keys * c.width)
    tasks += [(sim, [c.name for c in plain[k::WORKERS]], {}) for k in range(WORKERS)]
    for c in live:
        sc.program(c)  # built once, before the fork
    with mp.get_context("fork").Pool(WORKERS) as pool:
        results = pool.map(_sim_worker, [t for t in tasks if t[1]], chunksize=1)
    total = 0
    for names, n, rc, summary, bad, err in results:
        assert summary, (names, rc, err)
        assert (summary["mismatch"], summary["simerror"], summary["asmerror"]) == ("0", "0", "0"), (names, summary, bad)
        assert rc == 0 and int(summary["ok"]) == n and summary["outside"] == "0", (names, summary, bad, err)
        total += n
    assert total >= 2 * len(live)
    print("spill table in the simulator:", total, "records")


PARENT_CAP = {"mythril_amd/csrc/jit_asm.cpp": ('if (((sl + 1u) | 1u) > spill_cap()) fail("out of VGPRs (spill slots)");',
                                               'if ((sl | 1u) > spill_cap()) fail("out of VGPRs (spill slots)");')}
WRONG_SLOT = {"mythril_amd/csrc/jit_asm.cpp": (
    '" offset:" + std::to_string((uint32_t)at[j] * 4u));\n      x.l[j] = d;',
    '" offset:" + std::to_string((uint32_t)at[j + 1 < at.size() && at[j + 1] >= 0 ? j + 1 : j] * 4u));\n      x.l[j] = d;')}


def test_spill_mutants_fail_the_table(sim, tmp_path):  # noqa: F811
    """(1) The slot cap as it was (slot 159 accepted, the stride then 161): the emitter hands out
    kernels that declare 4 x 161 x 256 = 164,864 B and, solo, 641 x 256 = 164,096 B, which the
    simulator refuses at load, as the device's loader would, and nothing else in the suite did.
    (2) A reload that reads limb j from limb j + 1's slot: the model read-back rows differ."""
    exes = _mutants(tmp_path, {"parent_cap": PARENT_CAP, "wrong_slot": WRONG_SLOT})
    rng = random.Random(7)
    # (the sum alone watched: with the model rows the body is past the branch range, and that check
    # would send the four-wave attempt to the solo kernel whatever the cap lets through)
    (four,) = [c for c in sc.by_role("needs-160") if c.width == 256 and c.watch == "sum"]
    (solo,) = [c for c in sc.by_role("needs-640") if c.row == sc.REFUSED]
    recs = [record(1, sc.program(four)[1], None, rng.getrandbits(32), 0, 64 * 2 + 5),
            record(1, sc.program(solo)[1], None, rng.getrandbits(32), 0, 1)]
    rc, summary, lines, err = run_sim(exes["parent_cap"], b"".join(recs), {"MYTHGPU_JIT_ASM_CHECK": "1"})
    assert rc != 0 and summary["simerror"] == "2", (summary, lines, err[-2000:])
    assert "declares 164864 B of LDS" in lines[0] and "declares 164096 B of LDS" in lines[1], lines
    # the tree's own emitter: the first runs (solo), the second is refused
    rc, summary, lines, err = run_sim(sim, b"".join(recs), {"MYTHGPU_JIT_ASM_CHECK": "1"})
    assert rc == 0 and (summary["ok"], summary["outside"]) == ("1", "1"), (summary, lines, err[-2000:])
    # every boundary kernel that watches the XOR of its keys reloads keys for it: each record must mismatch
    spilling = [c for c in sc.BOUNDARY if c.watch == "model"]
    recs = _records(spilling, rng, assemble=False)
    rc, summary, lines, err = run_sim(exes["wrong_slot"], b"".join(recs))
    assert rc != 0 and int(summary["mismatch"]) == len(recs), (summary, lines[:5], err[-2000:])
    assert any("watch row" in ln for ln in lines), lines[:5]
