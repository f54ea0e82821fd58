"""The specialiser's analysis where it decides (CPU, no GPU): every case of
``tests/spec_fold_cases.py`` as its own program.  A search runs the program ``program.cpp`` folded
with the generator's ranges, known bits and value sets, so a wrong fold changes verdicts in every
engine alike and no kernel test can see it.  Here the specialised program (both lowerings) runs in
the oracle's evaluator of device ops (``oracle/kops.py``) on the candidates the C port generates, and
every verdict must equal the C port's on the UNSPECIALISED program: three seeds, windows of 2,048 at
0 and at a 63-bit start.  The table's own promises are checked on the C port alone (the reference
verdicts mix; a twin's compare takes both values) and on the lowered programs (a ``fires=True``
compare is gone from the program a search runs; a twin's is not).  The family programs the GPU
tests run go through both tiers' host compiles and the first tier's simulator, and the loader
refuses a fix record whose value does not fit the coordinate's width."""
import functools

import numpy as np
import pytest

from mythril_amd import native, search, ssa
from mythril_amd.smt import terms as T
from oracle import cport, kops
from tests import spec_fold_cases as S
from tests.test_asm_sim import record, run_sim, sim  # noqa: F401  (sim: fixture)

COMPARES = (kops.K_EQ, kops.K_ULT, kops.K_ULE, kops.K_SLT, kops.K_SLE)
WINDOWS = [(seed, start) for seed in S.SEEDS for start in S.STARTS]


def _count(spec, ops):
    return int(np.isin(spec["code"][:, 0], ops).sum())


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Per window: the generated coordinates, the C port's verdicts on the unspecialised program and
    its values of the case's compare and witness (watch rows)."""
    pr = S.single(name)
    watched = pr.watched([pr.cmp_nodes[0], pr.wit_nodes[0]])
    out = []
    for seed, start in WINDOWS:
        soa = cport.gen_soa(pr.prog, pr.blob, seed, start, S.WINDOW, pr.P.coord_words)
        want = cport.search(pr.prog, pr.blob, seed, start, S.WINDOW, verdicts=True)[2]
        ver, watch = cport.eval_soa(watched, soa, S.WINDOW, watch_words=2)
        assert np.array_equal(ver, want)  # the watch changes no verdict
        cmp_bits, wit_bits = S.bits_of(watch)
        out.append((soa, want, cmp_bits, wit_bits))
    return out


@pytest.mark.parametrize("name", S.NAMES)
def test_specialised_program_keeps_every_verdict(name):
    """Soundness: kops on the specialised program == the C port on the unspecialised one."""
    pr = S.single(name)
    native.check_program_gen(pr.prog, pr.blob)  # only generators the loader accepts
    progs = {interp: native.specialized_program(pr.prog, pr.blob, interp=interp) for interp in (False, True)}
    same = all(np.array_equal(progs[False][k], progs[True][k]) for k in ("code", "consts", "aux"))
    for (seed, start), (soa, want, _, _) in zip(WINDOWS, _reference(name)):
        for interp, spec in progs.items():
            if interp and same:
                continue  # one program, already run
            got = kops.verdicts(spec, soa, pr.widths, S.WINDOW)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (f"{name} (interp={interp}, seed {seed}, start {start:#x}): {bad.size} of {S.WINDOW} "
                                   f"verdicts differ, first at index {start + int(bad[0])}")


@pytest.mark.parametrize("name", S.NAMES)
def test_reference_carries_information(name):
    """The C port's verdicts hold both values in every window; a twin's compare (its witness) does
    too, so a fold of it would show; a compare meant to fold is constant there."""
    cs = S.by_name(name)
    for (seed, start), (_, want, cmp_bits, wit_bits) in zip(WINDOWS, _reference(name)):
        ones = int(want.sum())
        assert 0 < ones < S.WINDOW, (name, seed, hex(start), ones)
        if cs.fires is False and cs.show:
            assert 0 < int(wit_bits.sum()) < S.WINDOW, (name, seed, hex(start), int(wit_bits.sum()))
        if cs.fires is not False and not cs.lookup:
            assert int(cmp_bits.sum()) in (0, S.WINDOW), (name, seed, hex(start), int(cmp_bits.sum()))


@pytest.mark.parametrize("interp", [False, True], ids=["jit", "interp"])
@pytest.mark.parametrize("name", S.NAMES)
def test_fold_fires_where_the_table_says(name, interp):
    """Not vacuous: a ``fires=True`` compare (LOOKUP) is in the eval-mode lowering and not in the
    search's; ``fires="always"`` is in neither; every twin keeps its compares, also one whose
    compare the windows cannot show to take both values (``show=False``)."""
    cs = S.by_name(name)
    pr = S.single(name)
    ops = (kops.K_LOOKUP,) if cs.lookup else COMPARES
    searched = _count(native.specialized_program(pr.prog, pr.blob, interp=interp), ops)
    plain = _count(native.specialized_program(pr.prog, None, interp=interp), ops)
    if cs.fires is True:
        assert searched < plain, (name, searched, plain)
    elif cs.fires == "always":
        compare_nodes = [ssa.OPS[k] for k in ("EQ", "ULT", "ULE", "SLT", "SLE")]
        raw = sum(1 for n in pr.P.nodes if n[0] in compare_nodes)
        assert searched == plain < raw, (name, searched, plain, raw)
    else:
        assert searched == plain, (name, searched, plain)


def _one(w):
    x = T.BitVecVar(f"rf_fix_{w}", w)
    return ssa.flatten([T.eq(x, T.BitVecVal(1, w))])


@pytest.mark.parametrize("w", [1, 8, 33, 65, 255])
def test_loader_refuses_a_fix_value_above_the_width(w):
    """The record is applied after the mask to the width: a value bit at or above ``w`` would leave
    the coordinate wider than its width, so ``parse_gen`` refuses it (host-only checker); the bit
    ``w - 1`` outside the mask, and mask bits above ``w``, are taken."""
    P = _one(w)
    L = ssa.limbs(w)
    gb = search.GenBuilder(P)
    gb.fix(0, 1, 1)
    blob = gb.blob()
    off = S.const_word(blob, (int(blob[S.spec_word(0, 0)]) >> 8) - 1)
    blob[off + L - 1] |= 1 << (w % 32)          # mask: harmless
    blob[off + 2 * L - 1] |= 1 << ((w - 1) % 32)  # value: the top bit, outside the mask
    native.check_program_gen(P.to_bytes(), blob)
    blob[off + 2 * L - 1] |= 1 << (w % 32)
    with pytest.raises(native.EngineError, match="fixed-bit value exceeds the coordinate width") as ei:
        native.check_program_gen(P.to_bytes(), blob)
    assert ei.value.code == native.MG_E_INVALID


@pytest.mark.parametrize("name", ["or_ult_eq", "or_eq_slt", "or_ult_eq_decided"])
def test_or_of_less_and_equal_becomes_one_compare(name):
    """``Or(a < b, b == a)`` is ``a <= b``: one ULE / SLE, no ULT / SLT and only the probe's EQ."""
    pr = S.single(name)
    for gen in (None, pr.blob):
        spec = native.specialized_program(pr.prog, gen)
        le, lt = (kops.K_SLE, kops.K_SLT) if "slt" in name else (kops.K_ULE, kops.K_ULT)
        assert (_count(spec, (le,)), _count(spec, (lt,)), _count(spec, (kops.K_EQ,))) == (1, 0, 1), name


def test_table_covers_what_it_promises():
    """Every family is there, the widths where U256 changes word or limb, both raw-blob findings."""
    assert {c.family for c in S.CASES} == set(S.FAMILIES)
    assert {w for c in S.CASES for w, _ in c.coords} >= set(S.WIDTHS)
    assert {"raw_dict_entry_above_w", "raw_fix_value_outside_mask"} <= set(S.NAMES)
    assert sum(c.fires is True for c in S.CASES) >= 80 and sum(c.fires is False and c.show for c in S.CASES) >= 60


def test_first_tier_simulated_on_the_families(sim):  # noqa: F811
    """The first tier's kernels of every family program in the instruction-level simulator (mgj_gen
    verdicts per candidate, mgj_search first hit and count, early exit), assembled through comgr:
    all ``ok`` — its fix records with a value bit in a limb the mask leaves alone included, and
    the three-limb dictionary whose low limbs it compares by entry index."""
    recs = [record(0, S.group(fam).prog, S.group(fam).blob, seed, start, S.WINDOW, flags=1)
            for fam in S.FAMILIES for seed, start in ((S.SEEDS[0], S.STARTS[0]), (S.SEEDS[1], S.STARTS[1]))]
    rc, summary, bad, err = run_sim(sim, b"".join(recs), {"MYTHGPU_JIT_ASM_CHECK": "1"})
    assert summary, (rc, err[-2000:])
    assert rc == 0 and int(summary["ok"]) == len(recs) == int(summary["records"]), (summary, bad[:5], err[-2000:])
    for k in ("outside", "mismatch", "simerror", "asmerror"):
        assert int(summary[k]) == 0, (summary, bad[:5])


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_jit_kernels_of_the_families_compile_on_host(fam):
    """Both tiers accept every family program (no refusal to meet on the GPU) and their kernels
    compile for gfx950 on the host."""
    pr = S.group(fam)
    assert "mgj_search" in native.jit_source(pr.prog, pr.blob, compile=True)
    src = native.jit_asm(pr.prog, pr.blob, compile=True)
    assert "mgj_search:" in src and "mgj_gen:" in src


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_family_programs_keep_every_verdict(fam):
    """The programs the GPU tests run (one per family, the parity of its cases): accepted by the
    loader, sound in both lowerings on one window, and the reference mixes."""
    pr = S.group(fam)
    native.check_program_gen(pr.prog, pr.blob)
    seed, start, n = S.SEEDS[0], S.STARTS[1], 256
    soa = cport.gen_soa(pr.prog, pr.blob, seed, start, n, pr.P.coord_words)
    want = cport.search(pr.prog, pr.blob, seed, start, n, verdicts=True)[2]
    assert 0 < int(want.sum()) < n
    for interp in (False, True):
        got = kops.verdicts(native.specialized_program(pr.prog, pr.blob, interp=interp), soa, pr.widths, n)
        assert np.array_equal(got, want), (fam, interp, np.flatnonzero(got != want)[:4])
