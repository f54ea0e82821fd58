"""GEN3 at its edge parameters, on the CPU: the header's restatement (``tests/gen3_ref.py``, plain
big integers) against the C port (``oracle/bveval.c: gen_value``) over the case table of
``tests/gen3_edge_cases.py`` — span and count 0 (2^32), sums that wrap the width, shifts beyond the
coordinate's limbs, deltas that borrow through every limb, narrow coordinates, widths that are no
multiple of 32, clamps at the top of the range, a COPY chain of depth 64, a fix record on a COPY
source, a 65,535-entry dictionary.  Then: conditions on the restatement alone that make the
comparison mean something, the generator blobs ``parse_gen`` must refuse (host-only checker), the
first tier in the instruction-level simulator on the same programs and windows, and the 16-bit
probabilities ``GenBuilder`` stores.  (Test-side restatement; no reference file holds the generator:
it is this engine's own candidate stream)"""
import hashlib

import numpy as np
import pytest

from mythril_amd import native, search, ssa, workloads
from mythril_amd.smt import symbol_factory
from oracle import cport
from tests import gen3_edge_cases as E
from tests import gen3_ref as R
from tests.test_asm_sim import record, run_sim, sim  # noqa: F401  (sim: fixture)

WINDOWS = [(seed, start) for seed in E.SEEDS for start in E.STARTS]


# ---- (a) the restatement against the C port ----------------------------------------------------


@pytest.mark.parametrize("name", E.NAMES)
def test_restatement_matches_c_port(name):
    """Every limb of every coordinate, three windows x three seeds of 2,048 candidates."""
    c = E.case(name)
    for seed, start in WINDOWS:
        got = cport.gen_soa(c.prog, c.blob, seed, start, E.WINDOW, c.P.coord_words).astype(np.uint64)
        want = np.array(c.ref_rows(seed, start, E.WINDOW), dtype=np.uint64)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (name, hex(seed), hex(start), "row, candidate:", bad[:4].tolist())


@pytest.mark.parametrize("name", E.NAMES)
def test_probe_root_splits_every_window(name):
    """The probe root holds for between a quarter and three quarters of each window (C port)."""
    c = E.case(name)
    for start in E.STARTS:
        _, _, ver = cport.search(c.prog, c.blob, E.SEED0, start, E.WINDOW, verdicts=True)
        assert 0.25 <= float(ver.mean()) <= 0.75, (name, hex(start), float(ver.mean()))


# ---- (b) coverage, on the restatement alone ----------------------------------------------------


def _traces(c):
    for seed, start in WINDOWS:
        for i in range(start, start + E.WINDOW):
            yield R.gen_trace(c.specs, c.consts, c.widths, seed, i)


@pytest.mark.parametrize("name", ["mixed", "chain"])
def test_mixed_coverage(name):
    """Over the windows used every MIXED coordinate takes each alternative it gives a nonzero
    probability, draws each delta (+1, +2, -1, -2) where it has one, and has a value its clamp moved
    and one it left in place; the chain's last coordinate copies through at least 32 links."""
    c = E.case(name)
    mixed = c.mixed()
    alts = {m: set() for m in mixed}
    deltas = {m: set() for m in mixed}
    clamped = {m: set() for m in mixed}
    depth = 0
    for tr in _traces(c):
        for m in mixed:
            t = tr[m]
            alts[m].add(t["alt"])
            if t["delta"]:
                deltas[m].add(t["delta"])
            clamped[m].add(t["clamped"])
        depth = max(depth, tr[-1]["depth"])
    for m in mixed:
        s = c.specs[m]
        pc = (s[3] & 0xFFFF) if s[4] != R.NONE else 0
        pd = (s[3] >> 16) if s[2] else 0
        ps = s[5] & 0xFFFF
        want = {a for a, p in ((R.ALT_COPY, pc), (R.ALT_DICT, pd), (R.ALT_SMALL, ps),
                               (R.ALT_UNIFORM, 65536 - pc - pd - ps)) if p > 0}
        assert alts[m] == want, (name, m, alts[m], want)
        if (pc or pd) and s[6]:
            assert deltas[m] == {1, 2, -1, -2}, (name, m, deltas[m])
        else:
            assert not deltas[m]
        assert clamped[m] == ({True, False} if s[7] else {False}), (name, m, clamped[m])
    if name == "chain":
        assert len(mixed) == E.CHAIN_LEN and depth >= 32, depth
    else:
        # the table's promises about this program: wraps through all 8 limbs both ways, and a COPY of
        # a final value that has fixed bits
        assert sum(1 for m in mixed if c.specs[m][7]) == 3 and len(mixed) == 11


def test_mixed_delta_wraps_and_copy_sees_fixed_bits():
    c = E.case("mixed")
    t256 = E.top(256)
    up = down = fixed_copy = False
    for tr in _traces(c):
        t = tr[0]
        if t["alt"] == R.ALT_DICT and t["delta"]:
            up |= t["delta"] > 0 and t["v"] < 2 and t["v"] - t["delta"] < 0      # top or top - 1, plus
            down |= t["delta"] < 0 and t["v"] > t256 - 2 and t["v"] - t["delta"] > t256  # 0 or 1, minus
        t = tr[4]  # copies coordinate 3, whose final value has bits 100..107 fixed to 0xA5
        if t["alt"] == R.ALT_COPY and not t["delta"]:
            assert t["v"] == tr[3]["v"] and (t["v"] >> 100) & 0xFF == 0xA5
            fixed_copy = True
    assert up and down and fixed_copy


@pytest.mark.parametrize("name", ["range", "aligned"])
def test_range_and_aligned_wrap(name):
    """The cases whose sum can pass 2^w do so at least once."""
    c = E.case(name)
    can = {"range": [0, 2, 4, 5, 6, 7], "aligned": [0, 1, 2, 4, 5, 7]}[name]
    seen = {q: set() for q in can}
    for seed, start in WINDOWS[:3]:
        for i in range(start, start + E.WINDOW):
            tr = R.gen_trace(c.specs, c.consts, c.widths, seed, i)
            for q in can:
                seen[q].add(tr[q]["wrapped"])
    assert all(True in s for s in seen.values()), seen


# ---- (c) refusals, through the host-only checker ------------------------------------------------


def _two(w0=256, w1=256):
    a, b = symbol_factory.BitVecSym("rf_a", w0), symbol_factory.BitVecSym("rf_b", w1)
    BVV = symbol_factory.BitVecVal
    P = ssa.flatten([(a == BVV(1, w0)).raw, (b == BVV(2, w1)).raw])
    ix = {c.name: c.index for c in P.coords}
    assert ix["rf_a"] < ix["rf_b"]
    return P, ix["rf_a"], ix["rf_b"]


def _refused(P, blob, code, fragment):
    with pytest.raises(native.EngineError) as ei:
        native.check_program_gen(P.to_bytes(), blob)
    assert ei.value.code == code, ei.value
    assert fragment in str(ei.value), ei.value


def _spec_word(blob, c, k):
    return 4 + 8 * c + k


def test_checker_refuses_malformed_generators():
    INV = native.MG_E_INVALID
    P, a, b = _two()
    gb = search.GenBuilder(P)
    gb.dict(a, [])
    _refused(P, gb.blob(), INV, "empty dictionary")
    gb = search.GenBuilder(P)
    gb.dict(a, list(range(65536)))
    _refused(P, gb.blob(), INV, "dictionary larger than 65535 entries")
    gb = search.GenBuilder(P)
    gb.aligned(a, 0, 256, 4)
    _refused(P, gb.blob(), INV, "aligned generator")
    src = "copy source must be an earlier, generated coordinate of the same width"
    gb = search.GenBuilder(P)
    gb.mixed(a, [1], p_dict=.5, copy_from=b, p_copy=.2)  # later than the coordinate
    _refused(P, gb.blob(), INV, src)
    gb = search.GenBuilder(P)
    gb.mixed(a, [1], p_dict=.5, copy_from=a, p_copy=.2)  # itself
    _refused(P, gb.blob(), INV, src)
    gb = search.GenBuilder(P)
    gb.lazy(a)
    gb.mixed(b, [1], p_dict=.5, copy_from=a, p_copy=.2)
    _refused(P, gb.blob(), INV, src)
    P2, a2, b2 = _two(256, 255)
    gb = search.GenBuilder(P2)
    gb.mixed(b2, [1], p_dict=.5, copy_from=a2, p_copy=.2)  # another width
    _refused(P2, gb.blob(), INV, src)
    # clamps with lo + span > 2^w
    P3, a3, b3 = _two(20, 33)
    for c, clamp in ((a3, (0, 0)), (a3, ((1 << 20) - 4, 5)), (b3, ((1 << 33) - 10, 11)), (b3, ((1 << 32) + 1, 0))):
        gb = search.GenBuilder(P3)
        gb.mixed(c, [1], p_dict=.5, clamp=clamp)
        _refused(P3, gb.blob(), INV, "clamp range exceeds the coordinate width")
    for c, clamp in ((a3, ((1 << 20) - 4, 4)), (b3, ((1 << 33) - 10, 10)), (b3, (1 << 32, 0))):
        gb = search.GenBuilder(P3)
        gb.mixed(c, [1], p_dict=.5, clamp=clamp)
        native.check_program_gen(P3.to_bytes(), gb.blob())
    # records past the constants
    gb = search.GenBuilder(P)
    gb.mixed(a, [1], p_dict=.5, clamp=(5, 9))
    blob = gb.blob()
    blob[_spec_word(blob, a, 7)] = int(blob[2]) - 8 + 1  # L + 1 = 9 words needed, 8 left
    _refused(P, blob, INV, "clamp record out of range")
    gb = search.GenBuilder(P)
    gb.uniform(a)
    gb.fix(a, 0xFF, 0x11)
    blob = gb.blob()
    blob[_spec_word(blob, a, 0)] = (int(blob[2]) - 15 + 1) << 8  # 2 L = 16 words needed, 15 left
    _refused(P, blob, INV, "fixed-bit record out of range")
    gb = search.GenBuilder(P)
    blob = gb.blob()
    blob[_spec_word(blob, a, 0)] = 7
    _refused(P, blob, INV, "unknown generator kind")
    one = ssa.flatten([(symbol_factory.BitVecSym("rf_c", 64) == symbol_factory.BitVecVal(3, 64)).raw])
    _refused(one, search.GenBuilder(P).blob(), INV, "generator does not match program")


def _chain(n):
    BVV = symbol_factory.BitVecVal
    xs = [symbol_factory.BitVecSym(f"rf_ch{q:02d}", 64) for q in range(n)]
    P = ssa.flatten([(x == BVV(q, 64)).raw for q, x in enumerate(xs)])
    ix = [next(c.index for c in P.coords if c.name == f"rf_ch{q:02d}") for q in range(n)]
    assert ix == sorted(ix)
    gb = search.GenBuilder(P)
    gb.mixed(ix[0], [1, 2], p_dict=.5)
    for q in range(1, n):
        gb.mixed(ix[q], [], p_dict=0., copy_from=ix[q - 1], p_copy=.9)
    return P, gb.blob()


def test_checker_bounds_the_copy_chain():
    P, blob = _chain(65)  # static depth 64 = MG_GEN_MAX_COPY_DEPTH
    native.check_program_gen(P.to_bytes(), blob)
    native.check_program_gen(E.case("chain").prog, E.case("chain").blob)
    P, blob = _chain(66)
    with pytest.raises(native.EngineUnsupported, match="copy chain longer than MG_GEN_MAX_COPY_DEPTH"):
        native.check_program_gen(P.to_bytes(), blob)


def test_every_table_generator_passes_the_checker():
    for c in E.cases():
        native.check_program_gen(c.prog, c.blob)


# ---- (d) the first tier, in the simulator -------------------------------------------------------


def test_first_tier_simulated_on_the_table(sim):  # noqa: F811
    """Search records (mgj_gen verdicts per candidate, mgj_search first hit and count, early exit)
    of every table program over the three windows, assembled through comgr: all ``ok``."""
    recs = [record(0, c.prog, c.blob, E.SEED0, start, E.WINDOW, flags=1) for c in E.cases() for start in E.STARTS]
    rc, summary, bad, err = run_sim(sim, b"".join(recs), {"MYTHGPU_JIT_ASM_CHECK": "1"})
    assert summary, (rc, err[-2000:])
    assert rc == 0 and int(summary["ok"]) == len(recs) == int(summary["records"]), (summary, bad[:5], err[-2000:])
    for k in ("outside", "mismatch", "simerror", "asmerror"):
        assert int(summary[k]) == 0, (summary, bad[:5])


# ---- (e) GenBuilder's probabilities -------------------------------------------------------------


def test_genbuilder_probabilities_saturate():
    """``mixed(p = 1.0)`` stores 65535 ("always" up to 1/65536), not 65536 & 0xFFFF = 0 ("never")."""
    P, a, b = _two()
    gb = search.GenBuilder(P)
    gb.mixed(a, [1], p_dict=.25)
    gb.mixed(b, [1, 2], p_dict=1.0, copy_from=a, p_copy=1.0, p_delta=1.0, small_bits=9, p_small=1.0)
    blob = gb.blob()
    sb = [int(x) for x in blob[4 + 8 * b: 12 + 8 * b]]
    assert sb[0] == search.GEN_MIXED and sb[2] == 2
    assert sb[3] == 0xFFFFFFFF and sb[4] == a and sb[5] == (9 << 16) | 0xFFFF and sb[6] == 0xFFFF
    sa = [int(x) for x in blob[4 + 8 * a: 12 + 8 * a]]
    assert sa[3] == 0x4000 << 16 and sa[4] == R.NONE and sa[5] == 0 and sa[6] == 0
    gb.mixed(b, [1], p_dict=2.5, p_delta=-1.0)  # out of range either way: the nearest end
    sb = gb.specs[b]
    assert sb[3] == 0xFFFF << 16 and sb[6] == 0
    gb.mixed(b, [1], p_dict=65535.5 / 65536)  # the largest value below 1.0 is unchanged
    assert gb.specs[b][3] == 0xFFFF << 16


# the default generator's blobs before probabilities saturated: (bytes, sha256)
DEFAULT_BLOBS = {
    "suicide_kill": (4604, "1511aee09c5fdbbe8ee35bf9ed72167f55ff0e2df3979dd752d5f3e9eec74564"),
    "token_transfer_underflow": (7804, "6230fd18988625b28d241bf12af672bcfd8b156add42f68b3d70fd8882e48a12"),
    "etherstore_reentrancy": (5368, "5e0976c934a26131f0c12f3f190ea55e5f987839ea8c6c361675a9f86b1849e5"),
    "bectoken_batch_overflow": (5144, "bddb769ad211a89811f74030eb37e62b5bf51e462061f17634687f2652f1d9e5"),
    "walletlibrary_kill": (15616, "04098812f607e6aeaf44bb53283d331b89564d219ef6f6a6111edfdf16545568"),
    "sha3_keyed_mapping": (528, "5295c959fb1bfd8dd36c5eda2468825881fa0ebbaea5fa0500764cd68512b9c1"),
}


@pytest.mark.parametrize("name", sorted(DEFAULT_BLOBS))
def test_default_generator_blobs_unchanged(name):
    roots = [c.raw for c in workloads.WORKLOADS[name]()]
    _, blob = search.prepare(roots)
    b = np.ascontiguousarray(blob, dtype="<u4").tobytes()
    assert (len(b), hashlib.sha256(b).hexdigest()) == DEFAULT_BLOBS[name]


# ---- the window rule, host-only entry point -----------------------------------------------------


def test_split_range_refuses_windows_that_reach_2_64():
    top = 1 << 64
    for start, count in ((top - 64, 64), (top - 1, 1), (top - 640, 640), (1, top - 1)):
        with pytest.raises(native.EngineError, match="window reaches 2\\^64") as ei:
            native.split_range(start, count, 4)
        assert not isinstance(ei.value, native.EngineUnsupported)
    parts = native.split_range(top - 65, 64, 2)
    assert sum(n for _, n in parts) == 64 and parts[0][0] == top - 65
    assert parts[-1][0] + parts[-1][1] == top - 1
    assert [n for _, n in native.split_range(top - 1, 0, 2)] == [0, 0]  # an empty window anywhere
