"""The C restatement (oracle/bveval.c, used as the CPU baseline) agrees with the
Python restatement (oracle/bv.py) — CPU only."""
import numpy as np
import pytest

from helpers import RandomProgram, random_assignments
from mythril_amd import search, ssa, workloads
from oracle import cport
from oracle.bv import evaluate, model_from_coordinates


@pytest.mark.parametrize("seed", range(6))
def test_cport_eval_matches_python_oracle(seed):
    rp = RandomProgram(100 + seed, n_ops=50)
    roots = [rp.root] + rp.bools[-2:]
    P = ssa.flatten(roots)
    assigns = random_assignments(P, 48, seed)
    soa = ssa.soa_from_assignments(P, assigns)
    ver = cport.eval_soa(P.to_bytes(), soa, len(assigns))
    for i, a in enumerate(assigns):
        m = model_from_coordinates(P, a)
        want = int(all(evaluate(r, m) == 1 for r in roots))
        assert ver[i] == want, (seed, i)


@pytest.mark.parametrize("name", sorted(workloads.WORKLOADS), ids=workloads.test_id)
def test_cport_generator_matches_python_oracle_on_workloads(name):
    """Search-mode candidates (generator restated in C) evaluated by the C port agree
    with the Python oracle evaluating the same coordinates."""
    roots = [c.raw for c in workloads.WORKLOADS[name]()]
    P = ssa.flatten(roots)
    g = search.default_generator(P)
    first, hits, ver = cport.search(P.to_bytes(), g.blob(), 7, 1000, 64, threads=2, verdicts=True)
    assert ver.shape == (64,)
    assert hits == int(ver.sum())
    _against_the_oracle(P, roots, g.blob(), 7, 1000, ver)


def _against_the_oracle(P, roots, blob, seed, start, ver):
    """Each verdict equals the Python oracle's on the coordinates the GEN3 restatement
    (``tests/gen3_ref.py``, big integers) generates for that candidate."""
    from tests import gen3_ref as R

    specs, consts = R.split_blob(blob)
    widths = [c.width for c in P.coords]
    for q in range(len(ver)):
        m = model_from_coordinates(P, R.gen_values(specs, consts, widths, seed, start + q))
        assert ver[q] == int(all(evaluate(r, m) == 1 for r in roots)), (start + q,)


@pytest.mark.parametrize("name", ["w256_div_mg_11", "w256_exp_mixed_L33_lane0", "w64_div_signed_edges", "w33_shift_mixed"])
def test_cport_generator_matches_python_oracle_on_wave_cases(name):
    """The same on generator-form cases of the wave table (``tests/wave_op_cases.py``), whose windows
    hold hits and misses: both windows, first hit and hit count included."""
    from tests import wave_op_cases as W

    c = W.gen_case(name)
    for start in W.GEN_STARTS:
        first, hits, ver = cport.search(c.pb, c.blob, c.seed, start, 256, threads=2, verdicts=True)
        assert 0 < hits < 256 and hits == int(ver.sum()) and first == start + int(np.flatnonzero(ver)[0])
        _against_the_oracle(c.P, c.roots, c.blob, c.seed, start, ver)


def test_workload_selectors_are_keccak_of_signatures():
    from oracle.keccak import keccak256

    for sig, sel in workloads.SELECTORS.items():
        assert int.from_bytes(keccak256(sig.encode())[:4], "big") == sel


def test_cport_keccak_matches_kats_and_python_oracle():
    """The C restatement's Keccak-256 (oracle/bveval.c vkeccak) against the reference's
    KATs (tests/golden/keccak_kat.json) and oracle/keccak.py on random messages of 1, 31, 32, 64,
    100 and 128 bytes (one sponge block: the default library holds 1024 bits; longer inputs and
    further blocks run on the wide library in tests/test_wide_cpu.py)."""
    import random

    from helpers import load_json
    from mythril_amd.smt import terms as T
    from oracle.keccak import keccak256_int

    cases = []
    for kat in load_json("keccak_kat.json"):
        msg = bytes.fromhex(kat["msg_hex"])
        if msg:
            want = int(kat["digest"], 16) if "digest" in kat else None
            cases.append((msg, want, kat.get("selector")))
    rng = random.Random(3)
    for n in (1, 31, 32, 64, 100, 128):
        cases.append((bytes(rng.getrandbits(8) for _ in range(n)), None, None))
    for msg, want, sel in cases:
        x = T.BitVecVar(f"m{len(msg)}", 8 * len(msg))
        h = T.keccak256(x)
        P = ssa.flatten([T.BoolVal(True)], extra=[h])
        P.set_watch([P.term_node[h.id]])
        soa = ssa.soa_from_assignments(P, [[int.from_bytes(msg, "big")]])
        got = keccak256_int(msg)
        assert cport.eval_soa(P.to_bytes(), soa, 1)[0] == 1
        # the digest through an equality root (the C port reports verdicts only)
        root = T.mk("eq", T.BOOL, (h, T.BitVecVal(got, 256)))
        P2 = ssa.flatten([root])
        soa2 = ssa.soa_from_assignments(P2, [[int.from_bytes(msg, "big")]])
        assert cport.eval_soa(P2.to_bytes(), soa2, 1)[0] == 1, len(msg)
        if want is not None:
            assert got == want
        if sel is not None:
            assert got >> 224 == int(sel, 16)
