"""Values above 1024 bits and multi-block Keccak on the CPU: the references the GPU tests of
``tests/test_gpu_wide.py`` and the wide simulator records of ``tests/test_asm_sim.py`` stand on.

* the Python oracle's sponge (``oracle/keccak.py``: ``keccak_f``, rate 136) re-run with the
  FIPS-202 domain byte against ``hashlib.sha3_256`` — the permutation and the multi-block absorb;
* the wide build of the C port (``oracle/libbveval_wide.so``, ``-DMAXW=64``: 4096 bits) against
  the Python oracle (``oracle/bv.py``): Keccak over 1..512 bytes, wide-operator DAGs value by
  value, UNIFORM coordinates limb by limb against the documented formula;
* the default C port refuses what it cannot hold (a test that forgets ``wide`` fails loudly);
* the first tier's width boundary (2048 bits in, 2049 refused).

Reference anchor: SHA3 over a memory region hashes a ``Concat`` of any concrete length
(``mythril/laser/ethereum/keccak_function_manager.py:59-72``).
"""
import hashlib
import random

import pytest

from mythril_amd import native, search, ssa
from mythril_amd.smt import terms as T
from oracle import cport
from oracle.bv import evaluate_many, model_from_coordinates
from oracle.keccak import keccak256, keccak256_int, keccak_f
from tests.helpers import (LENS, WideRandomProgram, keccak_sweep_inputs, memory_region_queries, random_assignments,
                           wide_edge_values, wide_operator_terms)
from tests.test_gen3_spec import keys, uniform_raw


def _sponge(data: bytes, domain: int) -> bytes:
    """The absorb / squeeze of ``oracle.keccak.keccak256`` with the domain byte as a parameter."""
    rate = 136
    msg = bytearray(data)
    msg.append(domain)
    while len(msg) % rate:
        msg.append(0)
    msg[-1] |= 0x80
    st = [0] * 25
    for off in range(0, len(msg), rate):
        for i in range(rate // 8):
            st[i] ^= int.from_bytes(msg[off + 8 * i:off + 8 * i + 8], "little")
        st = keccak_f(st)
    return b"".join(st[i].to_bytes(8, "little") for i in range(4))


def test_reference_sponge_matches_hashlib_sha3():
    """SHA3-256 differs from Keccak-256 in the domain byte alone (0x06 for 0x01): the oracle's
    permutation under that byte equals hashlib over 0..300 bytes and at 407 / 408 / 409 (three
    blocks' edge) and 512, and under 0x01 it is ``oracle.keccak.keccak256`` itself."""
    rng = random.Random(0x5A3)
    for n in list(range(301)) + [407, 408, 409, 512]:
        data = bytes(rng.getrandbits(8) for _ in range(n))
        assert _sponge(data, 0x06) == hashlib.sha3_256(data).digest(), n
        assert _sponge(data, 0x01) == keccak256(data), n


def _watched(terms, roots=(T.BoolVal(True),)):
    P = ssa.flatten(list(roots), extra=list(terms))
    P.set_watch([P.term_node[t.id] for t in terms])
    return P, sum(ssa.limbs(t.width) for t in terms)


def _cport_values(P, terms, assigns, wide=True):
    soa = ssa.soa_from_assignments(P, assigns)
    ww = sum(ssa.limbs(t.width) for t in terms)
    ver, watch = cport.eval_soa(P.to_bytes(), soa, len(assigns), wide=wide, watch_words=ww)
    widths = [t.width for t in terms]
    return ver, [search.read_rows(watch, widths, i) for i in range(len(assigns))]


def test_wide_cport_keccak_length_sweep():
    """The wide C port's Keccak-256 over every length of ``LENS`` (1..512 bytes, one to four sponge
    blocks) equals the Python oracle's, on the pad bits' mirror images and random inputs."""
    rng = random.Random(0xC0DE)
    for n in LENS:
        x = T.BitVecVar(f"m{n}", 8 * n)
        h = T.keccak256(x)
        P, _ = _watched([h])
        inputs = keccak_sweep_inputs(n, rng)
        _, got = _cport_values(P, [h], [[v] for v in inputs])
        for v, g in zip(inputs, got):
            (want,) = evaluate_many([h], model_from_coordinates(P, [v]))
            assert want == keccak256_int(v.to_bytes(n, "big"))
            assert g[0] == want, (n, hex(v)[:40])


@pytest.mark.parametrize("seed", range(8))
def test_wide_cport_random_dags_match_python_oracle(seed):
    """Random DAGs over 1025 / 1088 / 2048 / 4096-bit variables (``WideRandomProgram``): every term
    of every candidate, and the verdict, against ``oracle/bv.py``."""
    rp = WideRandomProgram(400 + seed, n_ops=50)
    P = ssa.flatten(rp.roots, extra=rp.terms)
    P.set_watch([P.term_node[t.id] for t in rp.terms])
    assigns = random_assignments(P, 32, seed)
    rng = random.Random(seed)
    for a in assigns[::2]:  # edge_value draws many narrow values: fill half of the rows
        for c in P.coords:
            a[c.index] = rng.getrandbits(c.width)
    ver, got = _cport_values(P, rp.terms, assigns)
    for i, a in enumerate(assigns):
        m = model_from_coordinates(P, a)
        want = evaluate_many(rp.terms + rp.roots, m)
        for t, g, w in zip(rp.terms, got[i], want):
            assert g == w, (seed, i, T.to_sexpr(t, 2))
        assert ver[i] == int(all(want[len(rp.terms):])), (seed, i)


@pytest.mark.parametrize("w", [1025, 1056, 1088, 2047, 2048, 2049, 4096])
def test_wide_cport_operators_at_edges(w):
    """Every operator admitted above 256 bits on the edge pairs of ``wide_edge_values`` (carries
    through every limb, 2^1024 and its predecessor, differences in limb 0 / the top limb only)."""
    a, b, c, terms = wide_operator_terms(w)
    P, _ = _watched(terms)
    ci = {co.name: co.index for co in P.coords}
    pairs = wide_edge_values(w, random.Random(w))
    assigns = []
    for k, (x, y) in enumerate(pairs):
        row = [0] * len(P.coords)
        row[ci[a.params[0]]], row[ci[b.params[0]]], row[ci[c.params[0]]] = x, y, k & 1
        assigns.append(row)
    _, got = _cport_values(P, terms, assigns)
    for i, row in enumerate(assigns):
        want = evaluate_many(terms, model_from_coordinates(P, row))
        for t, g, v in zip(terms, got[i], want):
            assert g == v, (w, i, T.to_sexpr(t, 2))


@pytest.mark.parametrize("w", [1025, 1088, 2048, 4096])
def test_wide_cport_uniform_coordinates_follow_the_formula(w):
    """``gen_soa`` of a UNIFORM coordinate above 1024 bits: limb j of candidate i is u_j of the
    documented recurrence (``uniform_raw`` of tests/test_gen3_spec.py), the top limb masked."""
    x = T.BitVecVar("g3w", w)
    P = ssa.flatten([T.eq(x, T.BitVecVal(0, w))])
    (c,) = [co.index for co in P.coords if co.name == "g3w"]
    gb = search.GenBuilder(P)
    gb.uniform(c)
    L = ssa.limbs(w)
    seed = 0x6D797468
    for start in (0, 61, (1 << 40) | 0x800000FD):
        n = 70  # across a 64-index group boundary
        soa = cport.gen_soa(P.to_bytes(), gb.blob(), seed, start, n, L, wide=True)
        for i in range(n):
            want = uniform_raw(keys(start + i, seed), c, L)
            if w % 32:
                want[-1] &= (1 << (w % 32)) - 1
            assert [int(v) for v in soa[:, i]] == want, (w, start + i)


def test_default_cport_refuses_wide_programs():
    """The default library (MAXW 16) answers a 1032-bit program with an error from every entry
    point — never with verdicts — and takes the same program at 1024 bits."""
    for nbytes, ok in ((128, True), (129, False)):
        x = T.BitVecVar("rf", 8 * nbytes)
        root = T.bvcmp("bvult", T.keccak256(x), T.BitVecVal(1 << 255, 256))
        P, blob = search.prepare([root])
        pb = P.to_bytes()
        soa = ssa.soa_from_assignments(P, [[5] * len(P.coords)] * 4)
        cw = sum(ssa.limbs(c.width) for c in P.coords)
        ww = native.check_program(pb).watch_words  # the model read-back rows search.prepare set
        calls = [lambda: cport.eval_soa(pb, soa, 4), lambda: cport.eval_soa(pb, soa, 4, watch_words=ww),
                 lambda: cport.search(pb, blob, 1, 0, 8, verdicts=True), lambda: cport.gen_soa(pb, blob, 1, 0, 8, cw)]
        for call in calls:
            if ok:
                call()
            else:
                with pytest.raises(RuntimeError, match="failed: -2"):
                    call()
        # the wide library takes both
        assert cport.eval_soa(pb, soa, 4, wide=True).shape == (4,)


def test_wide_cport_memory_region_queries_carry_information():
    """The memory-region queries under their default generators: the wide C port's verdicts on 96
    generated candidates equal the Python oracle's on the same coordinates (``gen_soa``), and hold
    both values (a query nobody or everybody satisfies would compare nothing)."""
    for name, (roots, nbytes) in memory_region_queries().items():
        P, blob = search.prepare(roots)
        pb = P.to_bytes()
        n = 96
        ver = cport.search(pb, blob, 0x6D797468, 37, n, threads=2, verdicts=True, wide=True)[2]
        assert 0 < int(ver.sum()) < n, (name, int(ver.sum()))
        soa = cport.gen_soa(pb, blob, 0x6D797468, 37, n, sum(ssa.limbs(c.width) for c in P.coords), wide=True)
        row = {}
        acc = 0
        for c in P.coords:
            row[c.index] = acc
            acc += ssa.limbs(c.width)
        for i in range(n):
            a = [ssa.limbs_to_int([int(soa[row[c.index] + j, i]) for j in range(ssa.limbs(c.width))]) for c in P.coords]
            want = int(all(evaluate_many(roots, model_from_coordinates(P, a))))
            assert ver[i] == want, (name, i)


def test_first_tier_width_boundary():
    """``native.jit_asm`` takes a 2048-bit value (256-byte Keccak input, two sponge blocks) and
    refuses a 2049-bit one and a 257-byte Keccak input with EngineUnsupported: a tier that
    silently narrowed would emit a kernel here."""
    def prog(w, keccak):
        x = T.BitVecVar("tb", w)
        if keccak:
            root = T.bvcmp("bvult", T.keccak256(x), T.BitVecVal(1 << 255, 256))
        else:
            root = T.bvcmp("bvult", T.bvun("bvnot", x), x)
        return search.prepare([root])

    for w, keccak in ((2048, False), (2048, True)):
        P, blob = prog(w, keccak)
        assert "mgj_search:" in native.jit_asm(P.to_bytes(), blob)
        P.set_watch([])
        assert "mgj_eval:" in native.jit_asm(P.to_bytes(), None)
    for w, keccak in ((2049, False), (2056, True)):
        P, blob = prog(w, keccak)
        with pytest.raises(native.EngineUnsupported, match="wider than 2048 bits"):
            native.jit_asm(P.to_bytes(), blob)
        P.set_watch([])
        with pytest.raises(native.EngineUnsupported, match="wider than 2048 bits"):
            native.jit_asm(P.to_bytes(), None)
