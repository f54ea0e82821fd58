"""The wave table of ``tests/wave_op_cases.py`` on the GPU, explicit inputs: per width one program
that watches every operator term (UDIV, UREM, SDIV, SREM, SMOD, SHL, LSHR, ASHR, MUL, UMUL_NOOVF,
EXP at 256 and 64 bits, and the divisions by literal one-limb divisors), all of the width's waves
in one call, each wave at a candidate offset that is a multiple of 64 so that one wavefront
evaluates exactly its 64 pairs (the mapping is in the table module's docstring).  Every value of
every candidate is compared with ``oracle/bv.py`` under the supplied assignment, through the
interpreter (``mg_eval``), the O3 kernel and the first tier (``mg_jit_eval``), row-major and tiled.
One width runs again 37 candidates further on, so that every wavefront straddles two profiles.

Generator form (the table module's ``gen_case``: DICT coordinates that pin a profile, a third DICT
coordinate of thresholds): the interpreter, the O3 search kernel, the first tier and
``mg_search_batch`` against the C port on 4,096 candidates from index 0 and from an odd 63-bit
start: verdicts per candidate, first hit and hit count, early exit off and on.

No engine may refuse a program: a refusal raises in ``jit_compile`` and fails the test.

Reference anchor: a term's value is ``Model.eval(term, model_completion=True)``
(``mythril/laser/smt/model.py:45-59``)."""
import pytest

import numpy as np

from mythril_amd import native
from mythril_amd.native import tile_soa
from oracle import cport
from tests import wave_op_cases as W

pytestmark = pytest.mark.gpu

ENGINES = {"interp": None, "o3": dict(asm=False, o3=True, tiled=False), "tier1": dict(asm=True, o3=False, tiled=False),
           "o3_tiled": dict(asm=False, o3=True, tiled=True), "tier1_tiled": dict(asm=True, o3=False, tiled=True)}


def _run(engine, p, how):
    prog = engine.load(p.pb)
    try:
        assert engine.info(prog).watch_words == p.watch_words
        if how is None:
            return engine.eval(prog, p.soa, p.n, watch_words=p.watch_words)
        jh = engine.jit_compile(prog, 0, asm=how["asm"], tiled=how["tiled"], o3=how["o3"])
        try:
            flags = engine.jit_layout(jh)[0]  # the tier asked for, not a fall-back
            assert bool(flags & native.MG_JIT_ASM) == how["asm"] and bool(flags & native.MG_JIT_SOA_TILED) == how["tiled"]
            return engine.jit_eval(jh, tile_soa(p.soa) if how["tiled"] else p.soa, p.n, watch_words=p.watch_words)
        finally:
            engine.jit_free(jh)
    finally:
        engine.free(prog)


@pytest.mark.parametrize("how", list(ENGINES))
@pytest.mark.parametrize("w", W.WIDTHS)
def test_every_wave_bit_exact(engine, w, how):
    p = W.program(w)
    ver, watch = _run(engine, p, ENGINES[how])
    assert ver.all()
    bad = p.mismatches(watch)
    assert not bad, (w, how, bad)


@pytest.mark.parametrize("how", list(ENGINES))
def test_waves_straddling_wavefronts(engine, how):
    """Width 64 (EXP, every divisor class up to two limbs) from candidate 37 on."""
    p = W.program(64, 37)
    ver, watch = _run(engine, p, ENGINES[how])
    bad = p.mismatches(watch)
    assert ver.all() and not bad, (how, bad)


# ---- generator form ----------------------------------------------------------------------------------

N = W.GEN_COUNT
_ref = {}  # (case, start) -> the C port's (first hit, hits, verdicts), computed once
_trouble = []


@pytest.fixture(autouse=True)
def _stop_after_trouble():
    """A HIP error (a fault among them) ends the module: no further launch on that device."""
    if _trouble:
        pytest.fail("an earlier GPU step failed with a HIP error (%s): nothing more is started" % _trouble[0])


def _gpu(f, *a, **kw):
    try:
        return f(*a, **kw)
    except native.EngineError as e:
        if e.code == native.MG_E_HIP:
            _trouble.append(str(e)[:200])
        raise


class Loaded:
    def __init__(self, engine, case):
        self.case, self.ref = case, {}
        for start in W.GEN_STARTS:
            if (case.name, start) not in _ref:
                _ref[case.name, start] = cport.search(case.pb, case.blob, case.seed, start, N, threads=2, verdicts=True)
                assert N // 8 <= _ref[case.name, start][1] <= 7 * N // 8, (case.name, hex(start))
            self.ref[start] = _ref[case.name, start]
        self.prog = _gpu(engine.load, case.pb)
        self.gen = _gpu(engine.load_gen, self.prog, case.blob)

    def free(self, engine):
        engine.free_gen(self.gen)
        engine.free(self.prog)


@pytest.fixture
def loaded(engine, request):
    ld = Loaded(engine, W.gen_case(request.param))
    yield ld
    ld.free(engine)


def _check_kernel(engine, ld, asm):
    jh = _gpu(engine.jit_compile, ld.prog, ld.gen, gen_verdicts=True, asm=asm)
    try:
        assert bool(engine.jit_layout(jh)[0] & native.MG_JIT_ASM) == asm
        for start in W.GEN_STARTS:
            first, n, want = ld.ref[start]
            ver = _gpu(engine.jit_verdicts, jh, ld.case.seed, start, N)
            bad = np.flatnonzero(ver != want)
            assert bad.size == 0, (ld.case.name, asm, hex(start), bad.size, bad[:4])
            assert _gpu(engine.jit_search, jh, ld.case.seed, start, N, early_exit=False) == (first, n)
            assert _gpu(engine.jit_search, jh, ld.case.seed, start, N, early_exit=True)[0] == first
    finally:
        engine.jit_free(jh)


@pytest.mark.parametrize("loaded", W.gen_case_names(), indirect=True)
def test_generator_form_interpreter(engine, loaded):
    ld = loaded
    for start in W.GEN_STARTS:
        first, n, want = ld.ref[start]
        ver, _ = _gpu(engine.eval_generated, ld.prog, ld.gen, ld.case.seed, start, N)
        bad = np.flatnonzero(ver != want)
        assert bad.size == 0, (ld.case.name, hex(start), bad.size, bad[:4])
        assert _gpu(engine.search, ld.prog, ld.gen, ld.case.seed, start, N, early_exit=False) == (first, n)
        assert _gpu(engine.search, ld.prog, ld.gen, ld.case.seed, start, N, early_exit=True)[0] == first


@pytest.mark.parametrize("loaded", W.gen_case_names(), indirect=True)
def test_generator_form_o3_kernel(engine, loaded):
    _check_kernel(engine, loaded, asm=False)


@pytest.mark.parametrize("loaded", W.gen_case_names(), indirect=True)
def test_generator_form_first_tier(engine, loaded):
    _check_kernel(engine, loaded, asm=True)


@pytest.mark.parametrize("w", W.GEN_WIDTHS)
def test_generator_form_batch_path(engine, w):
    """Every generator-form case of a width in one ``mg_search_batch`` call, windows alternating."""
    lds = [Loaded(engine, W.gen_case(name)) for name in W.gen_case_names() if name.startswith(f"w{w}_")]
    try:
        reqs = [(ld.prog, ld.gen, ld.case.seed, W.GEN_STARTS[q % 2], N, None) for q, ld in enumerate(lds)]
        want = [ld.ref[W.GEN_STARTS[q % 2]][:2] for q, ld in enumerate(lds)]
        assert _gpu(engine.search_batch, reqs, early_exit=False) == want
        got = _gpu(engine.search_batch, reqs, early_exit=True)
        assert [g[0] for g in got] == [x[0] for x in want]
    finally:
        for ld in lds:
            ld.free(engine)
