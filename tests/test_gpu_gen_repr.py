"""Generator representations crossed with the operators that read them, on the GPU, every engine:
the table and the fuzz of ``tests/gen_repr_cases.py`` (dictionaries on each side of every threshold
at which a tier changes how it holds a coordinate, constant-valued coordinates of every kind, the
same dictionaries inside MIXED coordinates and as COPY sources; each read by every operator family).

Every table program on every path — the interpreter (``eval_generated`` verdicts, ``search`` first
hit and hit count, full sweep and early exit), the O3 kernel and the first tier (``jit_verdicts``,
``jit_search``) and ``mg_search_batch`` — against ``cport.search(..., verdicts=True)`` byte for
byte, over 4,096 candidates from 2^40 and from 2^40 + 37; 96 fuzz programs on the first tier.  The
corpus conditions (hits and misses in every window; an all-false, a mixed and an all-true group of
every guarded condition) are asserted from the C port before a GPU result is looked at.

Everything runs in this process.  After a HIP error nothing more is started: every later test of
the module fails at once.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``) over the GEN3 candidate stream."""
import numpy as np
import pytest

from mythril_amd import native
from oracle import cport
from tests import gen_repr_cases as G

pytestmark = pytest.mark.gpu
N = G.GPU_COUNT
STARTS = (G.ALIGNED, G.ODD)
FUZZ_PARTS = 4
_trouble = []
_ref = {}  # (program, start) -> the C port's (first hit, hits, verdicts), computed once


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
    """A program and its generator on the device, with the C port's answer per window (computed once,
    after the corpus conditions)."""

    def __init__(self, engine, case):
        self.case, self.seed = case, G.seed_of(case)
        self.ref = {}
        for start in STARTS:
            if (case.name, start) not in _ref:
                assert G.window_ok(case, self.seed, start, N), (case.name, hex(start))
                _ref[case.name, start] = cport.search(case.pb, case.blob, self.seed, start, N, threads=2, verdicts=True)
            self.ref[start] = _ref[case.name, start]
        self.prog = _gpu(engine.load, case.pb)
        self.gen = _gpu(engine.load_gen, self.prog, case.blob)

    def free(self, engine):
        engine.free_gen(self.gen)
        engine.free(self.prog)


@pytest.fixture
def loaded(engine, request):
    ld = Loaded(engine, G.program(request.param))
    yield ld
    ld.free(engine)


def _check_kernel(engine, ld, asm):
    """mgj_gen verdicts, mgj_search full sweep and early exit of one tier against the C port."""
    jh = _gpu(engine.jit_compile, ld.prog, ld.gen, gen_verdicts=True, asm=asm)
    try:
        assert bool(engine.jit_layout(jh)[0] & native.MG_JIT_ASM) == asm
        for start in STARTS:
            first, n, want = ld.ref[start]
            ver = _gpu(engine.jit_verdicts, jh, ld.seed, start, N)
            bad = np.flatnonzero(ver != want)
            assert bad.size == 0, (ld.case.name, asm, hex(start), bad.size, bad[:4])
            assert _gpu(engine.jit_search, jh, ld.seed, start, N, early_exit=False) == (first, n)
            assert _gpu(engine.jit_search, jh, ld.seed, start, N, early_exit=True)[0] == first
    finally:
        engine.jit_free(jh)


@pytest.mark.parametrize("loaded", G.program_names(), indirect=True)
def test_interpreter(engine, loaded):
    ld = loaded
    for start in STARTS:
        first, n, want = ld.ref[start]
        ver, _ = _gpu(engine.eval_generated, ld.prog, ld.gen, ld.seed, start, N)
        bad = np.flatnonzero(ver != want)
        assert bad.size == 0, (ld.case.name, hex(start), bad.size, bad[:4])
        assert _gpu(engine.search, ld.prog, ld.gen, ld.seed, start, N, early_exit=False) == (first, n)
        assert _gpu(engine.search, ld.prog, ld.gen, ld.seed, start, N, early_exit=True)[0] == first


@pytest.mark.parametrize("loaded", G.program_names(), indirect=True)
def test_o3_kernel(engine, loaded):
    _check_kernel(engine, loaded, asm=False)


@pytest.mark.parametrize("loaded", G.program_names(), indirect=True)
def test_first_tier(engine, loaded):
    _check_kernel(engine, loaded, asm=True)


@pytest.mark.parametrize("wc", sorted(G.WIDTH_CLASSES))
def test_batch_path(engine, wc):
    """Every table program of a width class in one mg_search_batch call, windows alternating."""
    lds = [Loaded(engine, G.program(name)) for name in G.program_names() if name.startswith(wc + "_")]
    try:
        reqs = [(ld.prog, ld.gen, ld.seed, STARTS[q % 2], N, None) for q, ld in enumerate(lds)]
        want = [ld.ref[STARTS[q % 2]][:2] for q, ld in enumerate(lds)]
        assert _gpu(engine.search_batch, reqs, early_exit=False) == want
        got = _gpu(engine.search_batch, reqs, early_exit=True)
        assert [g[0] for g in got] == [w[0] for w in want]
    finally:
        for ld in lds:
            ld.free(engine)


@pytest.mark.parametrize("part", range(FUZZ_PARTS))
def test_fuzz_first_tier(engine, part):
    """96 fuzz programs (guarded cones over shaped coordinates) on the first tier."""
    step = G.N_FUZZ_GPU // FUZZ_PARTS
    for s in range(part * step, (part + 1) * step):
        ld = Loaded(engine, G.fuzz_case(s))
        try:
            _check_kernel(engine, ld, asm=True)
        finally:
            ld.free(engine)
