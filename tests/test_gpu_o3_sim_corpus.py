"""The kernels on which the CPU simulator is judged (``tests/test_o3_sim_cpu.py``), on the MI355X: the
fuzz parts of ``tests/o3_corpus.py`` (random tier programs, LASER-shaped queries, the generator-
representation fuzz; the programs, generator seeds and start indices of the CPU test) and its two
``decided`` queries, compiled by the O3 tier (``jit_compile(..., gen_verdicts=True, o3=True)``) and
compared with the C port: ``mgj_gen`` verdicts of 4,096 candidates from the CPU test's start index,
``mgj_search`` first hit and hit count, and the early-exit first hit.  The table is run on the O3
kernel by ``tests/test_gpu_gen_repr.py``; the edge and fold programs and the workloads by their own
GPU tests.  Where simulator and hardware ever part on a corpus kernel, one of the two suites shows it.

Each test compiles eight programs.  After a HIP error nothing more is started: every later test of
the module fails at once.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``) over the GEN3 candidate stream."""
import numpy as np
import pytest

from mythril_amd import native
from oracle import cport
from tests import o3_corpus as O

pytestmark = pytest.mark.gpu
N = 4096
CHUNK = 8
GPU_PARTS = O.FUZZ_PARTS + ("decided",)
CHUNKS = [(p, lo) for p in GPU_PARTS
          for lo in range(0, len(O.FUZZ_SEEDS[p]) if p in O.FUZZ_SEEDS else 2, CHUNK)]
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


@pytest.mark.parametrize("part,lo", CHUNKS, ids=[f"{p}{lo}" for p, lo in CHUNKS])
def test_o3_kernel_on_the_corpus(engine, part, lo):
    for e in O.part(part)[lo:lo + CHUNK]:
        (start, _), = e.windows
        first, n, want = cport.search(e.pb, e.blob, e.seed, start, N, threads=2, verdicts=True)
        prog = _gpu(engine.load, e.pb)
        gen = _gpu(engine.load_gen, prog, e.blob)
        try:
            jh = _gpu(engine.jit_compile, prog, gen, gen_verdicts=True, o3=True)
            try:
                assert not engine.jit_layout(jh)[0] & native.MG_JIT_ASM, e.name
                ver = _gpu(engine.jit_verdicts, jh, e.seed, start, N)
                bad = np.flatnonzero(ver != want)
                assert bad.size == 0, (e.name, hex(start), bad.size, bad[:4])
                assert _gpu(engine.jit_search, jh, e.seed, start, N, early_exit=False) == (first, n), e.name
                assert _gpu(engine.jit_search, jh, e.seed, start, N, early_exit=True)[0] == first, e.name
            finally:
                engine.jit_free(jh)
        finally:
            engine.free_gen(gen)
            engine.free(prog)
