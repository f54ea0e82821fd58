"""The specialiser's case table on the GPU, every engine: ``tests/spec_fold_cases.py`` grouped into
one program per family (``coord_val``'s generator kinds with the raw blobs whose constants carry
bits outside the width or the mask, the operators' transfer functions, the deciders, LOOKUP
pruning).  The root of a program is the parity of all its case compares and a probe bit no analysis
decides: a correctly folded compare is a constant of it, a wrong one flips the verdict wherever the
truth differs — and so does an engine whose generator reads a constant differently from the C port,
or a first tier that compares dictionary coordinates by an entry index of unmasked entries.

Per program and window, against ``cport.search(..., verdicts=True)`` on the UNSPECIALISED program:
the interpreter's ``eval_generated`` verdicts and ``mg_search``; ``jit_verdicts`` and ``jit_search``
of the O3 kernel and of the first tier; one ``search_batch`` entry.  An early-exit search finds the
exact search's first hit.  Windows of 2,048: seed 1 from 0, seed 99 from a 63-bit start with bit 31
of the low word set.  Four programs, so four O3 compiles."""
import numpy as np
import pytest

from mythril_amd import native
from oracle import cport
from tests import spec_fold_cases as S

pytestmark = pytest.mark.gpu
N = S.WINDOW
WINDOWS = [(S.SEEDS[0], S.STARTS[0]), (S.SEEDS[1], S.STARTS[1])]


class Loaded:
    def __init__(self, engine, pr):
        self.pr = pr
        self.prog = engine.load(pr.prog)
        self.gen = engine.load_gen(self.prog, pr.blob)
        # the reference, once: the C port on the unspecialised program
        self.ref = {w: cport.search(pr.prog, pr.blob, w[0], w[1], N, verdicts=True) for w in WINDOWS}
        for w, (first, n, _) in self.ref.items():
            assert first is not None and 0 < n < N, (pr.name, w, n)
        self.jit = {}

    def kernel(self, engine, asm):
        """The O3 kernel or the first tier's, compiled once with mgj_gen.  A refusal fails the test."""
        if asm not in self.jit:
            self.jit[asm] = engine.jit_compile(self.prog, self.gen, gen_verdicts=True, asm=asm)
            assert bool(engine.jit_layout(self.jit[asm])[0] & native.MG_JIT_ASM) == asm
            print(self.pr.name, "first tier" if asm else "O3 kernel", "compile ms", round(engine.jit_info(self.jit[asm])[0], 1))
        return self.jit[asm]


@pytest.fixture(scope="module")
def loaded(engine):
    out = {fam: Loaded(engine, S.group(fam)) for fam in S.FAMILIES}
    yield out
    for ld in out.values():
        for j in ld.jit.values():
            engine.jit_free(j)
        engine.free_gen(ld.gen)
        engine.free(ld.prog)


def _same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (*what, f"{bad.size} of {N} verdicts differ", bad[:4].tolist())


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_interpreter(engine, loaded, fam):
    ld = loaded[fam]
    for (seed, start), (first, n, want) in ld.ref.items():
        ver, _ = engine.eval_generated(ld.prog, ld.gen, seed, start, N)
        _same(ver, want, (fam, seed, hex(start)))
        assert engine.search(ld.prog, ld.gen, seed, start, N, early_exit=False) == (first, n)
        assert engine.search(ld.prog, ld.gen, seed, start, N, early_exit=True)[0] == first


@pytest.mark.parametrize("asm", [False, True], ids=["o3", "first_tier"])
@pytest.mark.parametrize("fam", S.FAMILIES)
def test_compiled_kernels(engine, loaded, fam, asm):
    ld = loaded[fam]
    jh = ld.kernel(engine, asm)
    for (seed, start), (first, n, want) in ld.ref.items():
        _same(engine.jit_verdicts(jh, seed, start, N), want, (fam, asm, seed, hex(start)))
        assert engine.jit_search(jh, seed, start, N, early_exit=False) == (first, n)
        assert engine.jit_search(jh, seed, start, N, early_exit=True)[0] == first


def test_batch_path(engine, loaded):
    """Every family in one mg_search_batch call: entry for entry the C port's first hit and count."""
    reqs, want = [], []
    for q, fam in enumerate(S.FAMILIES):
        ld = loaded[fam]
        seed, start = WINDOWS[q % len(WINDOWS)]
        reqs.append((ld.prog, ld.gen, seed, start, N, None))
        want.append(ld.ref[(seed, start)][:2])
    assert engine.search_batch(reqs, early_exit=False) == want
    assert [f for f, _ in engine.search_batch(reqs, early_exit=True)] == [f for f, _ in want]
