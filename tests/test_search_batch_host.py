"""Host logic of the batched first launch (``search.search_many``, ``search_partitioned(batch=True)``,
``search(start=...)``) against a stand-in engine, and ``mg_search_batch`` before ``mg_init``: no GPU.

The stand-in hands out one program handle per load and answers a search of program ``p`` with the
first scripted hit index of ``p`` inside the window, else with a miss; every call is recorded.
Reference anchor: ``IndependenceSolver.check`` (``mythril/laser/smt/solver/independence_solver.py:
119-140``) solves the buckets one by one, keeps their order and fails when any bucket fails.
"""
import os
import subprocess
import sys
import threading
from pathlib import Path

from mythril_amd import partition, search, workloads

ROOT = Path(__file__).resolve().parent.parent
CHUNK = 1 << 12


class FakeEngine:
    def __init__(self, hits):
        self.hits = hits  # per loaded program, in load order: the hit index or None
        self.calls = []
        self.n_progs = 0

    def load(self, blob):
        self.n_progs += 1
        self.calls.append(("load", self.n_progs))
        return self.n_progs

    def load_gen(self, prog, blob):
        self.calls.append(("load_gen", prog))
        return 1000 + prog

    def free(self, h):
        self.calls.append(("free", h))

    def free_gen(self, h):
        self.calls.append(("free_gen", h))

    def _answer(self, prog, start, n, assign):
        # a continuation reloads its program: handle k of the second round is bucket order again
        want = self.hits[(prog - 1) % len(self.hits)]
        if want is not None and start <= want < start + n:
            if assign is not None:
                assign[:] = 0
            return want, 1
        return None, 0

    def search(self, prog, gh, seed, start, n, early_exit=True, assign=None):
        self.calls.append(("search", prog, start, n))
        return self._answer(prog, start, n, assign)

    def search_batch(self, reqs, early_exit=True):
        self.calls.append(("search_batch", [(r[0], r[3], r[4]) for r in reqs]))
        return [self._answer(r[0], r[3], r[4], r[5]) for r in reqs]

    def names(self):
        return [c[0] for c in self.calls]


def _buckets(w="suicide_kill"):
    roots = [c.raw for c in workloads.WORKLOADS[w]()]
    return roots, partition.partition(roots)


def test_search_many_makes_one_batch_and_continues_only_the_misses():
    roots, buckets = _buckets()
    assert len(buckets) == 3
    eng = FakeEngine([7, None, 0])
    # the second bucket misses [0, 4096); its reloaded program (handle 4) hits at 5000
    eng.hits = [7, None, 0, 5000]
    res = search.search_many(eng, buckets, chunk=CHUNK, jit="never", timeout_s=10)
    assert [r.index for r in res] == [7, 5000, 0]  # bucket order kept
    assert eng.names().count("search_batch") == 1
    batch = next(c for c in eng.calls if c[0] == "search_batch")[1]
    assert batch == [(1, 0, CHUNK), (2, 0, CHUNK), (3, 0, CHUNK)]
    singles = [c for c in eng.calls if c[0] == "search"]
    # one continuation, for the bucket that missed, from `chunk`, with the launch size that follows it
    assert singles == [("search", 4, CHUNK, 16 * CHUNK)]
    assert res[1].scanned == CHUNK + 16 * CHUNK and res[0].scanned == CHUNK
    assert all(r.model is not None for r in res)
    # every handle released
    assert eng.names().count("free") == eng.names().count("load") == 4
    assert eng.names().count("free_gen") == eng.names().count("load_gen") == 4


def test_search_partitioned_batch_keeps_bucket_order_and_merges():
    roots, buckets = _buckets()
    eng = FakeEngine([7, 11, 13])
    res = search.search_partitioned(eng, roots, batch=True, jit="never")
    assert res.index == (7, 11, 13) and res.buckets == 3
    assert eng.names().count("search_batch") == 1 and "search" not in eng.names()
    ver, scalars, arrays, funcs, progs = res.model
    assert ver == 1 and len(progs) == 3
    serial = FakeEngine([7, 11, 13])
    ref = search.search_partitioned(serial, roots, jit="never")  # the default stays serial
    assert "search_batch" not in serial.names() and serial.names().count("search") == 3
    assert ref.index == res.index and ref.model[0:4] == res.model[0:4]


def test_search_partitioned_batch_env_switch(monkeypatch):
    roots, _ = _buckets()
    monkeypatch.setenv("MYTHGPU_BATCH", "1")
    eng = FakeEngine([7, 11, 13])
    assert search.search_partitioned(eng, roots, jit="never").index == (7, 11, 13)
    assert eng.names().count("search_batch") == 1
    eng = FakeEngine([7, 11, 13])
    search.search_partitioned(eng, roots, jit="never", batch=False)  # the argument wins
    assert "search_batch" not in eng.names()


def test_search_partitioned_batch_is_none_when_a_bucket_gives_up():
    roots, _ = _buckets()
    eng = FakeEngine([7, None, None])
    res = search.search_partitioned(eng, roots, batch=True, jit="never", max_candidates=1 << 17)
    assert res.index is None and res.model is None and res.buckets == 3
    # the second bucket's continuation ran to its budget; the third's was not started
    starts = [c[2] for c in eng.calls if c[0] == "search"]
    assert starts and starts[0] == CHUNK and all(c[1] == 4 for c in eng.calls if c[0] == "search")


def test_cancel_is_honoured_before_the_batch():
    roots, buckets = _buckets()
    ev = threading.Event()
    ev.set()
    eng = FakeEngine([7, 11, 13])
    res = search.search_many(eng, buckets, cancel=ev)
    assert [r.index for r in res] == [None, None, None]
    assert eng.calls == []
    assert search.search_partitioned(eng, roots, batch=True, cancel=ev).index is None
    assert eng.calls == []


def test_cancel_is_honoured_before_a_continuation():
    _, buckets = _buckets()
    ev = threading.Event()

    class Cancelling(FakeEngine):
        def search_batch(self, reqs, early_exit=True):
            out = super().search_batch(reqs, early_exit)
            ev.set()
            return out

    eng = Cancelling([7, None, 0])
    res = search.search_many(eng, buckets, cancel=ev, jit="never")
    assert [r.index for r in res] == [7, None, 0]
    assert "search" not in eng.names()


def test_search_start_keyword_default_keeps_the_engine_calls():
    """``search()`` without ``start`` makes the calls it made before the keyword existed: first
    launch [0, chunk), then x16, then x4; with ``start=chunk`` the first launch is dropped and the rest of
    the sequence is the same."""
    roots = _buckets()[1][0]
    eng = FakeEngine([70000])
    r = search.search(eng, roots, jit="never", max_candidates=1 << 22)
    assert r.index == 70000 and r.scanned == CHUNK + 16 * CHUNK + 64 * CHUNK
    assert eng.calls == [("load", 1), ("load_gen", 1), ("search", 1, 0, CHUNK), ("search", 1, CHUNK, 16 * CHUNK),
                         ("search", 1, 17 * CHUNK, 64 * CHUNK), ("free_gen", 1001), ("free", 1)]
    eng2 = FakeEngine([70000])
    r2 = search.search(eng2, roots, jit="never", max_candidates=1 << 22, start=CHUNK)
    assert r2.index == 70000 and r2.scanned == r.scanned
    assert eng2.calls == [c for c in eng.calls if c != ("search", 1, 0, CHUNK)]
    assert r2.model[1:4] == r.model[1:4]


_BEFORE_INIT = """
from mythril_amd import build, native
build.build()
lib = native.load_library()
req = (native.SearchReq * 1)()
res = (native.SearchRes * 1)()
print(lib.mg_search_batch(1, req, 0, res), lib.mg_search_batch(0, None, 0, None))
"""


def test_search_batch_before_init():
    """A process that never called ``mg_init``: MG_E_NOTINIT for a non-empty batch; an empty one is
    MG_OK, as ``mg_jit_search_many`` answers n = 0."""
    from mythril_amd import native

    r = subprocess.run([sys.executable, "-c", _BEFORE_INIT], cwd=str(ROOT), env=dict(os.environ, PYTHONPATH=str(ROOT)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split()[-2:] == [str(native.MG_E_NOTINIT), str(native.MG_OK)]
