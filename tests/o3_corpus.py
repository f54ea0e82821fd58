"""The corpus on which the O3 tier's compiled kernels are judged, on the CPU simulator
(``tests/test_o3_sim_cpu.py``) and, its fuzz part, on the hardware (``tests/test_gpu_o3_sim_corpus.py``):
the same programs, generator seeds and start indices in both, so that a kernel the simulator passes
is a kernel the MI355X was asked about as well.

Every entry is ``Entry(name, pb, blob, seed, windows)``: the program as the engine receives it, its
generator blob and seed, and ``[(start, count)]``.  The fuzz parts take one unaligned window of 512
candidates with bit 31 of the low index word set (as ``test_gpu_sweep._windows`` builds them); their
program seeds are the first of each generator for which the C port alone finds a hit and a miss in
that window under the generator seed listed (``find_fuzz_seeds`` wrote the tables below; the CPU test
asserts the condition again before it looks at a tier).  ``decided`` is not a fuzz part: two LASER-shaped
queries no candidate of the window satisfies.  For such a program the compiler drops the per-wave
publication of hits and the block's wave counter becomes an LDS add without return (``ds_add_u32``), a
form the mixed windows above cannot hold; the kernel must report no hit and a count of 0."""
import functools
import random
from collections import namedtuple

Entry = namedtuple("Entry", "name pb blob seed windows")

FUZZ_COUNT = 64 * 8
N_FUZZ = 48  # per generator
PARTS = ("table", "edge", "fold", "tier", "laser", "repr", "workloads", "decided")
FUZZ_PARTS = ("tier", "laser", "repr")


def fuzz_start(kind: str, s: int) -> int:
    rng = random.Random(f"o3-corpus-{kind}-{s}")
    start = rng.getrandbits(63)
    return (start & ~0xFFFFFFFF) | 0x80000000 | rng.getrandbits(31) | 1  # bit 31 set, never group-aligned


def _fuzz_program(kind: str, s: int):
    """(pb, blob) of program seed ``s`` of fuzz generator ``kind``"""
    from mythril_amd import search

    if kind == "repr":
        from tests import gen_repr_cases as G

        c = G.fuzz_case(s)
        return bytes(c.pb), c.blob
    if kind == "tier":
        from tests.helpers import random_tier_program

        roots = random_tier_program(s, full=True)
    else:
        from tests.lasergen import laser_query

        roots = laser_query(s, full=True)
    P, blob = search.prepare(roots)
    return P.to_bytes(), blob


def mixed_window(pb, blob, seed, start, count=FUZZ_COUNT) -> bool:
    """a hit and a miss, by the C port alone"""
    from oracle import cport

    hits = cport.search(pb, blob, seed, start, count, threads=1)[1]
    return 0 < hits < count


def find_fuzz_seeds(kind: str, n: int = N_FUZZ, tries: int = 8):
    """[(program seed, generator seed)]: the first ``n`` program seeds, from 0 up, with a generator seed
    among the first ``tries`` (from 1) under which the window holds a hit and a miss."""
    out, s = [], 0
    while len(out) < n:
        pb, blob = _fuzz_program(kind, s)
        for g in range(1, 1 + tries):
            if mixed_window(pb, blob, g, fuzz_start(kind, s)):
                out.append((s, g))
                break
        s += 1
        if s > 40 * n:
            raise RuntimeError("no seeds for " + kind)
    return out


# (program seed, generator seed), by find_fuzz_seeds
FUZZ_SEEDS = {
    "tier": [
        (0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (10, 1), (11, 1), (12, 1), (13, 1), (14, 1), (15, 1),
        (17, 1), (19, 1), (20, 1), (21, 1), (22, 1), (23, 1), (30, 1), (31, 1), (33, 1), (35, 1), (36, 1), (37, 1),
        (38, 2), (39, 1), (40, 1), (46, 1), (47, 1), (49, 1), (51, 1), (52, 1), (54, 1), (55, 1), (56, 1), (57, 1),
        (60, 1), (61, 1), (63, 1), (64, 1), (66, 1), (67, 1), (68, 1), (69, 1), (70, 1), (72, 1), (73, 1), (75, 1),
    ],
    "laser": [
        (0, 1), (2, 1), (9, 2), (17, 1), (22, 1), (23, 1), (31, 8), (33, 1), (35, 1), (36, 2), (42, 1), (46, 2),
        (52, 8), (53, 2), (57, 1), (80, 1), (82, 1), (86, 1), (89, 1), (99, 1), (105, 2), (111, 1), (117, 1),
        (122, 1), (124, 7), (128, 1), (130, 3), (132, 1), (133, 3), (138, 1), (139, 2), (145, 4), (148, 1),
        (162, 4), (163, 1), (169, 2), (170, 1), (173, 1), (179, 1), (182, 1), (183, 1), (186, 1), (191, 1),
        (198, 1), (199, 1), (201, 1), (206, 1), (207, 1),
    ],
    "repr": [
        (0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (9, 1), (10, 1), (11, 1), (12, 1),
        (13, 1), (14, 1), (15, 1), (16, 1), (17, 1), (18, 1), (19, 1), (20, 1), (21, 1), (22, 1), (23, 1), (24, 1),
        (25, 1), (26, 1), (27, 1), (28, 1), (29, 1), (30, 1), (31, 1), (32, 1), (33, 1), (34, 1), (35, 1), (36, 1),
        (37, 1), (38, 1), (39, 1), (40, 1), (41, 1), (42, 1), (43, 1), (44, 1), (45, 1), (46, 1), (47, 1),
    ],
}


@functools.lru_cache(maxsize=None)
def part(name: str):
    """The entries of one corpus part, in a fixed order."""
    from mythril_amd import search, workloads

    out = []
    if name == "table":
        from tests import gen_repr_cases as G

        for n in G.program_names():
            c = G.program(n)
            out.append(Entry(n, bytes(c.pb), c.blob, G.seed_of(c), ((G.ALIGNED, G.SIM_COUNT), (G.ODD, G.SIM_COUNT))))
    elif name == "edge":  # the five probe programs, at test_gen3_edges_cpu's simulator windows
        from tests import gen3_edge_cases as E

        for c in E.cases():
            out.append(Entry("edge_" + c.name, bytes(c.prog), c.blob, E.SEED0, tuple((st, E.WINDOW) for st in E.STARTS)))
    elif name == "fold":  # one program per family, at test_spec_fold_cpu's simulator windows
        from tests import spec_fold_cases as S

        for fam in S.FAMILIES:
            g = S.group(fam)
            # a record carries one generator seed: the second window's seed gets an entry of its own
            for k, (seed, start) in enumerate(((S.SEEDS[0], S.STARTS[0]), (S.SEEDS[1], S.STARTS[1]))):
                out.append(Entry(f"fold_{fam}_{k}", bytes(g.prog), g.blob, seed, ((start, S.WINDOW),)))
    elif name in FUZZ_PARTS:
        for s, g in FUZZ_SEEDS[name]:
            pb, blob = _fuzz_program(name, s)
            out.append(Entry(f"{name}{s}", pb, blob, g, ((fuzz_start(name, s), FUZZ_COUNT),)))
    elif name == "decided":
        for s in (4, 7):
            pb, blob = _fuzz_program("laser", s)
            out.append(Entry(f"decided_laser{s}", pb, blob, 1, ((fuzz_start("laser", s), FUZZ_COUNT),)))
    elif name == "workloads":
        rng = random.Random("o3-corpus-workloads")
        for n in sorted(workloads.WORKLOADS):
            P, blob = search.prepare([c.raw for c in workloads.WORKLOADS[n]()])
            st = rng.getrandbits(63)
            wins = ((rng.getrandbits(40) << 6, 64 * 16), ((st & ~0xFFFFFFFF) | 0x80000000 | rng.getrandbits(31) | 1, 64 * 16))
            out.append(Entry(n, P.to_bytes(), blob, rng.getrandbits(32), wins))
    else:
        raise KeyError(name)
    return out
