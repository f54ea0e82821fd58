"""The device climb's population step on the CPU: ``mg_climb_select_host`` runs the very function
``k_climb_select`` runs (``csrc/climb_select.h``) over host arrays, and must give what
``search.next_population`` followed by ``search.population_seeds`` gives.  No GPU."""
import random

import numpy as np
import pytest

from mythril_amd import native, search, ssa
from mythril_amd.smt import terms as T

SLOTS = native.MG_SCORED_SLOTS
EMPTY = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def lib():
    from mythril_amd import build

    build.build()
    return native.load_library()


_PROGRAMS = {}


def _program(widths):
    """A program whose coordinates are scalars of the given widths (its roots do not matter)."""
    if widths not in _PROGRAMS:
        xs = [T.BitVecVar(f"cs{len(_PROGRAMS)}_{k}", w) for k, w in enumerate(widths)]
        P = ssa.flatten([T.eq(x, T.BitVecVal(1, w)) for x, w in zip(xs, widths)])
        assert [c.width for c in P.coords] == list(widths)
        _PROGRAMS[widths] = P
    return _PROGRAMS[widths]


def _case(rng, n_prev=None, n_win=None, beam=None, pool=4):
    widths = tuple(rng.choice([1, 8, 31, 32, 33, 40, 64, 100, 160, 200, 255, 256]) for _ in range(rng.randint(1, 3)))
    P = _program(widths)
    limbs = [ssa.limbs(w) for w in widths]
    n_rows = sum(limbs)
    values = [[rng.getrandbits(w) for _ in range(pool)] for w in widths]
    model = lambda: {c: rng.choice(values[c]) for c in range(len(widths))}
    n_prev = rng.randint(0, SLOTS) if n_prev is None else n_prev
    n_win = rng.randint(0, SLOTS) if n_win is None else n_win
    beam = rng.randint(1, SLOTS) if beam is None else beam
    start = rng.choice([0, 4096, (1 << 40) + 17])
    # indices: distinct among the winners and among the members, shared between the two now and then
    ipool = rng.sample(range(1 << 12), 48)
    previous = [(rng.randint(1, 3), start - 4096 + i if start >= 4096 and rng.random() < 0.5 else start + i, model())
                for i in rng.sample(ipool, n_prev)]
    if len({i for _, i, _ in previous}) != n_prev:  # (an earlier round's index met this round's)
        previous = [(v, start + 5000 + q, m) for q, (v, _, m) in enumerate(previous)]
    slots = rng.sample(range(SLOTS), n_win)
    rel = rng.sample(ipool, n_win)
    winners_by_slot = {s: (rng.randint(1, 3), start + r, model()) for s, r in zip(slots, rel)}
    # the watch rows: the seed rows scattered among other words
    ww = n_rows + rng.randint(0, 5)
    watch_row = rng.sample(range(ww), n_rows)
    srows = np.array([[rng.getrandbits(32) for _ in range(ww)] for _ in range(SLOTS)], dtype=np.uint32)
    words = np.full(SLOTS, EMPTY, dtype=np.uint64)
    for s, (v, i, m) in winners_by_slot.items():
        words[s] = (v << 48) | (i - start)
        r = 0
        for c, L in enumerate(limbs):
            for j in range(L):
                srows[s, watch_row[r]] = (m[c] >> (32 * j)) & 0xFFFFFFFF
                r += 1
    winners = [winners_by_slot[s] for s in sorted(winners_by_slot)]
    return P, n_rows, previous, winners, beam, start, words, srows, watch_row


def _prev_arrays(P, previous, n_rows):
    if not previous:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros((n_rows, 0), np.uint32)
    s = search.population_seeds(P, [m for _, _, m in previous])
    assert s.rows.shape == (n_rows, len(previous))
    return (np.array([v for v, _, _ in previous], np.uint32), np.array([i for _, i, _ in previous], np.uint64), s.rows)


def _check(case):
    P, n_rows, previous, winners, beam, start, words, srows, watch_row = case
    want = search.next_population(previous, winners, beam)
    pv, pi, pr = _prev_arrays(P, previous, n_rows)
    viol, index, rows = native.climb_select_host(words, srows, watch_row, start, pv, pi, pr, beam)
    assert viol == [v for v, _, _ in want] and index == [i for _, i, _ in want]
    if want:
        s = search.population_seeds(P, [m for _, _, m in want])
        assert np.array_equal(rows, s.rows)
        assert s.keep16 == search.warm_keep16(len(P.coords)) and (s.coord_has == (1 << len(want)) - 1).all()
    else:
        assert rows.shape == (n_rows, 0)
    return want


def _key(m):
    return tuple(sorted(m.items()))


def test_random_cases_against_the_python_rule():
    rng = random.Random(0xC11B)
    seen = {"dup among winners": 0, "dup of a member": 0, "violation tie, winner and member": 0,
            "violation tie, index decides": 0, "index shared by a winner and a member": 0, "cut at beam": 0,
            "fewer than beam": 0}
    for _ in range(400):
        case = _case(rng)
        _, _, previous, winners, beam, *_ = case
        want = _check(case)
        wk = [_key(m) for _, _, m in winners]
        seen["dup among winners"] += len(set(wk)) < len(wk)
        seen["dup of a member"] += bool(set(wk) & {_key(m) for _, _, m in previous})
        seen["violation tie, winner and member"] += bool({v for v, _, _ in winners} & {v for v, _, _ in previous})
        seen["violation tie, index decides"] += len({v for v, _, _ in winners}) < len(winners)
        seen["index shared by a winner and a member"] += bool({i for _, i, _ in winners} & {i for _, i, _ in previous})
        distinct = len({_key(m) for _, _, m in winners + previous})
        seen["cut at beam"] += distinct > beam
        seen["fewer than beam"] += distinct < beam and len(want) == distinct
    print(seen)
    assert all(n >= 20 for n in seen.values()), seen


def test_empty_previous_population_and_no_winners():
    rng = random.Random(7)
    for _ in range(40):
        case = _case(rng, n_prev=0)
        assert len(_check(case)) <= len(case[3])  # nothing but this round's winners
    for _ in range(10):
        case = _case(rng, n_win=0)
        assert len(_check(case)) <= len(case[2])  # the members again, de-duplicated and cut at beam
    assert _check(_case(rng, n_prev=0, n_win=0)) == []


def test_fewer_distinct_entries_than_beam():
    rng = random.Random(11)
    for _ in range(40):
        case = _case(rng, n_prev=rng.randint(8, 32), n_win=rng.randint(8, 32), beam=32, pool=1)
        want = _check(case)  # a pool of one value per coordinate: every entry is the same assignment
        assert len(want) == 1
    for _ in range(40):
        want = _check(_case(rng, beam=32, pool=2))
        assert len(want) <= 8


def test_full_house_at_beam_32():
    rng = random.Random(13)
    for _ in range(20):
        want = _check(_case(rng, n_prev=32, n_win=32, beam=32, pool=64))
        assert len(want) >= 16


def test_arguments_are_checked():
    rng = random.Random(17)
    P, n_rows, previous, winners, beam, start, words, srows, watch_row = _case(rng, n_prev=3, n_win=5)
    pv, pi, pr = _prev_arrays(P, previous, n_rows)
    for kw in ({"beam": 0}, {"beam": 33}, {"watch_row": [srows.shape[1]] * n_rows}):
        a = {"beam": beam, "watch_row": watch_row}
        a.update(kw)
        with pytest.raises(native.EngineError) as ei:
            native.climb_select_host(words, srows, a["watch_row"], start, pv, pi, pr, a["beam"])
        assert ei.value.code == native.MG_E_INVALID, kw
