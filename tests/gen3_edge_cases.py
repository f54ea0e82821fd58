"""The GEN3 edge-parameter case table shared by ``test_gen3_edges_cpu.py`` and
``test_gpu_gen3_edges.py``: one program per group of cases (RANGE, ALIGNED, DICT / FIXED / fix,
MIXED, the COPY chain), its generator built with chosen ``GenBuilder`` parameters, and a probe root
whose verdict depends on every bit of every coordinate.

Probe: for a coordinate ``x`` of width ``w <= 256`` the bit ``Extract(w-1, w-1, x * K)`` with a
fixed odd random ``K`` (every bit of ``x`` reaches the product's top bit); a 1-bit coordinate is
its own probe; a wider one is xor-folded into 256 bits first (the first tier and the interpreter's
light tiers refuse arithmetic wider than 256 bits).  The single root is ``xor(probe bits) == 1``.
The program watches its coordinate VAR nodes, so a watch row is a generated limb.
Test infrastructure only."""
from __future__ import annotations

import functools
import random

from mythril_amd import search, ssa
from mythril_amd.smt import Concat, Extract, symbol_factory
from tests import gen3_ref

SEED0 = 0x6D797468
WINDOW = 2048
_rng = random.Random(0x67656E33)
SEEDS = [SEED0, _rng.getrandbits(64), _rng.getrandbits(64)]
# from 0; ending at the last usable index, 2^64 - 2; 63 bits with bit 31 of the low word set
STARTS = [0, (1 << 64) - 1 - WINDOW, _rng.getrandbits(63) | 0x80000001]


def top(w):
    return (1 << w) - 1


class Case:
    """One program of the table.  ``coords``: [(width, spec function(gb, c, index of))] in coordinate order."""

    def __init__(self, name, coords):
        self.name = name
        rng = random.Random("gen3-edge-" + name)
        BVV = symbol_factory.BitVecVal
        syms = [symbol_factory.BitVecSym(f"e_{name}_{q:02d}", w) for q, (w, _) in enumerate(coords)]
        acc = None
        for x, (w, _) in zip(syms, coords):
            if w > 256:  # xor-fold into 256 bits
                f = Extract(255, 0, x)
                for lo in range(256, w, 256):
                    hi = min(lo + 255, w - 1)
                    part = Extract(hi, lo, x)
                    if hi - lo + 1 < 256:
                        part = Concat(BVV(0, 256 - (hi - lo + 1)), part)
                    f = f ^ part
                x, w = f, 256
            bit = x if w == 1 else Extract(w - 1, w - 1, x * BVV(rng.getrandbits(w) | 1, w))
            acc = bit if acc is None else acc ^ bit
        self.P = P = ssa.flatten([(acc == BVV(1, 1)).raw])
        by_name = {c.name: c.index for c in P.coords}
        self.index = [by_name[f"e_{name}_{q:02d}"] for q in range(len(coords))]
        assert self.index == sorted(self.index) and len(P.coords) == len(coords), (name, self.index)
        P.set_watch([P.coords[c].node for c in self.index])
        gb = search.GenBuilder(P)
        for q, (w, spec) in enumerate(coords):
            assert P.coords[self.index[q]].width == w
            spec(gb, self.index[q], self.index)
        self.blob = gb.blob()
        self.prog = P.to_bytes()
        self.widths = [c.width for c in P.coords]
        self.specs, self.consts = gen3_ref.split_blob(self.blob)

    def mixed(self):
        """Indices of the MIXED coordinates."""
        return [c for c, s in enumerate(self.specs) if (s[0] & 0xFF) == gen3_ref.MIXED]

    def ref_rows(self, seed, start, n):
        """The restatement's SoA rows [coord_words][n] (lists of ints)."""
        cols = [gen3_ref.soa_rows(gen3_ref.gen_values(self.specs, self.consts, self.widths, seed, start + q),
                                  self.widths) for q in range(n)]
        return [list(r) for r in zip(*cols)]


def _range(lo, span):
    return lambda gb, c, ix: gb.range(c, lo, span)


def _aligned(lo, p1, count):
    return lambda gb, c, ix: gb.aligned(c, lo, p1, count)


def _mixed(values, fix=None, copy_prev=False, **kw):
    def spec(gb, c, ix):
        gb.mixed(c, values, copy_from=ix[ix.index(c) - 1] if copy_prev else None, **kw)
        if fix:
            gb.fix(c, *fix)
    return spec


def _then_fix(spec, mask, val):
    def f(gb, c, ix):
        spec(gb, c, ix)
        gb.fix(c, mask, val)
    return f


CHAIN_LEN = 65  # static COPY depth 64 = MG_GEN_MAX_COPY_DEPTH


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(0xED6E5)
    t256 = top(256)
    range_case = Case("range", [
        (256, _range(t256 - 5, 100)),            # lo + span wraps the width
        (64, _range(7, 0)),                      # span 0 = 2^32
        (33, _range((1 << 33) - 3, 0xFFFFFFFF)),
        (32, _range(5, 1)),
        (20, _range((1 << 20) - 2, 77)),
        (8, _range(250, 9)),
        (1, _range(1, 2)),
        (512, _range((1 << 512) - 9, 0)),
    ])
    aligned_case = Case("aligned", [
        (256, _aligned(3, 255, 0)),
        (64, _aligned(1, 200, 5)),               # shift beyond the coordinate's limbs
        (33, _aligned((1 << 33) - 1, 31, 0)),
        (32, _aligned(9, 0, 0)),
        (20, _aligned(1, 19, 3)),
        (8, _aligned(0, 7, 1 << 32)),
        (512, _aligned(5, 250, 1000)),
        (256, _aligned(t256, 32, 1 << 31)),
    ])
    fmask = t256 ^ (0xFFFF << 64)  # everything but bits 64..79
    dict_case = Case("dictfix", [
        (256, lambda gb, c, ix: gb.dict(c, [rng.getrandbits(256)])),
        (32, lambda gb, c, ix: gb.dict(c, [rng.getrandbits(32) for _ in range(65535)])),
        (512, lambda gb, c, ix: gb.dict(c, [rng.getrandbits(512) for _ in range(3)])),
        (33, _then_fix(lambda gb, c, ix: gb.fixed(c, (1 << 33) - 1), 1 << 32, 0)),
        (256, _then_fix(lambda gb, c, ix: gb.uniform(c), fmask, rng.getrandbits(256) & fmask)),
    ])
    d256 = [t256, 1 << 255, rng.getrandbits(256)]
    link = dict(copy_prev=True, p_copy=.6, p_dict=.2, p_delta=.5, small_bits=1, p_small=.1)
    mixed_case = Case("mixed", [
        # the delta wraps both ways through all 8 limbs; small_bits > w
        (256, _mixed([0, 1, t256, t256 - 1], p_dict=.5, p_delta=.9, small_bits=300, p_small=.2)),
        (256, _mixed(d256, **link)),
        (256, _mixed(d256, **link)),
        (256, _mixed(d256, fix=(0xFF << 100, 0xA5 << 100), **link)),  # a COPY source with fixed bits
        (256, _mixed(d256, **link)),
        (256, _mixed(d256, **link)),
        # clamp at the top of the range, L = 2 and a partial top limb
        (33, _mixed([0, (1 << 33) - 1], p_dict=.6, p_delta=.99, clamp=((1 << 33) - 10, 10))),
        (16, _mixed([0, 65535, 7], p_dict=.4, p_delta=.99, small_bits=3, p_small=.3)),  # narrow
        (16, _mixed([], p_dict=0., copy_prev=True, p_copy=.5, p_delta=.99, small_bits=16, p_small=.2,
                    clamp=(100, 0x8000))),
        (64, _mixed([1], p_dict=.3, small_bits=0, p_small=.5, clamp=(0, 0))),  # clamp span 2^32
        (1, _mixed([0, 1], p_dict=.9, p_delta=.99, fix=(1, 1))),
    ])
    chain = [(64, _mixed([0, top(64), rng.getrandbits(64)], p_dict=.5, p_delta=.5))]
    chain += [(64, _mixed([], p_dict=0., copy_prev=True, p_copy=.97, p_delta=.6))] * (CHAIN_LEN - 1)
    chain_case = Case("chain", chain)
    return [range_case, aligned_case, dict_case, mixed_case, chain_case]


def case(name):
    return next(c for c in cases() if c.name == name)


NAMES = ["range", "aligned", "dictfix", "mixed", "chain"]
