"""One-constraint programs over generator-controlled MIXED coordinates: the table shared by
``tests/test_asm_class_facts_sim.py`` (CPU simulator) and ``tests/test_gpu_asm_class_facts.py``.

The first tier emits a MIXED coordinate (``jit_asm.cpp: gen_value``) as one body per alternative
(COPY, dictionary, SMALL, UNIFORM) behind a cascade of threshold tests on the group's choice word,
each body followed by the delta and the clamp.  The cases cross what those bodies know about their
own values: dictionaries whose entries sit on both sides of a clamp window's ends (so the +/-1 and
+/-2 deltas borrow in some groups and not in others), a dictionary with a non-zero top limb, three
and one entry; the delta present and absent; the clamp present and absent, and one whose window
ends at 2^32; COPY of a live source, of a dead one that is generated again (``regen_*``: a MIXED
source named only by a root the specialiser decides, so no code reads it; it is generated into the
copier's registers), of one whose high limbs
are literals of a fix record, and a two-deep chain; widths 8, 32, 64 and 256; shares that leave
two, three and four alternatives, one with a zero-share middle alternative.  One case adds ALIGNED
and RANGE coordinates, whose bases and spans are the scalar literals the kernel keeps in SGPRs.

The constraint compares the coordinate with a literal (every limb is read): ``x < K`` with K just
above the dictionary's small entries.  Test infrastructure only."""
from mythril_amd.smt import terms as T
from tests import lazy_cases as LC

LO, SPAN = 0x44, 0x100
D_EDGE = [0, 1, 2, LO - 1, LO, LO + SPAN - 1, LO + SPAN]
D_TOP = [(1 << 255) | 5, 7, (1 << 224) + 9, LO + 1]
D3 = [3, LO + 12, LO + SPAN]
D1 = [LO + 12]
K = LO + 13  # the literal every case compares with

# Windows (64-candidate groups): aligned, and from an odd index (a partial first and last group)
ALIGNED, ODD = LC.ALIGNED, LC.ODD
SIM_COUNT, GPU_COUNT = 64 * 96, 4096
SEEDS = (1, 5)


def _mask(w):
    return (1 << w) - 1


class Case(LC.Case):
    def __init__(self, w, shape, source=None, live=False, extra=()):
        x = LC._v("cf_x", w)
        roots = []
        if source == "folded":  # named before x by a root the specialiser decides from the source's fix record
            s = LC._v("cf_s", w)  # (its top bits are zero): no code reads s, so the copier generates it
            roots.append(LC._ult(s, LC._k(1 << (w - 2), w)))
        elif source:  # named before x (coordinate order); ``live``: read again after x
            s = LC._v("cf_s", w)
            roots.append(T.or_(T.eq(s, LC._k(D3[1], w)), LC._coin("cf_pre")))
        roots.append(LC._ult(x, LC._k(K & _mask(w), w)))
        if source and live:
            roots.append(T.or_(LC._ult(LC._v("cf_s", w), LC._k(1 << (w - 1), w)), LC._coin("cf_post")))
        roots += list(extra)
        super().__init__(roots, shape, conds=[], regions=None)
        self.w = w


def _mixed(vals, w=256, **kw):
    vals = [v & _mask(w) for v in vals]
    return lambda g, ix: g.mixed(ix["cf_x"], vals, **kw)


def _clamp(w=256, span=SPAN):
    return (LO & _mask(w), span)


def _copy(src_shape, **kw):
    def shape(g, ix):
        assert ix["cf_s"] < ix["cf_x"]
        src_shape(g, ix["cf_s"])
        g.mixed(ix["cf_x"], D3, copy_from=ix["cf_s"], **kw)
    return shape


def _chain(g, ix):
    assert ix["cf_s0"] < ix["cf_s"] < ix["cf_x"]
    g.dict(ix["cf_s0"], D_EDGE)
    g.mixed(ix["cf_s"], D3, p_dict=0.2, copy_from=ix["cf_s0"], p_copy=0.5, p_delta=0.5)
    g.mixed(ix["cf_x"], D1, p_dict=0.2, copy_from=ix["cf_s"], p_copy=0.5, p_delta=0.5, clamp=_clamp())


def _scalars(g, ix):
    g.mixed(ix["cf_x"], D_EDGE, p_dict=0.45, p_delta=0.5, small_bits=20, p_small=0.2, clamp=_clamp())
    g.aligned(ix["cf_al"], (0x1234567 << 32) | 0xFFF00000, 5, 0x30000)
    g.aligned(ix["cf_al2"], (0x1234567 << 32) | 0xFFF00000, 5, 0x30000)
    g.range(ix["cf_rg"], 0x9000000000, 0x12345)


FULL = dict(p_dict=0.45, small_bits=20, p_small=0.2)
BUILDERS = {
    # dictionaries x delta x clamp
    "edge_delta_clamp": lambda: Case(256, _mixed(D_EDGE, p_delta=0.5, clamp=_clamp(), **FULL)),
    "edge_clamp": lambda: Case(256, _mixed(D_EDGE, clamp=_clamp(), **FULL)),
    "edge_delta": lambda: Case(256, _mixed(D_EDGE, p_delta=0.5, **FULL)),
    "edge_plain": lambda: Case(256, _mixed(D_EDGE, **FULL)),
    "edge_delta_clamp_2p32": lambda: Case(256, _mixed(D_EDGE, p_delta=0.5, clamp=_clamp(span=(1 << 32) - LO), **FULL)),
    "top_delta_clamp": lambda: Case(256, _mixed(D_TOP, p_delta=0.5, clamp=_clamp(), **FULL)),
    "three_delta_clamp": lambda: Case(256, _mixed(D3, p_delta=0.5, clamp=_clamp(), **FULL)),
    "one_delta_clamp": lambda: Case(256, _mixed(D1, p_delta=0.5, clamp=_clamp(), **FULL)),
    "one_plain": lambda: Case(256, _mixed(D1, **FULL)),
    # COPY
    "copy_live": lambda: Case(256, _copy(lambda g, c: g.dict(c, D_EDGE), p_dict=0.2, p_copy=0.4, p_delta=0.5,
                                         clamp=_clamp(), small_bits=20, p_small=0.2), source=True, live=True),
    "copy_dead": lambda: Case(256, _copy(lambda g, c: g.dict(c, D_EDGE), p_dict=0.2, p_copy=0.4, p_delta=0.5,
                                         clamp=_clamp(), small_bits=20, p_small=0.2), source=True),
    "copy_dead_mixed": lambda: Case(256, _copy(lambda g, c: g.mixed(c, D_EDGE, p_dict=0.5, small_bits=20, p_small=0.2,
                                                                  p_delta=0.5),
                                               p_dict=0.2, p_copy=0.4, p_delta=0.5, clamp=_clamp(), small_bits=20,
                                               p_small=0.2), source=True),
    # ... whose source is generated again, into the copier's registers: plain, with a fix record that sets
    # high limbs whole, clamped, and narrow
    "regen_mixed": lambda: Case(256, _copy(lambda g, c: (g.mixed(c, D_EDGE, p_dict=0.5, small_bits=20, p_small=0.2,
                                                                p_delta=0.5), g.fix(c, 3 << 254, 0)),
                                           p_dict=0.2, p_copy=0.4, p_delta=0.5, clamp=_clamp(), small_bits=20,
                                           p_small=0.2), source="folded"),
    "regen_fix": lambda: Case(256, _copy(lambda g, c: (g.mixed(c, D_EDGE, p_dict=0.5, small_bits=20, p_small=0.2),
                                                        g.fix(c, (_mask(64) << 192) | 0xF0, (0x1234 << 200) | 0x40)),  # (top limbs set whole)
                                         p_dict=0.2, p_copy=0.5, p_delta=0.5, small_bits=20, p_small=0.1), source="folded"),
    "regen_clamped": lambda: Case(256, _copy(lambda g, c: (g.mixed(c, D_EDGE, p_dict=0.5, small_bits=20, p_small=0.2,
                                                                  p_delta=0.5, clamp=_clamp()), g.fix(c, 3 << 254, 0)),
                                             p_dict=0.2, p_copy=0.5, small_bits=20, p_small=0.1), source="folded"),
    "regen_w8": lambda: Case(8, lambda g, ix: (g.mixed(ix["cf_s"], [v & 255 for v in D_EDGE], p_dict=0.5, small_bits=4,
                                                        p_small=0.2, p_delta=0.5), g.fix(ix["cf_s"], 0xC0, 0),
                                               g.mixed(ix["cf_x"], [3, LO + 12], copy_from=ix["cf_s"], p_dict=0.2,
                                                       p_copy=0.5, p_delta=0.5)), source="folded"),
    "copy_fix": lambda: Case(256, _copy(lambda g, c: (g.uniform(c), g.fix(c, _mask(256) ^ _mask(40), 0)),
                                        p_dict=0.2, p_copy=0.5, small_bits=20, p_small=0.1), source=True),
    # widths (odd limb counts, unpaired registers)
    "w8": lambda: Case(8, _mixed(D_EDGE, w=8, p_delta=0.5, clamp=(LO, 0x40), p_dict=0.45, small_bits=4, p_small=0.2)),
    "w32": lambda: Case(32, _mixed(D_EDGE, w=32, p_delta=0.5, clamp=_clamp(32), **FULL)),
    "w64": lambda: Case(64, _mixed(D_EDGE, w=64, p_delta=0.5, clamp=_clamp(64), **FULL)),
    # alternatives left by the shares: two, three, four, and a zero-share middle one
    "two_alts": lambda: Case(256, _mixed(D_EDGE, p_dict=0.5, p_delta=0.5, clamp=_clamp())),
    "three_alts_low": lambda: Case(256, _mixed(D_EDGE, p_dict=0.6, small_bits=20, p_small=0.1)),
    "three_alts_high": lambda: Case(256, _mixed(D_EDGE, p_dict=0.1, small_bits=20, p_small=0.2)),
    "four_alts": lambda: Case(256, _copy(lambda g, c: g.dict(c, D_EDGE), p_dict=0.45, p_copy=0.1, small_bits=20,
                                         p_small=0.2), source=True),
    "zero_middle": lambda: Case(256, _copy(lambda g, c: g.dict(c, D_EDGE), p_dict=0.0, p_copy=0.3, small_bits=20,
                                           p_small=0.3), source=True),
    # scalar literals: ALIGNED bases (one shared by two coordinates), a RANGE span, the clamp's bounds
    "scalars": lambda: Case(256, _scalars, extra=[
        T.or_(LC._ult(LC._v("cf_al"), LC._v("cf_al2")), LC._coin("cf_c1")),
        T.or_(LC._ult(LC._v("cf_rg"), LC._k(0x9000009000)), LC._coin("cf_c2"))]),
}


class _Chain(Case):
    """x copies s, s copies s0 (named in that order by the roots)."""

    def __init__(self):
        s0, s, x = LC._v("cf_s0"), LC._v("cf_s"), LC._v("cf_x")
        roots = [T.or_(T.eq(s0, LC._k(2)), LC._coin("cf_pre0")), T.or_(T.eq(s, LC._k(D3[1])), LC._coin("cf_pre")),
                 LC._ult(x, LC._k(K))]
        LC.Case.__init__(self, roots, _chain, conds=[], regions=None)
        self.w = 256


BUILDERS["copy_chain"] = _Chain
