"""The specialiser's case table shared by ``test_spec_fold_cpu.py`` and ``test_gpu_spec_fold.py``:
one small term per transfer function and decider of ``program.cpp``'s range / known-bits / value-set
analysis (``Analysis::coord_val``, ``analyze``, ``decide``, ``decide_eq``, ``decide_mem``), over a few
coordinates with chosen ``GenBuilder`` parameters (and, where ``GenBuilder`` cannot say it, a patch
of the raw blob words), ending in ONE compare:

* ``fires=True``: the generator's facts are meant to decide it, so a search runs a folded program;
* ``fires=False``: the boundary twin, one step past where the fact stops holding.  Its compare takes
  both values inside the windows the tests sweep.  ``show=False``: it cannot — either the compare
  is constant and the analysis does not see it (a note about precision), or the windows cannot
  reach the other value (an alternative of probability 2^-16).  The tests assert of every twin
  that nothing folded;
* ``fires="always"``: folded with or without a generator (``x op x``).

A program (``Prog``) holds one case (CPU) or one family of cases (GPU).  Its single root is
``xor(order bit, case compares...)``: the order bit is the parity of bit 0 of every coordinate, in
table order (which also fixes the coordinate order a COPY needs), and of the multiply probe of the
GEN3 edge table, ``Extract(31, 31, p * K)``, on one UNIFORM 32-bit coordinate ``p`` — MUL has no
transfer function, so no root is ever decided and every verdict mixes.  A correctly folded compare
is a constant of that parity; a wrong one flips it wherever the truth differs.
Test infrastructure only."""
from __future__ import annotations

import functools
import random

import numpy as np

from mythril_amd import search, ssa
from mythril_amd.smt import terms as T

WINDOW = 2048
_rng = random.Random(0x5BEC0F01D)
SEEDS = [1, 99, _rng.getrandbits(64)]
# from 0, and 63 bits with bit 31 of the low word set
STARTS = [0, _rng.getrandbits(63) | 0x80000001]

WIDTHS = [1, 8, 33, 64, 65, 128, 255, 256]  # where U256 changes word or limb

C = T.BitVecVal


def top(w):
    return (1 << w) - 1


def eq(a, b):
    return T.eq(a, b)


def ult(a, b):
    return T.bvcmp("bvult", a, b)


def ule(a, b):
    return T.bvcmp("bvule", a, b)


def slt(a, b):
    return T.bvcmp("bvslt", a, b)


def sle(a, b):
    return T.bvcmp("bvsle", a, b)


def ext(hi, lo, a):
    return T.extract(hi, lo, a)


def bop(op, a, b):
    return T.bvbin(op, a, b)


class Case:
    """``coords``: [(width, spec(gb, c, ix))] in coordinate order; ``term(xs)``: the compare over their
    symbols; ``sites``: specs of the UF sites the term creates, in SSA order; ``patch(blob, ix)``:
    raw words; ``witness(xs)``: the Bool that must take both values for a twin (default: the
    compare); ``lookup``: the fold shows as fewer LOOKUPs, not fewer compares."""

    def __init__(self, family, name, coords, term, fires, patch=None, sites=(), witness=None, show=True,
                 lookup=False):
        self.family, self.name, self.coords, self.term, self.fires = family, name, coords, term, fires
        self.patch, self.sites, self.witness, self.show, self.lookup = patch, sites, witness, show, lookup


# ---- generator specs -----------------------------------------------------------------------------


def uni():
    return lambda gb, c, ix: gb.uniform(c)


def fixed(v):
    return lambda gb, c, ix: gb.fixed(c, v)


def rng(lo, span):
    return lambda gb, c, ix: gb.range(c, lo, span)


def dic(*values):
    return lambda gb, c, ix: gb.dict(c, list(values))


def ali(lo, p1, count):
    return lambda gb, c, ix: gb.aligned(c, lo, p1, count)


def mix(values, copy_prev=False, **kw):
    def spec(gb, c, ix):
        gb.mixed(c, list(values), copy_from=ix[ix.index(c) - 1] if copy_prev else None, **kw)
    return spec


def fix(spec, mask, val):
    def f(gb, c, ix):
        spec(gb, c, ix)
        gb.fix(c, mask, val)
    return f


def const_word(blob, off):
    """Index in the blob of word ``off`` of the generator's constants."""
    return 4 + 8 * int(blob[1]) + off


def spec_word(c, k):
    return 4 + 8 * c + k


# ---- the table -----------------------------------------------------------------------------------

CASES = []


def case(family, name, coords, term, fires, **kw):
    assert all(c.name != name for c in CASES), name
    CASES.append(Case(family, name, coords, term, fires, **kw))


def _coord_val_cases():
    F = "coord"
    r = random.Random(0xC0)
    for w in WIDTHS:
        v = r.getrandbits(w) | 1
        case(F, f"fixed_w{w}", [(w, fixed(v))], lambda x, v=v, w=w: eq(x[0], C(v, w)), True)
    d16 = sorted(r.getrandbits(64) for _ in range(16))
    d17 = sorted(r.getrandbits(64) for _ in range(17))
    case(F, "dict16_nonmember", [(64, dic(*d16))], lambda x: eq(x[0], C(d16[3] + 1, 64)), True)
    case(F, "dict17_member", [(64, dic(*d17))], lambda x: eq(x[0], C(d17[3], 64)), False)
    case(F, "dict17_nonmember", [(64, dic(*d17))], lambda x: eq(x[0], C(d17[3] + 1, 64)), False, show=False)
    case(F, "dict17_outside_hull", [(64, dic(*d17))], lambda x: ult(x[0], C(d17[0], 64)), True)
    for w in WIDTHS[1:]:
        span = 100 if w > 8 else 10
        lo = (1 << w) - span
        case(F, f"range_top_w{w}", [(w, rng(lo, span))], lambda x, lo=lo, w=w: ult(x[0], C(lo, w)), True)
        case(F, f"range_wraps_w{w}", [(w, rng(lo + 1, span))], lambda x, lo=lo, w=w: ult(x[0], C(lo + 1, w)), False)
    case(F, "range_w1", [(1, rng(1, 1))], lambda x: eq(x[0], C(1, 1)), True)
    case(F, "range_span0", [(64, rng(7, 0))], lambda x: ule(x[0], C(7 + top(32), 64)), True)
    case(F, "range_span0_half", [(64, rng(7, 0))], lambda x: ult(x[0], C(7 + (1 << 31), 64)), False)
    case(F, "range_span0_top_w33", [(33, rng(1 << 32, 0))], lambda x: ule(C(1 << 32, 33), x[0]), True)
    case(F, "aligned_shift_at_w", [(8, ali(0x35, 8, 3))], lambda x: eq(x[0], C(0x35, 8)), True)
    case(F, "aligned_shift_past_w33", [(33, ali(0x1234, 40, 0))], lambda x: eq(x[0], C(0x1234, 33)), True)
    case(F, "aligned_wraps_low_bits", [(8, ali(0xF5, 4, 4))], lambda x: eq(ext(3, 0, x[0]), C(5, 4)), True)
    case(F, "aligned_wraps_range", [(8, ali(0xF5, 4, 4))], lambda x: ult(x[0], C(0xF5, 8)), False)
    atop = 0x1000 + (15 << 12)
    case(F, "aligned_top", [(64, ali(0x1000, 12, 16))], lambda x: ule(x[0], C(atop, 64)), True)
    case(F, "aligned_below_top", [(64, ali(0x1000, 12, 16))], lambda x: ult(x[0], C(atop, 64)), False)
    # (cnt - 1) << p1 = 128 << 250 loses every bit: m = 0, 64 and 128 all give 3
    case(F, "aligned_step_loses_bits_low", [(256, ali(3, 250, 129))], lambda x: eq(ext(249, 0, x[0]), C(3, 250)), True)
    case(F, "aligned_step_loses_bits", [(256, ali(3, 250, 129))], lambda x: eq(x[0], C(3, 256)), False)
    clamp = dict(p_dict=.5, p_delta=.9, clamp=(1000, 50))
    case(F, "mixed_clamp", [(64, mix([0, top(64), 5], **clamp))], lambda x: ult(x[0], C(1050, 64)), True)
    case(F, "mixed_clamp_inside", [(64, mix([0, top(64), 5], **clamp))], lambda x: ult(x[0], C(1049, 64)), False)
    # COPY + DICT: probabilities that sum to 65536 leave no UNIFORM alternative; 65535 leaves one
    src = (64, rng(100, 101))
    case(F, "mixed_sum_65536", [src, (64, mix([100, 200], copy_prev=True, p_copy=.5, p_dict=.5))],
         lambda x: ule(x[1], C(200, 64)), True)
    case(F, "mixed_sum_65535", [src, (64, mix([100, 200], copy_prev=True, p_copy=.5, p_dict=32767 / 65536))],
         lambda x: ule(x[1], C(200, 64)), False, show=False)
    case(F, "mixed_sum_49152", [src, (64, mix([100, 200], copy_prev=True, p_copy=.5, p_dict=.25))],
         lambda x: ule(x[1], C(200, 64)), False)
    # the +/-2 delta: no wrap below needs 2 <= cd.lo, none above cd.hi + 2 <= 2^w - 1
    dl = dict(copy_prev=True, p_copy=.5, p_dict=.5, p_delta=.9)
    case(F, "mixed_delta_lo2", [(64, dic(2, 50)), (64, mix([2, 50], **dl))], lambda x: ule(x[1], C(52, 64)), True)
    case(F, "mixed_delta_lo1", [(64, dic(1, 50)), (64, mix([1, 50], **dl))], lambda x: ule(x[1], C(52, 64)), False)
    for w in (8, 256):
        case(F, f"mixed_delta_hi_top_w{w}", [(w, dic(10, top(w) - 2)), (w, mix([10, top(w) - 2], **dl))],
             lambda x, w=w: ule(C(8, w), x[1]), True)
        case(F, f"mixed_delta_hi_wraps_w{w}", [(w, dic(10, top(w) - 1)), (w, mix([10, top(w) - 1], **dl))],
             lambda x, w=w: ule(C(8, w), x[1]), False)
    case(F, "mixed_small_below_w", [(33, mix([3], p_dict=.5, small_bits=8, p_small=.5))],
         lambda x: ult(x[0], C(256, 33)), True)
    case(F, "mixed_small_above_w", [(33, mix([3], p_dict=.5, small_bits=40, p_small=.5))],
         lambda x: ult(x[0], C(256, 33)), False)
    case(F, "mixed_narrow", [(16, mix([7], p_dict=.5, small_bits=3, p_small=.5))], lambda x: ule(x[0], C(7, 16)), True)
    case(F, "mixed_narrow_wider", [(16, mix([7], p_dict=.5, small_bits=4, p_small=.5))],
         lambda x: ule(x[0], C(7, 16)), False)
    # a COPY of a source with fixed bits: the source is in [0x1A0, 0x1AF]
    fsrc = (64, fix(rng(0x100, 0x100), 0xF0, 0xA0))
    cp = mix([0x1A5], copy_prev=True, p_copy=.5, p_dict=.5)
    case(F, "copy_of_fixed_bits", [fsrc, (64, cp)], lambda x: ult(x[1], C(0x1B0, 64)), True)
    case(F, "copy_of_fixed_bits_inside", [fsrc, (64, cp)], lambda x: ult(x[1], C(0x1AF, 64)), False)
    # a fix record on every kind: bits 8..15 are 0x5A
    kinds = {"uniform": uni(), "range": rng(1 << 40, 1000), "dict": dic(1 << 40, 77, 0xFFFF), "aligned": ali(5, 3, 0),
             "fixed": fixed(0xFFFFFF), "mixed": mix([1 << 50, 3], p_dict=.3, p_delta=.9, small_bits=20, p_small=.3)}
    for k, sp in kinds.items():
        case(F, f"fix_on_{k}", [(64, fix(sp, 0xFF00, 0x5A00))], lambda x: eq(ext(15, 8, x[0]), C(0x5A, 8)), True)
    case(F, "fix_on_uniform_past_mask", [(64, fix(uni(), 0xFF00, 0x5A00))],
         lambda x: eq(ext(16, 9, x[0]), C(0x2D | 0x80, 8)), False)
    case(F, "fix_maps_set", [(8, fix(dic(0x10, 0x20, 0x30), 0x0F, 0x03))],
         lambda x: T.or_(eq(x[0], C(0x13, 8)), eq(x[0], C(0x23, 8)), eq(x[0], C(0x33, 8))), True)

    # raw blobs the loader accepts and GenBuilder never writes: constants with bits outside the width
    # or the mask (include/mythgpu.h: entries are masked to w; a fix record is (v & ~mask) | value)
    def dict_entry(e, v):
        def patch(blob, ix):
            blob[const_word(blob, int(blob[spec_word(ix[0], 1)]) + e)] = v
        return patch

    case(F, "raw_dict_entry_above_w", [(8, dic(5, 0xFF))], lambda x: eq(x[0], C(0xFF, 8)), False,
         patch=dict_entry(1, 0x1FF))

    def fix_value(v):
        def patch(blob, ix):
            off = (int(blob[spec_word(ix[0], 0)]) >> 8) - 1
            blob[const_word(blob, off + 1)] = v  # L = 1: {mask, value}
        return patch

    case(F, "raw_fix_value_outside_mask", [(8, fix(fixed(0), 0x01, 0x01))], lambda x: ult(C(0x7F, 8), x[0]), True,
         patch=fix_value(0x81))
    case(F, "raw_fixed_above_w", [(8, fixed(0xFF))], lambda x: eq(x[0], C(0xFF, 8)), True, patch=dict_entry(0, 0x1FF))

    def mixed_entries(blob, ix):
        off = int(blob[spec_word(ix[1], 1)])
        blob[const_word(blob, off)] = 0x1F0
        blob[const_word(blob, off + 1)] = 0x1F8

    case(F, "raw_mixed_entries_above_w", [(8, dic(0xF4)), (8, mix([0xF0, 0xF8], copy_prev=True, p_copy=.5, p_dict=.5))],
         lambda x: ule(C(0xF0, 8), x[1]), True, patch=mixed_entries)
    case(F, "raw_mixed_entries_above_w_inside", [(8, dic(0xF4)), (8, mix([0xF0, 0xF8], copy_prev=True, p_copy=.5, p_dict=.5))],
         lambda x: ule(C(0xF4, 8), x[1]), False, patch=mixed_entries)

    # a fix record over several limbs whose value has a bit in a limb where the mask has none: mask
    # bit 0, value bits 0 and w - 1, on every kind (the compiled generators once skipped such limbs)
    def fix_record(w, mask, value):
        def patch(blob, ix):
            off = (int(blob[spec_word(ix[0], 0)]) >> 8) - 1
            L = ssa.limbs(w)
            for j, v in enumerate(ssa.int_to_limbs(mask, w) + ssa.int_to_limbs(value, w)):
                blob[const_word(blob, off + j)] = v
            assert len(ssa.int_to_limbs(mask, w)) == L
        return patch

    low = {"uniform": uni(), "range": rng(10, 11), "dict": dic(1, 6, 9), "aligned": ali(5, 4, 100), "fixed": fixed(2),
           "mixed": mix([3, 5], p_dict=.5, p_delta=.9, small_bits=8, p_small=.3)}
    for w in (33, 64, 65, 256):
        tb = 1 << (w - 1)
        for k, sp in low.items():
            case(F, f"raw_fix_value_other_limb_{k}_w{w}", [(w, fix(sp, 1, 1))], lambda x, w=w, tb=tb: ule(C(tb, w), x[0]),
                 True, patch=fix_record(w, 1, 1 | tb))
        case(F, f"raw_fix_value_other_limb_below_w{w}", [(w, fix(uni(), 1, 1))],
             lambda x, w=w, tb=tb: ule(C(tb | tb >> 1, w), x[0]), False, patch=fix_record(w, 1, 1 | tb))

    # a three-limb dictionary whose second entry has bits above w = 65 (read as 7 + 2^64), against a
    # literal and as a membership; its low limbs are dictionary limbs of the first tier, the top one
    # is masked anew
    def entry_limb(e, L, j, v):
        def patch(blob, ix):
            blob[const_word(blob, int(blob[spec_word(ix[0], 1)]) + e * L + j)] = v
        return patch

    e1 = 7 | 1 << 64
    case(F, "raw_dict_entry_above_w65", [(65, dic(5, e1))], lambda x: eq(x[0], C(e1, 65)), False, patch=entry_limb(1, 3, 2, 7))
    case(F, "raw_dict_entry_above_w65_members", [(65, dic(5, e1))],
         lambda x: T.or_(eq(x[0], C(5, 65)), eq(C(e1, 65), x[0])), True, patch=entry_limb(1, 3, 2, 7))
    case(F, "raw_dict_entry_above_w65_limb", [(65, dic(5, e1))], lambda x: eq(ext(31, 0, x[0]), C(7, 32)), False,
         patch=entry_limb(1, 3, 2, 7))


def _operator_cases():
    F = "ops"
    case(F, "zext", [(8, rng(10, 11))], lambda x: ult(T.zero_extend(56, x[0]), C(21, 64)), True)
    case(F, "zext_inside", [(8, rng(10, 11))], lambda x: ult(T.zero_extend(56, x[0]), C(20, 64)), False)
    for wa, W in ((8, 16), (33, 65), (64, 128), (128, 256), (255, 256)):
        neg = (1 << (wa - 1)) + (1 << (wa - 4))  # 16 values from here share every bit above bit 3
        bound = C(top(W) - top(wa - 1), W)     # the least sign-extended negative value
        case(F, f"sext_sign0_w{wa}", [(wa, rng(10, 11))],
             lambda x, wa=wa, W=W: ult(T.sign_extend(W - wa, x[0]), C(21, W)), True)
        case(F, f"sext_sign1_w{wa}", [(wa, rng(neg, 16))],
             lambda x, wa=wa, W=W, b=bound: ule(b, T.sign_extend(W - wa, x[0])), True)
        case(F, f"sext_sign_unknown_w{wa}", [(wa, rng((1 << (wa - 1)) - 8, 16))],
             lambda x, wa=wa, W=W, b=bound: ule(b, T.sign_extend(W - wa, x[0])), False)
    case(F, "sext_w1", [(1, fixed(1))], lambda x: eq(T.sign_extend(7, x[0]), C(0xFF, 8)), True)
    for p in (63, 64, 65, 127, 128):
        case(F, f"extract_lo{p}", [(256, rng(5 << p, 0))], lambda x, p=p: eq(ext(p + 7, p, x[0]), C(5, 8)), True)
        case(F, f"extract_lo{p}_straddles", [(256, rng((5 << p) - 1, 2))], lambda x, p=p: eq(ext(p + 7, p, x[0]), C(5, 8)), False)
    case(F, "extract_lo255", [(256, rng(1 << 255, 0))], lambda x: eq(ext(255, 255, x[0]), C(1, 1)), True)
    # [0x0FF0, 0x1010] >> 0 does not fit 8 bits: the low byte runs 0xF0..0xFF, 0x00..0x10
    case(F, "extract_no_fit", [(64, rng(0x0FF0, 0x21))], lambda x: ult(ext(7, 0, x[0]), C(0x11, 8)), False)
    # [0x3000, 0x40FF] >> 8 fits 12 bits; the known bits alone only give [0, 0x7F]
    case(F, "extract_fits", [(64, rng(0x3000, 0x1100))], lambda x: ult(ext(19, 8, x[0]), C(0x41, 12)), True)
    case(F, "extract_fits_inside", [(64, rng(0x3000, 0x1100))], lambda x: ult(ext(19, 8, x[0]), C(0x40, 12)), False)
    case(F, "extract_set", [(64, dic(0x0100, 0x0600))], lambda x: eq(ext(15, 8, x[0]), C(3, 8)), True)
    case(F, "extract_set_member", [(64, dic(0x0100, 0x0600))], lambda x: eq(ext(15, 8, x[0]), C(6, 8)), False)
    cc = [(8, rng(3, 3)), (8, rng(10, 11))]
    case(F, "concat_range", cc, lambda x: ule(T.concat(x[0], x[1]), C(0x0514, 16)), True)
    case(F, "concat_range_inside", cc, lambda x: ult(T.concat(x[0], x[1]), C(0x0514, 16)), False)
    ck = [(64, uni()), (64, ali(5, 4, 0))]
    case(F, "concat_bits", ck, lambda x: eq(ext(3, 0, T.concat(x[0], x[1])), C(5, 4)), True)
    case(F, "concat_bits_past", ck, lambda x: eq(ext(4, 1, T.concat(x[0], x[1])), C(2, 4)), False)
    case(F, "concat_bits_high", [(64, ali(5, 4, 0)), (64, uni())],
         lambda x: eq(ext(67, 64, T.concat(x[0], x[1])), C(5, 4)), True)
    s4a, s4b = dic(1, 6, 9, 12), dic(2, 5, 8, 15)
    case(F, "concat_set_16", [(8, s4a), (8, s4b)], lambda x: eq(T.concat(x[0], x[1]), C(0x0603, 16)), True)
    case(F, "concat_set_16_member", [(8, s4a), (8, s4b)], lambda x: eq(T.concat(x[0], x[1]), C(0x0605, 16)), False)
    s3, s6 = dic(1, 6, 9), dic(2, 5, 8, 15, 20, 33)
    case(F, "concat_set_18", [(8, s3), (8, s6)], lambda x: eq(T.concat(x[0], x[1]), C(0x0603, 16)), False, show=False)
    case(F, "concat_set_18_member", [(8, s3), (8, s6)], lambda x: eq(T.concat(x[0], x[1]), C(0x0605, 16)), False)
    al = (64, ali(5, 4, 100))
    for name, f, want in (("and", lambda a: bop("bvand", a, C(0xFFFF, 64)), 5), ("or", lambda a: bop("bvor", a, C(3, 64)), 7),
                          ("xor", lambda a: bop("bvxor", a, C(0xF, 64)), 0xA), ("not", lambda a: T.bvun("bvnot", a), 0xA)):
        case(F, f"{name}_bits", [al], lambda x, f=f, v=want: eq(ext(3, 0, f(x[0])), C(v, 4)), True)
        case(F, f"{name}_bits_past", [al], lambda x, f=f, v=want: eq(ext(4, 1, f(x[0])), C(v >> 1, 4)), False)
    case(F, "and_unknown_operand", [al, (64, uni())], lambda x: eq(ext(3, 0, bop("bvand", x[0], x[1])), C(5, 4)), False)
    sa, sb = (8, dic(1, 6)), (8, dic(0x10, 0x60))
    case(F, "or_set", [sa, sb], lambda x: eq(bop("bvor", x[0], x[1]), C(0x31, 8)), True)
    case(F, "or_set_member", [sa, sb], lambda x: eq(bop("bvor", x[0], x[1]), C(0x61, 8)), False)
    case(F, "xor_set", [sa, sb], lambda x: eq(bop("bvxor", x[0], x[1]), C(0x31, 8)), True)
    case(F, "xor_set_member", [sa, sb], lambda x: eq(bop("bvxor", x[0], x[1]), C(0x16, 8)), False)
    ta, tb = (8, dic(0x0F, 0x33)), (8, dic(0x3C, 0x55))  # and: 0x0C, 0x05, 0x30, 0x11
    case(F, "and_set", [ta, tb], lambda x: eq(bop("bvand", x[0], x[1]), C(0x10, 8)), True)
    case(F, "and_set_member", [ta, tb], lambda x: eq(bop("bvand", x[0], x[1]), C(0x11, 8)), False)
    case(F, "not_set", [sa], lambda x: eq(T.bvun("bvnot", x[0]), C(0xFB, 8)), True)
    case(F, "not_set_member", [sa], lambda x: eq(T.bvun("bvnot", x[0]), C(0xF9, 8)), False)
    it = [(32, uni()), (64, rng(10, 11)), (64, rng(30, 11))]
    ite = lambda x: T.ite(ult(x[0], C(1 << 31, 32)), x[1], x[2])  # noqa: E731
    case(F, "ite_hull", it, lambda x: ule(ite(x), C(40, 64)), True)
    case(F, "ite_hull_inside", it, lambda x: ult(ite(x), C(40, 64)), False)
    case(F, "ite_hull_gap", it, lambda x: eq(ite(x), C(25, 64)), False, show=False)  # inside the hull: not decided
    for W in (8, 256):
        a = (W, rng(top(W) - 5, 3))
        case(F, f"add_hi_top_w{W}", [a, (W, rng(1, 3))], lambda x, W=W: ule(C(top(W) - 4, W), bop("bvadd", x[0], x[1])), True)
        case(F, f"add_hi_wraps_w{W}", [a, (W, rng(1, 4))], lambda x, W=W: ule(C(top(W) - 4, W), bop("bvadd", x[0], x[1])), False)
    a5, a6 = (64, ali(5, 4, 100)), (64, ali(6, 4, 100))
    case(F, "add_trailing_bits", [a5, a6], lambda x: eq(ext(3, 0, bop("bvadd", x[0], x[1])), C(0xB, 4)), True)
    case(F, "add_trailing_bits_past", [a5, a6], lambda x: eq(ext(4, 1, bop("bvadd", x[0], x[1])), C(5, 4)), False)
    case(F, "sub_trailing_bits", [a5, a6], lambda x: eq(ext(3, 0, bop("bvsub", x[0], x[1])), C(0xF, 4)), True)
    case(F, "sub_trailing_bits_past", [a5, a6], lambda x: eq(ext(4, 1, bop("bvsub", x[0], x[1])), C(7, 4)), False)
    case(F, "add_set", [(8, dic(1, 6)), (8, dic(10, 20))], lambda x: eq(bop("bvadd", x[0], x[1]), C(15, 8)), True)
    case(F, "add_set_member", [(8, dic(1, 6)), (8, dic(10, 20))], lambda x: eq(bop("bvadd", x[0], x[1]), C(16, 8)), False)
    case(F, "sub_set", [(8, dic(10, 20)), (8, dic(1, 6))], lambda x: eq(bop("bvsub", x[0], x[1]), C(10, 8)), True)
    case(F, "sub_set_member", [(8, dic(10, 20)), (8, dic(1, 6))], lambda x: eq(bop("bvsub", x[0], x[1]), C(9, 8)), False)
    for W in (8, 256):
        case(F, f"sub_no_borrow_w{W}", [(W, rng(50, 11)), (W, rng(40, 11))],
             lambda x, W=W: ule(bop("bvsub", x[0], x[1]), C(20, W)), True)
        case(F, f"sub_borrows_w{W}", [(W, rng(50, 11)), (W, rng(40, 12))],
             lambda x, W=W: ule(bop("bvsub", x[0], x[1]), C(20, W)), False)


def _decider_cases():
    F = "dec"
    for w in (8, 65, 256):
        b = 1 << (w - 2)
        A, B0, B1 = (w, rng(b + 10, 11)), (w, rng(b + 20, 11)), (w, rng(b + 21, 10))  # [10,20] [20,30] [21,30]
        case(F, f"eq_range_gap_w{w}", [A, B1], lambda x: eq(x[0], x[1]), True)
        case(F, f"eq_range_touch_w{w}", [A, B0], lambda x: eq(x[0], x[1]), False)
        case(F, f"ule_touch_w{w}", [A, B0], lambda x: ule(x[0], x[1]), True)
        case(F, f"ult_touch_w{w}", [A, B0], lambda x: ult(x[0], x[1]), False)
        case(F, f"ult_gap_w{w}", [A, B1], lambda x: ult(x[0], x[1]), True)
        case(F, f"ult_rev_touch_w{w}", [A, B0], lambda x: ult(x[1], x[0]), True)
        case(F, f"ule_rev_touch_w{w}", [A, B0], lambda x: ule(x[1], x[0]), False)
        case(F, f"ule_rev_gap_w{w}", [A, B1], lambda x: ule(x[1], x[0]), True)
    for w in (8, 64, 65, 256):
        s = 1 << (w - 1)
        lo, pos, neg = (w, rng(10, 11)), (w, rng(s - 28, 28)), (w, rng(s - 28, 29))  # up to s - 1; up to s
        case(F, f"slt_sign_outside_w{w}", [lo, pos], lambda x: slt(x[0], x[1]), True)
        case(F, f"slt_sign_inside_w{w}", [lo, neg], lambda x: slt(x[0], x[1]), False)
        case(F, f"sle_sign_outside_w{w}", [lo, pos], lambda x: sle(x[1], x[0]), True)
        case(F, f"sle_sign_inside_w{w}", [lo, neg], lambda x: sle(x[1], x[0]), False)
    a5, a6 = (64, ali(5, 4, 4)), (64, ali(6, 4, 4))
    case(F, "eq_bit_conflict", [a5, a6], lambda x: eq(x[0], x[1]), True)
    case(F, "eq_bits_agree", [a5, a5], lambda x: eq(x[0], x[1]), False)
    case(F, "eq_sets_disjoint", [(8, dic(1, 6)), (8, dic(3, 4))], lambda x: eq(x[0], x[1]), True)
    case(F, "eq_sets_meet", [(8, dic(1, 6)), (8, dic(3, 6))], lambda x: eq(x[0], x[1]), False)
    for name, f in (("eq", eq), ("ult", ult), ("ule", ule), ("slt", slt), ("sle", sle)):
        case(F, f"same_operand_{name}", [(65, uni())], lambda x, f=f: f(x[0], x[0]), "always")
    m = [(64, dic(1, 6, 9))]
    is_ = lambda x, *vs: [eq(x[0], C(v, 64)) for v in vs]  # noqa: E731
    case(F, "mem_or_inside", m, lambda x: T.or_(*is_(x, 1, 6, 9)), True)
    case(F, "mem_or_outside", m, lambda x: T.or_(*is_(x, 2, 3)), True)
    case(F, "mem_or_straddles", m, lambda x: T.or_(*is_(x, 1, 6)), False)
    case(F, "mem_and_not_inside", m, lambda x: T.and_(*[T.not_(e) for e in is_(x, 1, 6, 9)]), True)
    case(F, "mem_not_or_inside", m, lambda x: T.not_(T.or_(*is_(x, 1, 6, 9))), True)
    case(F, "mem_and_not_straddles", m, lambda x: T.and_(*[T.not_(e) for e in is_(x, 1, 6)]), False)
    case(F, "mem_and_of_ors_empty", m, lambda x: T.and_(T.or_(*is_(x, 1, 6)), T.or_(*is_(x, 9, 2))), True)
    case(F, "mem_and_of_ors_one", m, lambda x: T.and_(T.or_(*is_(x, 1, 6)), T.or_(*is_(x, 6, 9))), False)
    case(F, "mem_or_of_nots", m, lambda x: T.or_(T.not_(is_(x, 1)[0]), T.not_(is_(x, 6)[0])), True)
    case(F, "mem_swapped_literal", m, lambda x: T.or_(eq(C(1, 64), x[0]), eq(x[0], C(6, 64)), eq(C(9, 64), x[0])), True)
    # LASER's ULE / SLE, Or(a < b, a == b), with the EQ's operands swapped: rewritten to one compare
    ab = [(64, rng(10, 11)), (64, rng(15, 11))]
    case(F, "or_ult_eq", ab, lambda x: T.or_(ult(x[0], x[1]), eq(x[1], x[0])), False)
    case(F, "or_eq_slt", ab, lambda x: T.or_(eq(x[1], x[0]), slt(x[0], x[1])), False)
    case(F, "or_ult_eq_decided", [(64, rng(10, 11)), (64, rng(20, 11))],
         lambda x: T.or_(ult(x[0], x[1]), eq(x[1], x[0])), False, show=False)
    # 512-bit keys, Concat(key, slot) with a literal slot
    key = lambda a, slot: T.concat(a, C(slot, 256))  # noqa: E731
    b = 1 << 200
    case(F, "key512_heads_apart", [(256, rng(b + 10, 11)), (256, rng(b + 21, 10))],
         lambda x: eq(key(x[0], 3), key(x[1], 3)), True)
    case(F, "key512_heads_touch", [(256, rng(b + 10, 11)), (256, rng(b + 20, 11))],
         lambda x: eq(key(x[0], 3), key(x[1], 3)), False)
    case(F, "key512_tails_differ", [(256, rng(b + 10, 11)), (256, rng(b + 20, 11))],
         lambda x: eq(key(x[0], 3), key(x[1], 4)), "always")  # literal tails: no generator needed
    case(F, "key512_equal", [(256, fixed(b + 7)), (256, fixed(b + 7))], lambda x: eq(key(x[0], 3), key(x[1], 3)), True)
    case(F, "key512_symbolic_tails", [(256, fixed(b + 7)), (256, fixed(b + 7)), (256, dic(1, 6)), (256, dic(3, 6))],
         lambda x: eq(T.concat(x[0], x[2]), T.concat(x[1], x[3])), False)
    case(F, "key512_symbolic_tails_apart", [(256, fixed(b + 7)), (256, fixed(b + 7)), (256, dic(1, 6)), (256, dic(3, 4))],
         lambda x: eq(T.concat(x[0], x[2]), T.concat(x[1], x[3])), True)


def _lookup_cases():
    """f(k2) reads f(k1)'s value where the keys are equal (a LOOKUP over the earlier sites).  The
    site values are one of two bytes, so ``f(k1) == f(k2)`` mixes where the keys differ."""
    F = "lookup"
    bit = dic(0, 1)

    def f(name):
        return T.FuncDecl("sf_" + name, 64, 8)

    def two(name):
        return lambda x: eq(f(name)(x[0]), f(name)(x[1]))

    case(F, "prior_never_equal", [(64, rng(10, 11)), (64, rng(21, 10))], two("never"), True, sites=[bit, bit], lookup=True)
    case(F, "prior_may_equal", [(64, rng(10, 11)), (64, rng(20, 11))], two("may"), False, sites=[bit, bit], lookup=True,
         witness=lambda x: eq(x[0], x[1]))
    case(F, "prior_always_equal", [(64, fixed(7)), (64, fixed(7))], two("always"), True, sites=[bit, bit])

    def sites3(g, x, last):  # the sites in the order k1, k2, k3 (the first two compares fold always)
        return T.and_(eq(g(x[0]), g(x[0])), eq(g(x[1]), g(x[1])), last)

    def three(x):  # k3's priors: k1 decided unequal (dropped), k2 always equal (the default)
        g = f("three")
        return sites3(g, x, eq(g(x[1]), g(x[2])))

    case(F, "prior_dropped_then_default", [(64, rng(10, 11)), (64, fixed(30)), (64, fixed(30))], three, True,
         sites=[bit, bit, bit])

    def three_twin(x):  # k3 may equal k1 (kept); otherwise it is k2's: f(k1) == f(k3) where k1 is 15
        g = f("twin")
        return sites3(g, x, eq(g(x[0]), g(x[2])))

    case(F, "prior_kept_then_default", [(64, rng(10, 11)), (64, fixed(15)), (64, fixed(15))], three_twin, False,
         sites=[bit, bit, bit])


_coord_val_cases()
_operator_cases()
_decider_cases()
_lookup_cases()
FAMILIES = ["coord", "ops", "dec", "lookup"]
NAMES = [c.name for c in CASES]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def family(name):
    return [c for c in CASES if c.family == name]


# ---- programs ------------------------------------------------------------------------------------


class Prog:
    """One program over ``cases``: flattened once; ``blob`` its generator; ``cmp_nodes`` the node of
    each case's compare and ``wit_nodes`` of its witness, for the C port's watch rows."""

    def __init__(self, name, cases):
        self.name, self.cases = name, list(cases)
        K = random.Random("spec-fold-" + name).getrandbits(32) | 1
        p = T.BitVecVar(f"s_{name}__probe", 32)
        order = None
        syms, cmps, wits = [], [], []
        for cs in self.cases:
            xs = [T.BitVecVar(f"s_{cs.name}_{q:02d}", w) for q, (w, _) in enumerate(cs.coords)]
            syms.append(xs)
            for x in xs:
                order = ext(0, 0, x) if order is None else bop("bvxor", order, ext(0, 0, x))
        order = bop("bvxor", order, ext(31, 31, bop("bvmul", p, C(K, 32))))  # the probe is the last scalar
        root = eq(order, C(1, 1))
        for cs, xs in zip(self.cases, syms):
            cmps.append(cs.term(xs))
            wits.append(cs.witness(xs) if cs.witness else cmps[-1])
            root = T.xor_(root, cmps[-1])
        self.P = P = ssa.flatten([root], extra=wits)
        self.cmp_nodes = [P.term_node[t.id] for t in cmps]
        self.wit_nodes = [P.term_node[t.id] for t in wits]
        by = {c.name: c.index for c in P.coords if c.kind == ssa.COORD_SCALAR}
        gb = search.GenBuilder(P)
        gb.uniform(by[f"s_{name}__probe"])
        self.index = []
        sites = iter(P.sites)
        used = set()
        for cs, xs in zip(self.cases, syms):
            ix = [by[x.params[0]] for x in xs]
            assert ix == sorted(ix), (cs.name, ix)
            self.index.append(ix)
            for c, (w, spec) in zip(ix, cs.coords):
                assert P.coords[c].width == w
                spec(gb, c, ix)
                used.add(c)
        # UF sites, in SSA order: every case's sites are its own function's
        for cs in self.cases:
            for spec in cs.sites:
                c = next(sites).index
                spec(gb, c, [c])
                used.add(c)
        assert next(sites, None) is None and len(used) + 1 == len(P.coords), (name, len(used), len(P.coords))
        blob = gb.blob()
        for cs, ix in zip(self.cases, self.index):
            if cs.patch:
                cs.patch(blob, ix)
        self.blob = blob
        self.prog = P.to_bytes()
        self.widths = [c.width for c in P.coords]

    def watched(self, nodes):
        """The program's bytes with ``nodes`` watched (the C port's ``bv_eval_watch``)."""
        self.P.set_watch(nodes)
        try:
            return bytes(self.P.to_bytes())
        finally:
            self.P.set_watch([])


@functools.lru_cache(maxsize=None)
def single(name):
    return Prog(name, [by_name(name)])


@functools.lru_cache(maxsize=None)
def group(fam):
    return Prog("family_" + fam, family(fam))


def bits_of(watch: np.ndarray) -> np.ndarray:
    """Watch rows of 1-bit nodes as uint8 [rows][n]."""
    return (watch & 1).astype(np.uint8)
