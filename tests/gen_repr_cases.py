"""How a generated coordinate is held, crossed with the operators that read it: the case table and
the fuzz builder shared by ``tests/test_gen_repr_cpu.py`` and ``tests/test_gpu_gen_repr.py``.

Each compiled tier picks a representation for a generated coordinate from its generator kind and
size.  The first tier (``jit_asm.cpp: dict()``, ``plan_lds``): a dictionary of width ``w < 32`` with
``n * w <= 32`` is one literal read with a bit-field extract; one entry is that entry's literals; two
or more entries are staged in LDS (pair reads, or b32 reads under MYTHGPU_JIT_ASM_LDS_B32) unless
the table does not fit or MYTHGPU_JIT_ASM_NO_LDS is set, and then up to 4 entries are a
``v_cndmask`` chain and more a global gather; limbs equal in every entry are literals in each form.
The O3 tier (``jit.cpp: packed_dict``, ``select_dict_max``, ``plan_dict_lds``): ``w <= 32`` and
``n * w <= 64`` is a 64-bit literal, up to 4 entries are selects, more are gathers, or LDS reads
once three coordinates of a program gather.  FIXED coordinates, a RANGE of span 1, an ALIGNED of
count 1 and a fix record over every bit are literals.  ``shapes()`` puts a coordinate on each side of
each of those thresholds; the programs (``program_names()``) have every shaped coordinate read by
every consumer of ``FAMILIES``, a root per (shape, family).

A root is ``half`` (``lazy_cases._half`` at the value's width) of the family's fold: the xor of
the family's consumer values of that shape (zero-extended to one width), times an odd literal so that a wrong low limb reaches the
bits an unsigned compare with a uniform limit looks at.  A program holds at most ``PER_PROGRAM``
shapes (a root each, which holds for about seven candidates in eight, and a program's verdict must stay
informative), grouped by width class and family.

``fuzz_case(seed)``: ``ITE(a == b, cone, z)`` (or the else-arm form) behind ``lazy_cases``'
generator-controlled condition, the cone a random expression over the tier's operators whose
variables take random shapes of the table.

Seeds were picked once on the CPU (``find_seeds``) so that every window a test uses holds hits and
misses and, for the fuzz, every group class of the guarded condition.  Test infrastructure only."""
from __future__ import annotations

import functools
import random

from mythril_amd.smt import terms as T
from oracle import cport
from tests import lazy_cases as LC

# Windows: the simulator's (64 x 24 candidates) and the GPU's (4,096), aligned and from an odd index
ALIGNED, ODD = LC.ALIGNED, LC.ODD
SIM_COUNT, GPU_COUNT = 64 * 24, 4096
PER_PROGRAM = 20  # shapes (a root each) per table program, at most
# ... of the division and EXP families above 32 bits (loops in the first tier; the O3 tier compiles a
# 256-bit shape's ten divisions in about a second)
# A first-tier kernel's group loop is one 16-bit branch: a body past 32,767 dwords does not assemble,
# which bounds the division programs (about 700 instructions per 256-bit division).
PER_PROGRAM_HEAVY = {"div": {"narrow": 5, "w32": 13, "w64": 6, "w160": 3, "w256": 2},
                     "heavy": {"w64": 10, "w160": 4, "w256": 4}}


def top(w):
    return (1 << w) - 1


# ---- (a) shapes ----------------------------------------------------------------------------------

def entries(w, n, tag="", partial=False, equal=False):
    """n entries of width w: entry 0 has the top bit of the width, the last of three or more is 0;
    ``partial``: every entry agrees with entry 0 in the limbs above the lowest two (w = 64: in the
    high limb); ``equal``: all entries are entry 0."""
    rng = random.Random(f"gen-repr-{w}-{n}-{tag}")
    vals = [rng.getrandbits(w) | (1 << (w - 1))]
    seen = set(vals)
    while len(vals) < n:
        v = rng.getrandbits(w)
        if partial:
            keep = top(w) ^ (top(32) if w <= 64 else top(64))
            v = (vals[0] & keep) | (v & ~keep & top(w))
        if equal:
            v = vals[0]
        if v in seen and not equal and (1 << w) > 2 * n:
            continue
        seen.add(v)
        vals.append(v)
    if n >= 3 and not equal and not partial:
        vals[-1] = 0
    return vals


class Shape:
    """One way to generate the coordinate x.  ``how``: 'dict', 'mixed' (the dictionary as a MIXED
    coordinate's DICT alternative), 'copy' (x is a DICT coordinate and a later MIXED coordinate copies
    it; the consumers read that one), 'fixed', 'range1', 'aligned1', 'fixall'."""

    def __init__(self, how, w, values=(), tag=""):
        self.how, self.w, self.values = how, w, list(values)
        self.name = f"{how}{w}" + (f"n{len(self.values)}" if how in ("dict", "mixed", "copy") else "") + tag

    def apply(self, g, ix, x, src=None):
        """Shape coordinate named x (``src``: the earlier coordinate a 'copy' shape copies)."""
        w, vals = self.w, self.values
        if self.how == "dict":
            g.dict(ix[x], vals)
        elif self.how == "mixed":
            g.mixed(ix[x], vals, p_dict=0.6, small_bits=min(w, 20), p_small=0.2)
        elif self.how == "copy":
            assert ix[src] < ix[x], (src, x)
            g.dict(ix[src], vals)
            g.mixed(ix[x], vals[:1], p_dict=0.2, copy_from=ix[src], p_copy=0.6)
        elif self.how == "fixed":
            g.fixed(ix[x], vals[0])
        elif self.how == "range1":
            g.range(ix[x], vals[0], 1)
        elif self.how == "aligned1":
            g.aligned(ix[x], vals[0], min(w - 1, 5), 1)
        elif self.how == "fixall":
            g.uniform(ix[x])
            g.fix(ix[x], top(w), vals[0])
        else:
            raise ValueError(self.how)

    def literals(self):
        """(a literal x can equal, one it cannot) for the compares."""
        inside = self.values[len(self.values) // 2]
        if self.how in ("mixed", "copy"):
            return inside, (inside + 1) & top(self.w)  # the UNIFORM rest can take any value
        taken = set(self.values)
        outside = next(v & top(self.w) for v in range(inside + 1, inside + 2 + len(taken)) if v & top(self.w) not in taken) \
            if (1 << self.w) > len(taken) else inside
        return inside, outside


# DICT (w, n) on each side of: the first tier's n * w = 32; the O3 tier's n * w = 64 and its w <= 32;
# selects against the next form (4 and 5 = select_dict_max and one more); the LDS forms
DICT_PAIRS = [
    (32, 1), (32, 2), (31, 1), (31, 2), (24, 1), (16, 2), (16, 3), (11, 2), (11, 3), (8, 4), (8, 5), (4, 8), (4, 9),
    (1, 32), (1, 33),
    (32, 3), (16, 4), (16, 5), (8, 8), (8, 9), (1, 64), (1, 65), (33, 1), (64, 1),
    (64, 4), (64, 5), (160, 4), (160, 5), (256, 4), (256, 5),
    (160, 17), (160, 96), (256, 17), (256, 96),
]
CONST_WIDTHS = [1, 8, 31, 32, 33, 64, 256]
WIDTH_CLASSES = {"narrow": (1, 4, 8, 11, 16, 24, 31), "w32": (32,), "w64": (33, 64), "w160": (160,), "w256": (256,)}


@functools.lru_cache(maxsize=None)
def shapes():
    out = []
    dicts = [(w, n, "", {}) for w, n in DICT_PAIRS]
    dicts += [(8, 4, "eq", {"equal": True}), (64, 3, "eq", {"equal": True}), (256, 5, "eq", {"equal": True}),
              (64, 3, "part", {"partial": True}), (64, 17, "part", {"partial": True}),
              (256, 3, "part", {"partial": True}), (256, 17, "part", {"partial": True})]
    for w, n, tag, kw in dicts:
        vals = entries(w, n, tag, **kw)
        for how in ("dict", "mixed", "copy"):
            out.append(Shape(how, w, vals, tag))
    for w in CONST_WIDTHS:
        rng = random.Random(f"gen-repr-const-{w}")
        for how in ("fixed", "range1", "aligned1", "fixall"):
            out.append(Shape(how, w, [rng.getrandbits(w) | (1 << (w - 1))]))
    assert len({s.name for s in out}) == len(out)
    return out


def width_class(w):
    return next(k for k, ws in WIDTH_CLASSES.items() if w in ws)


# ---- consumers -----------------------------------------------------------------------------------

def _bin(op, a, b):
    return T.bvbin(op, a, b)


def half(x, name):
    """``lazy_cases._half`` at x's width: x below a uniform coordinate of its own, or the coin."""
    return T.or_(LC._ult(x, LC._v(name + "_lim", x.width)), LC._coin(name))


def _fit(t):
    """At most 256 bits (the tiers' bound for arithmetic): the top 256 of a wider value."""
    return t if t.width <= 256 else T.extract(t.width - 1, t.width - 256, t)


def _fold(values, bools, rng):
    """One value: the xor of ``values`` zero-extended to their widest (at least 32 bits), each Bool
    as a random 32-bit literal or 0, times an odd literal."""
    values = [_fit(v) for v in values]
    w = max([32] + [v.width for v in values])
    acc = None
    for v in values:
        v = T.zero_extend(w - v.width, v) if v.width < w else v
        acc = v if acc is None else _bin("bvxor", acc, v)
    for b in bools:
        v = T.ite(b, T.BitVecVal(rng.getrandbits(w) | 1, w), T.BitVecVal(0, w))
        acc = v if acc is None else _bin("bvadd", acc, v)
    return _bin("bvmul", acc, T.BitVecVal(rng.getrandbits(w) | 1, w))


def _arith(x, x2, y, sh, p, rng):
    vs = []
    for op in ("bvmul", "bvadd", "bvsub", "bvand", "bvor", "bvxor"):
        vs += [_bin(op, x, y), _bin(op, y, x)]
    return vs + [T.bvun("bvneg", x), T.bvun("bvnot", x)], []


def _div(x, x2, y, sh, p, rng):
    vs = []
    for op in ("bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod"):
        vs += [_bin(op, x, y), _bin(op, y, x)]
    return vs, []


def _shift(x, x2, y, sh, p, rng):
    w = x.width
    amount = _bin("bvand", y, T.BitVecVal((2 * w - 1) & top(w), w))  # amounts below and above the width
    vs = []
    for op in ("bvshl", "bvlshr", "bvashr"):
        vs += [_bin(op, x, amount), _bin(op, y, x)]
    return vs, []


def _cmp(x, x2, y, sh, p, rng):
    inside, outside = sh.literals()
    bs = []
    for other in (y, T.BitVecVal(inside, x.width), T.BitVecVal(outside, x.width), x2):
        bs.append(T.eq(x, other))
        for op in ("bvult", "bvule", "bvslt", "bvsle"):
            bs += [T.bvcmp(op, x, other), T.bvcmp(op, other, x)]
    return [], bs


def _struct(x, x2, y, sh, p, rng):
    w = x.width
    y8 = T.BitVecVar(p + "_y8", 8)
    vs = [T.extract(min(w - 1, 7), 0, x), T.extract(w - 1, w // 2, x)]
    if w > 40:
        vs.append(T.extract(39, 24, x))  # across limbs 0 and 1
    if w > 140:
        vs.append(T.extract(135, 60, x))  # from limb 1 into limb 4
    for k in (1, 32, 40):
        vs += [T.zero_extend(k, x), T.sign_extend(k, x)]
    vs += [T.concat(x, y8), T.concat(y8, x)]
    vs.append(T.ite(T.bvcmp("bvult", y8, T.BitVecVal(128, 8)), x, y))  # x as an arm
    vs.append(T.ite(T.eq(x, x2), y, T.bvun("bvnot", y)))               # x == x' as the condition
    return vs, []


def _lookup(x, x2, y, sh, p, rng):
    w = x.width
    arr = T.ArrayVar(p + "_A", w, 64)
    f = T.FuncDecl(p + "_f", w, 64)
    return [T.select(arr, x), T.select(arr, x2), T.select(arr, y), T.app(f, x), T.app(f, x2), T.app(f, y)], []


def _heavy(x, x2, y, sh, p, rng):
    w = x.width
    vs = []
    if w >= 8:  # EXP: exponents of at most 4 bits (a wave runs to its largest exponent's length)
        small = T.BitVecVal(15, w)
        vs = [T.bvexp(x, _bin("bvand", y, small)), T.bvexp(y, _bin("bvand", x, small))]
    return vs, [T.bvcmp("bvumul_noovfl", x, y), T.bvcmp("bvumul_noovfl", y, x)]


FAMILIES = {"arith": _arith, "div": _div, "shift": _shift, "cmp": _cmp, "struct": _struct, "lookup": _lookup,
            "heavy": _heavy}


class Program(LC.Case):
    """``lazy_cases.Case`` with the table's shapes: ``items`` = [(Shape, prefix)], one root each."""

    def __init__(self, name, family, items):
        self.name, self.family, self.items = name, family, items
        rng = random.Random("gen-repr-prog-" + name)
        roots = []
        for sh, p in items:
            w = sh.w
            x, x2, y = LC._v(p + "_x", w), LC._v(p + "_x2", w), LC._v(p + "_y", w)
            vs, bs = FAMILIES[family](x, x2, y, sh, p, rng)
            if sh.how == "copy":  # the source is read too, and named before the coordinate that copies it
                s, s2 = LC._v(p + "_s", w), LC._v(p + "_s2", w)
                roots.append(T.or_(T.eq(s, s2), LC._coin(p + "_pre")))
            roots.append(half(_fold(vs, bs, rng), p))

        def shape(g, ix):
            for sh, p in items:
                sh.apply(g, ix, p + "_x", p + "_s")
                if p + "_x2" in ix:
                    sh.apply(g, ix, p + "_x2", p + "_s2")

        super().__init__(roots, shape, conds=[], regions=None)


def _chunks(wc, fam):
    """The shapes of a width class in equal parts of at most the family's size."""
    mine = [s for s in shapes() if width_class(s.w) == wc]
    step = PER_PROGRAM_HEAVY.get(fam, {}).get(wc, PER_PROGRAM)
    parts = (len(mine) + step - 1) // step
    return [mine[k::parts] for k in range(parts)]


@functools.lru_cache(maxsize=None)
def program_names():
    return [f"{wc}_{fam}_{k}" for wc in WIDTH_CLASSES for fam in FAMILIES for k in range(len(_chunks(wc, fam)))]


@functools.lru_cache(maxsize=None)
def program(name):
    wc, fam, k = name.split("_")
    return Program(name, fam, [(s, f"r_{fam[:2]}_{s.name}") for s in _chunks(wc, fam)[int(k)]])


def shapes_of(name):
    return [s for s, _ in program(name).items]


# ---- (b) the fuzz --------------------------------------------------------------------------------

FUZZ_WIDTHS = (8, 16, 31, 32, 33, 64, 160, 256)
FUZZ_DICT_N = (1, 2, 3, 4, 5, 8, 9, 17, 96)


def _random_shape(rng, w):
    how = rng.choice(["uniform", "uniform", "range", "dict", "dict", "dict", "mixed", "fixed", "aligned"])
    if how in ("dict", "mixed"):
        n = rng.choice(FUZZ_DICT_N)
        if w < 16:
            n = min(n, 1 << (w - 1))
        tag = rng.choice(["", "", "part", "eq"]) if w >= 64 and n > 1 else ""
        return Shape(how, w, entries(w, n, "fz" + tag, partial=tag == "part", equal=tag == "eq"))
    return (how, w, rng.getrandbits(w), rng.choice([1, 2, 77, 1 << 16]))


class Fuzz(LC.Case):
    def __init__(self, seed):
        rng = random.Random(f"gen-repr-fuzz-{seed}")
        p = f"z{seed}"
        w = rng.choice(FUZZ_WIDTHS)
        self.w, self.else_arm = w, rng.random() < 0.4
        kinds = {}
        count = [0]

        def var(width=w):
            if kinds and rng.random() < 0.3:
                same = [n for n, k in kinds.items() if k[0] == width]
                if same:
                    return LC._v(rng.choice(same), width)
            name = f"{p}_v{count[0]}"
            count[0] += 1
            kinds[name] = (width, _random_shape(rng, width))
            return LC._v(name, width)

        arr = T.ArrayVar(p + "_A", w, w)
        f = T.FuncDecl(p + "_f", w, w)

        def expr(depth):
            if depth == 0:
                return var()
            k = rng.random()
            a = expr(depth - 1)
            if k < 0.40:
                return _bin(rng.choice(["bvadd", "bvsub", "bvmul", "bvand", "bvor", "bvxor"]), a, expr(depth - 1))
            if k < 0.50:
                return T.bvun(rng.choice(["bvnot", "bvneg"]), a)
            if k < 0.60:
                hi = rng.randrange(w)
                lo = rng.randrange(hi + 1)
                part = T.extract(hi, lo, a)
                fill = w - part.width
                if not fill:
                    return part
                return rng.choice([T.zero_extend, T.sign_extend])(fill, part) if rng.random() < 0.6 else \
                    T.concat(part, T.extract(fill - 1, 0, expr(depth - 1)))
            if k < 0.75:
                c = T.bvcmp(rng.choice(["bvult", "bvule", "bvslt", "bvsle"]), a, expr(depth - 1)) if rng.random() < 0.7 \
                    else T.eq(a, var())
                return T.ite(c, expr(depth - 1), var())
            if k < 0.85:
                return T.select(arr, a) if rng.random() < 0.5 else T.app(f, a)
            if k < 0.93:
                return _bin(rng.choice(["bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod", "bvshl", "bvlshr", "bvashr"]),
                            a, var())
            return T.bvexp(a, _bin("bvand", var(), T.BitVecVal(7, w))) if w >= 8 else a

        cone = expr(rng.randint(1, 3))
        if cone.op == "bvvar":  # (depth 1 may draw nothing but a variable)
            cone = _bin("bvadd", cone, var())
        a, b = LC._pair(p)
        z = LC._v(p + "_z", w)
        r = T.ite(T.eq(a, b), z, cone) if self.else_arm else T.ite(T.eq(a, b), cone, z)
        roots = [LC._pre(p, b)]
        if self.else_arm:  # the shared arm is read before the ITE (lazy_cases.case_else_arm)
            roots.append(half(z, p + "_c0"))
        roots += [half(r, p + "_c1"), half(LC._v(p + "_t", w), p + "_c2")]

        def shape(g, ix):
            for name, (width, sh) in kinds.items():
                if name not in ix:
                    continue
                if isinstance(sh, Shape):
                    sh.apply(g, ix, name)
                elif sh[0] == "range":
                    g.range(ix[name], sh[2], sh[3])
                elif sh[0] == "fixed":
                    g.fixed(ix[name], sh[2])
                elif sh[0] == "aligned":
                    g.aligned(ix[name], sh[2], min(width - 1, 4), sh[3])

        super().__init__(roots, shape, [(p + "_a", p + "_b")], regions=None)
        self.name = f"fuzz{seed}"


@functools.lru_cache(maxsize=4096)
def fuzz_case(seed):
    return Fuzz(seed)


N_FUZZ_SIM, N_FUZZ_GPU = 1000, 96

# ---- seeds -----------------------------------------------------------------------------------------

SEED = 1  # the generator seed of every program ...
# ... but these, under which a window lacked a hit or a group class (find_seeds)
SEEDS = {}


def seed_of(case):
    return SEEDS.get(case.name, SEED)


def window_ok(case, seed, start, count):
    """The corpus conditions of one (program, window), from the C port alone: every guarded condition
    has an all-false, a mixed and an all-true group, and the verdicts hold hits and misses."""
    for c in range(len(case.conds)):
        if min(case.group_classes(seed, start, count, c)) == 0:
            return False
    sat = int(cport.search(case.pb, case.blob, seed, start, count, threads=2, verdicts=True)[2].sum())
    return 0 < sat < count


def find_seeds(cases, tries=200):
    """{name: seed} for the cases SEED does not serve (writing SEEDS)."""
    out = {}
    for case in cases:
        for seed in range(SEED, SEED + tries):
            if all(window_ok(case, seed, st, n) for st in (ALIGNED, ODD) for n in (SIM_COUNT, GPU_COUNT)):
                break
        else:
            raise RuntimeError("no seed for " + case.name)
        if seed != SEED:
            out[case.name] = seed
    return out
