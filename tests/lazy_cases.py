"""Probe programs for the first tier's guarded select arms (``jit_asm.cpp: plan_lazy``), shared by
``tests/test_asm_lazy_sim.py`` (CPU simulator) and ``tests/test_gpu_asm_lazy.py``.

Every guarded condition is an equality ``a == b`` of two coordinates the generator controls:
``b`` draws from a three-entry dictionary, ``a`` is MIXED with a COPY alternative (of ``b``: the
condition holds in every lane of the group), a DICT alternative (96 entries holding ``b``'s three:
about one lane in 96 holds, so a group is usually mixed) and the UNIFORM rest (no lane holds).
``group_classes`` counts, from the C port's generated coordinates alone, how many groups of a
window are all-false, mixed and all-true; the seeds below were picked on the CPU so that every
window a test uses holds at least one group of each class.
"""
import random

import numpy as np

from mythril_amd import search
from mythril_amd.smt import terms as T
from oracle import cport

W = 256
VALS = list(search.ACTORS)
_rng = random.Random(0x1A27)
BIG = VALS + [_rng.getrandbits(160) for _ in range(93)]          # a's dictionary: b's entries and 93 others
TABLE = [_rng.getrandbits(256) for _ in range(24)]               # a cone's dictionary (staged in LDS)


def _v(name, w=W):
    return T.BitVecVar(name, w)


def _k(v, w=W):
    return T.BitVecVal(v % (1 << w), w)


def _ult(a, b):
    return T.bvcmp("bvult", a, b)


def _add(a, b):
    return T.bvbin("bvadd", a, b)


def _coin(name):
    """True for three candidates in four: the conjunction of a case's roots stays satisfiable for a
    fair share of them, so a wrong select shows as a wrong verdict."""
    return _ult(_v(name, 32), _k(0xC0000000, 32))


def _half(x, name):
    """A root that reads every limb of x: x below a uniform coordinate of its own, or the coin.  (A
    compare with a literal would be pushed into an ITE's arms by the specialiser, leaving a Bool
    ITE, which lives on lane masks and is not guarded.)"""
    return T.or_(_ult(x, _v(name + "_lim")), _coin(name))


class Case:
    def __init__(self, roots, shape, conds, regions, env=None):
        self.roots, self.shape, self.conds, self.regions, self.env = roots, shape, conds, regions, env or {}
        self.P, _ = search.prepare(roots)
        g = search.default_generator(self.P, roots=roots)
        ix = {c.name: c.index for c in self.P.coords}
        sites = {c.index for c in self.P.sites}
        for c in self.P.coords:  # only the shapes below: no COPY link the propagated generator adds
            if c.index not in sites:
                g.uniform(c.index)
        for a, b in conds:
            assert ix[b] < ix[a], "the MIXED side copies an earlier coordinate"
            g.dict(ix[b], VALS)
            g.mixed(ix[a], BIG, p_dict=0.34, copy_from=ix[b], p_copy=0.33)
        shape(g, ix)
        self.blob = g.blob()
        self.pb = self.P.to_bytes()
        self.ix = ix

    def rows(self, name):
        """SoA rows (first, limbs) of coordinate ``name``."""
        at = 0
        for c in self.P.coords:
            n = (c.width + 31) // 32
            if c.name == name:
                return at, n
            at += n
        raise KeyError(name)

    def words(self):
        return sum((c.width + 31) // 32 for c in self.P.coords)

    def lanes_true(self, seed, start, count, cond=0):
        """Per candidate of [start, start + count): whether condition ``cond`` holds (C port)."""
        soa = cport.gen_soa(self.pb, self.blob, seed, start, count, self.words())
        a, b = self.conds[cond]
        (ra, n), (rb, _) = self.rows(a), self.rows(b)
        return np.all(soa[ra:ra + n] == soa[rb:rb + n], axis=0)

    def group_classes(self, seed, start, count, cond=0):
        """(all-false, mixed, all-true) groups among the aligned 64-candidate groups the window touches
        (a group cut by the window's ends is classed over all 64 of its lanes, as the wave sees it)."""
        g0, g1 = start // 64, (start + count + 63) // 64
        t = self.lanes_true(seed, g0 * 64, (g1 - g0) * 64, cond).reshape(-1, 64).sum(axis=1)
        return int((t == 0).sum()), int(((t > 0) & (t < 64)).sum()), int((t == 64).sum())


def _pair(p):
    return _v(p + "_a"), _v(p + "_b")


def _pre(p, b):
    """The first root: names b before a (coordinate order), and is an ASSERT ahead of every guard."""
    return T.or_(T.eq(b, _k(VALS[1])), _coin(p + "_pre"))


def _cone_shape(p):
    def shape(g, ix):
        g.mixed(ix[p + "_m"], TABLE, p_dict=0.6, small_bits=20, p_small=0.2)
    return shape


def case_true_arm():
    """ITE(a == b, m + x, z): the true arm's cone holds an ADD, a MIXED coordinate with a dictionary
    in LDS and a uniform one; z dies at the ITE (selected in place).  ASSERTs before and after."""
    p = "lt"
    a, b = _pair(p)
    r = T.ite(T.eq(a, b), _add(_v(p + "_m"), _v(p + "_x")), _v(p + "_z"))
    roots = [_pre(p, b), _half(r, p + "_c0"), _half(_v(p + "_t"), p + "_c1")]
    return Case(roots, _cone_shape(p), [(p + "_a", p + "_b")], regions=1)


def case_else_arm():
    """ITE(a == b, z, m + x) with z read by an earlier root: the true arm is shared (no cone), the
    else arm is guarded on "every lane true" and z's registers die at the ITE."""
    p = "le"
    a, b = _pair(p)
    z = _v(p + "_z")
    r = T.ite(T.eq(a, b), z, _add(_v(p + "_m"), _v(p + "_x")))
    roots = [_pre(p, b), _half(z, p + "_c0"), _half(r, p + "_c1"), _half(_v(p + "_t"), p + "_c2")]
    return Case(roots, _cone_shape(p), [(p + "_a", p + "_b")], regions=1)


def case_nested():
    """A guarded ITE inside a guarded ITE's cone: ITE(a == b, ITE(c == d, p + q, r) + s, z)."""
    p = "ln"
    a, b = _pair(p)
    c, d = _v(p + "2_a"), _v(p + "2_b")
    inner = T.ite(T.eq(c, d), _add(_v(p + "_p"), _v(p + "_m")), _v(p + "_r"))
    r = T.ite(T.eq(a, b), _add(inner, _v(p + "_s")), _v(p + "_z"))
    roots = [_pre(p, b), T.or_(T.eq(d, _k(VALS[2])), _coin(p + "_pre2")), _half(r, p + "_c0"),
             _half(_v(p + "_t"), p + "_c1")]
    return Case(roots, _cone_shape(p), [(p + "_a", p + "_b"), (p + "2_a", p + "2_b")], regions=2)


def case_copy_source(link=True):
    """ITE(a == b, x, z) where x looks exclusive to the arm but is the COPY source of coordinate w,
    generated later: x is generated outside every region (no guard at all here: z is read again,
    so the else arm cannot be selected in place either).  ``link=False``: w copies nothing, and the
    arm is guarded."""
    p = "lc" if link else "lu"
    a, b = _pair(p)
    x, z, w = _v(p + "_x"), _v(p + "_z"), _v(p + "_w")
    r = T.ite(T.eq(a, b), x, z)
    roots = [_pre(p, b), _half(r, p + "_c0"), _half(w, p + "_c1"), _half(z, p + "_c2")]

    def shape(g, ix):
        assert ix[p + "_x"] < ix[p + "_w"]
        if link:
            g.mixed(ix[p + "_w"], TABLE, p_dict=0.3, copy_from=ix[p + "_x"], p_copy=0.5)
        else:
            g.mixed(ix[p + "_w"], TABLE, p_dict=0.3)

    return Case(roots, shape, [(p + "_a", p + "_b")], regions=0 if link else 1)


def case_shared_arm():
    """s = x + y is the true arm of two ITEs and read once more afterwards: no cone, no guard."""
    p = "ls"
    a, b = _pair(p)
    c, d = _v(p + "2_a"), _v(p + "2_b")
    s = _add(_v(p + "_x"), _v(p + "_y"))
    r1 = T.ite(T.eq(a, b), s, _v(p + "_z1"))
    r2 = T.ite(T.eq(c, d), s, _v(p + "_z2"))
    roots = [_pre(p, b), T.or_(T.eq(d, _k(VALS[2])), _coin(p + "_pre2")), _half(r1, p + "_c0"),
             _half(r2, p + "_c1"), _half(s, p + "_c2")]
    return Case(roots, lambda g, ix: None, [(p + "_a", p + "_b"), (p + "2_a", p + "2_b")], regions=0)


def case_copy_path():
    """ITE(a == b, m + x, z) with z read again afterwards: the result takes fresh registers, copied
    from z before the branch."""
    p = "lp"
    a, b = _pair(p)
    z = _v(p + "_z")
    r = T.ite(T.eq(a, b), _add(_v(p + "_m"), _v(p + "_x")), z)
    roots = [_pre(p, b), _half(r, p + "_c0"), _half(z, p + "_c1")]
    return Case(roots, _cone_shape(p), [(p + "_a", p + "_b")], regions=1)


def case_lookup(priors):
    """An uninterpreted function read at ``priors + 1`` keys, the last one a: its canonicalising
    LOOKUP tests a against every earlier key (b first).  One prior is guarded by default, three with
    MYTHGPU_JIT_ASM_LAZY_PRIORS=3."""
    p = "lk%d" % priors
    a, b = _pair(p)
    f = T.FuncDecl(p + "_f", W, W)
    keys = [b] + [_v(p + "_k%d" % i) for i in range(priors - 1)] + [a]
    apps = [T.app(f, k) for k in keys]
    acc = apps[0]
    for x in apps[1:-1]:
        acc = T.bvbin("bvxor", acc, x)
    roots = [_pre(p, b), T.or_(_ult(apps[-1], acc), _coin(p + "_c0")), _half(_v(p + "_t"), p + "_c1")]

    def shape(g, ix):
        for i in range(priors - 1):
            g.dict(ix[p + "_k%d" % i], VALS)

    # (one region per lookup of the chain: the sites after the first test 1 .. priors earlier keys)
    return Case(roots, shape, [(p + "_a", p + "_b")], regions=priors,
                env={"MYTHGPU_JIT_ASM_LAZY_PRIORS": str(priors)} if priors > 1 else {})


def case_many_bools(n=26):
    """n Bools (lane masks) computed before a guarded ITE and read after it: more than the SGPR pairs
    a region may leave taken, so masks move to their VGPR form before the branch."""
    p = "lb"
    a, b = _pair(p)
    ks = [_v(p + "_k%d" % i, 64) for i in range(n)]
    bools = [_ult(k, _k(1 << 63, 64)) for k in ks]
    r = T.ite(T.eq(a, b), _add(_v(p + "_m"), _v(p + "_x")), _v(p + "_z"))
    last = [T.xor_(bools[i], bools[(i + 5) % n]) for i in range(n)]
    roots = [_pre(p, b), T.or_(*bools), _half(r, p + "_c0"), T.or_(T.and_(*last[:n // 2]), T.or_(*last[n // 2:]))]
    return Case(roots, _cone_shape(p), [(p + "_a", p + "_b")], regions=1)


BUILDERS = {
    "true_arm": case_true_arm,
    "else_arm": case_else_arm,
    "nested": case_nested,
    "copy_source": case_copy_source,
    "copy_source_unlinked": lambda: case_copy_source(link=False),
    "shared_arm": case_shared_arm,
    "copy_path": case_copy_path,
    "lookup_1": lambda: case_lookup(1),
    "lookup_3": lambda: case_lookup(3),
    "many_bools": case_many_bools,
}

# Windows: 64 x 8 candidates, aligned and starting at an odd index (a partial first and last group)
ALIGNED, ODD, COUNT = 1 << 40, (1 << 40) + 37, 64 * 8
# seed per case: both windows hold an all-false, a mixed and an all-true group of every condition
SEEDS = {'true_arm': 1, 'else_arm': 1, 'nested': 4, 'copy_source': 1, 'copy_source_unlinked': 1, 'shared_arm': 4,
         'copy_path': 1, 'lookup_1': 1, 'lookup_3': 1, 'many_bools': 3}
# (seed, group base) of the true-arm case: exactly one lane holds, lane 0 / lane 63
SINGLE_LANE = {0: (1, 1099511697088), 63: (1, 1099511640384)}


def find_seed(case, tries=4000):
    """The first seed under which both windows hold every class of every condition (picking SEEDS)."""
    for seed in range(1, tries):
        if all(min(case.group_classes(seed, st, COUNT, c)) > 0
               for st in (ALIGNED, ODD) for c in range(len(case.conds))):
            return seed
    raise RuntimeError("no seed")


def find_single_lane(case, lane, seed=1, groups=1 << 15):
    t = case.lanes_true(seed, ALIGNED, 64 * groups).reshape(-1, 64)
    only = np.flatnonzero((t.sum(axis=1) == 1) & t[:, lane])
    return seed, ALIGNED + 64 * int(only[0])
