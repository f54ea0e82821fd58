"""Waves for the operators whose code path depends on the data: EXP, the divisions, the variable
shifts and the multiplies, as a table of plain big integers.

A *wave* is 64 operand pairs (a, b) at one width that one wavefront evaluates together, so the
table decides what a ballot sees: the exponent limbs that are live, the remainder width ``NB`` of
the division loop, the lanes of the one-limb path, the wave's longest quotient.

Candidate-to-lane mapping of the explicit-input entry points (read from the kernels):

* ``mg_eval`` (``run_body.inc``): blocks of one 64-lane wave; a block's group ``g`` evaluates the
  candidates ``base + 64 g + lane`` with ``base`` a multiple of 64, so candidates ``64 k .. 64 k + 63``
  share a wave with candidate ``i`` in lane ``i % 64``.  Lanes past the end re-evaluate the last
  candidate, so a partial last wave sees that candidate's operands in its idle lanes.
* ``mg_jit_eval``, O3 kernel (``jit.cpp`` ``mgj_eval``): 256-thread blocks, candidate
  ``i = 256 block + thread`` and a stride of ``256 blocks``: wave ``t / 64`` of a block holds the 64
  consecutive candidates from a multiple of 64, lane ``i % 64``.  The ``tiled`` SoA changes only the
  address of candidate ``i``'s word (``((i / 64) rows + r) 64 + i % 64``), not which lane evaluates it.
* ``mg_jit_eval``, first tier (``jit_asm.cpp``): 64 candidates per group from a multiple of 64, lane
  ``i % 64``, in both layouts (the tiled one reads whole 64-candidate blocks).

So in every engine and in both layouts a wave of the table placed at a candidate offset that is a
multiple of 64 is one wavefront, lane = position in the wave, and no other placement is needed.  At
an offset that is no multiple of 64 each wavefront holds the tail of one wave and the head of the
next (``test_gpu_wave_ops`` runs one width that way).

Every wave has a *profile* name.  Nothing here calls the code under test: the decisions a wave takes
are computed by the restatements below (``exp_decisions``, ``div_decisions``, ``mg_step``), written
from the operators' definitions and, for the one-limb step, from Moller & Granlund, "Improved
division by invariant integers" (IEEE TC 2011), Algorithm 4.  ``self_check`` tags every wave with its
decisions and asserts that every value the table promises is reached; ``tests/test_wave_ops_cpu.py``
runs it.

What the restatements prove unreachable, and the table therefore does not hold:

* the second correction, (0, 1) and (1, 1), at the top limb position (7 of a 256-bit dividend).  All
  four combinations occur elsewhere ((1, 1): the cheap test ``r > q0`` misfires on a non-negative
  candidate remainder and the second correction undoes it; about 0.1 % of random steps each).  At
  the top the step's high word ``u1`` is below ``2^sh``, ``sh`` the divisor's leading zeros.  With
  ``(2^32 + v) dn = 2^64 - k``, ``1 <= k <= dn``, the true quotient exceeds the estimate
  ``q1 + q0 / 2^32`` by ``(u1 k + u0 (2^32 - dn)) / (2^32 dn) < 2^(sh - 32) + (2^32 - dn) / dn``.  Either
  form of the second correction needs that above 1, so ``dn < 2^31 / (1 - 2^(sh - 33))``; ``dn`` is a
  multiple of ``2^sh`` from ``2^31`` on, which leaves ``dn = 2^31`` (``v = 2^32 - 1``, ``k = dn``), where
  the estimate is ``2 u1 + (u0 - u1) / 2^32``: it then takes ``u0 >= 2^31`` with ``u0 < u1``, or
  ``2 u1 > 2^32``, and ``u1 < 2^31``.  ``self_check`` asserts positions 0..6 and that no wave of the
  table takes the second correction at the top.  Below a top limb of one bit (widths 65 and 33) the
  next position is out of reach as well: its high word is the top step's remainder, below
  ``2^(sh + 1)``, the same bound gives ``dn < 2^31 / (1 - 2^(sh - 32))``, again only ``dn = 2^31``, and
  there ``u1 < dn = 2^31`` at every position.  Dropped, as ``mg_dropped`` lists them: (w, (0, 1) and
  (1, 1), top position) at every width; (65, (0, 1) and (1, 1), 1); (33, (0, 1) and (1, 1), 0).  Every
  other (combination, position) is asserted at every width of 32 bits and more, and a search that
  finds no dividend for one fails the table.
* a carry out of the division loop's remainder at ``NB`` = 8 limbs (and at ``NB`` = all limbs of any
  width): a divisor with bit ``32 NB - 1`` = the width's top bit leaves a quotient of one bit, so the
  loop takes one step from a remainder ``a >> 1`` whose top bit is clear.  The waves ``div_top_full``
  hold such divisors; ``self_check`` asserts that the restated loop never carries there.  ``NB`` = 2 and
  4 carry at every width above 64 and 128 bits.

Test infrastructure only."""
from __future__ import annotations

import functools
import random

from mythril_amd.smt import terms as T

LANES = 64
WIDTHS = (256, 255, 160, 65, 64, 33, 32, 8, 1)
EXP_WIDTHS = (256, 64)
EXP_LENGTHS = (0, 1, 2, 3, 4, 7, 8, 9, 30, 31, 32, 33, 34, 63, 64, 65, 127, 128, 129, 255, 256)
QLENS = (0, 1, 2, 31, 32, 33, 64, 128, 223, 224, 255)
ONE_LIMB_DIVISORS = (1, 2, 3, 7, 10, 641, 1 << 16, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 2, (1 << 32) - 1)
CLASSES = {1: (1, 32), 2: (33, 64), 3: (65, 128), 4: (129, 256)}  # divisor bit lengths
DIV_OPS = ("bvudiv", "bvurem", "bvsdiv", "bvsrem", "bvsmod")
SHIFT_OPS = ("bvshl", "bvlshr", "bvashr")
M32 = (1 << 32) - 1
COMBOS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (first, second correction) of a 2/1 step


def top(w):
    return (1 << w) - 1


def nbits(rng, n):
    """A random integer of exactly n bits (0 for n = 0)."""
    return 0 if n == 0 else (1 << (n - 1)) | rng.getrandbits(n - 1)


def limbs_of(x, n=8):
    return [(x >> (32 * i)) & M32 for i in range(n)]


class Wave:
    __slots__ = ("family", "width", "name", "pairs", "tags")

    def __init__(self, family, width, name, pairs):
        assert len(pairs) == LANES, (name, len(pairs))
        m = top(width)
        assert all(0 <= a <= m and 0 <= b <= m for a, b in pairs), name
        self.family, self.width, self.name, self.pairs, self.tags = family, width, name, list(pairs), None

    def __repr__(self):
        return f"Wave({self.family}, w{self.width}, {self.name})"


# ---- restatements ----------------------------------------------------------------------------------

def exp_decisions(exponents):
    """What a wave's ballots give EXP: the live exponent limbs, the longest exponent inside the top
    live limb (m), the even number of leading bits skipped and the 2-bit steps left."""
    live = max((e.bit_length() + 31) // 32 for e in exponents)
    if live == 0:
        return {"live": 0, "m": 0, "skip": 0, "steps": 0}
    m = max(((e >> (32 * (live - 1))) & M32).bit_length() for e in exponents)
    skip = (32 - m) & ~1
    return {"live": live, "m": m, "skip": skip, "steps": 16 * live - skip // 2}


def exp_by_digits(base, e, d, width):
    """base ** e mod 2^width by left-to-right 2-bit digits under the wave's decisions ``d``: equals
    ``pow`` exactly when the digits stay aligned to the exponent's bit 0 and no set bit is skipped."""
    m256 = top(256)
    ex = (e << (32 * (8 - d["live"]))) & m256 if d["live"] else 0
    ex = (ex << d["skip"]) & m256
    r = 1
    for _ in range(d["steps"]):
        dg = ex >> 254
        ex = (ex << 2) & m256
        r = (r ** 4 * base ** dg) & m256
    return r & top(width)


def mg_step(u1, u0, d, v, beta=1 << 32):
    """One 2/1 division step of (u1, u0) by the normalised d with reciprocal v (Algorithm 4):
    (q, r, first correction, second correction, the candidate sum carried out of two words)."""
    full = v * u1 + ((u1 + 1) * beta) + u0
    wrap = full >= beta * beta
    q1, q0 = (full // beta) % beta, full % beta
    r = (u0 - q1 * d) % beta
    c1 = r > q0
    if c1:
        q1, r = (q1 - 1) % beta, (r + d) % beta
    c2 = r >= d
    if c2:
        q1, r = (q1 + 1) % beta, r - d
    return q1, r, c1, c2, wrap


def reciprocal(dn, beta=1 << 32):
    return (beta * beta - 1) // dn - beta


def one_limb_steps(a, d, nlimbs=8):
    """Long division of a by the one-limb d: per limb position (top first) the corrections taken.
    Returns (q, r, {position: (c1, c2, wrap)})."""
    sh = 32 - d.bit_length()
    dn = d << sh
    v = reciprocal(dn)
    x = a << sh
    rr = x >> (32 * nlimbs)
    q, steps = 0, {}
    for i in range(nlimbs - 1, -1, -1):
        ui = (x >> (32 * i)) & M32
        q1, rr, c1, c2, wrap = mg_step(rr, ui, dn, v)
        q |= q1 << (32 * i)
        steps[i] = (int(c1), int(c2), wrap)
    return q, rr >> sh, steps


def loop_carry(a, b, nb):
    """The restoring loop over the quotient's bits only, remainder kept in ``nb`` limbs: does the
    remainder's top bit (bit 32 nb - 1) leave on a shift?  Returns (q, r, carried)."""
    la, lb = a.bit_length(), b.bit_length()
    n = la - lb + 1 if la >= lb else 0
    rem, carried, q = (a >> n) if n else a, False, 0
    for it in range(n - 1, -1, -1):
        carried |= bool(rem >> (32 * nb - 1))
        rem = (rem << 1) | ((a >> it) & 1)
        q <<= 1
        if rem >= b:
            rem -= b
            q |= 1
    return q, rem, carried


def div_class(b):
    return 0 if b == 0 else next(k for k, (lo, hi) in CLASSES.items() if lo <= b.bit_length() <= hi)


def div_decisions(pairs, width):
    """What a wave's divisions decide, for the unsigned operands as given.  ``paths``: per lane
    'zero' / 'one' (a one-limb divisor) / 'loop'; ``nb``: the interpreter's remainder limbs (a ballot
    over the loop lanes: 8, 4 or 2; None without one); ``nb_tier``: the first tier's (the wave's widest
    divisor over all lanes, of 1 / 2 / 4 / all limbs); ``n``: the quotient lengths; ``carry``: lanes
    whose remainder carries out of ``nb`` limbs (``carry_tier``: of ``nb_tier``); ``mg``: the correction
    combinations per limb position over the one-limb lanes; ``wrap``: a candidate sum wrapped."""
    paths = ["zero" if b == 0 else ("one" if b <= M32 else "loop") for _, b in pairs]
    loops = [(a, b) for (a, b), p in zip(pairs, paths) if p == "loop"]
    nb = None
    if loops:
        nb = 8 if any(b >> 128 for _, b in loops) else (4 if any(b >> 64 for _, b in loops) else 2)
    all_limbs = (width + 31) // 32
    widest = max((b.bit_length() + 31) // 32 for _, b in pairs)
    nb_tier = next(k for k in sorted({1, 2, 4, all_limbs}) if k >= widest and k <= all_limbs) if widest else 1
    ns, nq1 = set(), set()
    for a, b in pairs:
        if b:
            la, lb = a.bit_length(), b.bit_length()
            n = la - lb + 1 if la >= lb else 0
            ns.add(n)
            if n == 1:
                nq1.add(int(a >= b))
    mg, wrap = {}, False
    for (a, b), p in zip(pairs, paths):
        if p == "one":
            q, r, steps = one_limb_steps(a, b)
            assert (q, r) == divmod(a, b), (a, b)
            for i, (c1, c2, w_) in steps.items():
                mg.setdefault(i, set()).add((c1, c2))
                wrap |= w_
    carry = sum(loop_carry(a, b, nb)[2] for a, b in loops) if nb else 0
    carry_tier = sum(loop_carry(a, b, nb_tier)[2] for a, b in loops)
    for a, b in loops:
        assert loop_carry(a, b, 8)[:2] == divmod(a, b)
    return {"paths": sorted(set(paths)), "path_lanes": paths, "nb": nb, "nb_tier": nb_tier, "n": ns, "n1_quotients": nq1,
            "carry": carry, "carry_tier": carry_tier, "mg": mg, "wrap": wrap,
            "classes": sorted({div_class(b) for _, b in pairs})}


def shift_decisions(pairs, width):
    """Per lane: the amount below / at / above the width, or with limb 0 zero and a higher limb set."""
    out = set()
    for _, s in pairs:
        if s >> 32 and not s & M32:
            out.add("high_only")
        out.add("below" if s < width else ("at" if s == width else "above"))
    return out


# ---- waves -----------------------------------------------------------------------------------------

def _rng(*key):
    return random.Random("wave-ops-" + "-".join(str(k) for k in key))


def exp_bases(w, rng):
    m = top(w)
    return [0, 1, 2, 3, 1 << (w - 1), m, rng.getrandbits(w) | 1, (rng.getrandbits(w) & ~1 & m) | 2]


def _exp_waves(w):
    out = []
    lengths = [L for L in EXP_LENGTHS if L <= w]
    for L in lengths:
        rng = _rng("exp", w, L)
        bases = exp_bases(w, rng)
        exps = [nbits(rng, L) for _ in range(LANES)]
        if L:
            exps[1] = top(L)
            exps[2] = 1 << (L - 1)
        out.append(Wave("exp", w, f"exp_uniform_L{L}", [(bases[i % 8], exps[i]) for i in range(LANES)]))
        if L == 0:
            continue
        shorter = [x for x in lengths if x < L]
        for lane in (0, 63):
            short = [nbits(rng, shorter[i % len(shorter)] if i < 2 * len(shorter) else rng.randrange(L)) for i in range(LANES)]
            pairs = [(bases[(i + 5) % 8], short[i]) for i in range(LANES)]
            pairs[lane] = (rng.getrandbits(w) | 1, nbits(rng, L))  # the single long lane: an odd base
            out.append(Wave("exp", w, f"exp_mixed_L{L}_lane{lane}", pairs))
    return out


def _divisor(rng, k, w, i=None):
    """A divisor of class k at width w: its shortest, its longest and the full-limb edges first."""
    lo, hi = CLASSES[k]
    hi = min(hi, w)
    edge = [lo, hi, min(hi, lo + 31)]
    L = edge[i] if i is not None and i < len(edge) else rng.randint(lo, hi)
    return top(L) if i == 1 and rng.random() < 0.5 else nbits(rng, L)


def _dividend(rng, w):
    r = rng.random()
    if r < 0.2:
        return max(0, top(w) - rng.randrange(3))
    return nbits(rng, rng.randint(0, w)) if r < 0.7 else rng.getrandbits(w)


def classes_at(w):
    return [k for k, (lo, _) in CLASSES.items() if lo <= w]


def _div_class_waves(w):
    out = []
    ks = classes_at(w)
    for k in ks:
        rng = _rng("divclass", w, k)
        base = [(_dividend(rng, w), _divisor(rng, k, w, i)) for i in range(LANES)]
        out.append(Wave("div", w, f"div_all_c{k}", base))
        for j in ks:
            if j == k:
                continue
            for lane in (0, 63):
                pairs = [(_dividend(rng, w), _divisor(rng, k, w)) for _ in range(LANES)]
                pairs[lane] = (top(w) - rng.randrange(1 << min(w, 8)), _divisor(rng, j, w, 1 if j > k else None))
                out.append(Wave("div", w, f"div_c{k}_out_c{j}_lane{lane}", pairs))
        pairs = [(_dividend(rng, w), 0 if i % 2 else _divisor(rng, k, w)) for i in range(LANES)]
        out.append(Wave("div", w, f"div_zero_mix_c{k}", pairs))
    rng = _rng("divzero", w)
    out.append(Wave("div", w, "div_all_zero", [(_dividend(rng, w), 0) for _ in range(LANES)]))
    return out


def _qlen_pair(rng, w, n, wide=True, ge=None):
    """(a, b) with a quotient of n bits: la - lb + 1 = n (n = 0: la < lb); ``wide``: a divisor above
    one limb where the width allows; ``ge`` (n = 1): a >= b or a < b."""
    if n == 0:
        lb = rng.randint(33 if wide and w >= 33 else 1, w)
        return nbits(rng, rng.randrange(lb)), nbits(rng, lb)
    hi = w - n + 1
    lb = rng.randint(33 if wide and hi >= 33 else 1, hi)
    la = lb + n - 1
    a, b = nbits(rng, la), nbits(rng, lb)
    if ge is not None and (a >= b) != ge:
        a, b = b, a
        if ge and a < b:
            a = b
    if ge is False and a == b:
        return _qlen_pair(rng, w, n, wide, ge) if lb > 1 else (a, b)
    return a, b


def _div_qlen_waves(w):
    out = []
    ns = [n for n in QLENS if n <= w]
    rng = _rng("qlen", w)
    for n in ns:
        pairs = [_qlen_pair(rng, w, n, wide=i % 4 != 3, ge=(i % 2 == 0) if n == 1 and w > 1 else None) for i in range(LANES)]
        out.append(Wave("div", w, f"div_qlen_{n}", pairs))
    pairs = [_qlen_pair(rng, w, ns[i % len(ns)], wide=i % 3 != 2, ge=(i % 2 == 0) if ns[i % len(ns)] == 1 and w > 1 else None)
             for i in range(LANES)]
    out.append(Wave("div", w, "div_qlen_mixed", pairs))
    return out


def _carry_pair(rng, w, nb):
    """A lane whose remainder has bit 32 nb - 1 set before a shift (chosen with ``loop_carry``)."""
    bits = 32 * nb
    for _ in range(10_000):
        b = rng.choice([top(bits), top(bits) - rng.randrange(1, 1 << 16), nbits(rng, bits), (1 << (bits - 1)) + 1 + rng.getrandbits(20)])
        t = rng.randint(1, w - bits)
        rem = rng.randint(1 << (bits - 1), b - 1)
        a = (rem << t) | rng.getrandbits(t)
        if loop_carry(a, b, nb)[2]:
            return a, b
    raise AssertionError(("no carrying lane", w, nb))


def _div_carry_waves(w):
    out = []
    for nb in (2, 4):
        if w <= 32 * nb:
            continue
        rng = _rng("carry", w, nb)
        pairs = []
        for i in range(LANES):
            if i % 4 == 3:  # a lane without the carry, a divisor of the same class with bit 32 nb - 1 clear
                pairs.append((_dividend(rng, w), nbits(rng, rng.randint(32 * nb // 2 + 1, 32 * nb - 1))))
            else:
                pairs.append(_carry_pair(rng, w, nb))
        out.append(Wave("div", w, f"div_carry_nb{nb}", pairs))
    if w > 32:  # the top bit of the width set in the divisor: one quotient bit, no carry (docstring)
        rng = _rng("topfull", w)
        pairs = []
        for i in range(LANES):
            b = [top(w), 1 << (w - 1), (1 << (w - 1)) + 1][i] if i < 3 else nbits(rng, w)
            a = [top(w), b, b - 1, b + 1, rng.getrandbits(w)][i % 5] & top(w)
            pairs.append((a, b))
        out.append(Wave("div", w, "div_top_full", pairs))
    return out


def one_limb_divisors(w):
    return [d for d in ONE_LIMB_DIVISORS if d <= top(w)]


def _mg_dividend(rng, d, combo, w, p, tries=600):
    """A w-bit dividend whose step by d at limb position p takes ``combo`` = (first, second
    correction): the limbs from p + 3 up are drawn once, the lower ones redrawn until the restated
    step agrees (None if the search gives up)."""
    nl = (w + 31) // 32
    sh = 32 - d.bit_length()
    dn = d << sh
    v = reciprocal(dn)
    low = min(w, 32 * (p + 3))
    a_hi = (rng.getrandbits(w) >> low) << low
    x_hi = a_hi << sh
    rr0 = x_hi >> (32 * nl)
    for i in range(nl - 1, p + 3, -1):
        rr0 = mg_step(rr0, (x_hi >> (32 * i)) & M32, dn, v)[1]
    for _ in range(tries):
        a = a_hi | rng.getrandbits(low)
        x = a << sh
        rr = rr0 if p + 3 < nl else x >> (32 * nl)
        for i in range(min(nl - 1, p + 3), p - 1, -1):
            _, rr, c1, c2, _ = mg_step(rr, (x >> (32 * i)) & M32, dn, v)
        if (int(c1), int(c2)) == combo:
            return a
    return None


def mg_positions(w, combo):
    """The limb positions at which ``combo`` can occur in a w-bit dividend: all of them, less
    ``mg_dropped`` (module docstring)."""
    return [p for p in range((w + 31) // 32) if (w, combo, p) not in mg_dropped(w)]


def mg_dropped(w):
    """{(width, combination, position)} proven impossible: the second correction at the top limb, and
    below a top limb of one bit (w = 32 k + 1) at the next position too."""
    nl = (w + 31) // 32
    out = {(w, c, nl - 1) for c in COMBOS if c[1]}
    if w % 32 == 1 and nl > 1:
        out |= {(w, c, nl - 2) for c in COMBOS if c[1]}
    return out


def _mg_waves(w):
    """Dividends chosen with the restated step: per combination a wave whose lane i takes it at limb
    position i mod (positions); for the second correction the divisor is searched too (few divisors
    leave room for it).  A wave of wrapping candidate sums."""
    out = []
    nl = (w + 31) // 32
    if w < 32:
        return out
    m = top(w)
    for combo in COMBOS:
        rng = _rng("mg", w, combo)
        pos = mg_positions(w, combo)
        if not pos:
            continue
        fixed = one_limb_divisors(w)
        pairs = []
        for i in range(LANES):
            p = pos[i % len(pos)]
            a = None
            if not combo[1] and i < 2 * len(fixed):
                a, d = _mg_dividend(rng, fixed[i % len(fixed)], combo, w, p), fixed[i % len(fixed)]
            for _ in range(200):
                if a is not None:
                    break
                d = nbits(rng, rng.randint(2, 32))
                if combo[1]:  # room for the second correction grows with k = 2^64 - (2^32 + v) dn
                    dn = d << (32 - d.bit_length())
                    if 2 * ((1 << 64) - ((1 << 32) + reciprocal(dn)) * dn) < dn:
                        continue
                a = _mg_dividend(rng, d, combo, w, p)
            for d2 in fixed:  # (below a narrow top limb some combinations need d = 1 or a power of two)
                if a is None:
                    a, d = _mg_dividend(rng, d2, combo, w, p), d2
            if a is None:
                raise AssertionError(("no dividend for", w, combo, p))
            pairs.append((a, d))
        out.append(Wave("div", w, f"div_mg_{combo[0]}{combo[1]}", pairs))
    # the candidate sum v u1 + (u1 + 1) 2^32 + u0 reaches 2^64: with d = 2^32 - 1 - e (v = e + 1) a running
    # remainder d - 1 and u0 >= (e + 1)(e + 2); the remainder d - 1 comes from a limb d - 1 under zero limbs
    if w >= 64:
        rng = _rng("mgwrap", w)
        pairs = []
        for i in range(LANES):
            e = rng.choice([0, 0, 1, 2, rng.randrange(64)])
            d = top(32) - e
            j = i % (nl - 1)
            u0 = rng.randint((e + 1) * (e + 2), M32)
            a = ((d - 1) << (32 * (j + 1))) | (u0 << (32 * j)) | rng.getrandbits(32 * j)
            pairs.append((a & m, d))
        out.append(Wave("div", w, "div_mg_wrap", pairs))
    return out


def _one_limb_waves(w):
    rng = _rng("onelimb", w)
    ds = one_limb_divisors(w)
    hi = min(32, w)
    pairs = []
    for i in range(LANES):
        d = ds[i % len(ds)] if i < 2 * len(ds) or w == 1 else nbits(rng, rng.randint(1, hi))
        k = rng.getrandbits(w) // d
        a = [k * d, k * d + 1 if k * d < top(w) else 1, k * d - 1 if k else d - 1, top(w), rng.getrandbits(w)][i % 5]
        pairs.append((a, d))
    return [Wave("div", w, "div_one_limb", pairs)]


def neg(x, w):
    return (-x) & top(w)


def _signed_waves(w):
    rng = _rng("signed", w)
    m, int_min = top(w), 1 << (w - 1)
    ks = classes_at(w)
    pairs = []
    for i in range(LANES):  # the four sign combinations over magnitudes of every class
        a = nbits(rng, rng.randint(1, max(1, w - 1))) & (m >> 1)
        b = (_divisor(rng, ks[(i // 4) % len(ks)], w) & (m >> 1)) or (1 & (m >> 1))
        pairs.append((neg(a, w) if i & 1 else a, neg(b, w) if i & 2 else b))
    out = [Wave("div", w, "div_signed_combos", pairs)]
    xs = [1 & m, m, int_min, (int_min - 1) & m, (int_min + 1) & m, 3 & m, neg(3, w), rng.getrandbits(w), rng.getrandbits(w) | int_min]
    edges = [(int_min, m), (int_min, 1 & m), (int_min, int_min), (m, m), (m, 1 & m), (1 & m, m)]
    edges += [(x, int_min) for x in xs] + [(x, 0) for x in xs] + [(int_min, x) for x in xs] + [(x, m) for x in xs]
    while len(edges) < LANES:
        edges.append((rng.getrandbits(w) | int_min, rng.getrandbits(w) | (int_min if len(edges) & 1 else 0)))
    out.append(Wave("div", w, "div_signed_edges", edges[:LANES]))
    return out


def _divlit_waves(w):
    """Dividends for the literal divisors (the b column holds the literal the wave was made for; the
    literal-divisor program reads only a): multiples, multiples +- 1, 2^w - 1, dividends chosen
    with the restated step."""
    out = []
    for d in one_limb_divisors(w):
        rng = _rng("divlit", w, d)
        pairs = []
        for i in range(LANES):
            k = rng.getrandbits(w) // d
            if i % 8 < 5 or w < 32:
                a = [k * d, k * d + 1 if k * d < top(w) else 1, k * d - 1 if k else d - 1, top(w), rng.getrandbits(w) | (1 << (w - 1))][i % 8 % 5]
            else:
                combo = COMBOS[(i % 8 - 5 + i // 8) % 4]
                pos = mg_positions(w, combo) or [0]
                a = _mg_dividend(rng, d, combo, w, pos[(i // 8) % len(pos)], tries=300)
                a = rng.getrandbits(w) if a is None else a  # (most literals leave no room for the second correction)
            pairs.append((a, d))
        out.append(Wave("divlit", w, f"div_lit_{d}", pairs))
    return out


def shift_amounts(w):
    cand = [0, 1, 31, 32, 33, w - 1, w, w + 1, 255, 256, 1 << 32, 1 << 255, top(w)]
    out = []
    for s in cand:
        if 0 <= s <= top(w) and s not in out:
            out.append(s)
    return out


def _shift_value(rng, w, sign):
    v = rng.getrandbits(w) if rng.random() < 0.8 else top(w)
    return (v | (1 << (w - 1))) if sign else (v & (top(w) >> 1))


def _shift_waves(w):
    amts = shift_amounts(w)
    rng = _rng("shift", w)
    out = [Wave("shift", w, "shift_mixed", [(_shift_value(rng, w, (i // len(amts)) & 1), amts[i % len(amts)]) for i in range(LANES)])]
    for s in amts:
        label = str(s) if s < 1024 else ("ones" if s == top(w) else f"2p{s.bit_length() - 1}")
        out.append(Wave("shift", w, f"shift_uniform_{label}",
                        [(_shift_value(rng, w, i & 1), s) for i in range(LANES)]))
    return out


def _mul_waves(w):
    rng = _rng("mul", w)
    m = top(w)
    edge = []
    for k in range(1, w + 1):  # 2^k - 1 divides 2^w - 1 when k divides w: products exactly 2^w - 1
        if w % k == 0:
            edge += [(top(k), m // top(k)), (m // top(k), top(k))]
    for i in sorted({1, 2, w // 2, w - 1} & set(range(1, w))):  # exactly 2^w, and 2^w + small
        edge += [(1 << i, 1 << (w - i)), ((1 << i) + 1, 1 << (w - i)), (1 << i, ((1 << (w - i)) + 1) & m),
                 (1 << i, (1 << (w - i)) - 1)]
    edge += [(1, m), (m, 1), (1, rng.getrandbits(w)), (rng.getrandbits(w), 1), (0, m), (m, 0), (m, m), (m, 2 & m)]
    edge = [(a & m, b & m) for a, b in edge][:LANES]
    while len(edge) < LANES:
        edge.append((rng.getrandbits(w), nbits(rng, rng.randint(0, max(1, w // 4)))))
    out = [Wave("mul", w, "mul_edges", edge)]
    h = w // 2
    half = []
    for i in range(LANES):  # operands of exactly w/2 and w/2 + 1 bits: the product straddles 2^w
        la, lb = [(h, h), (h, h + 1), (h + 1, h), (h + 1, h + 1)][i % 4]
        la, lb = min(la, w), min(lb, w)
        a, b = (top(la), top(lb)) if i < 4 else (nbits(rng, la), nbits(rng, lb))
        half.append((a, b))
    out.append(Wave("mul", w, "mul_half", half))
    out.append(Wave("mul", w, "mul_random", [(rng.getrandbits(w), rng.getrandbits(w)) for _ in range(LANES)]))
    return out


@functools.lru_cache(maxsize=None)
def waves(w):
    """Every wave of width w, in a fixed order."""
    out = []
    if w in EXP_WIDTHS:
        out += _exp_waves(w)
    out += _div_class_waves(w) + _div_qlen_waves(w) + _div_carry_waves(w) + _one_limb_waves(w) + _mg_waves(w)
    out += _signed_waves(w) + _divlit_waves(w) + _shift_waves(w) + _mul_waves(w)
    assert len({x.name for x in out}) == len(out)
    return out


def assignments(w, pad=0):
    """The width's waves as (a, b) rows in table order, after ``pad`` filler rows (``pad`` no multiple
    of 64: every wavefront straddles two waves)."""
    rows = [[3, 5 & top(w)]] * pad
    for wave in waves(w):
        rows += [[a, b] for a, b in wave.pairs]
    return rows


# ---- programs --------------------------------------------------------------------------------------

def variables(w):
    return T.BitVecVar(f"wv_a{w}", w), T.BitVecVar(f"wv_b{w}", w)


@functools.lru_cache(maxsize=None)
def operator_terms(w):
    """One program's watched terms over (a, b): every operator of the table, and the literal
    divisors.  {name: term}."""
    a, b = variables(w)
    out = {op: T.bvbin(op, a, b) for op in DIV_OPS + SHIFT_OPS + ("bvmul",)}
    out["bvumul_noovfl"] = T.bvcmp("bvumul_noovfl", a, b)
    if w in EXP_WIDTHS:
        out["bvexp"] = T.bvexp(a, b)
    return out


@functools.lru_cache(maxsize=None)
def literal_terms(w):
    a, _ = variables(w)
    out = {}
    for d in one_limb_divisors(w):
        K = T.BitVecVal(d, w)
        for op in DIV_OPS:
            out[f"{op}_lit{d}"] = T.bvbin(op, a, K)
    return out


def all_terms(w):
    t = dict(operator_terms(w))
    t.update(literal_terms(w))
    return t


# ---- generator form --------------------------------------------------------------------------------
# The search kernels draw operands, so a profile is pinned instead of a lane: a and b are DICT
# coordinates whose entries are one wave's operands (every draw stays inside the profile), and a third
# DICT coordinate k holds thresholds for the root ``fold(xor of the family's results) <u k``, taken
# from the quartiles of the oracle's folds so that between 1/8 and 7/8 of a window satisfy the root
# (asserted under the C port in tests/test_wave_ops_cpu.py).

GEN_WIDTHS = (256, 64, 33)
FAMILY_OPS = {"exp": ("bvexp",), "div": DIV_OPS, "shift": SHIFT_OPS, "mul": ("bvmul", "bvumul_noovfl")}
# the profiles pinned in generator form: (family, wave name); a width keeps those it has
GEN_PROFILES = (
    ("exp", "exp_uniform_L8"), ("exp", "exp_mixed_L33_lane0"), ("exp", "exp_mixed_L64_lane63"),
    ("exp", "exp_uniform_L129"), ("exp", "exp_mixed_L256_lane0"),
    ("div", "div_all_c1"), ("div", "div_all_c2"), ("div", "div_all_c3"), ("div", "div_all_c4"),
    ("div", "div_zero_mix_c2"), ("div", "div_carry_nb2"), ("div", "div_carry_nb4"), ("div", "div_mg_01"),
    ("div", "div_mg_11"), ("div", "div_mg_wrap"), ("div", "div_signed_edges"),
    ("shift", "shift_mixed"), ("mul", "mul_edges"),
)
GEN_COUNT = 4096
SIM_COUNT = 64 * 6
GEN_STARTS = (0, 0x5A5A5A5A5A5A5A5B & ((1 << 63) - 1))  # index 0; an odd 63-bit start


def fold(x):
    """The low 8 bits (or the whole narrower value) of x xor-folded onto itself by literal shifts."""
    w = x.width
    for sft in (128, 64, 32, 16, 8):
        if sft < w:
            x = T.bvbin("bvxor", x, T.bvbin("bvlshr", x, T.BitVecVal(sft, w)))
    return T.extract(7, 0, x) if w > 8 else x


def fold_int(v, w):
    for sft in (128, 64, 32, 16, 8):
        if sft < w:
            v ^= v >> sft
    return v & top(min(8, w))


class GenCase:
    def __init__(self, w, family, wave):
        from mythril_amd import search
        from oracle.bv import OracleModel, evaluate_many

        self.name = f"w{w}_{wave.name}"
        self.width, self.family, self.wave = w, family, wave
        a, b = variables(w)
        ops = operator_terms(w)
        acc = None
        for op in FAMILY_OPS[family]:
            t = ops[op]
            if t.sort == T.BOOL:
                t = T.ite(t, T.BitVecVal(top(w) // 3, w), T.BitVecVal(top(w) // 5 * 2, w))
            acc = t if acc is None else T.bvbin("bvxor", acc, t)
        f = fold(acc)
        k = T.BitVecVar(f"wv_k{w}", f.width)
        self.roots = [T.bvcmp("bvult", f, k)]
        self.a_vals = sorted({x for x, _ in wave.pairs})
        self.b_vals = sorted({y for _, y in wave.pairs})
        rng = _rng("gen", self.name)
        sample = [(rng.choice(self.a_vals), rng.choice(self.b_vals)) for _ in range(256)]
        folds = sorted(fold_int(evaluate_many([acc], OracleModel({a.params[0]: x, b.params[0]: y}))[0], w) for x, y in sample)
        self.k_vals = sorted({min(folds[len(folds) * q // 4] + 1, top(f.width)) for q in (1, 2, 3)})
        self.P, _ = search.prepare(self.roots)
        g = search.default_generator(self.P, roots=self.roots)
        ix = {c.name: c.index for c in self.P.coords}
        g.dict(ix[a.params[0]], self.a_vals)
        g.dict(ix[b.params[0]], self.b_vals)
        g.dict(ix[k.params[0]], self.k_vals)
        self.blob = g.blob()
        self.pb = self.P.to_bytes()
        self.seed = rng.getrandbits(32)


@functools.lru_cache(maxsize=None)
def gen_case_names():
    out = []
    for w in GEN_WIDTHS:
        have = {x.name for x in waves(w)}
        out += [f"w{w}_{name}" for fam, name in GEN_PROFILES if name in have]
    return out


@functools.lru_cache(maxsize=None)
def gen_case(name):
    w, wname = name.split("_", 1)
    w = int(w[1:])
    fam = next(f for f, n in GEN_PROFILES if n == wname)
    return GenCase(w, fam, next(x for x in waves(w) if x.name == wname))


class Program:
    """The width's program (every operator and literal-divisor term watched, root ``true``), its
    waves as SoA rows after ``pad`` filler candidates, and the oracle's watch rows for them."""

    def __init__(self, w, pad=0):
        import numpy as np

        from mythril_amd import ssa
        from oracle.bv import OracleModel, evaluate_many

        self.width, self.pad = w, pad
        self.names = list(all_terms(w))
        terms = [all_terms(w)[n] for n in self.names]
        self.P = ssa.flatten([T.BoolVal(True)], extra=terms)
        entries = [self.P.term_node[t.id] for t in terms]
        self.P.set_watch(entries)
        self.widths = [self.P.node_width[e] for e in entries]
        self.watch_words = sum((x + 31) // 32 for x in self.widths)
        a, b = variables(w)
        col = {a.params[0]: 0, b.params[0]: 1}
        rows = assignments(w, pad)
        self.n = len(rows)
        self.soa = ssa.soa_from_assignments(self.P, [[r[col[c.name]] for c in self.P.coords] for r in rows])
        self.pb = self.P.to_bytes()
        want = np.zeros((self.watch_words, self.n), dtype=np.uint32)
        for i, r in enumerate(rows):
            vals = evaluate_many(terms, OracleModel({a.params[0]: r[0], b.params[0]: r[1]}))
            at = 0
            for v, tw in zip(vals, self.widths):
                for j in range((tw + 31) // 32):
                    want[at + j, i] = (int(v) >> (32 * j)) & M32
                at += (tw + 31) // 32
        self.want = want

    def mismatches(self, watch, limit=6):
        """[(term, wave, lane, got, want)] of the first differing values."""
        import numpy as np

        out = []
        bad = np.argwhere(np.asarray(watch) != self.want)
        seen = set()
        for row, i in bad:
            at = 0
            for name, tw in zip(self.names, self.widths):
                L = (tw + 31) // 32
                if at <= row < at + L:
                    break
                at += L
            if (name, i) in seen:
                continue
            seen.add((name, i))
            k = int(i) - self.pad
            wave = waves(self.width)[k // LANES].name if k >= 0 else "filler"
            got = sum(int(watch[at + j, i]) << (32 * j) for j in range(L))
            want = sum(int(self.want[at + j, i]) << (32 * j) for j in range(L))
            out.append((name, wave, k % LANES, hex(got), hex(want)))
            if len(out) >= limit:
                break
        return out


@functools.lru_cache(maxsize=None)
def program(w, pad=0):
    return Program(w, pad)


# ---- the self-check --------------------------------------------------------------------------------

def tag(wave):
    if wave.tags is None:
        if wave.family == "exp":
            d = exp_decisions([e for _, e in wave.pairs])
            for b, e in wave.pairs:
                assert exp_by_digits(b, e, d, wave.width) == pow(b, e, 1 << wave.width), (wave.name, b, e)
            wave.tags = d
        elif wave.family in ("div", "divlit"):
            wave.tags = div_decisions(wave.pairs, wave.width)
        elif wave.family == "shift":
            wave.tags = {"amounts": shift_decisions(wave.pairs, wave.width)}
        else:
            wave.tags = {}
    return wave.tags


def _steps_are_exact():
    beta = 1 << 6
    for d in range(beta // 2, beta):
        v = reciprocal(d, beta)
        for u1 in range(d):
            for u0 in range(beta):
                q, r, c1, c2, _ = mg_step(u1, u0, d, v, beta)
                assert (q, r) == divmod(u1 * beta + u0, d), (d, u1, u0)
    rng = _rng("mg-random")
    seen = {}
    for _ in range(200_000):
        d = nbits(rng, 32)
        u1, u0 = rng.randrange(d), rng.getrandbits(32)
        q, r, c1, c2, _ = mg_step(u1, u0, d, reciprocal(d))
        assert (q, r) == divmod((u1 << 32) | u0, d)
        seen[(int(c1), int(c2))] = seen.get((int(c1), int(c2)), 0) + 1
    return seen


def check_width(w, summary=None):
    """Tags the width's waves and asserts what the table promises at that width, family by family
    (each assertion carries the width and the wave, value or position that is missing)."""
    summary = {} if summary is None else summary
    if True:
        ws = waves(w)
        summary["waves"] = summary.get("waves", 0) + len(ws)
        by = {x.name: tag(x) for x in ws}
        if w in EXP_WIDTHS:
            ms = set()
            for L in (x for x in EXP_LENGTHS if x <= w):
                live = (L + 31) // 32
                want = {"live": live, "m": L - 32 * (live - 1) if L else 0}
                names = [f"exp_uniform_L{L}"] + ([f"exp_mixed_L{L}_lane0", f"exp_mixed_L{L}_lane63"] if L else [])
                for n in names:
                    t = by[n]
                    assert (t["live"], t["m"]) == (want["live"], want["m"]), (w, n, t)
                    assert t["skip"] % 2 == 0 and t["steps"] == 16 * live - t["skip"] // 2
                    ms.add(t["m"])
                for lane in (0, 63) if L else ():
                    pairs = by and next(x for x in ws if x.name == f"exp_mixed_L{L}_lane{lane}").pairs
                    assert [i for i, (_, e) in enumerate(pairs) if e.bit_length() == L] == [lane]
                    assert {e.bit_length() for _, e in pairs} >= {x for x in EXP_LENGTHS if x < L}
            assert ms >= {0, 1, 2, 3, 4, 7, 8, 9, 30, 31, 32}, ms
            assert {by[n]["skip"] for n in by if n.startswith("exp_")} >= {0, 2, 22, 24, 28, 30}
        div = {n: t for n, t in by.items() if n.startswith("div_") and "lit" not in n}
        ks = classes_at(w)
        for k in ks:
            assert div[f"div_all_c{k}"]["classes"] == [k]
            assert div[f"div_zero_mix_c{k}"]["classes"] == [0, k]
            for j in ks:
                if j != k:
                    for lane in (0, 63):
                        wave = next(x for x in ws if x.name == f"div_c{k}_out_c{j}_lane{lane}")
                        assert [div_class(b) for _, b in wave.pairs] == [j if i == lane else k for i in range(LANES)]
        if w > 32:
            assert {t["nb"] for t in div.values()} >= {{2: 2, 3: 4, 4: 8}[k] for k in ks if k > 1}
            assert {"zero", "one", "loop"} <= {p for t in div.values() for p in t["paths"]}
            assert any(t["paths"] == ["loop", "one"] or t["paths"] == ["loop", "one", "zero"] for t in div.values())
        limbs = (w + 31) // 32
        assert {t["nb_tier"] for t in div.values()} >= {k for k in (1, 2, 4, limbs) if k <= limbs}
        ns = {n for n in QLENS if n <= w}
        assert div["div_qlen_mixed"]["n"] >= ns, (w, div["div_qlen_mixed"]["n"])
        for n in ns:
            assert div[f"div_qlen_{n}"]["n"] == {n}, (w, n, div[f"div_qlen_{n}"]["n"])
        if w > 1:
            assert div["div_qlen_1"]["n1_quotients"] == {0, 1}
        for nb in (2, 4):
            if w > 32 * nb:
                t = div[f"div_carry_nb{nb}"]
                assert t["nb"] == nb and t["nb_tier"] == nb and t["carry"] >= 40 and t["carry_tier"] >= 40, (w, nb, t)
        if w > 32:
            t = div["div_top_full"]
            assert t["carry"] == 0 and t["carry_tier"] == 0 and t["nb"] == {2: 2, 3: 4, 4: 8}[ks[-1]]
        if w >= 32:
            for combo in COMBOS:
                for p in mg_positions(w, combo):
                    assert combo in div[f"div_mg_{combo[0]}{combo[1]}"]["mg"].get(p, ()), (w, combo, p)
            # the dropped (width, combination, position): proven impossible (docstring); no wave takes one
            for _, c, p in mg_dropped(w):
                assert not any(c in t["mg"].get(p, ()) for t in by.values() if "mg" in t), (w, c, p)
            summary.setdefault("mg", {})[w] = {c: sorted(p for p in range(limbs) if any(c in t["mg"].get(p, ()) for t in div.values()))
                                               for c in COMBOS}
        if w >= 64:
            assert div["div_mg_wrap"]["wrap"]
        assert {b for _, b in next(x for x in ws if x.name == "div_one_limb").pairs} >= set(one_limb_divisors(w))
        for d in one_limb_divisors(w):
            pairs = next(x for x in ws if x.name == f"div_lit_{d}").pairs
            assert any(a % d == 0 for a, _ in pairs) and any(a == top(w) for a, _ in pairs)
            assert d == 1 or (any(a % d == 1 for a, _ in pairs) and any(a % d == d - 1 for a, _ in pairs)), (w, d)
        sg = next(x for x in ws if x.name == "div_signed_combos").pairs
        if w > 1:
            assert {(a >> (w - 1), b >> (w - 1)) for a, b in sg} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        se = next(x for x in ws if x.name == "div_signed_edges").pairs
        im, m = 1 << (w - 1), top(w)
        assert {(im, m), (im, 1 & m), (1 & m, im), (m, 0), (3 & m, 0)} <= set(se)
        amts = set(shift_amounts(w))
        assert {s for _, s in next(x for x in ws if x.name == "shift_mixed").pairs} == amts
        assert amts >= {0, w - 1, w & m} and (w <= 32 or (1 << 32) in amts)
        seen = set().union(*(t["amounts"] for n, t in by.items() if n.startswith("shift_")))
        assert seen >= {"below", "at"} | ({"above"} if w > 1 else set()) | ({"high_only"} if w > 32 else set()), (w, seen)
        for n in (x for x in by if x.startswith("shift_uniform")):
            assert {a >> (w - 1) for a, _ in next(x for x in ws if x.name == n).pairs} == {0, 1} or w == 1
        me = next(x for x in ws if x.name == "mul_edges").pairs
        prods = {a * b for a, b in me}
        assert m in prods and (w == 1 or 1 << w in prods) and (w < 4 or any(0 < p - (1 << w) <= 4 for p in prods)), w
        assert any(a == 1 for a, _ in me) and any(b == 1 for _, b in me)
        mh = next(x for x in ws if x.name == "mul_half").pairs
        if w >= 8:
            assert {(a.bit_length(), b.bit_length()) for a, b in mh} == {(w // 2 + i, w // 2 + j) for i in (0, 1) for j in (0, 1)}
            assert {a * b > m for a, b in mh} == {False, True}
    return summary


def self_check():
    """Every width's ``check_width`` and the exactness of the restated step; returns a summary."""
    summary = {"waves": 0, "mg_random": _steps_are_exact()}
    for w in WIDTHS:
        check_width(w, summary)
    return summary
