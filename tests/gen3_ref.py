"""The GEN3 candidate generator restated from ``include/mythgpu.h`` ("candidate generator (search
mode), format GEN3"), every kind, in arbitrary-precision Python integers: no limb loops, so it
shares no carry, borrow or shift code with the four implementations it is compared with (the C port
``oracle/bveval.c``, the interpreter, the O3 kernel's emitted source, the first tier).  The one
place limbs appear is the raw uniform stream, which the header defines limb by limb.

Also the key and hash helpers the other generator tests use (``test_gen3_spec.py``,
``seeded_ref.py``, the wide-value tests).  Test infrastructure only."""
from __future__ import annotations

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
NONE = 0xFFFFFFFF
NARROW_BITS = 16  # MG_GEN_NARROW_BITS
UNIFORM, RANGE, DICT, MIXED, ALIGNED, FIXED, LAZY = range(7)
ALT_COPY, ALT_DICT, ALT_SMALL, ALT_UNIFORM = range(4)


def fmix64(x):
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def group_key(seed, idx):
    """G of candidate idx."""
    return fmix64((idx >> 6) ^ fmix64(seed ^ 0xBB67AE8584CAA73B))


def lane_key(seed, idx):
    """K of candidate idx."""
    return group_key(seed, idx) ^ fmix64((idx & 63) ^ fmix64(seed ^ 0x6A09E667F3BCC908))


def keys(idx, seed):
    """(K_lo, K_hi, G_lo, G_hi) of candidate idx."""
    G, K = group_key(seed, idx), lane_key(seed, idx)
    return K & M32, K >> 32, G & M32, G >> 32


def salt(c, j):
    return (c * 0x9E3779B9 + j * 0x85EBCA6B + 0x27D4EB2F) & M32


def fin(x):
    x ^= x >> 16
    x = ((x & 0xFFFFFF) * 0x9E3779) & M32
    x ^= x >> 15
    return x


def rnd(k, c, j):
    return (fin(k[0] ^ salt(c, j)) + k[1]) & M32


def rnd_at(seed, i, c, j):
    """rnd(c, j) of candidate i under seed."""
    return rnd(keys(i, seed), c, j)


def wsel(k, c):
    return ((k[2] ^ salt(c, 0xFFFE)) * 0x9E3779B1 + k[3]) & M32


def uniform_raw(k, c, L):
    u = []
    for j in range(L):
        if j < 2:
            u.append(rnd(k, c, j))
        else:
            s = (7 * j + 3) % 31 + 1
            u.append(((((u[j - 1] << 32) | u[j - 2]) >> s) + u[j - 2]) & M32)
    return u


def value(limbs, w):
    return sum(x << (32 * j) for j, x in enumerate(limbs)) & ((1 << w) - 1)


# ---- every kind -------------------------------------------------------------------------------


def split_blob(blob):
    """(specs [n_coords][8], consts) of a generator blob."""
    b = [int(x) for x in blob]
    n, nc = b[1], b[2]
    specs = [b[4 + 8 * c: 12 + 8 * c] for c in range(n)]
    consts = b[4 + 8 * n: 4 + 8 * n + nc]
    return specs, consts


def _const(consts, off, L):
    return value(consts[off:off + L], 32 * L)


def _limbs(w):
    return (w + 31) // 32


def mixed_choice(spec, k, c):
    """(alternative, delta applies) of a MIXED coordinate in the group of key k: both per group."""
    n = spec[2]
    pc = (spec[3] & 0xFFFF) if spec[4] != NONE else 0
    pd = (spec[3] >> 16) if n else 0
    ps = spec[5] & 0xFFFF
    ws = wsel(k, c)
    s = ws >> 16
    if s < pc:
        alt = ALT_COPY
    elif s < pc + pd:
        alt = ALT_DICT
    elif s < pc + pd + ps:
        alt = ALT_SMALL
    else:
        alt = ALT_UNIFORM
    return alt, alt in (ALT_COPY, ALT_DICT) and (ws & 0xFFFF) < (spec[6] & 0xFFFF)


def mixed_delta(k, c):
    """The signed per-lane delta of a COPY / DICT draw (applied when the group's choice says so)."""
    h = rnd(k, c, 0xFFFF)
    d = 1 + (h & 1)
    return -d if (h >> 1) & 1 else d


def clamp_record(spec, consts, w):
    """(lo, span) of a MIXED coordinate's clamp record (span 0 already read as 2^32), or None."""
    if not spec[7]:
        return None
    L = _limbs(w)
    off = spec[7] - 1
    return _const(consts, off, L), consts[off + L] or (1 << 32)


def gen_trace(specs, consts, widths, seed, i):
    """Per coordinate a dict: ``v`` the final value; for MIXED also ``alt``, ``delta`` (the signed
    delta applied, 0 = none), ``depth`` (COPY links walked to reach a generated value), ``pre`` (the
    value before the clamp) and ``clamped``.  ``wrapped``: a RANGE / ALIGNED sum passed 2^w."""
    k = keys(i, seed)
    out = []
    for c, (spec, w) in enumerate(zip(specs, widths)):
        L = _limbs(w)
        mask = (1 << w) - 1
        kind = spec[0] & 0xFF
        t = {}
        if kind == UNIFORM:
            v = value(uniform_raw(k, c, L), w)
        elif kind == RANGE:
            r = rnd(k, c, 0)
            v = _const(consts, spec[1], L) + ((r * spec[2]) >> 32 if spec[2] else r)
            t["wrapped"] = v > mask
        elif kind == DICT:
            e = ((rnd(k, c, 0xFFFF) >> 16) * spec[2]) >> 16
            v = _const(consts, spec[1] + e * L, L)
        elif kind == ALIGNED:
            r = rnd(k, c, 0)
            m = (r * spec[3]) >> 32 if spec[3] else r
            v = _const(consts, spec[1], L) + (m << spec[2])
            t["wrapped"] = v > mask
        elif kind == FIXED:
            v = _const(consts, spec[1], L)
        elif kind == LAZY:
            v = 0  # never generated
        elif kind == MIXED:
            alt, with_delta = mixed_choice(spec, k, c)
            h = rnd(k, c, 0xFFFF)
            small = (1 << min(w, spec[5] >> 16)) - 1
            t.update(alt=alt, delta=0, depth=0)
            if alt == ALT_COPY:
                v = out[spec[4]]["v"]
                t["depth"] = 1 + out[spec[4]].get("depth", 0)
            elif alt == ALT_DICT:
                e = ((h >> 16) * spec[2]) >> 16
                v = _const(consts, spec[1] + e * L, L)
            else:
                v = (h & 0xFFFF) if w <= NARROW_BITS else value(uniform_raw(k, c, L), 32 * L)
                if alt == ALT_SMALL:
                    v &= small
            if with_delta:
                t["delta"] = mixed_delta(k, c)
                v = (v + t["delta"]) % (1 << (32 * L))
            v &= mask
            t["pre"] = v
            cl = clamp_record(spec, consts, w)
            t["clamped"] = False
            if cl is not None and not (cl[0] <= v < cl[0] + cl[1]):
                v = cl[0] + (((v & M32) * cl[1]) >> 32)
                t["clamped"] = True
        else:
            raise ValueError(f"GEN3 kind {kind}")
        v &= mask
        if spec[0] >> 8:  # the fixed-bit record, last
            off = (spec[0] >> 8) - 1
            v = (v & ~_const(consts, off, L)) | _const(consts, off + L, L)
        t["v"] = v
        out.append(t)
    return out


def gen_values(specs, consts, widths, seed, i):
    """The value of every coordinate of candidate i under seed."""
    return [t["v"] for t in gen_trace(specs, consts, widths, seed, i)]


def soa_rows(values, widths):
    """The SoA limb rows (mg_eval layout: coordinates in order, limb 0 first) of one candidate."""
    return [(v >> (32 * j)) & M32 for v, w in zip(values, widths) for j in range(_limbs(w))]
