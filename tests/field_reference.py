"""Plain reference and case generator for the per-item self-test of the field and scalar primitives (csrc/selftest_ops.h).

The reference works on Python integers only: a limb vector means sum v_i * 2^ceil(25.5 i); every op's expected result is
computed mod p (or mod L) from that value, and each output must also meet its op's documented output bound (tight, canonical,
the reference layout's normal form).  The cases sit AT each primitive's documented input contract (fe25519.h): every limb at
floor(k T_i), one limb at its maximum, alternating maximum and zero, carry ripples, special values in tight / +2p / +4p form, and
random limbs inside the bound.  Nothing here feeds a primitive limbs outside its contract: what it does there is undefined.

Used by tests/test_device_source_on_host.py (the g++ build of the device headers) and tests/test_gpu_field_bounds.py (the device)."""
import random
import zlib

import numpy as np

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
BITS = [26, 25] * 5
POS = [sum(BITS[:i]) for i in range(10)]                # ceil(25.5 i)
MASK = [(1 << b) - 1 for b in BITS]
T = [1 << b for b in BITS]
P_LIMBS = [(P >> POS[i]) & MASK[i] for i in range(10)]
SQRT_M1 = pow(2, (P - 1) // 4, P)
D = (-121665 * pow(121666, P - 2, P)) % P
REF10_LIMB_MAX = 2**29 - 16                             # fe_from_ref10's input contract, |limb| <= this (include/kyber_ed25519.h)

# op codes: selftest_ops.h fe_selftest_op
OPS = {"fe_mul": 0, "fe_mul_b6": 1, "fe_sq": 2, "fe_sq_b2": 3, "fe_sqn": 4, "fe_add": 5, "fe_addw": 6, "fe_sub": 7, "fe_subw": 8,
       "fe_sub4": 9, "fe_neg": 10, "fe_reduce_weak": 11, "fe_canon": 12, "fe_to_words": 13, "fe_from_words": 14, "fe_is_negative": 15,
       "fe_is_nonzero": 16, "fe_invert": 17, "fe_pow22523": 18, "fe_invert_gcd": 19, "fe_select": 20, "fe_cswap_f": 21, "fe_cswap_g": 22,
       "fe_from_ref10": 23, "fe_to_ref10": 24, "sc_reduce512": 25, "sc_reduce256": 26, "sc_muladd": 27, "sc_recode": 28,
       "sc_pow_mod8L_signed": 29}
SLOW = {"fe_invert", "fe_pow22523", "fe_invert_gcd", "fe_sqn", "sc_pow_mod8L_signed"}
SPECIAL = [0, 1, 2, 3, 19, P - 1, P - 2, P + 1, P + 2, P + 18, 2**255 - 1, 2**255 - 20, (P - 1) // 2, (P + 1) // 2, SQRT_M1, P - SQRT_M1, D,
           P - D, 2**254, 2**26, 2**26 - 1, 2**51, 2**51 - 1, 2**128, 2**255 - 2**230]


def kT(k):
    """the bound "k T": limb_i <= floor(k * T_i)"""
    return [int(k * t) for t in T]


def value(limbs):
    """sum v_i 2^POS_i of one limb vector (signed or unsigned entries)"""
    return sum(int(v) << POS[i] for i, v in enumerate(limbs))


def values(A):
    """values of the rows of an (n, >=10) array of limbs, as Python integers (int32 arrays: signed limbs)"""
    a = A[:, :10].astype(np.int64).astype(object)
    return list((a * np.array([1 << x for x in POS], dtype=object)).sum(axis=1))


def words_value(W, nwords):
    w = W[:, :nwords].astype(object)
    return list((w * np.array([1 << (32 * i) for i in range(nwords)], dtype=object)).sum(axis=1))


def tight_limbs(v):
    """the 255-bit value v (< 2^255, NOT reduced) in canonical limb positions"""
    assert 0 <= v < 2**255
    return [(v >> POS[i]) & MASK[i] for i in range(10)]


def ref10_normal(v):
    """the limbs fe_from_bytes (fe.rs:67-122) yields for the 32 little-endian bytes of v: restated carry by carry"""
    s = v.to_bytes(32, "little")
    ld3 = lambda o: s[o] | (s[o + 1] << 8) | (s[o + 2] << 16)
    ld4 = lambda o: ld3(o) | (s[o + 3] << 24)
    h = [ld4(0), ld3(4) << 6, ld3(7) << 5, ld3(10) << 3, ld3(13) << 2, ld4(16), ld3(20) << 7, ld3(23) << 5, ld3(26) << 4, (ld3(29) & 8388607) << 2]
    c = (h[9] + (1 << 24)) >> 25; h[0] += c * 19; h[9] -= c << 25
    for i in (1, 3, 5, 7):
        c = (h[i] + (1 << 24)) >> 25; h[i + 1] += c; h[i] -= c << 25
    for i in (0, 2, 4, 6, 8):
        c = (h[i] + (1 << 25)) >> 26; h[i + 1] += c; h[i] -= c << 26
    return h


def is_tight(limbs):
    return all(int(limbs[i]) <= int(1.01 * T[i]) for i in range(10))


def is_canonical(limbs):
    return all(int(limbs[i]) <= MASK[i] for i in range(10)) and value(limbs[:10]) < P


def is_ref10_normal(s):
    return all(abs(int(s[i])) <= (2**25 if i % 2 == 0 else 2**24) for i in range(10))


# ---- case generation -------------------------------------------------------------------------------------------------------------------

def limb_cases(rng, mx, n, lo=None):
    """n limb vectors inside the per-limb bounds lo_i <= v_i <= mx_i (lo = 0 by default), structured cases first"""
    lo = lo or [0] * 10
    clip = lambda v: [min(max(int(x), lo[i]), mx[i]) for i, x in enumerate(v)]
    out = [list(mx), list(lo), [0] * 10 if lo == [0] * 10 else clip([0] * 10)]
    for i in range(10):
        out.append(clip([mx[j] if j == i else 0 for j in range(10)]))
        out.append(clip([lo[j] if j == i else 0 for j in range(10)]))
        out.append([mx[j] if j != i else lo[j] for j in range(10)])
    for par in (0, 1):
        out.append([mx[j] if j % 2 == par else lo[j] for j in range(10)])
    for d in (0, 1):
        out.append(clip([MASK[j] + d for j in range(10)]))               # carry ripples: every limb at its mask (+1)
        out.append(clip([MASK[j] + d if j < 9 else 0 for j in range(10)]))
    for v in SPECIAL:
        t = tight_limbs(v % 2**255)
        for k in (0, 2, 4, 8, 16):                                        # the same value plus k p limb-wise
            w = [t[i] + k * P_LIMBS[i] for i in range(10)]
            if all(lo[i] <= w[i] <= mx[i] for i in range(10)):
                out.append(w)
    for _ in range(max(0, n - len(out))):
        r = rng.random()
        if r < 0.6:
            out.append([rng.randint(lo[i], mx[i]) for i in range(10)])
        elif r < 0.9:                                                     # near the maximum in every limb
            out.append([max(lo[i], mx[i] - rng.randrange(1 << rng.randrange(1, 12))) for i in range(10)])
        else:                                                             # near the minimum
            out.append([min(mx[i], lo[i] + rng.randrange(1 << rng.randrange(1, 12))) for i in range(10)])
    return out[:n]


def word_cases(rng, nwords, n, specials=()):
    out = [[0] * nwords, [0xffffffff] * nwords]
    for v in list(specials) + [P, P - 1, P + 1, L, L - 1, L + 1, 2 * L, 8 * L, 8 * L - 1, 2**252 - 1, 2**252, 2**255 - 1, 2**255, 2**256 - 1]:
        if 0 <= v < 2**(32 * nwords):
            out.append([(v >> (32 * i)) & 0xffffffff for i in range(nwords)])
    for pat in (0x88888888, 0x77777777, 0x80000000, 0x7fffffff, 0x0fffffff):
        out.append([pat] * nwords)
    while len(out) < n:
        r = rng.random()
        if r < 0.7:
            out.append([rng.getrandbits(32) for _ in range(nwords)])
        else:
            v = rng.choice([L, P, 2**252]) * rng.randrange(1, 1 << 8) + rng.randrange(-(1 << 20), 1 << 20)
            v %= 2**(32 * nwords)
            out.append([(v >> (32 * i)) & 0xffffffff for i in range(nwords)])
    return out[:n]


def _pad(rows, width=16, dtype=np.uint32):
    A = np.zeros((len(rows), width), dtype=np.int64)
    for i, r in enumerate(rows):
        A[i, :len(r)] = r
    return (A & 0xffffffff).astype(dtype)


def _pairs(rng, fs, gs, n):
    """n (f, g) pairs: the first structured cases of each side against each other, then random pairings"""
    k = min(len(fs), len(gs), 48)
    out = [(fs[i], gs[j]) for i in range(k) for j in range(k)]
    while len(out) < n:
        out.append((fs[rng.randrange(len(fs))], gs[rng.randrange(len(gs))]))
    return out[:n]


# per op: the operand contracts (fe25519.h), as pairs of bounds for two-operand ops
MUL_B6_BOUNDS = [(6.3, 1.0), (6.0, 1.05), (3.0, 2.1), (2.1, 3.0), (1.9, 3.3), (2.5, 2.5), (1.01, 1.01), (6.3 / 3.3, 3.3)]


def cases(op, n=None, seed=0):
    """(A, B, C, PARAM) for n items of op (uint32 arrays: 16 words per item, one parameter per item)"""
    rng = random.Random(zlib.crc32(op.encode()) + 7919 * seed)
    if n is None:
        n = 4096 if op in SLOW else 16384
    z = [[0] * 10]
    if op in ("fe_mul",):
        pr = _pairs(rng, limb_cases(rng, kT(6), n), limb_cases(rng, kT(3.3), n), n)
    elif op == "fe_mul_b6":
        pr = []
        for kf, kg in MUL_B6_BOUNDS:
            m = n // len(MUL_B6_BOUNDS)
            pr += _pairs(rng, limb_cases(rng, kT(kf), m), limb_cases(rng, kT(kg), m), m)
    elif op in ("fe_sq", "fe_sq_b2", "fe_sqn", "fe_invert", "fe_pow22523"):
        k = 3.3 if op == "fe_sq" else 2.5
        pr = [(f, z[0]) for f in limb_cases(rng, kT(k), n)]
    elif op in ("fe_add", "fe_addw"):
        pr = _pairs(rng, limb_cases(rng, [2**31 - 1] * 10, n), limb_cases(rng, [2**31] * 10, n), n)
    elif op in ("fe_sub", "fe_subw"):
        pr = _pairs(rng, limb_cases(rng, kT(30), n), limb_cases(rng, kT(1.99), n), n)
    elif op == "fe_sub4":
        pr = _pairs(rng, limb_cases(rng, kT(28), n), limb_cases(rng, kT(3.99), n), n)
    elif op == "fe_neg":
        pr = [(f, z[0]) for f in limb_cases(rng, kT(1.99), n)]
    elif op == "fe_reduce_weak":
        pr = [(f, z[0]) for f in limb_cases(rng, [2**32 - 1] * 10, n)]
    elif op in ("fe_canon", "fe_to_words", "fe_is_negative", "fe_is_nonzero", "fe_invert_gcd", "fe_to_ref10"):
        pr = [(f, z[0]) for f in limb_cases(rng, [2**31] * 10, n)]
    elif op == "fe_from_words":
        pr = [(f, z[0]) for f in word_cases(rng, 8, n, SPECIAL)]
    elif op in ("fe_select", "fe_cswap_f", "fe_cswap_g"):
        pr = _pairs(rng, limb_cases(rng, [2**32 - 1] * 10, n), limb_cases(rng, [2**32 - 1] * 10, n), n)
    elif op == "fe_from_ref10":
        m = REF10_LIMB_MAX
        pr = [(f, z[0]) for f in limb_cases(rng, [m] * 10, n, lo=[-m] * 10)]
    elif op == "sc_reduce512":
        pr = [(f, z[0]) for f in word_cases(rng, 16, n)]
    elif op in ("sc_reduce256", "sc_recode"):
        pr = [(f, z[0]) for f in word_cases(rng, 8, n)]
    elif op == "sc_muladd":
        a, b, c = word_cases(rng, 8, n), word_cases(rng, 8, n), word_cases(rng, 8, n)
        rng.shuffle(b); rng.shuffle(c)
        A, B, C = _pad(a), _pad(b), _pad(c)
        return A, B, C, np.zeros(n, np.uint32)
    elif op == "sc_pow_mod8L_signed":
        xs, es = [0, 1, 2, 3, 7, 8, 0xffffffff, 0xfffffffe, 0x80000000], [0, 1, 2, 3, 31, 0xffffffff, 0x80000000]
        pairs = [(x, e) for x in xs for e in es]
        while len(pairs) < n:
            pairs.append((rng.getrandbits(rng.choice([3, 8, 16, 32])), rng.getrandbits(rng.choice([1, 3, 5, 8, 16, 32]))))
        A = _pad([[x] for x, _ in pairs[:n]])
        prm = np.array([e for _, e in pairs[:n]], dtype=np.uint32)
        return A, np.zeros_like(A), np.zeros_like(A), prm
    else:
        raise KeyError(op)
    A = _pad([p[0] for p in pr])
    B = _pad([p[1] for p in pr])
    C = np.zeros_like(A)
    if op == "fe_sqn":
        prm = np.array([rng.choice([1, 2, 3, 5, 10]) if rng.random() < 0.8 else rng.choice([20, 50, 100, 255]) for _ in range(len(pr))], dtype=np.uint32)
    elif op in ("fe_select", "fe_cswap_f", "fe_cswap_g"):
        prm = np.array([i & 1 for i in range(len(pr))], dtype=np.uint32)
    else:
        prm = np.zeros(len(pr), np.uint32)
    return A, B, C, prm


# ---- expected results ------------------------------------------------------------------------------------------------------------------

def check(op, A, B, C, prm, out, limit=10):
    """the items of `out` (n x 16 words) that do not hold op's result: list of (item, why), at most `limit`"""
    n = len(out)
    bad = []

    def fail(i, why):
        if len(bad) < limit:
            bad.append((i, why))

    u = out.astype(np.int64)
    if op in ("fe_mul", "fe_mul_b6", "fe_sq", "fe_sq_b2", "fe_sqn", "fe_reduce_weak", "fe_invert", "fe_pow22523", "fe_invert_gcd", "fe_canon",
              "fe_from_ref10", "fe_from_words"):
        fa = values(A.view(np.int32)) if op == "fe_from_ref10" else (words_value(A, 8) if op == "fe_from_words" else values(A))
        fb = values(B)
        got = values(u)
        for i in range(n):
            a = fa[i]
            want = {"fe_mul": lambda: a * fb[i], "fe_mul_b6": lambda: a * fb[i], "fe_sq": lambda: a * a, "fe_sq_b2": lambda: a * a,
                    "fe_sqn": lambda: pow(a, 1 << int(prm[i]), P), "fe_reduce_weak": lambda: a, "fe_canon": lambda: a, "fe_from_ref10": lambda: a,
                    "fe_invert": lambda: pow(a, P - 2, P), "fe_invert_gcd": lambda: pow(a, P - 2, P), "fe_pow22523": lambda: pow(a, (P - 5) // 8, P),
                    "fe_from_words": lambda: a % 2**255}[op]() % P
            if op == "fe_from_words":
                ok = got[i] == a % 2**255 and all(u[i, j] <= MASK[j] for j in range(10))
            elif op == "fe_canon":
                ok = got[i] == want and is_canonical(u[i])
            elif op == "fe_invert_gcd":
                ok = got[i] % P == want and all(u[i, j] <= MASK[j] for j in range(10))
            else:
                ok = got[i] % P == want and is_tight(u[i])
            if not ok or any(u[i, 10:]):
                fail(i, f"{op}: limbs {list(u[i, :10])} = {got[i]:#x}, want {want:#x} mod p")
    elif op in ("fe_add", "fe_addw", "fe_sub", "fe_subw", "fe_sub4", "fe_neg", "fe_select", "fe_cswap_f", "fe_cswap_g"):
        a, b = A[:, :10].astype(np.int64), B[:, :10].astype(np.int64)
        p2, p4 = np.array([2 * x for x in P_LIMBS]), np.array([4 * x for x in P_LIMBS])
        c = prm.astype(np.int64)[:, None] != 0
        want = {"fe_add": lambda: a + b, "fe_addw": lambda: a + b, "fe_sub": lambda: a + p2 - b, "fe_subw": lambda: a + p2 - b,
                "fe_sub4": lambda: a + p4 - b, "fe_neg": lambda: p2 - a, "fe_select": lambda: np.where(c, b, a),
                "fe_cswap_f": lambda: np.where(c, b, a), "fe_cswap_g": lambda: np.where(c, a, b)}[op]()
        assert (want >= 0).all() and (want < 2**32).all(), f"{op}: a case outside the contract"
        for i in np.nonzero((u[:, :10] != want).any(axis=1) | (u[:, 10:] != 0).any(axis=1))[0]:
            fail(int(i), f"{op}: limbs {list(u[i, :10])}, want {list(want[i])}")
        vw, va, vb = values(u), values(A), values(B)
        for i in range(n):                                                      # (the same statement mod p)
            d = {"fe_add": va[i] + vb[i], "fe_addw": va[i] + vb[i], "fe_sub": va[i] - vb[i], "fe_subw": va[i] - vb[i], "fe_sub4": va[i] - vb[i],
                 "fe_neg": -va[i]}.get(op)
            if d is not None and (vw[i] - d) % P:
                fail(i, f"{op}: value")
    elif op in ("fe_to_words", "fe_is_negative", "fe_is_nonzero", "fe_to_ref10"):
        fa = values(A)
        for i in range(n):
            v = fa[i] % P
            if op == "fe_to_words":
                ok = words_value(u[i:i + 1], 8)[0] == v and not u[i, 8:].any()
            elif op == "fe_is_negative":
                ok = int(u[i, 0]) == (v & 1) and not u[i, 1:].any()
            elif op == "fe_is_nonzero":
                ok = int(u[i, 0]) == (v != 0) and not u[i, 1:].any()
            else:
                s = out[i, :10].view(np.int32).astype(np.int64)
                ok = list(s) == ref10_normal(v) and is_ref10_normal(s) and value(s) % P == v and not u[i, 10:].any()
            if not ok:
                fail(i, f"{op}: {list(u[i])} for value {v:#x}")
    elif op in ("sc_reduce512", "sc_reduce256", "sc_muladd"):
        x = words_value(A, 16 if op == "sc_reduce512" else 8)
        y, z = words_value(B, 8), words_value(C, 8)
        got = words_value(u, 8)
        for i in range(n):
            want = (x[i] * y[i] + z[i]) % L if op == "sc_muladd" else x[i] % L
            if got[i] != want or u[i, 8:].any():
                fail(i, f"{op}: {got[i]:#x}, want {want:#x}")
    elif op == "sc_recode":
        x = words_value(A, 8)
        got = words_value(u, 8)
        add = sum(8 << (4 * k) for k in range(63))
        for i in range(n):
            b = x[i] + add
            e63 = b >> 252
            digits = [((got[i] >> (4 * k)) & 15) - 8 for k in range(63)]
            ok = got[i] == b % 2**256 and int(u[i, 8]) == (e63 if e63 <= 8 else 0) and not u[i, 9:].any()
            ok = ok and sum(d << (4 * k) for k, d in enumerate(digits)) + (e63 << 252) == x[i]      # the digits spell the scalar
            if not ok:
                fail(i, f"sc_recode: {list(u[i, :9])} for {x[i]:#x}")
    elif op == "sc_pow_mod8L_signed":
        for i in range(n):
            v0 = pow(int(A[i, 0]), int(prm[i]), 8 * L)
            mag, neg = words_value(u[i:i + 1], 8)[0], int(u[i, 8])
            want = (v0, 0) if v0 < 4 * L else (8 * L - v0, 1)
            v = -mag if neg else mag
            if (mag, neg) != want or (v - pow(int(A[i, 0]), int(prm[i]), L)) % L or u[i, 9:].any():
                fail(i, f"sc_pow_mod8L_signed({int(A[i, 0])}, {int(prm[i])}): {(mag, neg)}, want {want}")
    else:
        raise KeyError(op)
    return bad
