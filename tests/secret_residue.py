"""What a call with secret inputs must not leave behind in the engine's buffers: a plain reference of every secret-derived intermediate
(Python integers and the CPU oracle, nothing of the engine), a decoder of the projective records the kernels stage in device scratch,
and the searches the secret-hygiene tests run over kyb_diag_scratch_read's copies.

Needles, per item of a call:
  * scalars (32 bytes, little-endian): each secret input as given and mod L; Schnorr: h x mod L; EdDSA: both halves of SHA-512(seed), the
    clamped a, a mod L, the nonce r = SHA-512(prefix || M) mod L and the two unreduced 64-byte hashes; PriPoly::eval cut into segments:
    the partial values k_pripoly_eval_part forms (kernels_verify.hip).
  * points (their 32-byte encodings): the partial points of the fixed base in four window quarters — P_q = (sum of e_i 64^i over the
    windows i of quarter q) B and the two staged sums P_0 + P_2, P_1 + P_3 (k_mul_base64_quarters, kernels_base.hip) — and the four
    pieces of the four-workgroup variable-base product, k_j 2^(b_j) P (k_mul_coop, kernels_coop.hip).
A point is found in a buffer of projective records by normalising every record (one batched inversion) and looking its encoding up;
scalars and encodings are found in byte buffers by a plain substring search."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import bigint_model as M  # noqa: E402

P, L = M.P, M.L
IDENTITY = (1).to_bytes(32, "little")
NTHREADS = max(1, min(16, os.cpu_count() or 1))

# ---- scalars ------------------------------------------------------------------------------------------------------------------


def le32(v: int) -> bytes:
    return (v % 2**256).to_bytes(32, "little")


def _int(b) -> int:
    return int.from_bytes(bytes(b), "little")


def scalar_needles(s) -> list:
    """a secret scalar as given and reduced mod L"""
    s = bytes(s)
    return [s, le32(_int(s) % L)]


def schnorr_needles(x, k, msg: bytes, r_enc: bytes, a_enc: bytes) -> list:
    """schnorr::sign(x, k, msg): both inputs, and h x mod L (s = k + h x)"""
    h = _int(hashlib.sha512(r_enc + a_enc + msg).digest()) % L
    return scalar_needles(x) + scalar_needles(k) + [le32(h * _int(x) % L)]


def eddsa_secrets(seed, msg: bytes):
    """(a, r): the clamped secret scalar and the nonce of EdDSA::sign (eddsa_sig.rs), as 32-byte strings"""
    a, prefix = M.eddsa_expand(bytes(seed))
    return a, le32(_int(hashlib.sha512(prefix + msg).digest()) % L)


def eddsa_needles(seed, msg: bytes, r_enc: bytes, a_enc: bytes) -> list:
    """the seed, SHA-512(seed) and both of its halves, the clamped a and a mod L, SHA-512(prefix || M) and the nonce r = that mod L, and h a mod L
    (r_enc, a_enc: the encodings of r B and a B, which the challenge h hashes)"""
    seed = bytes(seed)
    d = hashlib.sha512(seed).digest()
    a, prefix = M.eddsa_expand(seed)
    hr = hashlib.sha512(prefix + msg).digest()
    r = le32(_int(hr) % L)
    h = _int(hashlib.sha512(r_enc + a_enc + msg).digest()) % L
    return [seed, le32(_int(seed) % L), d, d[:32], d[32:], a, le32(_int(a) % L), hr, r, le32(h * _int(a) % L)]


def pripoly_segments(m: int, t: int, k: int) -> int:
    """the segment count launch_pripoly_eval picks (engine.hip): evaluations x segments fill the chip"""
    evals = m * k
    segs = 1 if evals >= 65536 else 65536 // evals
    segs = max(1, min(segs, t // 8, 64))
    return segs


def pripoly_partials(coeffs, indices, segs: int) -> list:
    """the partial values k_pripoly_eval_part leaves in scratch when segs > 1: segment s of polynomial g at x = index + 1 is
    sum_{j in [s len, min(t, (s + 1) len))} c_j x^j mod L — the segment's Horner value times x^(s len); 32 bytes each, in the kernel's order"""
    c = np.asarray(coeffs, dtype=np.uint8)
    m, t = c.shape[0], c.shape[1]
    ln = (t + segs - 1) // segs
    cs = [[_int(c[g, j]) for j in range(t)] for g in range(m)]
    out = []
    for g in range(m):
        for idx in np.asarray(indices).reshape(-1).tolist():
            x = int(idx) + 1
            for s in range(segs):
                lo, hi = s * ln, min(t, (s + 1) * ln)
                out.append(le32(sum(cs[g][j] * pow(x, j, L) for j in range(lo, hi)) % L))
    return out


# ---- points ------------------------------------------------------------------------------------------------------------------


def base64_digits(s) -> tuple:
    """(sign, e): the signed radix-64 digits the fixed-base kernels add up (ge_scalarmult.h, sc_recode64): the magnitude of the integer
    the reference multiplies by (its top-digit quirk included), made odd by adding L, then e_i = 2 c_i - 63 (i < 42) and e_42 = 2 c_42 + 1
    for the 6-bit groups c_i of (mag >> 1); sum e_i 64^i = mag.  sign = -1: every part is negated."""
    eff = M.effective_scalar(bytes(s))
    sign, mag = (-1, -eff) if eff < 0 else (1, eff)
    if mag % 2 == 0:
        mag = (mag + L) % 2**256
    w = mag >> 1
    e = [2 * ((w >> (6 * i)) & 63) - 63 for i in range(42)] + [2 * (w >> 252) + 1]
    return sign, e


QUARTERS = ((0, 11), (11, 22), (22, 33), (33, 43))      # windows of wavefront q (the last one 33..42)


def quarter_subscalars(s) -> list:
    """the multipliers of B of the partial points P_0 .. P_3, then P_0 + P_2 and P_1 + P_3, as integers mod L"""
    sign, e = base64_digits(s)
    q = [sign * sum(e[i] << (6 * i) for i in range(a, b)) for a, b in QUARTERS]
    return [v % L for v in q + [q[0] + q[2], q[1] + q[3]]]


def quarter_points(orc, scalars) -> np.ndarray:
    """(n, 6, 32) encodings of P_0 .. P_3, P_0 + P_2, P_1 + P_3 for every scalar (the oracle's fixed base, batched)"""
    sc = np.asarray(scalars, dtype=np.uint8).reshape(-1, 32)
    subs = np.frombuffer(b"".join(le32(v) for s in sc for v in quarter_subscalars(s)), dtype=np.uint8).reshape(-1, 32)
    return orc.mul_base_batch(subs, NTHREADS).reshape(-1, 6, 32)


COOP_CUTS = (0, 144, 210, 241, 256)                          # bit ranges of the four pieces (KYB_COOP_CUT1..3, kernels_coop.hip)


def coop_piece_multipliers(s) -> list:
    """k_mul_coop in four workgroups: piece j multiplies P by ((mag >> b_j) mod 2^(len_j)) 2^(b_j), mag = |the integer the reference
    multiplies by| (the sign goes onto the sum, not the pieces); mod L, for points of the prime-order subgroup"""
    eff = M.effective_scalar(bytes(s))
    mag = -eff if eff < 0 else eff
    return [(((mag >> lo) & ((1 << (hi - lo)) - 1)) << lo) % L for lo, hi in zip(COOP_CUTS, COOP_CUTS[1:])]


def coop_pieces(orc, scalars, pts_ext) -> np.ndarray:
    """(n, 4, 32) encodings of the four pieces of every item"""
    sc = np.asarray(scalars, dtype=np.uint8).reshape(-1, 32)
    subs = np.frombuffer(b"".join(le32(v) for s in sc for v in coop_piece_multipliers(s)), dtype=np.uint8).reshape(-1, 32)
    pts = np.repeat(np.asarray(pts_ext, dtype=np.int32).reshape(-1, 40), 4, axis=0)
    return orc.mul_batch(subs, pts, NTHREADS).reshape(-1, 4, 32)


# ---- records of device scratch ------------------------------------------------------------------------------------------------

LIMB_OFFSETS = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)   # unsigned radix-2^25.5 limbs (fe25519.h)


def fe_ints(limbs) -> list:
    """(N, 10) uint32 limbs -> N Python integers (not reduced: limbs may carry more than their 26 / 25 bits)"""
    a = np.asarray(limbs, dtype=np.uint32).astype(np.uint64)
    pairs = (a[:, 0::2] + (a[:, 1::2] << np.uint64(26))).tolist()           # limb pairs: offsets 0, 51, 102, 153, 204
    return [p0 + (p1 << 51) + (p2 << 102) + (p3 << 153) + (p4 << 204) for p0, p1, p2, p3, p4 in pairs]


def fe_limbs(v: int, extra_p: int = 0) -> list:
    """tight limbs of v mod p (plus extra_p times p: an unreduced representation of the same element)"""
    v = v % P + extra_p * P
    out = []
    for k in range(10):
        bits = 26 if k % 2 == 0 else 25
        out.append(v & ((1 << bits) - 1) if k < 9 else v)
        v >>= bits
    assert all(x < 2**32 for x in out)
    return out


def encodings_of(X: list, Y: list, Z: list) -> list:
    """the encodings of the projective points (X : Y : Z), one batched inversion (Montgomery's trick); all-zero records and Z = 0 mod p
    are skipped"""
    keep = [i for i in range(len(Z)) if Z[i] % P != 0]
    if not keep:
        return []
    pre, acc = [], 1
    for i in keep:
        pre.append(acc)
        acc = acc * Z[i] % P
    inv = pow(acc, P - 2, P)
    out = [b""] * len(keep)
    for j in range(len(keep) - 1, -1, -1):
        i = keep[j]
        zi = inv * pre[j] % P
        inv = inv * Z[i] % P
        x, y = X[i] * zi % P, Y[i] * zi % P
        out[j] = (y | ((x & 1) << 255)).to_bytes(32, "little")
    return out


def proj_records(buf: bytes):
    """buffer 4 (per-stream projective staging, store_proj in device_tables.h): uint4 [8 planes][proj_items], 256 bytes behind; a record's
    dwords 0..9 X, 10..19 Y, 20..29 Z -> (X, Y, Z) limb arrays of the records that are not all zero"""
    items = (len(buf) - 256) // 128
    if items <= 0:
        return (np.zeros((0, 10), np.uint32),) * 3
    w = np.frombuffer(buf, dtype=np.uint32, count=items * 32).reshape(8, items, 4).transpose(1, 0, 2).reshape(items, 32)
    w = w[w[:, :30].any(axis=1)]
    return w[:, 0:10], w[:, 10:20], w[:, 20:30]


def ext_records(buf: bytes, words: int = 40):
    """records of `words` dwords, X Y Z in dwords 0..29 (buffer 7: the pieces of k_mul_coop, extended (X Z : Y Z : Z^2 : X Y))"""
    n = len(buf) // (4 * words)
    w = np.frombuffer(buf, dtype=np.uint32, count=n * words).reshape(n, words)
    w = w[w[:, :30].any(axis=1)]
    return w[:, 0:10], w[:, 10:20], w[:, 20:30]


def record_encodings(records) -> list:
    X, Y, Z = records
    return encodings_of(fe_ints(X), fe_ints(Y), fe_ints(Z))


def find_points(records, needles) -> list:
    """the needle encodings that some record of `records` represents"""
    want = set(bytes(n) for n in needles)
    return sorted(want.intersection(record_encodings(records)))


def find_bytes(buf: bytes, needles) -> list:
    """the needles (byte strings of at least 8 bytes, not all zero) found anywhere in buf, at any byte offset"""
    by_prefix: dict = {}
    for nd in needles:
        nd = bytes(nd)
        assert len(nd) >= 8
        if any(nd):
            by_prefix.setdefault(nd[:8], set()).add(nd)
    if not by_prefix or len(buf) < 8:
        return []
    keys = np.frombuffer(b"".join(by_prefix), dtype=np.uint64)
    found = set()
    for o in range(8):
        a = np.frombuffer(buf, dtype=np.uint64, count=(len(buf) - o) // 8, offset=o)
        for j in np.nonzero(np.isin(a, keys))[0].tolist():
            pos = o + 8 * j
            for nd in by_prefix[buf[pos:pos + 8]]:
                if buf[pos:pos + len(nd)] == nd:
                    found.add(nd)
    return sorted(found)
