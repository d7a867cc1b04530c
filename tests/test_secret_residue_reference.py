"""The reference the secret-hygiene GPU test searches with (tests/secret_residue.py), checked on its own: its needles are the values the
kernels form (against the oracle and hashlib), and its decoder finds points written in the device's record layouts — so a clean answer on
the GPU means the buffers are clean, not that the search is blind.  CPU only."""
import hashlib
import random

import numpy as np

import secret_residue as R
import synth

L, P = R.L, R.P


def _specials():
    rnd = random.Random(7)
    ints = [1, L - 1, L, L + 1, 2**66 - 1, 2**132, 2**198 - 1, 2**198 + 1, 2**255 - 19, 2**256 - 1, 2**252, 9 * 2**252 - 1]
    out = [v.to_bytes(32, "little") for v in ints]
    for top in (0x7F, 0x80, 0x8F, 0x90, 0xFF):
        out += [bytes(rnd.getrandbits(8) for _ in range(31)) + bytes([top]) for _ in range(2)]
    return out + [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(24)]


def test_quarter_partials_add_up_to_the_product(oracle):
    """sum of the four quarters' multipliers = the integer the reference multiplies B by; P_0 + P_2 and P_1 + P_3 add up to s B"""
    for s in _specials():
        sign, e = R.base64_digits(s)
        assert sign * sum(d << (6 * i) for i, d in enumerate(e)) % L == R.M.effective_scalar(s) % L, s.hex()
        assert all(abs(d) <= 63 and d % 2 == 1 for d in e[:42]), s.hex()
        subs = R.quarter_subscalars(s)
        assert sum(subs[:4]) % L == R.M.effective_scalar(s) % L
        assert (subs[4] + subs[5]) % L == R.M.effective_scalar(s) % L
    sc = np.frombuffer(b"".join(_specials()[:20]), dtype=np.uint8).reshape(-1, 32)
    pts = R.quarter_points(oracle, sc)
    for i in range(sc.shape[0]):
        want = oracle.mul_base(sc[i].tobytes())
        staged = [R.M.decode(pts[i, q].tobytes()) for q in (4, 5)]
        assert R.M.encode(R.M.add(*staged)) == want
        four = [R.M.decode(pts[i, q].tobytes()) for q in range(4)]
        assert R.M.encode(R.M.add(R.M.add(four[0], four[1]), R.M.add(four[2], four[3]))) == want


def test_coop_pieces_add_up_to_the_product(oracle):
    """the four pieces of k_mul_coop (144 / 66 / 31 / 15 bits) add up to |s| P"""
    sc = np.frombuffer(b"".join(_specials()[:12]), dtype=np.uint8).reshape(-1, 32)
    pts = oracle.mul_base_ext_batch(synth.scalars(sc.shape[0], 5, b"point"))
    pieces = R.coop_pieces(oracle, sc, pts)
    for i in range(sc.shape[0]):
        eff = R.M.effective_scalar(sc[i].tobytes())
        assert sum(R.coop_piece_multipliers(sc[i].tobytes())) % L == abs(eff) % L
        total = R.M.IDENT
        for q in range(4):
            total = R.M.add(total, R.M.decode(pieces[i, q].tobytes()))
        want = oracle.mul(R.le32(abs(eff) % L), pts[i])
        assert R.M.encode(total) == want


def _proj_buffer(points, items, rnd, unreduced):
    """a synthetic buffer 4 (store_proj layout): the points at random records, each (x Z : y Z : Z) with a random Z; some limbs unreduced"""
    w = np.zeros((8, items, 4), dtype=np.uint32)
    where = rnd.sample(range(items), len(points))
    for j, ((x, y), i) in enumerate(zip(points, where)):
        z = rnd.randrange(1, P)
        extra = 1 if (unreduced and j % 2) else 0
        f = R.fe_limbs(x * z, extra) + R.fe_limbs(y * z, extra) + R.fe_limbs(z, 0) + [0, 0]
        w[:, i, :] = np.array(f, dtype=np.uint32).reshape(8, 4)
    return w.tobytes() + bytes(256), where


def test_record_decoder_finds_every_planted_point_and_nothing_else(oracle):
    rnd = random.Random(11)
    sc = synth.scalars(40, 77)
    encs = oracle.mul_base_batch(sc)
    pts = [R.M.decode(e.tobytes()) for e in encs[:24]]
    buf, _ = _proj_buffer(pts, 1024, rnd, unreduced=True)
    # records that are not points of the list: noise and a Z = 0 record (skipped, not an error)
    noise = bytearray(buf)
    w = np.frombuffer(noise, dtype=np.uint32, count=1024 * 32).reshape(8, 1024, 4)
    free = [i for i in range(1024) if not w[:, i, :].any()]
    for i in free[:50]:
        w[:, i, :] = np.array([rnd.getrandbits(25) for _ in range(30)] + [0, 0], dtype=np.uint32).reshape(8, 4)
    w[:5, free[50], :] = 7
    found = R.find_points(R.proj_records(bytes(noise)), [e.tobytes() for e in encs])
    assert found == sorted(e.tobytes() for e in encs[:24])
    assert R.find_points(R.proj_records(bytes(noise)), [e.tobytes() for e in encs[24:]]) == []
    # the pieces layout (40-dword records, extended X Z : Y Z : Z^2 : X Y)
    recs = np.zeros((64, 40), dtype=np.uint32)
    for i, (x, y) in enumerate(pts[:10]):
        z = rnd.randrange(1, P)
        recs[3 * i] = R.fe_limbs(x * z * z, i % 2) + R.fe_limbs(y * z * z) + R.fe_limbs(z * z) + R.fe_limbs(x * y * z * z)
    assert R.find_points(R.ext_records(recs.tobytes()), [e.tobytes() for e in encs]) == sorted(e.tobytes() for e in encs[:10])


def test_byte_search_at_any_offset():
    rnd = random.Random(3)
    buf = bytearray(rnd.getrandbits(8) for _ in range(1 << 16))
    needles = [bytes(rnd.getrandbits(8) for _ in range(32)) for _ in range(20)] + [hashlib.sha512(b"x").digest()]
    for j, nd in enumerate(needles[:11]):
        pos = 1000 * j + j % 8 + 1
        buf[pos:pos + len(nd)] = nd
    buf[-32:] = needles[11]
    assert R.find_bytes(bytes(buf), needles) == sorted(needles[:12])
    assert R.find_bytes(bytes(buf), [bytes(32)]) == []                  # all-zero strings are never needles


def test_eddsa_needles_match_hashlib_and_the_oracle(oracle):
    seeds, msgs = synth.scalars(6, 31, b"seed"), synth.messages(6, 31)
    for seed, msg in zip(seeds, msgs):
        seed = seed.tobytes()
        a, prefix, pub = oracle.eddsa_expand(seed)
        d = hashlib.sha512(seed).digest()
        a2, r = R.eddsa_secrets(seed, msg)
        assert a2 == a and prefix == d[32:]
        hr = hashlib.sha512(prefix + msg).digest()
        assert r == oracle.sc_reduce64(hr)
        sig = oracle.eddsa_sign(seed, msg)
        assert sig[:32] == oracle.mul_base(r) and pub == oracle.mul_base(a)
        nd = R.eddsa_needles(seed, msg, sig[:32], pub)
        assert nd[2] == d and nd[3] == d[:32] and nd[4] == d[32:] and nd[5] == a and nd[7] == hr and nd[8] == r
        assert nd[6] == oracle.sc_reduce32(a)
        assert R.le32((R._int(r) + R._int(nd[9])) % L) == sig[32:]          # s = r + h a: the challenge product is the one signing forms
        x, k = seed, synth.scalars(1, 32, b"k")[0].tobytes()
        s2 = oracle.schnorr_sign(x, k, msg)
        sn = R.schnorr_needles(x, k, msg, s2[:32], oracle.mul_base(x))
        assert R.le32((R._int(k) + R._int(sn[-1])) % L) == s2[32:]


def test_pripoly_partials_add_up_to_the_shares(oracle):
    """the segment count of launch_pripoly_eval, and partial values that add up (mod L) to PriPoly::eval at every index"""
    m, t, k = 3, 43, 40
    segs = R.pripoly_segments(m, t, k)
    assert segs == 5
    assert R.pripoly_segments(1, 4096, 65536) == 1 and R.pripoly_segments(1, 4096, 4096) == 16 and R.pripoly_segments(1, 1000, 10) == 64
    coeffs = synth.raw256(m * t, 9, b"coef").reshape(m, t, 32)
    idx = np.arange(k, dtype=np.uint32) * 7 + 3
    parts = R.pripoly_partials(coeffs, idx, segs)
    assert len(parts) == m * k * segs
    for g in range(m):
        for i in range(k):
            acc = sum(R._int(parts[(g * k + i) * segs + s]) for s in range(segs)) % L
            assert R.le32(acc) == oracle.pripoly_eval(coeffs[g], int(idx[i]))
