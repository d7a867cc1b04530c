"""Secret hygiene, searched for every secret-DERIVED value (the include/kyber_ed25519.h "secrets" paragraph): after a call with secret inputs —
also after a call whose k-th launch was refused (diag.fail_launch_after = 1, 2, 3) — none of the values tests/secret_residue.py derives from
the call's secrets is left in any of the context's buffers (kyb_diag_scratch_read 0..7): not the scalars and what is computed from them
(reduced forms, expanded EdDSA keys and nonces, h x, segments of a secret polynomial), and not the partial points of the fixed base in
quarters or the pieces of the four-workgroup variable-base product, which are found in the projective records of buffers 4 and 7 by
normalising every record.  Buffer 4 may hold the call's RESULTS (the public s B of mul_base, R and A of signing, the s P of kyb_mul_batch,
deferred s B): they are left out of the needles by name, and two positive controls show that the decoder does find them there.

Every size comes from the routing of engine.hip (base_coop_lim, base_quarters, the signing hand-overs, quad_max_items) applied to the device's
compute units and the engine's options; none is written down here."""
import numpy as np
import pytest

import kyber_rs_amd
import secret_residue as R
import synth

pytestmark = pytest.mark.gpu
SAMPLE = 8192                    # items per scalar array whose partial points are computed (all of them below that; evenly spread above, both ends included)


@pytest.fixture(scope="module")
def image():
    e = kyber_rs_amd.Engine(0, crosscheck=True)
    return e.base_table()


def fresh(image):
    e = kyber_rs_amd.Engine(0, build_table=False, private=True, crosscheck=True)
    e.base_table_import(image)
    return e


def routing(e):
    """the size limits of engine.hip for one host thread (host_load = 1)"""
    cus = e.device_info()["compute_units"]
    opt = e.get_option
    quarters = opt("mul_base.quarters") != 0 and opt("mul_base.radix") == 64
    assert quarters, "the mid-size fixed-base form is off: these sizes would not reach it"
    base_coop_lim = min(opt("coop.base_max_items"), 5 * cus)          # base_coop_lim(): one item per wavefront up to here (COOP_BASE_TO_QUARTERS_PER_CU)
    return {"cus": cus, "base_coop_lim": base_coop_lim, "quarters_max": 128 * cus, "verify_max": opt("coop.verify_max_items"),
            "quad_max": opt("ladder.quad_max_items")}


def _sample(n):
    if n <= SAMPLE:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), np.linspace(0, n - 1, SAMPLE - 512).astype(np.int64)]))


def _quarters(orc, sc):
    """encodings of the partial points of the sampled items of one scalar array"""
    return [p.tobytes() for p in R.quarter_points(orc, sc[_sample(sc.shape[0])]).reshape(-1, 32)]


def _scalars(sc):
    return [nd for s in sc for nd in R.scalar_needles(s)]


class Case:
    def __init__(self, name, call, secrets, points, results, buffers=range(8), secret_results=False):
        """call(engine) runs the call; secrets: byte needles; points: encodings of secret-derived points; results: encodings buffer 4 may hold
        (secret_results: shared secrets, which the staging buffers 0, 1, 2 and the piece records 7 must not hold either)"""
        self.name, self.call, self.buffers = name, call, tuple(buffers)
        self.results = set(results)
        self.secrets = [s for s in secrets if any(s)]
        self.points = sorted(set(points) - self.results - {R.IDENTITY})
        self.cleared_results = sorted(self.results) if secret_results else []


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _blob(msgs):
    off = np.zeros(len(msgs) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return np.frombuffer(b"".join(msgs) + b"\0", dtype=np.uint8).copy(), off


def _cases(orc, rt):
    cus, bcl, qmax = rt["cus"], rt["base_coop_lim"], rt["quarters_max"]
    cases = []
    s_all = synth.scalars(70000, 41)
    k_all = synth.scalars(70000, 42, b"k")
    msgs_all = synth.messages(qmax, 43)

    # ---- fixed base: the results s B are public
    def mul_base_case(n, dev):
        s = s_all[:n]
        res = [e.tobytes() for e in orc.mul_base_batch(s[_sample(n)], R.NTHREADS)]
        if dev:
            def call(e):
                out = _torch().zeros((n, 32), dtype=_torch().uint8, device="cuda")
                e.mul_base_dev(_dev(s), out_enc=out)
                e.sync()
        else:
            def call(e):
                e.mul_base(s)
        return Case(f"mul_base{'_dev' if dev else ''} {n}", call, _scalars(s), _quarters(orc, s), res)
    for n in (1, bcl + 1, qmax, qmax + 1, 70000):
        cases.append(mul_base_case(n, False))
    for n in (bcl + 1, qmax):
        cases.append(mul_base_case(n, True))

    # ---- signing: R = k B and A = x B are public
    first = 3 * bcl // 4 + 1                        # the first size past the one-item kernel (4 n > 3 base_coop_lim)
    seam = 8 * cus + 37                              # odd, the nonce / key seam (item n of the 2 n multiplications) inside a 64-item group
    assert seam % 64 and 2 * seam <= qmax and 4 * seam > 3 * bcl
    sign_sizes = (first, seam, 64 * cus, 64 * cus + 1)
    for n in sign_sizes:
        x, k, msgs = s_all[:n], k_all[:n], msgs_all[:n]
        idx = _sample(n)
        r_enc = orc.mul_base_batch(k[idx], R.NTHREADS)
        a_enc = orc.mul_base_batch(x[idx], R.NTHREADS)
        secrets = _scalars(x) + _scalars(k) + [R.schnorr_needles(x[i], k[i], msgs[i], r_enc[j].tobytes(), a_enc[j].tobytes())[-1] for j, i in enumerate(idx)]
        points = _quarters(orc, k) + _quarters(orc, x)
        res = [e.tobytes() for e in r_enc] + [e.tobytes() for e in a_enc]
        pubs = orc.mul_base_batch(x, R.NTHREADS)
        cases.append(Case(f"schnorr_sign {n}", lambda e, x=x, k=k, m=msgs: e.schnorr_sign(x, k, m), secrets, points, res))
        cases.append(Case(f"schnorr_sign {n} with pubs", lambda e, x=x, k=k, m=msgs, p=pubs: e.schnorr_sign(x, k, m, pubs=p), secrets, points, res))

        def sign_dev(e, x=x, k=k, m=msgs):
            blob, off = _blob(m)
            sig = _torch().zeros((len(m), 64), dtype=_torch().uint8, device="cuda")
            e.sign_dev(_dev(x), _dev(k), _dev(blob), _dev(off.astype(np.int32)), sig)
            e.sync()
        cases.append(Case(f"sign_dev {n}", sign_dev, secrets, points, res))
        # EdDSA: the seeds; the expanded keys a and nonces r and everything on the way to them
        seeds = synth.scalars(n, 44 + n, b"seed")
        ar = [R.eddsa_secrets(sd, m) for sd, m in zip(seeds, msgs)]
        a_arr = np.frombuffer(b"".join(a for a, _ in ar), dtype=np.uint8).reshape(n, 32)
        r_arr = np.frombuffer(b"".join(r for _, r in ar), dtype=np.uint8).reshape(n, 32)
        er, ea = orc.mul_base_batch(r_arr[idx], R.NTHREADS), orc.mul_base_batch(a_arr, R.NTHREADS)
        secrets = [nd for j, i in enumerate(idx) for nd in R.eddsa_needles(seeds[i], msgs[i], er[j].tobytes(), ea[i].tobytes())]
        secrets += _scalars(seeds) + _scalars(a_arr) + _scalars(r_arr)
        points = _quarters(orc, r_arr) + _quarters(orc, a_arr)
        res = [e.tobytes() for e in er] + [ea[i].tobytes() for i in idx]
        cases.append(Case(f"eddsa_sign {n}", lambda e, sd=seeds, m=msgs: e.eddsa_sign(sd, m), secrets, points, res))
        cases.append(Case(f"eddsa_sign {n} with pubs", lambda e, sd=seeds, m=msgs, p=ea: e.eddsa_sign(sd, m, pubs=p), secrets, points, res))

    # ---- variable base (Diffie-Hellman): the products s P are shared secrets the header leaves in buffer 4 (and nowhere else)
    pts = orc.mul_base_ext_batch(synth.scalars(1, 45, b"point"))
    for n in (1, 9 * cus, 64 * cus, 20000, 70000):
        k = k_all[:n]
        p_ext = np.repeat(pts, n, axis=0)
        idx = _sample(n)[:2048]
        res = [e.tobytes() for e in orc.mul_batch(k[idx], p_ext[idx], R.NTHREADS)]
        pieces = [p.tobytes() for p in R.coop_pieces(orc, k[idx], p_ext[idx]).reshape(-1, 32)]
        cases.append(Case(f"mul {n}", lambda e, k=k, p=p_ext: e.mul(k, pts_ext=p), _scalars(k), pieces, res, secret_results=True))

    # ---- PriPoly::eval cut into segments
    m, t, kk = 3, 43, 40
    segs = R.pripoly_segments(m, t, kk)
    assert segs > 1
    coeffs = synth.raw256(m * t, 46, b"coef").reshape(m, t, 32)
    ix = (np.arange(kk, dtype=np.uint32) * 5 + 2)
    cases.append(Case(f"pripoly_eval {m} x {t} at {kk} ({segs} segments)", lambda e: e.pripoly_eval(coeffs, ix),
                      _scalars(coeffs.reshape(-1, 32)) + R.pripoly_partials(coeffs, ix, segs), [], []))

    # ---- a deferred flush of fixed-base nodes: the arena keeps its values (documented); the per-stream scratch does not keep their parts
    nd = 6 * cus
    assert bcl < nd <= qmax
    ds = synth.scalars(nd, 47, b"defer")

    def deferred(e):
        for i in range(nd):
            e.defer_mul_base(ds[i].tobytes())
        e.defer_flush()
    cases.append(Case(f"deferred flush of {nd} defer_mul_base", deferred, _scalars(ds), _quarters(orc, ds),
                      [r.tobytes() for r in orc.mul_base_batch(ds, R.NTHREADS)], buffers=range(4, 8)))
    return cases


def _check(e, case, where):
    """the buffers of e searched for the needles of case; returns the number of buffers checked"""
    checked = 0
    for which in case.buffers:
        buf = e.scratch_read(which)
        if which in (4, 7):
            recs = R.proj_records(buf) if which == 4 else R.ext_records(buf)
            hits = R.find_points(recs, case.points)
            assert not hits, f"{case.name} ({where}): {len(hits)} secret-derived point(s) in buffer {which}, e.g. partial/piece {hits[0].hex()}"
            if which == 7:
                found = R.find_bytes(buf, case.secrets + case.cleared_results)
                assert not found, f"{case.name} ({where}): {len(found)} secret value(s) in buffer {which}"
        else:
            found = R.find_bytes(buf, case.secrets + case.points + (case.cleared_results if which < 3 else []))
            assert not found, f"{case.name} ({where}): {len(found)} secret-derived value(s) in buffer {which}, e.g. {found[0].hex()}"
        checked += 1
    return checked


def test_no_secret_derived_value_stays_behind(image, oracle):
    e0 = fresh(image)
    try:
        rt = routing(e0)
    finally:
        e0.close()
    cases = _cases(oracle, rt)
    checked, failed_calls = 0, 0
    for case in cases:
        for fail_launch in (0, 1, 2, 3):
            e = fresh(image)
            try:
                if fail_launch:
                    e.set_option("diag.fail_launch_after", fail_launch)
                try:
                    case.call(e)
                    failed = False
                except kyber_rs_amd.KyberHipError:
                    failed = True
                e.set_option("diag.fail_launch_after", 0)
                if fail_launch and not failed:
                    break                                  # the call has fewer launches than that
                failed_calls += failed
                checked += _check(e, case, f"launch {fail_launch} refused" if fail_launch else "completed")
            finally:
                e.close()
    print(f"{len(cases)} cases, {failed_calls} failed calls, {checked} buffers searched")
    assert failed_calls >= len(cases)                                  # every call has a first launch to refuse
    assert checked >= sum(len(c.buffers) for c in cases) + 4 * failed_calls


def test_the_decoder_sees_what_buffer_4_holds(image, oracle):
    """positive controls: the documented results of a kyb_mul_batch and of a mid-size mul_base ARE found in buffer 4 by the same decoder"""
    e0 = fresh(image)
    try:
        rt = routing(e0)
    finally:
        e0.close()
    k = synth.scalars(20000, 51, b"k")
    p_ext = np.repeat(oracle.mul_base_ext_batch(synth.scalars(1, 52, b"point")), 20000, axis=0)
    s = synth.scalars(rt["base_coop_lim"] + 1, 53)
    for name, call, want in (
            ("mul 20,000", lambda e: e.mul(k, pts_ext=p_ext), oracle.mul_batch(k[:512], p_ext[:512], R.NTHREADS)),
            (f"mul_base {s.shape[0]}", lambda e: e.mul_base(s), oracle.mul_base_batch(s[:512], R.NTHREADS))):
        e = fresh(image)
        try:
            call(e)
            found = R.find_points(R.proj_records(e.scratch_read(4)), [w.tobytes() for w in want])
        finally:
            e.close()
        assert len(found) == len(want), f"{name}: the decoder found {len(found)} of {len(want)} results in buffer 4"
