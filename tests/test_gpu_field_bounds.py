"""Field arithmetic and reference-limb import at their documented bounds, on the device.

* Every field and scalar primitive through the cross-check build's per-lane self-test (k_fe_selftest, selftest_ops.h) on the cases of
  tests/field_reference.py — each at its own input contract: the device output equals the host twin (the g++ build of the same
  headers, tests/hostcheck/device_src_host.cpp) limb for limb, its value equals Python's, and it meets the op's output bound.  The
  device runs code the host never compiles: the KYB_ASM_COLUMNS product columns, the asm doublings, the 64-bit additions.
* The cooperative primitives (coop25519.h) through kyb_diag_coop on loose quads at their stated bounds: limb-exact against the lane
  model tools/coop_model.py, values against Python, and cmul4 against the one-lane fe_mul on the same operands.
* Every entry point that reads reference-layout (`ext`) limbs, fed points whose limbs sit at both ends of the documented bound
  |limb| <= 2^29 - 16 (include/kyber_ed25519.h), through the one-lane and the cooperative import, against the oracle on the
  normalized point; and every `ext` output in exactly the limbs fe.rs:67-122 gives its value."""
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest

import field_reference as R
import synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KATS = json.load(open(os.path.join(HERE, "golden", "kats.json")))
COOP_KEYS = ("coop.max_items", "coop.base_max_items", "coop.ladder_max_items", "coop.ladder_enc_max_items")


@pytest.fixture(scope="module")
def hostlib():
    """the host twin, built by build() (__graft_entry__.build_devsrc_host); missing is a failure, not a skip"""
    import __graft_entry__
    path = __graft_entry__.DEVSRC_HOST_LIB
    assert os.path.exists(path), f"{path} is missing: run `python __graft_entry__.py build` first"
    lib = ctypes.CDLL(path)
    lib.hd_overflows.restype = ctypes.c_long
    lib.hd_fe_selftest.argtypes = [ctypes.c_uint32, ctypes.c_size_t] + [ctypes.c_void_p] * 5
    return lib


@pytest.fixture(scope="module")
def xlib(xengine):
    import kyber_rs_amd
    xengine.device_info()                      # makes the fixture's context current on this thread
    return kyber_rs_amd.load_library(crosscheck=True)


def _run(fn, op, A, B, C, prm):
    arrs = [np.ascontiguousarray(x, dtype=np.uint32) for x in (A, B, C, prm)]
    out = np.zeros((len(A), 16), np.uint32)
    rc = fn(R.OPS[op], len(A), *(x.ctypes.data for x in arrs), out.ctypes.data)
    assert rc in (None, 0), rc
    return out


@pytest.mark.parametrize("op", list(R.OPS))
def test_device_primitive_equals_host_twin_and_python(op, xlib, hostlib):
    A, B, C, prm = R.cases(op)
    base = hostlib.hd_overflows()
    dev = _run(xlib.kyb_diag_fe, op, A, B, C, prm)
    host = _run(hostlib.hd_fe_selftest, op, A, B, C, prm)
    assert hostlib.hd_overflows() == base, f"{op}: a case overflows on the overflow-checked host build"
    diff = np.nonzero((dev != host).any(axis=1))[0]
    assert len(diff) == 0, f"{op}: device != host twin for {len(diff)} items, first {int(diff[0])}: A={list(A[diff[0], :10])} B={list(B[diff[0], :10])} param={int(prm[diff[0]])} dev={list(dev[diff[0]])} host={list(host[diff[0]])}"
    bad = R.check(op, A, B, C, prm, dev)
    assert not bad, bad


# ---- cooperative primitives (kyb_diag_coop) at their stated bounds ----------------------------------------------------------------

def _coop_model():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import coop_model as M
    return M


def _quads(rng, mx, count):
    """count quads of four limb vectors each inside per-limb bounds mx (lanes 10..15 of a row: 0)"""
    vecs = R.limb_cases(rng, mx, 4 * count)
    rng.shuffle(vecs)
    vecs = R.limb_cases(rng, mx, 60)[:60] + vecs                      # the structured cases first, in every row position
    M = _coop_model()
    return [M.quad_from_limbs([vecs[4 * q + r] for r in range(4)]) for q in range(count)]


def test_coop_primitives_at_their_bounds(xlib, xengine):
    """cmul4 (op 0: F <= 1.01T, G <= 4T), csq4 (8: F <= 1.01T), cnorm (1: limbs < 2^31), csub (5: b <= 2T), the layout round trip (7):
    limb-exact against tools/coop_model.py, values against Python; cmul4's value == the one-lane fe_mul's on the same operands;
    the two inversions (2: cinv, 9: the wavefront's safegcd) on tight quads against pow(z, p - 2, p)"""
    M = _coop_model()
    c = M.lane_consts()
    rng = random.Random(31)
    act = (np.arange(64) & 15) < 10

    def run(op, A, B=None):
        A = np.ascontiguousarray(A, dtype=np.uint32)
        B = np.zeros(64, np.uint32) if B is None else np.ascontiguousarray(B, dtype=np.uint32)
        out = np.zeros(64, np.uint32)
        assert xlib.kyb_diag_coop(op, A.ctypes.data, B.ctypes.data, out.ctypes.data) == 0
        return out.astype(np.uint64)

    def same(op, got, want, *ops):
        assert np.array_equal(got[act], np.asarray(want)[act]), (op, [list(o[:10]) for o in ops], list(got[:10]), list(np.asarray(want)[:10]))

    tight, four, two, big = R.kT(1.01), R.kT(4), R.kT(2), [2**31 - 1] * 10
    Fs, Gs = _quads(rng, tight, 48), _quads(rng, four, 48)
    fe_a, fe_b = [], []
    for F, G in zip(Fs, Gs):
        got = run(0, F, G)
        same("cmul4", got, M.cmul4(c, F, G), F, G)
        fv, gv, hv = M.raw_ints_from_quad(F), M.raw_ints_from_quad(G), M.raw_ints_from_quad(got)
        assert [h % R.P for h in hv] == [f * g % R.P for f, g in zip(fv, gv)]
        assert all(R.is_tight(got[16 * r:16 * r + 10]) for r in range(4))
        for r in range(4):
            fe_a.append(list(F[16 * r:16 * r + 10])); fe_b.append(list(G[16 * r:16 * r + 10]))
        got = run(8, F)
        same("csq4", got, M.cmul4(c, F, F), F)
    # cmul4 == fe_mul on the same operands, value for value (the one-lane product on the device, same self-test build)
    A, B = R._pad(fe_b), R._pad(fe_a)                                 # fe_mul(G <= 4T as f <= 6T, F tight as g <= 3.3T)
    one = _run(xlib.kyb_diag_fe, "fe_mul", A, B, np.zeros_like(A), np.zeros(len(A), np.uint32))
    cm = np.concatenate([run(0, F, G).reshape(4, 16)[:, :10] for F, G in zip(Fs, Gs)])
    assert [v % R.P for v in R.values(one)] == [v % R.P for v in R.values(cm)]
    for V in _quads(rng, big, 48):
        same("cnorm", run(1, V), M.cnorm(c, V), V)
        assert [v % R.P for v in M.raw_ints_from_quad(run(1, V))] == [v % R.P for v in M.raw_ints_from_quad(V)]
        same("round trip", run(7, V), V, V)
    for Aq, Bq in zip(_quads(rng, R.kT(25), 48), _quads(rng, two, 48)):
        Bq = np.minimum(Bq, np.array(M.P2 + [0] * 6 + M.P2 + [0] * 6 + M.P2 + [0] * 6 + M.P2 + [0] * 6, dtype=np.uint64))      # b <= 2p limb-wise
        got = run(5, Aq, Bq)
        same("csub", got, M.csub(c, Aq, Bq), Aq, Bq)
    for Z in _quads(rng, tight, 12):
        zv = [v % R.P for v in M.raw_ints_from_quad(Z)]
        assert [v % R.P for v in M.raw_ints_from_quad(run(2, Z))] == [pow(v, R.P - 2, R.P) for v in zv]
        row0 = np.tile(Z[:16], 4)
        assert [v % R.P for v in M.raw_ints_from_quad(run(9, row0))] == [pow(zv[0], R.P - 2, R.P)] * 4
    for vals in ([0, 1, R.P - 1, 2], [R.SQRT_M1, R.D, (R.P - 1) // 2, (R.P + 1) // 2]):
        Z = M.quad_from_ints(c, vals)
        assert M.ints_from_quad(run(2, Z)) == [pow(v, R.P - 2, R.P) for v in vals]


# ---- the reference-limb (ext) boundary ---------------------------------------------------------------------------------------------

EDGE = R.REF10_LIMB_MAX


def _coord_values(ext):
    e = np.asarray(ext, dtype=np.int64)
    return [R.value(e[10 * k:10 * k + 10]) % R.P for k in range(4)]


def _normalize(ext):
    """the point's reference-layout normal form with Z = 1 (what the oracle sees)"""
    x, y, z, _ = _coord_values(ext)
    zi = pow(z, R.P - 2, R.P)
    ax, ay = x * zi % R.P, y * zi % R.P
    return np.array(R.ref10_normal(ax) + R.ref10_normal(ay) + R.ref10_normal(1) + R.ref10_normal(ax * ay % R.P), dtype=np.int32)


Z_EDGES = [[EDGE] * 10, [-EDGE] * 10, [EDGE if i % 2 else -EDGE for i in range(10)], [-EDGE if i % 2 else EDGE for i in range(10)],
           [-EDGE if i % 2 else 0 for i in range(10)], [EDGE if i % 2 == 0 else 0 for i in range(10)]]


def _carry_moves(s, rng):
    """carry-equivalent loose form of one coordinate: s_i -= k 2^bits_i, s_{i+1} += k (x 19 at the wrap), limbs kept inside the bound"""
    s = list(s)
    for i in rng.sample(range(10), 5):
        k = rng.choice([16, 15, -15, -16, 7, -7])
        t = list(s)
        t[i] -= k << R.BITS[i]
        t[(i + 1) % 10] += 19 * k if i == 9 else k
        if all(abs(v) <= EDGE for v in t):
            s = t
    return s


def loose_forms(ext, rng):
    """representations of the point `ext` whose limbs reach both ends of the documented bound: Z = lambda with lambda's limbs at +-EDGE
    (X, Y, T scaled by the same lambda), carry-equivalent moves and limb-wise multiples of p on every coordinate"""
    x, y, z, t = _coord_values(_normalize(ext))
    forms = []
    for zl in Z_EDGES:
        lam = R.value(zl) % R.P
        assert lam != 0
        coords = [R.ref10_normal(x * lam % R.P), R.ref10_normal(y * lam % R.P), zl, R.ref10_normal(t * lam % R.P)]
        forms.append(sum(coords, []))
    for _ in range(2):
        zl = rng.choice(Z_EDGES)
        lam = R.value(zl) % R.P
        coords = [_carry_moves(R.ref10_normal(v * lam % R.P), rng) for v in (x, y)] + [zl, _carry_moves(R.ref10_normal(t * lam % R.P), rng)]
        forms.append(sum(coords, []))
    k = rng.choice([7, -7, 5, -3])
    forms.append(sum([[v + k * R.P_LIMBS[i] for i, v in enumerate(R.ref10_normal(c))] for c in (x, y, 1, t)], []))
    out = np.array(forms, dtype=np.int64)
    assert (np.abs(out) <= EDGE).all()
    for f in out:
        assert _coord_values(_normalize(f))[:2] == [x, y]
    return out.astype(np.int32)


def _points(oracle, n_random):
    """identity, small-order and mixed-order points of the known-answer set, then ordinary ones"""
    pts = []
    for q in KATS["quirk_mul"]:
        if q["ok"]:
            e, ok = oracle.decode(bytes.fromhex(q["point"]))
            if ok and not any(np.array_equal(e, p) for p in pts):
                pts.append(np.asarray(e, dtype=np.int32))
    pts += [np.asarray(oracle.mul_base_ext(bytes(s)), dtype=np.int32) for s in synth.scalars(n_random, 77)]
    return pts


@pytest.fixture()
def both_imports(engine):
    """yields the engine twice: batch (one-lane fe_from_ref10) kernels, then the one-item-per-wavefront kernels (cnorm of word + 16p)"""
    old = [engine.get_option(k) for k in COOP_KEYS]

    def routes():
        for v in (0, 1 << 20):
            for k in COOP_KEYS:
                engine.set_option(k, v)
            yield "coop" if v else "one-lane", engine
    try:
        yield routes
    finally:
        for k, v in zip(COOP_KEYS, old):
            engine.set_option(k, v)


def _assert_eq(what, got, want, loose):
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got, want):
        i = int(np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0][0])
        edge = [int(v) for v in np.asarray(loose).reshape(len(got), -1)[i] if abs(int(v)) == EDGE]
        pytest.fail(f"{what}: item {i} differs from the oracle (limbs at the edge {edge[:4]}...): got {got[i]}, want {want[i]}")


def test_ext_inputs_at_the_documented_limb_bound(both_imports, oracle):
    """every entry point that reads reference limbs, fed loose forms whose limbs sit at +-(2^29 - 16), both imports, == the oracle on the
    normalized point"""
    rng = random.Random(2929)
    pts = _points(oracle, 6)
    loose, norm = [], []
    for p in pts:
        f = loose_forms(p, rng)
        loose += list(f)
        norm += [_normalize(p)] * len(f)
    loose, norm = np.array(loose, np.int32), np.array(norm, np.int32)
    n = len(loose)
    s = synth.scalars(n, 5)
    want_mul = oracle.mul_batch(s, norm)
    want_enc = np.stack([np.frombuffer(oracle.encode(e), np.uint8) for e in norm])
    want_checks = np.array([oracle.point_checks_ext(e) for e in norm], np.uint8)
    perm = np.roll(np.arange(n), 1)
    want_add = np.stack([np.frombuffer(oracle.encode(oracle.add(norm[i], norm[j])), np.uint8) for i, j in zip(range(n), perm)])
    m, t = 4, 5
    sc_lc = synth.scalars(m * t, 6).reshape(m, t, 32)
    lc_pts, lc_norm = loose[:m * t].reshape(m, t, 40), norm[:m * t].reshape(m, t, 40)
    want_lc = np.stack([np.frombuffer(oracle.lincomb(sc_lc[g], lc_norm[g]), np.uint8) for g in range(m)])
    want_sum = []
    for g in range(m):
        acc = lc_norm[g, 0]
        for j in range(1, t):
            acc = oracle.add(acc, lc_norm[g, j])
        want_sum.append(np.frombuffer(oracle.encode(acc), np.uint8))
    idx = np.array([0, 1, 7, 1000], np.uint32)
    want_poly = np.stack([np.frombuffer(oracle.pubpoly_eval(lc_norm[0], int(k)), np.uint8) for k in idx])
    want_multi = np.stack([[np.frombuffer(oracle.pubpoly_eval(lc_norm[g], int(k)), np.uint8) for k in idx] for g in range(m)])
    xs = synth.scalars(8, 8)
    ks = synth.scalars(8, 9)
    msgs = synth.messages(8, 10)
    pubs = oracle.mul_base_ext_batch(xs)
    sigs = oracle.schnorr_sign_batch(xs, ks, msgs)
    pub_loose = np.stack([loose_forms(p, rng)[i % 6] for i, p in enumerate(pubs)])
    for route, eng in both_imports():
        _assert_eq(f"mul [{route}]", eng.mul(s, pts_ext=loose), want_mul, loose)
        _assert_eq(f"mul public [{route}]", eng.mul(s, pts_ext=loose, public=True), want_mul, loose)
        _assert_eq(f"encode [{route}]", eng.encode(loose), want_enc, loose)
        _assert_eq(f"point_checks [{route}]", eng.point_checks(pts_ext=loose), want_checks, loose)
        _assert_eq(f"equal [{route}]", eng.equal(loose, norm), np.ones(n, np.uint8), loose)
        _assert_eq(f"equal, other point [{route}]", eng.equal(loose, norm[perm]), np.array([int(np.array_equal(norm[i], norm[j])) for i, j in zip(range(n), perm)], np.uint8), loose)
        _assert_eq(f"add [{route}]", np.stack([np.frombuffer(oracle.encode(e), np.uint8) for e in eng.add(loose, loose[perm])]), want_add, loose)
        _assert_eq(f"lincomb [{route}]", eng.lincomb(sc_lc, pts_ext=lc_pts), want_lc, lc_pts.reshape(m, -1))
        _assert_eq(f"lincomb public [{route}]", eng.lincomb(sc_lc, pts_ext=lc_pts, public=True), want_lc, lc_pts.reshape(m, -1))
        _assert_eq(f"sum [{route}]", eng.sum_points(lc_pts), np.stack(want_sum), lc_pts.reshape(m, -1))
        _assert_eq(f"pubpoly_eval [{route}]", eng.pubpoly_eval(lc_pts[0], idx), want_poly, np.tile(lc_pts[0].reshape(1, -1), (len(idx), 1)))
        _assert_eq(f"pubpoly_eval_multi [{route}]", eng.pubpoly_eval_multi(lc_pts, np.tile(idx, (m, 1))).reshape(m, -1), want_multi.reshape(m, -1), lc_pts.reshape(m, -1))
        _assert_eq(f"verify_points [{route}]", eng.verify_points(pub_loose, msgs, sigs), np.zeros(8, np.uint8), pub_loose)
        for i in range(0, n, max(1, n // 8)):
            assert eng.defer_get(eng.defer_input(loose[i])) == want_enc[i].tobytes(), f"defer_input [{route}]: item {i}"
        eng.defer_flush()


def test_ext_input_at_the_bound_device_pointers(engine, oracle):
    """the _dev form of the variable-base multiplication on the same loose forms (device-resident limbs)"""
    import torch
    rng = random.Random(2930)
    pts = _points(oracle, 2)
    loose = np.concatenate([loose_forms(p, rng) for p in pts])
    norm = np.stack([_normalize(p) for p in pts for _ in range(len(loose) // len(pts))])
    s = synth.scalars(len(loose), 11)
    dev = torch.device("cuda:0")
    ts, tp = torch.from_numpy(np.ascontiguousarray(s)).to(dev), torch.from_numpy(loose).to(dev)
    out = torch.zeros((len(loose), 32), dtype=torch.uint8, device=dev)
    engine.mul_dev(ts, pts_ext=tp, out_enc=out)
    torch.cuda.synchronize()
    _assert_eq("mul_dev", out.cpu().numpy(), oracle.mul_batch(s, norm), loose)


def test_ext_outputs_are_the_reference_normal_form(both_imports, oracle):
    """a sample of every `ext` output (mul / mul_base want_ext, add, sum, decode): each coordinate's limbs are exactly fe.rs:67-122's
    limbs for its value"""
    pts = np.stack(_points(oracle, 10))
    n = len(pts)
    s = synth.raw256(n, 12)

    def normal(ext, what):
        for e in np.asarray(ext).reshape(-1, 40):
            for k, v in enumerate(_coord_values(e)):
                assert list(e[10 * k:10 * k + 10]) == R.ref10_normal(v), (what, k, list(e))
    for route, eng in both_imports():
        normal(eng.mul(s, pts_ext=pts, want_ext=True)[1], f"mul [{route}]")
        normal(eng.mul_base(s, want_ext=True)[1], f"mul_base [{route}]")
        normal(eng.add(pts, pts[::-1]), f"add [{route}]")
        normal(eng.sum_points(pts[: (n // 4) * 4].reshape(4, -1, 40), want_ext=True)[1], f"sum [{route}]")
        enc = oracle.encode_batch(pts)
        normal(eng.decode(enc)[0], f"decode [{route}]")
