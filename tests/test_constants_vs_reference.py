"""The curve constants this repo DERIVES (tools/gen_constants.py for the HIP side, oracle_init() for
the oracle) equal, by value, the literals the reference carries in
src/group/edwards25519/constants.rs (D :60-63, D2 :65-68, SQRT_M1 :56-58, BASEEXT :70-87,
BASE :89-3738, PRIME / PRIME_ORDER :16-27).  Those literals are stored as numbers in
tests/golden/reference_constants.json (written by tests/golden/make_golden.py)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bigint_model as M  # noqa: E402

BITS = [26, 25] * 5
P = M.P


def limbs_value(nums):
    v, off = 0, 0
    for x, b in zip(nums, BITS):
        v += x << off
        off += b
    return v % P


@pytest.fixture(scope="module")
def ref():
    return json.load(open(os.path.join(HERE, "golden", "reference_constants.json")))


def test_field_constants(ref, oracle):
    import gen_constants as G
    d, d2, sm1 = (limbs_value(ref["field_elements"][k]) for k in ("D", "D2", "SQRT_M1"))
    assert d == M.D == G.D and d2 == (2 * M.D) % P == G.D2 and sm1 == M.SQRT_M1 == G.SQRT_M1
    assert int.from_bytes(oracle.const_bytes(0), "little") == d
    assert int.from_bytes(oracle.const_bytes(1), "little") == d2
    assert int.from_bytes(oracle.const_bytes(2), "little") == sm1
    assert int(ref["prime"]) == P and int(ref["prime_order"]) == M.L


def test_generated_header_is_current():
    import subprocess
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_constants.py"), "--check"]) == 0


def test_baseext_is_the_base_point(ref, oracle):
    X, Y, Z, T = (limbs_value(ref["baseext"][k]) for k in "xyzt")
    zi = pow(Z, P - 2, P)
    assert (X * zi % P, Y * zi % P) == M.B            # Z != 1 in the reference, same point
    assert T * Z % P == X * Y % P
    assert oracle.encode(oracle.base()) == M.encode(M.B)


def test_base_table_values(ref, oracle):
    """BASE[i][j] == (j+1) * 256^i * B as (y+x, y-x, 2dxy): all 256 entries against the oracle's
    regenerated table, and a sample against the big-int model."""
    ents = ref["base"]
    assert len(ents) == 256 and all(len(c) == 10 for e in ents for c in e)
    for n, (a, b, c) in enumerate(ents):
        i, j = divmod(n, 8)
        want = (limbs_value(a), limbs_value(b), limbs_value(c))
        t = oracle.base_table_bytes(i, j)
        got = tuple(int.from_bytes(t[32 * k:32 * k + 32], "little") for k in range(3))
        assert got == want, (i, j)
        if n % 37 == 0:
            x, y = M.mul_int((j + 1) * 256**i, M.B)
            assert want == ((y + x) % P, (y - x) % P, 2 * M.D * x * y % P)
