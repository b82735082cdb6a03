"""
What the reference's own build returned, pinned for the tests that compare with it.

tests/test_oracle_vs_ref.py, test_sphere.py and test_weno_orders.py compare the oracle bit for bit with the flang build
of the reference's Fortran (oracle/_ref) and with the reference's generated weno.f90.  Both need the reference tree,
which a checkout of this repository does not have.  tests/test_gpu_ref_pins.py holds the device to the same pins for the
cases of tests/ref_cases.py.  For every case those tests run, tests/golden/ref_pins.json holds a
SHA-256 digest of the reference's exact result (float64 bytes, C order, with -0.0 read as +0.0 and every NaN as one NaN:
equal digests <=> np.array_equal(..., equal_nan=True)) and its CFL number as a hex float, so the comparison runs
everywhere.  Where oracle/_ref is present the tests compare with the live build as well.

Regenerate (needs oracle/_ref and the reference tree):
    PCL_WRITE_REF_PINS=1 python -m pytest tests/test_oracle_vs_ref.py tests/test_sphere.py tests/test_weno_orders.py \
        -m "not gpu"
"""
import atexit
import hashlib
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_pins.json")
WRITE = os.environ.get("PCL_WRITE_REF_PINS") == "1"

with open(PATH) as f:
    _pins = json.load(f)


def digest(x):
    """array: 'shape:sha256' of its canonical float64 bytes; list of str: 'n:sha256' of the lines"""
    if isinstance(x, (list, tuple)) and all(isinstance(s, str) for s in x):
        return "%d:%s" % (len(x), hashlib.sha256("\n".join(x).encode()).hexdigest())
    a = np.asarray(x, dtype=np.float64)
    a = np.where(np.isnan(a), np.nan, a + 0.0).astype("<f8")
    return "%s:%s" % ("x".join(str(n) for n in a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def _entry(out, cfl):
    e = {"out": digest(out)}
    if cfl is not None:
        e["cfl"] = float(cfl).hex() if np.ndim(cfl) == 0 else digest(cfl)     # a group of runs: their CFL numbers as a vector
    return e


def check(key, out, cfl=None):
    """`out` (and `cfl`) equal what the reference returned for case `key`"""
    if WRITE:
        return
    assert key in _pins, "no pinned reference result for %s (tests/ref_pins.py: regenerate)" % key
    assert _entry(out, cfl) == _pins[key], key


def record(key, out, cfl=None):
    """the reference's own result for case `key` (kept only when regenerating the pins)"""
    if WRITE:
        _pins[key] = _entry(out, cfl)


@atexit.register
def _save():
    if WRITE:
        with open(PATH, "w") as f:
            json.dump(_pins, f, indent=0, sort_keys=True)
            f.write("\n")
