"""The cases of tests/golden/cavity_reference_cpp_golden.npz (the reference's compiled CPU class, executed: see
tests/golden/make_reference_cavity_cpp_golden.py) in the form the parity tests use, each with the recorded numbers under
"want".  Shared by tests/test_reference_cpp_golden.py (no GPU) and tests/test_gpu_reference_cpp_golden.py; touches neither a
GPU nor the package."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cavity_reference_cpp_golden.npz")
NON_FINITE = ("nan_coordinate", "inf_photon_z")
SENTINEL = -7.25       # what the driver wrote into m_force before the reference's computeForces


@functools.lru_cache(maxsize=None)
def load():
    """(cases, generated_by).  The arrays are read-only: every test sees the same bits."""
    g = np.load(GOLDEN)
    n = g["n"]
    start = np.concatenate([[0], np.cumsum(n)])
    cases = []
    for k in range(len(n)):
        s = slice(int(start[k]), int(start[k + 1]))
        types = str(g["types"][k]).split("|")
        c = {"name": str(g["name"][k]), "position": g["position"][s], "typeid": g["typeid"][s], "tag_high": g["tag_high"][s],
             "charge": g["charge"][s], "image": g["image"][s], "types": types, "box": tuple(float(x) for x in g["box"][k]),
             "L_typeid": types.index("L"),
             "params": dict(zip(("omegac", "couplstr", "phmass"), (float(x) for x in g["params"][k]))),
             "want": {"force": g["force"][s], "energies": g["energies"][k], "dipole": g["dipole"][k],
                      "photon_idx": int(g["photon_idx"][k]), "K": float(g["K"][k])}}
        for a in (c["position"], c["typeid"], c["tag_high"], c["charge"], c["image"], *c["want"].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        cases.append(c)
    return cases, str(g["generated_by"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, finite_case=True):
    """Equal bit patterns (so -0.0 != +0.0).  In a non-finite case: finite entries by bits, the others NaN where NaN and the
    same infinity where infinite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    if finite_case:
        return bool(np.array_equal(bits(got), bits(want)))
    fin = np.isfinite(want)
    return bool(np.array_equal(bits(got[fin]), bits(want[fin])) and np.array_equal(got[~fin], want[~fin], equal_nan=True))
