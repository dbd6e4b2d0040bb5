"""The CPU oracle against the reference's compiled class, executed NOW -- beyond what a committed fixture can hold.

Runs where oracle/_ref/cavity_reference_cpu exists and starts (oracle.build_reference() makes it where a checkout of the
reference is present); anywhere else the module skips and says why.  Never a GPU test.  A few hundred seeded random cases
up to N = 5000 and three long ones, where the order of the sequential sum matters most, each bit for bit against both builds
of oracle/cavity_ref.c."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle
from oracle import reference_run
from reference_cpp_cases import same_bits


def _why_not():
    exe = oracle.REFERENCE_CPU
    if not os.path.exists(exe):
        return f"{os.path.relpath(exe)} is not built (no checkout of the reference on this machine)"
    with tempfile.TemporaryDirectory(prefix="cavref_") as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        open(fin, "wb").close()
        try:
            rc = subprocess.run([exe, fin, fout], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
        except OSError as e:
            return f"{os.path.relpath(exe)} does not start: {e}"
        if rc.returncode != 0:
            return f"{os.path.relpath(exe)} does not start: exit status {rc.returncode}, {rc.stderr.decode(errors='replace')[-200:]}"
    return None


_WHY_NOT = _why_not()
if _WHY_NOT:
    print(f"tests/test_reference_cpp_live.py skipped: {_WHY_NOT}")
pytestmark = pytest.mark.skipif(_WHY_NOT is not None, reason=_WHY_NOT or "")


def _random_case(rng, n, image_scale=None, kind=None):
    l_id = int(rng.integers(0, 3))
    types = ["O", "N"]
    types.insert(l_id, "L")
    others = [t for t in range(3) if t != l_id]
    box = tuple(float(x) for x in rng.uniform(5.0, 60.0, 3))
    tid = rng.choice(others, n).astype(np.int32)
    charge = rng.uniform(-1, 1, n)
    scale = image_scale if image_scale is not None else int(rng.choice([0, 1, 1, 1, 100_000]))
    image = (rng.integers(-3, 4, (n, 3)) * scale).astype(np.int32)
    if kind is None:
        kind = rng.choice(["photon", "photon", "photon", "charged", "several", "none"]) if n else "none"
    if kind != "none":
        at = int(rng.choice([0, n // 2, n - 1, rng.integers(0, n)]))
        tid[at] = l_id
        charge[at] = float(rng.uniform(-8, 8)) if kind == "charged" else 0.0
        if kind == "several":
            tid[rng.integers(0, n, 3)] = l_id
    tag_high = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if rng.uniform() < 0.2 else None
    return {"name": f"{kind}{n}", "position": rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(box), "typeid": tid,
            "tag_high": tag_high, "charge": charge, "image": image, "types": types, "box": box, "L_typeid": l_id,
            "params": {"omegac": float(10.0 ** rng.uniform(-3, 0)), "couplstr": float(10.0 ** rng.uniform(-4, 0)),
                       "phmass": float(rng.choice([1.0, 1.0, 0.37, 1.7]))}}


def _check(cases):
    got = reference_run.run(oracle.REFERENCE_CPU, cases)
    for opt in ("O2", "O3"):
        ref = oracle.RefOracle(opt)
        for c, want in zip(cases, got):
            p = ref.make_params(c["params"]["omegac"], c["params"]["couplstr"], c["params"]["phmass"])
            assert same_bits(p["K"], want["K"]), (opt, c["name"], "K")
            out = ref.compute(reference_run.pos4_of(c), c["charge"], c["image"], c["box"], c["L_typeid"], p)
            assert out["photon_idx"] == want["photon_idx"], (opt, c["name"])
            for key in ("force", "energies") + (("dipole",) if want["photon_idx"] >= 0 else ()):
                assert same_bits(out[key], want[key]), (opt, c["name"], key)


def test_random_cases_bit_for_bit():
    rng = np.random.default_rng(20261020)
    sizes = [int(n) for n in rng.integers(0, 5001, 260)] + [int(n) for n in rng.integers(0, 70, 60)]
    _check([_random_case(rng, n) for n in sizes])


@pytest.mark.parametrize("n,image_scale", [(100_000, 1), (1_000_001, 1), (300_007, 100_000)])
def test_long_cases_bit_for_bit(n, image_scale):
    _check([_random_case(np.random.default_rng(n), n, image_scale, kind="photon")])
