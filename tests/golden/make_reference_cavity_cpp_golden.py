#!/usr/bin/env python3
"""REFERENCE-EXECUTED fixture for the cavity force: the reference's own compiled CPU class, run.

Run in the BUILD container only (`python tests/golden/make_reference_cavity_cpp_golden.py`); the reference's checkout does not
exist on the GPU box and nothing of it travels: this script writes INPUTS and OUTPUT NUMBERS into
tests/golden/cavity_reference_cpp_golden.npz and nothing else.  Running it again reproduces the file byte for byte (the
archive is written with fixed member dates).

What executes: the reference's src/CavityForceCompute.cc and CavityForceCompute.h, unmodified, compiled by g++ with the flags
of oracle/Makefile's libcavref.so (-O2 -ffp-contract=off, no -march) next to a driver of our own
(oracle/reference_driver/cavity_reference_driver.cc), on top of tests/stubs/hoomd_force_reference, which declares the
HOOMD-blue names the class touches.  Those stand-ins are host containers; the one piece of arithmetic in them is vec3's
component-wise +, -, +=, scalar * vec3 and dot = a.x*b.x + a.y*b.y + a.z*b.z, written from memory of HOOMD-blue's header and
NOT verified against it.  CavityForceCompute.h names pybind11::dict; this container's pybind11 and libpython satisfy it.
The -O0 and -O3 builds of the same sources must write the same bytes, or this script stops.

Recorded per case: the inputs (position, typeid, high word of the type tags, charge, image, box, type names, omegac /
couplstr / phmass) and, from the run, m_force (every entry pre-filled with -7.25 by the driver, so the reference's memset and
every store are visible), the three energies, findPhotonParticle's index, what computeDipoleMoment returns for that index
(for -1, the no-photon cases, it skips nobody; computeForces never gets that far), and K of cavity_force_params.

Cases are small on purpose (the whole file stays below the largest fixture already committed); the sizes sit on both sides
of 64, 256, 512 and 1024 and reach 2049, so that the multi-block kernels see several blocks at either unroll.  Every finite
case is conditioned so that parity at 1e-10 with a SEQUENTIAL sum is satisfiable a priori: 2 N eps sum|c_i r_i| <= 1e-10 |d|
is asserted below.  (Inputs whose sequential sum itself loses eight digits belong to tests/test_reference_cpp_live.py and
to the exact-sum checks of tests/test_gpu_dispatch_matrix.py.)
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "cavity_reference_cpp_golden.npz")

BOX = (31.0, 17.5, 23.25)
PRM = {"omegac": 0.0091, "couplstr": 1e-3, "phmass": 1.0}
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1024, 1025, 2049)


def make_case(name, n, seed, photon_at, l_id=2, box=BOX, image_range=3, image_scale=1, photon_charge=0.0, params=PRM):
    """random_cfg of tests/parity_support.py with the type id of 'L' free: molecules draw from the two other ids."""
    rng = np.random.default_rng(seed)
    types = ["O", "N"]
    types.insert(l_id, "L")
    others = [t for t in range(3) if t != l_id]
    pos = rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(box)
    tid = rng.choice(others, n).astype(np.int32)
    charge = rng.uniform(-1, 1, n)
    image = (rng.integers(-image_range, image_range + 1, (n, 3)) * image_scale).astype(np.int32)
    if photon_at is not None:
        tid[photon_at] = l_id
        charge[photon_at] = photon_charge
    return {"name": name, "position": pos, "typeid": tid, "tag_high": np.zeros(n, dtype=np.uint32), "charge": charge,
            "image": image, "types": types, "box": tuple(box), "params": dict(params)}


def all_cases():
    cases = []
    for k, n in enumerate(SIZES):
        where = None if n == 0 else (0, n // 2, n - 1)[k % 3]
        cases.append(make_case(f"size_{n}", n, 1000 + n, where))
    for l_id in (0, 1, 2):
        for j, place in enumerate(("first", "middle", "last")):
            n = 257 if j == l_id else 65
            cases.append(make_case(f"photon_{place}_L{l_id}", n, 2000 + 10 * l_id + j, (0, n // 2, n - 1)[j], l_id=l_id))
    cases.append(make_case("no_photon", 257, 3001, None))
    c = make_case("three_L", 257, 3002, 5)
    for extra in (100, 256):
        c["typeid"][extra] = 2                                   # keep their (non-zero) charges
    cases.append(c)
    cases.append(make_case("charged_photon", 257, 3003, 128, photon_charge=7.5))
    c = make_case("zero_charges", 65, 3004, 40)
    c["charge"][:] = 0.0
    cases.append(c)
    c = make_case("photon_at_origin", 65, 3005, 64)
    c["position"][64] = 0.0
    c["image"][64] = 0
    cases.append(c)
    cases.append(make_case("phmass_1p7", 65, 3006, 0, params={"omegac": 0.31, "couplstr": 0.27, "phmass": 1.7}))
    cases.append(make_case("cubic_box", 65, 3007, 33, box=(40.0, 40.0, 40.0)))
    cases.append(make_case("images_zero", 257, 3008, 256, image_range=0))
    cases.append(make_case("images_1e5", 513, 3009, 300, image_scale=100_000))
    c = make_case("garbage_tag_high_words", 65, 3010, 31)
    c["tag_high"] = np.random.default_rng(3010).integers(0, 1 << 32, 65, dtype=np.uint64).astype(np.uint32)
    c["tag_high"][:4] = (0xFFFFFFFF, 0x7FF00000, 0xFFF80000, 0x80000000)
    c["tag_high"][31] = 0xDEADBEEF
    cases.append(c)
    c = make_case("nan_coordinate", 65, 3011, 64)
    c["position"][17, 0] = np.nan
    c["charge"][17] = 0.625
    cases.append(c)
    c = make_case("inf_photon_z", 65, 3012, 20)
    c["position"][20, 2] = np.inf
    cases.append(c)
    return cases


NON_FINITE = ("nan_coordinate", "inf_photon_z")


def assert_conditioned(case, res):
    """The sequential sum of this case is within 1e-10 of ANY other order a priori (see the module docstring)."""
    n = len(case["charge"])
    if case["name"] in NON_FINITE or res["photon_idx"] < 0:
        return
    r = case["position"] + case["image"].astype(np.float64) * np.asarray(case["box"])
    t = np.abs(case["charge"][:, None] * r)
    t[res["photon_idx"]] = 0.0
    lhs = 2 * n * np.finfo(float).eps * t.sum(axis=0).max()
    assert lhs <= 1e-10 * np.abs(res["dipole"]).max(), (case["name"], lhs, res["dipole"])


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    import oracle
    from oracle import reference_run

    assert oracle.build_reference(), "needs a checkout of the reference (build container only)"
    cases = all_cases()
    res, raw = reference_run.run(oracle.REFERENCE_CPU, cases, keep_bytes=True)
    for opt in ("_O0", "_O3"):
        _, other = reference_run.run(oracle.REFERENCE_CPU + opt, cases, keep_bytes=True)
        assert other == raw, f"the {opt[1:]} build of the reference writes other bytes than -O2"
    for c, r in zip(cases, res):
        assert_conditioned(c, r)
    n = np.array([len(c["charge"]) for c in cases], dtype=np.int64)
    cat = lambda key, dtype, cols: np.concatenate([np.asarray(c[key], dtype=dtype).reshape(len(c["charge"]), *cols)
                                                   for c in cases])
    arrays = dict(
        generated_by=np.array("reference src/CavityForceCompute.cc + src/CavityForceCompute.h executed through "
                              "oracle/reference_driver/cavity_reference_driver.cc on tests/stubs/hoomd_force_reference; "
                              "g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math (no -march); "
                              "-O0 and -O3 wrote the same bytes"),
        name=np.array([c["name"] for c in cases]),
        n=n,
        types=np.array(["|".join(c["types"]) for c in cases]),
        box=np.array([c["box"] for c in cases], dtype=np.float64),
        params=np.array([[c["params"][k] for k in ("omegac", "couplstr", "phmass")] for c in cases], dtype=np.float64),
        position=cat("position", np.float64, (3,)),
        typeid=cat("typeid", np.int32, ()),
        tag_high=cat("tag_high", np.uint32, ()),
        charge=cat("charge", np.float64, ()),
        image=cat("image", np.int32, (3,)),
        force=np.concatenate([r["force"] for r in res]),
        energies=np.array([r["energies"] for r in res]),
        dipole=np.array([r["dipole"] for r in res]),
        photon_idx=np.array([r["photon_idx"] for r in res], dtype=np.int32),
        K=np.array([r["K"] for r in res]),
    )
    write_npz(OUT, arrays)
    print(f"wrote {OUT}: {len(cases)} cases, {int(n.sum())} particles, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
