"""File format of oracle/reference_driver/cavity_reference_driver.cc, and one call that runs it -- TEST INFRASTRUCTURE.

A case is a dict in the form the parity tests use (tests/parity_support.random_cfg): position (N,3), typeid (N,), charge (N,),
image (N,3), types (list of names), box (3), params {omegac, couplstr, phmass}; optionally tag_high (N,) uint32, the high word
of pos.w (HOOMD keeps the type id in the low one).  Nothing here reads the reference: the programs under oracle/_ref/ are built
by oracle.build_reference() where a checkout of it exists.
"""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np


def pos4_of(case) -> np.ndarray:
    """(N,4) float64 as HOOMD lays out pos: x, y, z and the type tag (low word: type id, high word: tag_high or 0)."""
    n = len(case["charge"])
    w = np.asarray(case["typeid"], dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    if case.get("tag_high") is not None:
        w = w | (np.asarray(case["tag_high"], dtype=np.uint64) << np.uint64(32))
    out = np.empty((n, 4), dtype=np.float64)
    out[:, :3] = np.asarray(case["position"], dtype=np.float64).reshape(n, 3)
    out[:, 3] = w.view(np.float64)
    return out


def write_cases(path: str, cases) -> None:
    with open(path, "wb") as f:
        for c in cases:
            n = len(c["charge"])
            f.write(np.array([n, len(c["types"])], dtype="<u4").tobytes())
            for name in c["types"]:
                raw = name.encode("ascii")
                assert 0 < len(raw) < 16
                f.write(raw.ljust(16, b"\0"))
            p = c["params"]
            f.write(np.array(list(c["box"]) + [p["omegac"], p["couplstr"], p["phmass"]], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(pos4_of(c), dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(c["charge"], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(np.asarray(c["image"]).reshape(n, 3), dtype="<i4").tobytes())


def read_results(path: str, cases):
    raw = open(path, "rb").read()
    out, at = [], 0
    for c in cases:
        n = len(c["charge"])
        force = np.frombuffer(raw, dtype="<f8", count=4 * n, offset=at).reshape(n, 4).copy()
        at += 32 * n
        tail = np.frombuffer(raw, dtype="<f8", count=7, offset=at).copy()
        at += 56
        ints = np.frombuffer(raw, dtype="<i4", count=2, offset=at)
        at += 8
        assert int(ints[1]) == n, "result file out of step with the cases"
        out.append({"force": force, "energies": tail[:3], "dipole": tail[3:6], "K": float(tail[6]),
                    "photon_idx": int(ints[0])})
    assert at == len(raw), "result file longer than the cases"
    return out


def run(exe: str, cases, keep_bytes: bool = False):
    """Results of `exe` (one of oracle/_ref/cavity_reference_cpu*) for the cases, in order."""
    with tempfile.TemporaryDirectory(prefix="cavref_") as tmp:
        fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "results.bin")
        write_cases(fin, cases)
        subprocess.run([exe, fin, fout], check=True, stdout=subprocess.DEVNULL)
        res = read_results(fout, cases)
        if keep_bytes:
            with open(fout, "rb") as f:
                return res, f.read()
        return res
