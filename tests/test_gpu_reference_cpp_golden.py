"""Every route to the cavity-force kernels against the numbers the reference's own compiled CPU class wrote
(tests/golden/cavity_reference_cpp_golden.npz; tests/golden/make_reference_cavity_cpp_golden.py says how).  Run with `-m gpu`
on an MI355X.  NO oracle call is involved: `refout` is the recorded force, energies, dipole and photon index, K is the
recorded K, and the exactly rounded dipole is math.fsum over the fixture's inputs, computed here.

Routes, each taking every finite case with N >= 1:
  - CavityForceComputeHIP on its defaults (single block up to N = 1024, one launch above);
  - the same object with `small_system_max_n` = 0 and the tunables that force one, two and three launches at these small N,
    `reduce_unroll` 1 and 2, `map_nt_store` 0 and 1; the path taken is checked against the dispatcher's mirror of
    tests/test_gpu_dispatch_matrix.py through n_partials and the charged profile slots, as that module does;
  - cavmd_compute_soa with packed strides;
  - all cases (N = 0 and the two non-finite ones included) as one ragged CavityForceBatch.
Bounds: P1 to P5 of parity_support.check_parity at its default tolerance (tests/test_gpu_parity.py is the contract), and
exactly: the photon index, force[:, 3] == 0, molecular z == 0, all four entries of an L-typed particle that is not the photon
== 0, and all-zero output without a photon.  The two non-finite cases follow test_non_finite_inputs_stay_non_finite: what is
non-finite in the reference is non-finite here (the flavour is not part of the contract), what is finite there is finite here
and within the same bounds.

REFUSED lists what a route cannot take, with the status it must return."""
import math

import numpy as np
import pytest
import torch

import cavitymd
from cavitymd import _capi
from oracle import reference_run
from parity_support import check_parity
from reference_cpp_cases import NON_FINITE, load
from test_gpu_dispatch_matrix import TUNABLE_DEFAULTS, Rig, dispatch_mirror, soa_eval

pytestmark = pytest.mark.gpu

CASES, _ = load()
TOL = 1e-10

# (case, route) -> status: N = 0 leaves the object with empty arrays, whose device pointers are null
REFUSED = {("size_0", "hoomd"): _capi.CAVMD_ERR_INVALID_VALUE, ("size_0", "soa"): _capi.CAVMD_ERR_INVALID_VALUE}


def _refout(c):
    """What check_parity reads of an oracle evaluation, from the recorded numbers; dipole_exact from the inputs alone."""
    want = c["want"]
    out = {"force": want["force"], "energies": want["energies"], "dipole": want["dipole"], "photon_idx": want["photon_idx"],
           "params": dict(c["params"], K=want["K"])}
    if want["photon_idx"] >= 0 and c["name"] not in NON_FINITE:
        r = c["position"] + c["image"].astype(np.float64) * np.asarray(c["box"])[None, :]
        t = np.delete(c["charge"][:, None] * r, want["photon_idx"], axis=0)
        out["dipole_exact"] = np.array([math.fsum(t[:, k].tolist()) for k in range(3)])
    return out


REFOUT = {c["name"]: _refout(c) for c in CASES}


def check_structure(c, gpu):
    """The exact part: photon index, .w, molecular z, later L-typed rows, no photon."""
    want, f = c["want"], gpu["force"]
    assert gpu["photon_idx"] == want["photon_idx"], c["name"]
    assert f.shape == want["force"].shape and not np.isnan(f[:, 3]).any()
    assert np.all(f[:, 3] == 0.0), c["name"]
    L = np.nonzero(c["typeid"] == c["L_typeid"])[0]
    assert gpu["n_L"] == len(L), c["name"]
    if want["photon_idx"] < 0:
        assert not f.any() and not np.asarray(gpu["energies"]).any(), c["name"]
        return
    mol = np.arange(len(f)) != want["photon_idx"]
    assert np.all(f[mol, 2] == 0.0), c["name"]
    assert not f[L[1:]].any(), c["name"]


def check_non_finite(c, gpu):
    """Non-finite where the reference is, finite and within P1 to P3 where it is finite."""
    want = c["want"]
    for key in ("dipole", "energies"):
        w, g = np.asarray(want[key]), np.asarray(gpu[key])
        fin = np.isfinite(w)
        assert not np.isfinite(g[~fin]).any() and np.isfinite(g[fin]).all(), (c["name"], key, g, w)
        assert np.all(np.abs(g[fin] - w[fin]) <= TOL * np.abs(w[fin]) + 1e-300), (c["name"], key, g, w)
    w, g = want["force"][:, :3], gpu["force"][:, :3]
    fin = np.isfinite(w)
    assert not np.isfinite(g[~fin]).any() and np.isfinite(g[fin]).all(), c["name"]
    # force scales from the finite components only (a NaN d_x poisons every x force, nothing else)
    p, pidx = REFOUT[c["name"]]["params"], want["photon_idx"]
    q = np.where(np.isfinite(c["position"][pidx]), c["position"][pidx], 0.0) + c["image"][pidx] * np.asarray(c["box"])
    d = np.where(np.isfinite(want["dipole"]), want["dipole"], 0.0)
    S = p["couplstr"] * np.abs(c["charge"]) * (np.abs(q[:2]).max() + p["couplstr"] / p["K"] * np.abs(d[:2]).max())
    S[pidx] = p["K"] * np.abs(q).max() + p["couplstr"] * np.abs(d[:2]).max()
    S3 = np.broadcast_to(S[:, None], w.shape)
    assert np.all(np.abs(g[fin] - w[fin]) <= TOL * S3[fin] + 1e-300), c["name"]


def check(c, gpu):
    check_structure(c, gpu)
    if c["name"] in NON_FINITE:
        check_non_finite(c, gpu)
    else:
        check_parity(c, gpu, REFOUT[c["name"]])


# ---- CavityForceComputeHIP ---------------------------------------------------------------------------------------------
class System:
    """One case on the device (type tags with the recorded high words) and its compute object, profile slots on."""

    def __init__(self, c):
        self.case = c
        pos4 = torch.from_numpy(reference_run.pos4_of(c)).cuda()
        pd = cavitymd.ParticleData(pos4, torch.from_numpy(np.array(c["charge"])).cuda(),
                                   torch.from_numpy(np.array(c["image"])).cuda(), c["types"], c["box"])
        self.sysdef = cavitymd.SystemDefinition(pd)
        p = c["params"]
        self.comp = cavitymd.CavityForceComputeHIP(self.sysdef, p["omegac"], p["couplstr"], p["phmass"])
        self.ws = self.comp.workspace
        self.ws.profile_enable(True)
        self.ws.profile_read()
        self.cus = self.ws.device_info()["compute_units"]

    def run(self, tunables, expect_path):
        full = dict(TUNABLE_DEFAULTS, **tunables)
        for k, v in full.items():
            self.ws.set_tunable(k, v)
        n = len(self.case["charge"])
        m = dispatch_mirror(n, self.cus, full)
        if expect_path is not None:
            assert m["path"] == expect_path, (m["path"], expect_path, n, tunables)
        self.comp.getForceArray().fill_(float("nan"))                    # every entry must be overwritten
        self.comp.compute(0)
        torch.cuda.synchronize()
        res = self.comp.getResult()
        ms, launches = self.ws.profile_read()
        assert launches == 1
        assert res.n_partials == m["n_partials"], ("mirror drifted: grid", res.n_partials, m, n, tunables)
        assert tuple(x > 0.0 for x in ms) == m["launches"], ("mirror drifted: launches", ms, m, n, tunables)
        return {"force": self.comp.getForceArray().cpu().numpy(), "energies": np.array(res.energy[:]),
                "dipole": np.array(res.dipole[:]), "photon_idx": res.photon_idx, "n_L": res.n_photon_typed, "path": m["path"]}


@pytest.fixture(scope="module")
def systems():
    return {c["name"]: System(c) for c in CASES if len(c["charge"]) >= 1}


def _routes():
    out = [("defaults", {}, None)]
    for path, tun in (("single_launch", {"persistent": 1}), ("two_launches", {"persistent": 0, "fused_finalize": 1}),
                      ("three_launches", {"persistent": 0, "fused_finalize": 0})):
        for unroll in (1, 2):
            for nts in (0, 1):
                out.append((f"{path}-unroll{unroll}-nt{nts}",
                            dict(tun, small_system_max_n=0, reduce_unroll=unroll, map_nt_store=nts), path))
    return out


@pytest.mark.parametrize("label,tunables,path", _routes(), ids=[r[0] for r in _routes()])
def test_compute_object_against_the_recorded_reference(systems, label, tunables, path):
    seen = set()
    for c in CASES:
        if (c["name"], "hoomd") in REFUSED:
            continue
        gpu = systems[c["name"]].run(tunables, path)
        seen.add(gpu["path"])
        check(c, gpu)
    # the defaults: one workgroup up to N = 1024, the single launch for 1025 and 2049
    assert seen == ({"single_block", "single_launch"} if path is None else {path})


def test_empty_system_is_refused_by_the_single_routes():
    """N = 0: torch gives empty arrays a null device pointer, and both entry points answer null array pointers with
    CAVMD_ERR_INVALID_VALUE before they look at N.  (The batch takes the empty system: see below.)"""
    c = CASES[[x["name"] for x in CASES].index("size_0")]
    assert len(c["charge"]) == 0
    ws = _capi.Workspace(1)
    pos = torch.empty((0, 4), dtype=torch.float64, device="cuda")
    chg = torch.empty((0,), dtype=torch.float64, device="cuda")
    img = torch.empty((0, 3), dtype=torch.int32, device="cuda")
    frc = torch.empty((0, 4), dtype=torch.float64, device="cuda")
    tid = torch.empty((0,), dtype=torch.int32, device="cuda")
    prm = _capi.make_params(c["params"]["omegac"], c["params"]["couplstr"], c["params"]["phmass"])
    with pytest.raises(_capi.CavmdError) as e:
        ws.compute_hoomd(0, 0, pos.data_ptr(), chg.data_ptr(), img.data_ptr(), c["box"], c["L_typeid"], prm, frc.data_ptr())
    assert e.value.status == REFUSED[("size_0", "hoomd")]
    with pytest.raises(_capi.CavmdError) as e:
        ws.compute_soa(0, 0, (pos.data_ptr(), 24), (tid.data_ptr(), 4), (img.data_ptr(), 12), (chg.data_ptr(), 8), c["box"],
                       c["L_typeid"], prm, (frc.data_ptr(), 24), None)
    assert e.value.status == REFUSED[("size_0", "soa")]


# ---- cavmd_compute_soa, packed strides -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tunables", [{}, {"reduce_unroll": 1, "fused_finalize": 0}, {"reduce_unroll": 2}],
                         ids=["defaults", "unroll1-three_launches", "unroll2"])
def test_strided_entry_point_against_the_recorded_reference(tunables):
    rig = Rig(4096)
    for c in CASES:
        if (c["name"], "soa") in REFUSED:
            continue
        check(c, soa_eval(rig, c, "packed", tunables))             # (soa_eval checks the path taken against its mirror)


# ---- one ragged batch ------------------------------------------------------------------------------------------------------
def test_ragged_batch_against_the_recorded_reference():
    pds = [cavitymd.ParticleData(torch.from_numpy(reference_run.pos4_of(c)).cuda(),
                                 torch.from_numpy(np.array(c["charge"])).cuda(),
                                 torch.from_numpy(np.array(c["image"])).cuda(), c["types"], c["box"]) for c in CASES]
    batch = cavitymd.CavityForceBatch([cavitymd.SystemDefinition(pd) for pd in pds], [c["params"] for c in CASES])
    for f in batch.forces:
        f.fill_(float("nan"))
    batch.compute(0)
    torch.cuda.synchronize()
    res = batch.results()
    assert len(res) == len(CASES) == 37
    for c, f, r in zip(CASES, batch.forces, res):
        assert r.n_particles == len(c["charge"])
        gpu = {"force": f.cpu().numpy(), "energies": np.array(r.energy[:]), "dipole": np.array(r.dipole[:]),
               "photon_idx": r.photon_idx, "n_L": r.n_photon_typed}
        if len(c["charge"]) == 0:
            assert r.photon_idx == -1 and r.n_partials == 0 and not gpu["energies"].any() and gpu["force"].shape == (0, 4)
            continue
        check(c, gpu)
