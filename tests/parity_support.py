"""What the parity tests of the cavity force share (tests/test_gpu_parity.py, tests/test_gpu_dispatch_matrix.py,
tests/test_gpu_batch.py, tests/test_hoomd_marshalling.py): one evaluation on the GPU and one by the CPU oracle, the force scales
of the tolerances, the parity check itself (P1 to P5 of tests/test_gpu_parity.py) and the random configuration they start
from.  Importing this module touches neither a GPU nor the package: cavitymd is imported where it is used, so that the module
loads wherever tests/ is on the path."""
import numpy as np
import torch


def to_device(cfg, device="cuda"):
    import cavitymd
    pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                           cfg["box"], device=device)
    return cavitymd.SystemDefinition(pd)


def gpu_eval(cfg, tunables=None):
    import cavitymd
    sysdef = to_device(cfg)
    p = cfg["params"]
    comp = cavitymd.CavityForceComputeHIP(sysdef, p["omegac"], p["couplstr"], p["phmass"])
    for k, v in (tunables or {}).items():
        comp.workspace.set_tunable(k, v)
    comp.getForceArray().fill_(float("nan"))  # every entry must be overwritten
    comp.compute(0)
    torch.cuda.synchronize()
    res = comp.getResult()
    return {"force": comp.getForceArray().cpu().numpy(), "energies": np.array(comp.getEnergies()),
            "dipole": np.array(res.dipole[:]), "dipole_lo": np.array(res.dipole_lo[:]), "photon_idx": res.photon_idx,
            "n_L": res.n_photon_typed, "q": np.array(res.q[:]), "Dq": np.array(res.Dq[:]), "result": res, "comp": comp}


def ref_eval(ref, oracle_mod, cfg):
    p = ref.make_params(cfg["params"]["omegac"], cfg["params"]["couplstr"], cfg["params"]["phmass"])
    pos4 = oracle_mod.pack_pos(cfg["position"], cfg["typeid"])
    out = ref.compute(pos4, cfg["charge"], cfg["image"], cfg["box"], cfg["L_typeid"], p)
    out["params"] = p
    out["pos4"] = pos4
    if out["photon_idx"] >= 0:
        hi, lo = ref.dipole_exact(pos4, cfg["charge"], cfg["image"], cfg["box"], out["photon_idx"])
        out["dipole_exact"] = hi
    return out


def force_scales(cfg, refout):
    p = refout["params"]
    g, K = p["couplstr"], p["K"]
    pidx = refout["photon_idx"]
    box = np.asarray(cfg["box"])
    q = cfg["position"][pidx] + cfg["image"][pidx] * box
    d = refout["dipole"]
    s_mol = g * np.abs(cfg["charge"]) * (np.abs(q[:2]).max() + (g / K) * np.abs(d[:2]).max())
    s_L = K * np.abs(q).max() + g * np.abs(d[:2]).max()
    S = s_mol.copy()
    S[pidx] = s_L
    return S


def forces_from_dipole(cfg, refout, d):
    """Forces the reference formulas give for a prescribed dipole (used with the exactly rounded one)."""
    p = refout["params"]
    g, K = p["couplstr"], p["K"]
    pidx = refout["photon_idx"]
    box = np.asarray(cfg["box"])
    q = cfg["position"][pidx] + cfg["image"][pidx] * box
    Dq = np.array([q[0] + (g / K) * d[0], q[1] + (g / K) * d[1]])
    F = np.zeros((len(cfg["charge"]), 4))
    s = (-g) * cfg["charge"]
    F[:, 0] = s * Dq[0]
    F[:, 1] = s * Dq[1]
    F[cfg["typeid"] == cfg["L_typeid"]] = 0.0
    F[pidx, :3] = [-K * q[0] - g * d[0], -K * q[1] - g * d[1], -K * q[2] - g * 0.0]
    return F


def check_parity(cfg, gpu, refout, tol=1e-10):
    assert gpu["photon_idx"] == refout["photon_idx"]
    assert not np.isnan(gpu["force"]).any(), "force entries left unwritten"
    if refout["photon_idx"] < 0:
        assert not gpu["force"].any() and not gpu["energies"].any()
        return {}
    d_ref, d_gpu, d_exact = refout["dipole"], gpu["dipole"], refout["dipole_exact"]
    # P1
    assert np.abs(d_gpu - d_ref).max() <= tol * np.abs(d_ref).max() + 1e-300
    # GPU dipole is the correctly rounded sum to within 2 ulp
    assert np.all(np.abs(d_gpu - d_exact) <= 2 * np.spacing(np.abs(d_exact)) + 1e-300)
    # P2
    for k in range(3):
        e_ref, e_gpu = refout["energies"][k], gpu["energies"][k]
        assert abs(e_gpu - e_ref) <= tol * abs(e_ref) + 1e-300, ("energy", k, e_gpu, e_ref)
    # P3
    S = force_scales(cfg, refout)
    diff = np.abs(gpu["force"][:, :3] - refout["force"][:, :3])
    assert np.all(diff <= tol * S[:, None] + 1e-300), float((diff / (S[:, None] + 1e-300)).max())
    # P4
    F_exact = forces_from_dipole(cfg, refout, d_exact)
    err_gpu = np.abs(gpu["force"][:, :3] - F_exact[:, :3])
    err_ref = np.abs(refout["force"][:, :3] - F_exact[:, :3])
    assert np.all(err_gpu <= err_ref + 1e-14 * S[:, None] + 1e-300)
    # P5
    mol = np.ones(len(S), dtype=bool)
    mol[refout["photon_idx"]] = False
    assert np.all(gpu["force"][mol, 2] == 0.0) and np.all(gpu["force"][:, 3] == 0.0)
    raw_rel = diff[mol, :2] / (np.abs(refout["force"][mol, :2]) + 1e-300)
    return {"max_scaled_force_err": float((diff / (S[:, None] + 1e-300)).max()),
            "max_raw_rel_force_err": float(raw_rel.max()) if raw_rel.size else 0.0,
            "dipole_rel_err_vs_ref": float(np.abs(d_gpu - d_ref).max() / max(np.abs(d_ref).max(), 1e-300))}


def random_cfg(n, seed, photon_at=None, L=(31.0, 17.5, 23.25), image_range=3, photon_charge=0.0):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(L)
    tid = rng.integers(0, 2, n).astype(np.int32)
    charge = rng.uniform(-1, 1, n)
    if photon_at is not None:
        tid[photon_at] = 2
        charge[photon_at] = photon_charge
    image = rng.integers(-image_range, image_range + 1, (n, 3)).astype(np.int32)
    return {"name": f"rand{n}", "seed": seed, "position": pos, "typeid": tid, "charge": charge, "image": image,
            "types": ["O", "N", "L"], "box": L, "L_typeid": 2,
            "params": {"omegac": 0.0091, "couplstr": 1e-3, "phmass": 1.0}}
