"""The captured outer step of the impulse multiple-time-step scheme on the GPU: B = 4 copies of the host twin's 12 charged
dimers and the photon (tests/mts_twin.py), the long part of the Ewald sum evaluated and kicked with every n = 4 steps.  Run with
`-m gpu` on an MI355X.
    kick(long, n / 2);  n x {step one; cavity, molecular, short; step two};  long;  kick(long, n / 2);  ledger
  1. 50 replays of the captured outer step give the bytes of 50 eager outer steps;
  2. the ledger's ewald_short + ewald_long and universe_total beside the host twin's series, and the drift at dt over dt / 2;
  3. the example runs (it lives in a directory of its own, examples/mts/, as the run clock's does)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import cavitymd
import device_start_cases as cases
import device_start_twin as twin
import mts_twin
from water_systems import HARMONIC, LJ
from water_systems import thermal as _thermal

pytestmark = pytest.mark.gpu

B, N_INNER = 4, 4
ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


class Run:
    """cavity, molecular and split Coulomb forces, integrator and ledger over B copies of the dimers, started as the twin is"""

    def __init__(self, dt, capacity):
        c, bonds, bond_typeid = cases.dimers_config()
        r_cut = cases.DIMERS_R_CUT
        self.sysdefs = [cavitymd.SystemDefinition(cavitymd.ParticleData.from_arrays(c["position"], c["typeid"], c["charge"], c["image"],
                                                                                    c["types"], c["box"], device="cuda")) for _ in range(B)]
        v0, mass = _thermal(c)
        self.velocities = [torch.from_numpy(np.concatenate([v0, mass[:, None]], axis=1)).cuda() for _ in range(B)]
        self.cavity = cavitymd.CavityForceBatch(self.sysdefs, [c["params"]] * B)
        lj = {pair: dict(p, r_cut=min(p["r_cut"], r_cut)) for pair, p in LJ.items()}
        self.mol = cavitymd.MolecularForceBatch(self.sysdefs, [bonds] * B, [bond_typeid] * B, HARMONIC, lj)
        self.coulomb = cavitymd.CoulombForceBatch(self.sysdefs, [bonds] * B, r_cut=r_cut, accuracy=cases.DIMERS_ACCURACY, split=True)
        self.integrator = cavitymd.VerletBatch(self.cavity, self.velocities,
                                               extra_forces=[[m, s] for m, s in zip(self.mol.forces, self.coulomb.short.forces)])
        self.ledger = cavitymd.BatchEnergyLedger(self.cavity, self.velocities,
                                                 terms=[("molecular", self.mol), ("ewald_short", self.coulomb.short),
                                                        ("ewald_long", self.coulomb.long)], capacity=capacity)
        self.integrator.set_inputs(dt)
        self.cavity.compute()
        self.mol.compute()
        self.coulomb.compute(parts="both")
        self.integrator.prime()
        self.integrator.kick_table(self.coulomb.long)                              # before any capture
        self.ledger.record()
        torch.cuda.synchronize()

    def outer(self):
        self.integrator.kick(self.coulomb.long, 0.5 * N_INNER)
        for _ in range(N_INNER):
            self.integrator.step_one()
            self.cavity.compute()
            self.mol.compute()
            self.coulomb.compute(parts="short")
            self.integrator.step_two()
        self.coulomb.compute(parts="long")
        self.integrator.kick(self.coulomb.long, 0.5 * N_INNER)
        self.ledger.record()

    def graph(self):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.outer()
        return g

    def state_bytes(self):
        torch.cuda.synchronize()
        out = []
        for k, sd in enumerate(self.sysdefs):
            pd = sd.getParticleData()
            out.append((pd.getPositions().cpu().numpy().tobytes(), pd.getImages().cpu().numpy().tobytes(),
                        self.velocities[k].cpu().numpy().tobytes(), self.coulomb.forces[k].cpu().numpy().tobytes(),
                        self.coulomb.forces_long[k].cpu().numpy().tobytes()))
        return out, self.ledger.read().tobytes()

    def close(self):
        for obj in (self.ledger, self.integrator, self.coulomb, self.mol, self.cavity):
            obj.close()


def test_fifty_replays_of_the_outer_step_equal_fifty_eager_outer_steps():
    results = []
    for captured in (False, True):
        run = Run(cases.DRIFT_DT, 64)
        if captured:
            g = run.graph()
            assert run.integrator.state()["steps"].tolist() == [0] * B             # capturing ran nothing
            for _ in range(50):
                g.replay()
        else:
            for _ in range(50):
                run.outer()
        state, rows = run.state_bytes()
        assert run.integrator.state()["steps"].tolist() == [50 * N_INNER] * B
        assert run.integrator.state()["out_of_box"].tolist() == [0] * B
        assert all(s == state[0] for s in state)                                   # the copies stay copies
        moved = run.coulomb.forces_long[0].cpu().numpy()
        assert np.isfinite(moved).all() and moved[:-1, :3].any()
        results.append((state, rows))
        run.close()
    assert results[0] == results[1]


def test_the_ledger_follows_the_host_twin_and_the_drift_is_second_order():
    """The tolerance tests/test_gpu_ewald_reciprocal.py grants its NVE run beside its twin: the device and the host evaluate the
    same expressions and differ by rounding per step, so the energies stay together within 1e-3 of the integrator's own drift.
    The band of the drift ratio is the host's, [3.5, 4.5] (tests/test_coulomb_parts_abi.py).  Measured on an MI355X: see
    profiles/coulomb_parts/README.md."""
    DT, STEPS = cases.DRIFT_DT, cases.DRIFT_STEPS
    drift, series = {}, {}
    for dt, steps in ((DT, STEPS), (0.5 * DT, 2 * STEPS)):
        run = Run(dt, steps // N_INNER + 1)
        g = run.graph()
        for _ in range(steps // N_INNER):
            g.replay()
        rows = run.ledger.read()
        assert rows.shape == (B, steps // N_INNER + 1) and run.integrator.state()["out_of_box"].tolist() == [0] * B
        H = rows["universe_total"]
        assert np.isfinite(H).all() and all(H[k].tobytes() == H[0].tobytes() for k in range(B))
        drift[dt] = twin.drift(H[0])
        series[dt] = rows[0]
        run.close()
    ratio = drift[DT] / drift[0.5 * DT]
    host = mts_twin.Dimers("direct").run_mts(DT, STEPS, N_INNER)
    host_total = mts_twin.system_total(host)
    total_apart = float(np.abs(series[DT]["universe_total"] - host_total).max())
    ewald = series[DT]["ewald_short"] + series[DT]["ewald_long"]
    ewald_apart = float(np.abs(ewald - (host[:, 2] + host[:, 3])).max())
    print(f"\nn = {N_INNER}: drift of universe_total over {STEPS} steps at dt = {DT}: {drift[DT]:.4e}; at dt / 2: {drift[0.5 * DT]:.4e}; "
          f"ratio {ratio:.4f}; the host twin's drift {twin.drift(host_total):.4e}; largest |universe_total - twin|: {total_apart:.3e}; "
          f"largest |ewald_short + ewald_long - twin|: {ewald_apart:.3e}")
    assert total_apart <= 1e-3 * drift[DT], (total_apart, drift[DT])
    assert ewald_apart <= 1e-3 * drift[DT], (ewald_apart, drift[DT])
    assert 3.5 <= ratio <= 4.5, (drift, ratio)


def test_the_example_runs():
    example = os.path.join(ROOT, "examples", "mts", "batch_mts_coulomb_in_one_graph.py")
    done = subprocess.run([sys.executable, example, "2", "16"], cwd=ROOT, stdin=subprocess.DEVNULL, capture_output=True, text=True,
                          timeout=180)
    assert done.returncode == 0, done.stdout + done.stderr
    print("\n" + done.stdout)
    lines = [re.search(r"^n = (\d): B = 2, 16 MD steps; ewald_short (\S+), ewald_long (\S+); worst excursion of universe_total (\S+) "
                       r"hartree; (\S+) us per MD step$", line) for line in done.stdout.strip().splitlines()]
    assert [m.group(1) for m in lines if m] == ["1", "4"], done.stdout
    assert all(np.isfinite(float(x)) for m in lines for x in m.groups()[1:]), done.stdout
