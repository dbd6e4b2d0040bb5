"""The ledger's conserved column under a bath, on the GPU.  Run with `-m gpu` on an MI355X.

``cavmd_ledger_row.universe_total`` = system_total + reservoir_total is the one number a user of the batch MD step watches, and
the other tests hold the baths to mirrors of the contract bit for bit, which cannot notice a contract that is wrong.  Here
B = 4 copies of the 12 charged dimers and the photon of tests/thermostatted_twin.py (N = 25) run 200 thermostatted steps with
that twin's parameters, under different seeds, and every system's universe_total must stay inside the twin's band while
system_total itself moves by ten bands: the reservoirs are what close the balance.  The band is three times the largest
excursion the HOST twin shows over 8 seeds (tests/test_thermostatted_twin.py); it is never taken from a device run.
  "row_bussi"   the full step of test_gpu_ledger's forty steps: the photon under the integrator's row bath, the molecules under
                the Bussi batch, the ledger's row taken before the step's Bussi launch;
  "group"       the with_bath step of tests/checkpoint_runs.Run: a LangevinBathBatch on the molecules in place of step two.
Each runs eagerly and from ONE captured graph with the same seeds (rows drawn by StepDraw at a fixed dt): the two series must be
the same bytes, as the replay tests of every object in the step guarantee.  The row configuration also runs eagerly with the
torch-drawn inputs of the forty-steps test.
A tally taken with the velocity from before the kick leaves the band by a factor of three at least on every seed of the twin."""
import numpy as np
import pytest
import torch

import cavitymd
import device_start_cases as cases
import thermostatted_twin as twin
from water_systems import HARMONIC, KT, LJ
from water_systems import thermal as _thermal

pytestmark = pytest.mark.gpu

B = 4
START_SEED, DRAW_SEED = 5, 2025


class _Md:
    """B copies of cases.dimers_config with the twin's forces, start and baths; `draws`: "step_draw" (one launch of the
    library's generator per step) or "torch" (the draw_inputs of the integrator and the thermostat)"""

    def __init__(self, configuration, draws="step_draw"):
        assert configuration in twin.CONFIGURATIONS and draws in ("step_draw", "torch")
        cfg, bonds, bond_typeid = cases.dimers_config()
        self.configuration, self.draws, self.dt = configuration, draws, twin.DT[configuration]
        mass = _thermal(cfg)[1]
        n = len(mass)
        photon = int(np.flatnonzero(cfg["typeid"] == cfg["L_typeid"])[0])
        molecules = np.delete(np.arange(n), photon)
        assert n == 25 and photon == n - 1 and mass[photon] == 1.0 and np.array_equal(mass, twin.dimers().mass)
        self.sysdefs, self.velocities = [], []
        for _ in range(B):
            pd = cavitymd.ParticleData.from_arrays(cfg["position"], cfg["typeid"], cfg["charge"], cfg["image"], cfg["types"],
                                                   cfg["box"], device="cuda")
            self.sysdefs.append(cavitymd.SystemDefinition(pd))
            self.velocities.append(torch.from_numpy(np.concatenate([np.zeros((n, 3)), mass[:, None]], axis=1)).cuda())
        r_cut = cases.DIMERS_R_CUT
        self.cavity = cavitymd.CavityForceBatch(self.sysdefs, cfg["params"])
        self.molecular = cavitymd.MolecularForceBatch(self.sysdefs, [bonds] * B, [bond_typeid] * B, HARMONIC,
                                                      {pair: dict(p, r_cut=min(p["r_cut"], r_cut)) for pair, p in LJ.items()})
        self.coulomb = cavitymd.CoulombForceBatch(self.sysdefs, [bonds] * B, r_cut=r_cut, accuracy=cases.DIMERS_ACCURACY)
        with_row = configuration == "row_bussi"
        self.integrator = cavitymd.VerletBatch(self.cavity, self.velocities,
                                               extra_forces=[[m, c] for m, c in zip(self.molecular.forces, self.coulomb.forces)],
                                               langevin_index=photon if with_row else None)
        self.thermalizer = cavitymd.BatchThermalizer(self.velocities, twin.START_KT[configuration], seed=START_SEED,
                                                     cavity=self.cavity, place_photon=True, finite_q=True, zero_momentum=True)
        self.thermostat = self.bath = None
        if with_row:
            self.thermostat = cavitymd.BussiReservoirBatch(kT=twin.BUSSI_KT, tau=twin.BUSSI_TAU)
            self.thermostat.attach(self.velocities, translational_dof=3.0 * len(molecules) - 3.0, members=[molecules] * B)
            reservoirs = [("bussi", self.thermostat), ("langevin", self.integrator)]
            self.draw = cavitymd.StepDraw(DRAW_SEED, self.integrator, self.thermostat, dt=self.dt, gamma=twin.ROW_GAMMA, kT=KT)
        else:
            gamma = twin.GROUP_RATE * mass
            gamma[photon] = 0.0
            self.bath = cavitymd.LangevinBathBatch(self.integrator, [torch.from_numpy(gamma).cuda() for _ in range(B)], KT,
                                                   seed=twin.GROUP_SEED)
            reservoirs = [("bath", self.bath)]
            self.draw = cavitymd.StepDraw(DRAW_SEED, self.integrator, dt=self.dt)
        self.ledger = cavitymd.BatchEnergyLedger(self.cavity, self.velocities,
                                                 terms=[("molecular", self.molecular), ("coulomb", self.coulomb)],
                                                 reservoirs=reservoirs, clock=self.draw, capacity=twin.STEPS)
        assert self.ledger.capacity >= 200
        # the documented order of a start (include/cavmd.h, "the start of a batch")
        self.cavity.compute()
        self.thermalizer.thermalize()
        self.forces()
        self.integrator.prime()
        torch.cuda.synchronize()

    def forces(self):
        self.cavity.compute()
        self.molecular.compute()
        self.coulomb.compute()

    def step(self):
        self.draw.fill()                                                     # the rows of both tables and the ledger's clock
        if self.draws == "torch":
            self.integrator.draw_inputs(self.dt, gamma=twin.ROW_GAMMA, kT=KT)
        self.integrator.step_one()
        self.forces()
        (self.bath if self.bath is not None else self.integrator).step_two()
        self.ledger.record()                                                 # before this step's thermostat launch
        if self.thermostat is not None:
            if self.draws == "torch":
                self.thermostat.draw_inputs(0, self.dt)
            self.thermostat.step_async()

    def run(self, captured):
        if captured:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.step()
            assert list(self.ledger.rows()) == [0] * B                       # a capture runs nothing
            for _ in range(twin.STEPS):
                graph.replay()
        else:
            for _ in range(twin.STEPS):
                self.step()
        series, state = self.ledger.read(), self.integrator.state()
        assert series.shape == (B, twin.STEPS) and list(self.ledger.rows()) == [twin.STEPS] * B
        assert state["steps"].tolist() == [twin.STEPS] * B and state["out_of_box"].tolist() == [0] * B
        return series

    def close(self):
        for obj in (self.ledger, self.draw, self.bath, self.thermalizer, self.integrator, self.coulomb, self.molecular, self.cavity):
            if obj is not None:
                obj.close()
        if self.thermostat is not None:
            self.thermostat.detach()


def _run(configuration, captured, draws="step_draw"):
    md = _Md(configuration, draws)
    try:
        return md.run(captured)
    finally:
        md.close()


def _assert_conserved(series, configuration, what):
    band = twin.BAND[configuration]
    assert band == 3.0 * twin.MEASURED[configuration][0] > 0.0
    names = ("bussi", "langevin") if configuration == "row_bussi" else ("bath",)
    print()
    for k in range(B):
        row = series[k]
        universe, system = row["universe_total"], row["system_total"]
        excursion, moved = twin.excursion(universe), twin.excursion(system)
        print(f"{configuration}, {what}, system {k}: worst excursion of universe_total over {twin.STEPS} steps {excursion:.4e} "
              f"(band {band:.4e}); system_total moved by {moved:.4e} (at least {twin.LIVENESS * band:.4e}); reservoirs at the end "
              f"{ {name: float(row[name][-1]) for name in names} }")
        assert np.isfinite(universe).all() and np.all(np.diff(row["time"]) == twin.DT[configuration])
        # the column is the header's sum, and every reservoir is alive
        assert np.array_equal(universe, system + row["reservoir_total"])
        for name in names:
            assert len(set(row[name])) >= twin.STEPS - 1, name
        assert excursion <= band, (configuration, what, k, excursion, band)
        assert moved >= twin.LIVENESS * band, (configuration, what, k, moved, band)
    # the systems are different runs
    assert len({series[k]["universe_total"].tobytes() for k in range(B)}) == B


@pytest.fixture(scope="module", params=twin.CONFIGURATIONS)
def eager(request):
    torch.cuda.manual_seed(20251021)
    return request.param, _run(request.param, captured=False)


def test_universe_total_stays_inside_the_twins_band_eagerly(eager):
    configuration, series = eager
    _assert_conserved(series, configuration, "eager")


def test_universe_total_stays_inside_the_band_from_one_graph_and_replays_the_eager_bytes(eager):
    configuration, want = eager
    series = _run(configuration, captured=True)
    _assert_conserved(series, configuration, "captured")
    assert series.tobytes() == want.tobytes()


def test_universe_total_stays_inside_the_band_with_torch_drawn_inputs():
    torch.cuda.manual_seed(20251022)
    _assert_conserved(_run("row_bussi", captured=False, draws="torch"), "row_bussi", "eager, torch draws")
