"""Free particles in the group bath of include/cavmd.h (cavmd_bath_step_two): a numpy twin of the run, held to the three closed
forms of tests/langevin_twin.py.  What tests/test_bath_abi.py checks on the host, and where the acceptance band of
tests/test_gpu_bath_batch.py comes from.

The step is NOT restated here: it is ``mirror_step_one`` of tests/verlet_mirror.py and ``mirror_bath_step_two`` of
tests/bath_mirror.py, the mirror the kernel is pinned to bit for bit, with the contract's own Philox variates.  The parameters,
``ratios`` and ``closed_forms`` are langevin_twin's.  516 particles as three systems of N = 1, 2 and 513 (one lane, two lanes,
past one 512-particle tile), every particle coupled with the same gamma and mass, no photon, zero forces; system i draws under
the key LangevinBathBatch gives it for `seed`."""
from types import SimpleNamespace

import numpy as np

import bath_mirror
from langevin_twin import BOX, BURN_IN, COUNTED, DT, EXPECTED, GAMMA, KT, MASS, closed_forms, member_sd, ratios  # noqa: F401
from verlet_mirror import mirror_step_one

SIZES = (1, 2, 513)
PARTICLES = sum(SIZES)
MISTAKES = ("frozen_step_counter", "tally_with_pre_kick_velocity")
# The acceptance band of the three figures around langevin_twin.EXPECTED = (1, 1, 0) in tests/test_gpu_bath_batch.py: 6 standard
# deviations across the 24 seeds of `run` at these very sizes, steps and parameters, as printed by tests/test_bath_abi.py (which
# fails if these literals are not that run's figures).  Not from a GPU run.  That run: seeds 0..23, standard deviations 0.00165,
# 0.00136, 0.000069 around means 0.99958, 0.99961, -0.00001, worst single seed 0.0033 from the expected.
BAND = (0.0099, 0.0082, 0.000411)
BAND_DIGITS = (0.5e-4, 0.5e-4, 0.5e-6)      # how closely the literals are held to the run

def systems():
    """the twin's three systems at rest, as dicts of tests/verlet_mirror.py"""
    out = []
    for n in SIZES:
        vel = np.zeros((n, 4))
        vel[:, 3] = MASS
        out.append({"N": n, "box": BOX, "pos": np.zeros((n, 4)), "vel": vel, "image": np.zeros((n, 3), dtype=np.int32),
                    "forces": [np.zeros((n, 4))], "net": None, "accel": np.zeros((n, 3)), "langevin": -1, "steps": 0,
                    "out_of_box": 0, "reservoir": 0.0})
    return out


def baths(seed):
    return [{"gamma": np.full(n, GAMMA), "kT": KT, "seed": bath_mirror.item_key(seed, i), "draws": 0, "coupled": 0, "reservoir": 0.0}
            for i, n in enumerate(SIZES)]


def run(seed, mistake=None, burn_in=BURN_IN, counted=COUNTED) -> np.ndarray:
    """the 516 free particles from rest through burn_in + counted steps -> the three figures of langevin_twin.ratios over the
    counted steps"""
    assert mistake is None or mistake in MISTAKES
    ss, bs = systems(), baths(seed)
    row = SimpleNamespace(dt=DT, langevin_gamma=0.0, langevin_coeff=0.0, uniform=(0.0, 0.0, 0.0), skip=0)
    sums = np.zeros(2)
    start = 0.0
    tally_velocity = "before" if mistake == "tally_with_pre_kick_velocity" else "after"
    for step in range(burn_in + counted):
        if step == burn_in:
            sums[:] = 0.0
            start = sum(b["reservoir"] for b in bs)
        for s, b in zip(ss, bs):
            mirror_step_one(s, row)
            half = s["vel"][:, :3]
            sums[1] += float((half * half).sum())
            if mistake == "frozen_step_counter":                             # the planted mistake: every step draws block 0
                b["draws"] = 0
            bath_mirror.mirror_bath_step_two(s, row, b, tally_velocity=tally_velocity)
            full = s["vel"][:, :3]
            sums[0] += float((full * full).sum())
    assert all(s["steps"] == burn_in + counted and s["out_of_box"] == 0 for s in ss)
    assert [b["coupled"] for b in bs] == list(SIZES)
    gain = (sum(b["reservoir"] for b in bs) - start) / PARTICLES             # per particle
    return ratios(sums[0], sums[1], 3 * PARTICLES * counted, gain, counted)
