#!/usr/bin/env python3
"""REFERENCE-EXECUTED fixture for WHEN the F(k,t) tracker takes further references and what it correlates with them.

Run on the build machine only (`python tests/golden/make_reference_field_autocorr_golden.py`); it needs a checkout of the
reference next to this repository (the path make_reference_python_golden.py names) and writes
tests/golden/reference_field_autocorr_golden.npz and nothing else.  The tests read the .npz and never this script.

What executes: the reference's own FieldAutocorrelationTracker (src/cavitymd/analysis.py:260-418), loaded and driven exactly
as make_reference_python_golden.py does it -- on tests/stubs/hoomd, containers only -- over 14 seeded frames of the
501-particle stand-in with output_period_steps = 1 and reference_interval_steps = 3, once with max_references = 3 and once
with max_references = 2 (the cap bites).  The existing fixtures ran the tracker with max_references = 1; nothing there pins
when references appear.  The tracker's own text files keep six decimals, so the generator wraps the tracker's bound
compute_field_autocorr and stores every value it returned, at full precision.

Stored per run `field_autocorr/<run>/`: after act(t) the number of references (`n_references`, frame 0 = construction), each
reference's `timestep` (`reference_timesteps`), and `F[t, r]` = the value returned for reference r at step t (NaN where the
tracker did not correlate: frame 0, and reference r before and AT the step that took it).  Inputs: `frames` (wrapped
positions), `wavevectors`.  Numbers only."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_python_golden as base  # noqa: E402  (the loader and the array holders; its main() is not run)

OUT = os.path.join(HERE, "reference_field_autocorr_golden.npz")
N_FRAMES, KMAG, NK, INTERVAL = 14, 1.0, 50, 3
RUNS = {"max3": 3, "max2": 2}


def main():
    ref = base.load_reference_package()
    import hoomd
    analysis = ref["analysis"]
    c = base.diatomic_stand_in(12)
    L = c["box"]
    rng = np.random.default_rng(19)
    frames = [c["position"]]
    for _ in range(N_FRAMES - 1):
        r = frames[-1] + 0.05 * rng.normal(size=frames[-1].shape)
        frames.append(r - np.floor((r + L / 2) / L) * L)          # stay wrapped
    out = {"field_autocorr/frames": np.array(frames), "field_autocorr/box": L,
           "field_autocorr/reference_interval_steps": np.int64(INTERVAL), "field_autocorr/runs": np.array(list(RUNS))}
    tmp = tempfile.mkdtemp(prefix="refgolden_field_")
    cwd = os.getcwd()
    os.chdir(tmp)                          # the tracker writes its text files into the working directory
    try:
        for run, max_refs in RUNS.items():
            st = base.State(frames[0], c["typeid"], c["image"], c["charge"], c["box"])
            sim = base.Sim(st, hoomd, dt=2.0)
            tr, _ = base.quiet(analysis.FieldAutocorrelationTracker, sim, "density_correlation", kmag=KMAG, num_wavevectors=NK,
                               output_period_steps=1, max_references=max_refs, reference_interval_steps=INTERVAL)
            returned = []
            bound = tr.compute_field_autocorr

            def wrapped(field0, field_t, _bound=bound, _returned=returned):
                v = _bound(field0, field_t)
                _returned.append(v)
                return v
            tr.compute_field_autocorr = wrapped
            F = np.full((N_FRAMES, max_refs), np.nan)
            n_refs = [len(tr.references)]
            for t in range(1, N_FRAMES):
                st.p.position = frames[t]
                sim.timestep = t
                before = len(tr.references)
                del returned[:]
                base.quiet(tr.act, t)
                assert len(returned) == before       # one value per reference that was active BEFORE this step's new one
                F[t, :before] = returned
                n_refs.append(len(tr.references))
            key = f"field_autocorr/{run}/"
            out[key + "max_references"] = np.int64(max_refs)
            out[key + "wavevectors"] = np.array(tr.wavevectors)
            out[key + "n_references"] = np.array(n_refs, dtype=np.int64)
            out[key + "reference_timesteps"] = np.array([r["timestep"] for r in tr.references], dtype=np.int64)
            out[key + "F"] = F
            print(f"{run}: references at steps {out[key + 'reference_timesteps'].tolist()}, n_references {n_refs}")
    finally:
        os.chdir(cwd)
    out["generated_by"] = np.array("tests/golden/make_reference_field_autocorr_golden.py executing the reference's "
                                   "src/cavitymd/analysis.py FieldAutocorrelationTracker on tests/stubs/hoomd (containers only)")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
