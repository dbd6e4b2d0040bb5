#!/usr/bin/env python3
"""REFERENCE-EXECUTED fixture for the Bussi reservoir thermostat's rule (row f4).

Run in the BUILD container only (`python tests/golden/make_reference_bussi_golden.py`); /root/reference does not exist on
the GPU box and nothing of it travels: this script writes INPUTS and OUTPUT NUMBERS into
tests/golden/bussi_reference_golden.npz and nothing else.

What executes: the reference's own header src/BussiReservoirThermostat.h (getRescalingFactorsOne :43-98,
compute_rescale_factor :177-225, the reservoir getters) and the src/Thermostat.h it includes, compiled by g++ with the flags
of oracle/Makefile (-O2 -ffp-contract=off, no -march) into a driver of our own (DRIVER below), on top of
tests/stubs/hoomd_thermostat, which declares the HOOMD-blue names those headers touch with NO arithmetic: ComputeThermo
returns the kinetic energies and degrees of freedom the driver prescribes, the set point is a stored number, and the
distributions of the stand-in RandomNumbers.h hand out the next value of an injected stream and log what was asked for.
Thermostat.h names pybind11::tuple; this container's pybind11 and libpython satisfy it.

Recorded per call: the inputs, the raised exception ("requires non-zero initial momenta") or the factors, all four reservoir
counters after the call, c = exp(-dt / tau) as the driver's copy of the reference's expression computes it (the same libm,
the same flags: tests compare bits only where the running machine's exp agrees), and the draws the reference consumed --
how many, which distribution, with which parameters.  Cases: random single calls (fresh thermostat each), an edge table
(fresh thermostat each) and three 300-step sequences on one thermostat object (counters cumulative).
"""
import os
import subprocess
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))
REF_SRC = "/root/reference/src"
STUBS = os.path.join(ROOT, "tests", "stubs", "hoomd_thermostat")
OUT = os.path.join(HERE, "bussi_reference_golden.npz")

# columns of one call
IN_COLS = ("fresh", "K_t", "dof_t", "K_r", "dof_r", "dt", "set_T", "tau", "draw0", "draw1", "draw2", "draw3")
OUT_COLS = ("throws", "alpha_t", "alpha_r", "reservoir_t", "reservoir_r", "instantaneous_t", "instantaneous_r", "c",
            "n_draws", "kind0", "kind1", "kind2", "kind3", "param0_0", "param0_1", "param0_2", "param0_3",
            "param1_0", "param1_1", "param1_2", "param1_3")

DRIVER = r"""
#include "BussiReservoirThermostat.h"

#include <cstdio>

using namespace hoomd;
using namespace hoomd::md;

// argv[1]: rows of 12 doubles  {fresh, K_t, dof_t, K_r, dof_r, dt, set_T, tau, draw0..draw3}
// argv[2]: rows of 21 doubles  {throws, alpha_t, alpha_r, reservoir_t, reservoir_r, instantaneous_t, instantaneous_r, c,
//                               n_draws, kind[4], param0[4], param1[4]}   (kind -1: not drawn)
int main(int argc, char** argv)
{
    if (argc != 3)
        return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo)
        return 2;
    auto T = std::make_shared<Variant>(0.0);
    auto group = std::make_shared<ParticleGroup>();
    auto thermo = std::make_shared<ComputeThermo>();
    auto sysdef = std::make_shared<SystemDefinition>();
    std::unique_ptr<BussiReservoirThermostat> th;
    double in[12];
    uint64_t timestep = 0;
    while (fread(in, sizeof(double), 12, fi) == 12)
    {
        if (in[0] != 0.0 || !th)
            th.reset(new BussiReservoirThermostat(T, group, thermo, sysdef, in[7]));
        th->setTau(in[7]);
        thermo->m_translational_kinetic_energy = in[1];
        thermo->m_translational_dof = in[2];
        thermo->m_rotational_kinetic_energy = in[3];
        thermo->m_rotational_dof = in[4];
        T->m_value = in[6];
        standin_draws().assign(in + 8, in + 12);
        standin_log().clear();
        double out[21] = {0.0};
        try
        {
            const std::array<Scalar, 2> f = th->getRescalingFactorsOne(timestep, in[5]);
            out[1] = f[0];
            out[2] = f[1];
        }
        catch (const std::runtime_error&)
        {
            out[0] = 1.0;
        }
        out[3] = th->getReservoirEnergyTranslational();
        out[4] = th->getReservoirEnergyRotational();
        out[5] = th->getInstantaneousReservoirTranslational();
        out[6] = th->getInstantaneousReservoirRotational();
        const Scalar deltaT = in[5];
        const Scalar m_tau = in[7];
        out[7] = (m_tau != 0.0) ? exp(-deltaT / m_tau) : 0.0; // compute_rescale_factor's time_decay_factor
        out[8] = (double)standin_log().size();
        for (int i = 0; i < 4; ++i)
        {
            const bool drawn = i < (int)standin_log().size();
            out[9 + i] = drawn ? standin_log()[i].kind : -1.0;
            out[13 + i] = drawn ? standin_log()[i].param0 : 0.0;
            out[17 + i] = drawn ? standin_log()[i].param1 : 0.0;
        }
        if (fwrite(out, sizeof(double), 21, fo) != 21)
            return 3;
        ++timestep;
    }
    fclose(fo);
    fclose(fi);
    return 0;
}
"""

DOFS = (0.0, 1.0, 2.0, 3.0, 297.0, 2999997.0)


def _stream(rng, dof_t, dof_r):
    """Four injected values, in the order the reference is expected to consume them (normal, then gamma for more than one
    degree of freedom, per class with degrees of freedom); unused slots hold values that must stay unconsumed.  Which were
    consumed is what the driver records, not what this function assumes."""
    s = []
    for dof in (dof_t, dof_r):
        if dof != 0:
            s.append(float(rng.standard_normal() * rng.choice([1.0, 4.0])))
            if dof > 1:
                s.append(float(rng.gamma((dof - 1) / 2, 1.0)))
    while len(s) < 4:
        s.append(float(rng.uniform(100.0, 200.0)))
    return s


def random_cases(rng, n):
    """The spans of test_scalar_rule_matches_the_oracle_bit_for_bit; a quarter with rotational degrees of freedom."""
    rows = []
    for _ in range(n):
        dof_t = float(rng.choice(DOFS))
        set_T = float(10.0 ** rng.uniform(-4, 1))
        K_t = float(0.5 * max(dof_t, 1.0) * set_T * 10.0 ** rng.uniform(-3, 3))
        dt = float(10.0 ** rng.uniform(-3, 0))
        tau = float(rng.choice([0.0, dt * 20, 10.0 ** rng.uniform(-3, 3)]))
        if rng.uniform() < 0.25:
            dof_r = float(rng.choice(DOFS[1:]))
            K_r = float(0.5 * dof_r * set_T * 10.0 ** rng.uniform(-3, 3))
        else:
            dof_r, K_r = 0.0, 0.0
        rows.append([1.0, K_t, dof_t, K_r, dof_r, dt, set_T, tau] + _stream(rng, dof_t, dof_r))
    return rows


def edge_cases():
    """(name, row) of the reference's edges; every case a fresh thermostat."""
    e = []

    def add(name, K_t, dof_t, dt, set_T, tau, draws, K_r=0.0, dof_r=0.0):
        d = list(draws) + [150.0] * (4 - len(draws))
        e.append((name, [1.0, K_t, dof_t, K_r, dof_r, dt, set_T, tau] + d))

    add("dt_zero", 2.5, 297.0, 0.0, 1.5, 0.5, [0.3, 140.0])
    add("dt_zero_tau_zero", 2.5, 297.0, 0.0, 1.5, 0.0, [-0.3, 140.0], 1.0, 3.0)
    add("K_t_zero_throws", 0.0, 297.0, 0.01, 1.5, 0.5, [0.3, 140.0])
    add("K_t_zero_dof_3_throws", 0.0, 3.0, 0.01, 1.5, 0.0, [0.3, 1.0])
    add("K_r_zero_throws", 2.5, 297.0, 0.01, 1.5, 0.5, [0.3, 140.0, 0.2, 1.0], 0.0, 3.0)
    add("K_t_zero_dof_zero", 0.0, 0.0, 0.01, 1.5, 0.5, [0.3, 1.0])
    add("dof_t_zero_rotational_draws_first", 7.0, 0.0, 0.01, 1.5, 0.5, [0.7, 1.2, 9.0, 9.0], 2.0, 3.0)
    add("dof_t_one_no_gamma", 0.75, 1.0, 0.02, 1.5, 0.4, [-0.6, 2.0, 3.0, 4.0], 1.0, 1.0)
    add("dof_t_two", 0.75, 2.0, 0.02, 1.5, 0.4, [-0.6, 0.8, 3.0, 4.0])
    add("c_rounds_to_one_tiny_dt", 3.0, 297.0, 1e-17, 1.5, 1.0, [0.3, 140.0])
    add("c_rounds_to_one_huge_tau", 3.0, 297.0, 1e-300, 1.5, 1e300, [-2.0, 140.0])
    add("c_rounds_to_one_neg_R40", 3.0, 3.0, 1e-18, 1.5, 1.0, [-40.0, 1.5])
    add("set_T_zero_tau_zero_R_pos", 3.0, 297.0, 0.01, 0.0, 0.0, [0.5, 140.0])
    add("set_T_zero_tau_zero_R_neg", 3.0, 297.0, 0.01, 0.0, 0.0, [-0.5, 140.0])
    add("set_T_zero_tau_zero_R_zero", 3.0, 3.0, 0.01, 0.0, 0.0, [0.0, 1.0])
    add("set_T_zero_tau_pos", 3.0, 297.0, 0.01, 0.0, 0.5, [0.5, 140.0])
    add("K_subnormal", 2.0 ** -1060 * 5, 3.0, 0.01, 1e-300, 0.5, [0.4, 1.1])
    add("K_subnormal_lowbit", 2.0 ** -1074 * 12345, 297.0, 0.01, 1e-300, 0.0, [-0.4, 150.0])
    add("K_subnormal_overflowing_v", 2.0 ** -1060 * 7, 3.0, 0.01, 1.5, 0.5, [0.4, 1.1])
    add("K_huge", 1.234567891234e300, 2999997.0, 0.01, 1.5, 0.5, [0.4, 1.5e6])
    add("K_huge_neg_R", 9.87654321e299, 297.0, 0.05, 1.5, 0.0, [-1.5, 150.0])
    add("K_huge_sign_term_overflow", 1.7e308 / 2, 297.0, 0.01, 1e-300, 0.5, [-3.0, 150.0])
    add("R_zero_tau_zero", 3.0, 297.0, 0.01, 1.5, 0.0, [0.0, 140.0])
    add("R_negzero_tau_zero", 3.0, 297.0, 0.01, 1.5, 0.0, [-0.0, 140.0])
    add("R_zero_tau_zero_dof_1", 3.0, 1.0, 0.01, 1.5, 0.0, [0.0, 77.0])
    add("R_negzero_tau_zero_dof_3", 3.0, 3.0, 0.01, 1.5, 0.0, [-0.0, 0.9])
    add("R_pos40_tau_zero", 3.0, 297.0, 0.01, 1.5, 0.0, [40.0, 140.0])
    add("R_neg40_tau_zero", 3.0, 297.0, 0.01, 1.5, 0.0, [-40.0, 140.0])
    add("R_neg40_tau_pos", 3.0, 297.0, 0.01, 1.5, 0.5, [-40.0, 140.0])
    add("R_pos40_tau_pos", 3.0, 297.0, 0.01, 1.5, 0.5, [40.0, 140.0])
    add("R_neg40_dof_big", 1.5 * 2999997 / 2, 2999997.0, 0.01, 1.5, 0.05, [-40.0, 1.5e6])
    add("R_neg40_rotational", 3.0, 297.0, 0.01, 1.5, 0.5, [0.1, 140.0, -40.0, 1.0], 2.0, 3.0)
    return e


def sequences(rng):
    """Three 300-step runs of one thermostat object with rotational degrees of freedom: counters accumulate."""
    runs = []
    for s, (dof_t, dof_r, dt, set_T, tau) in enumerate([(297.0, 3.0, 0.01, 1.5, 0.5), (2999997.0, 2.0, 0.02, 3.2e-4, 0.2),
                                                        (3.0, 297.0, 0.005, 0.7, 5.0)]):
        rows = []
        for step in range(300):
            K_t = float(0.5 * dof_t * set_T * rng.uniform(0.5, 1.5))
            K_r = float(0.5 * dof_r * set_T * rng.uniform(0.5, 1.5))
            t = tau
            if step % 37 == 11:
                t = 0.0                    # instantaneous thermalisation
            d = _stream(rng, dof_t, dof_r)
            if step % 41 == 7:
                d[0] = -abs(d[0]) - 3.0    # push towards the negative branch
            this_dt = 0.0 if step == 150 else dt
            if s == 2 and step == 200:
                K_t = 0.0                  # throws: counters must stay where they were
            rows.append([1.0 if step == 0 else 0.0, K_t, dof_t, K_r, dof_r, this_dt, set_T, t] + d)
        runs.append(rows)
    return runs


def run_driver(rows):
    tmp = tempfile.mkdtemp(prefix="bussigolden_")
    src = os.path.join(tmp, "driver.cc")
    exe = os.path.join(tmp, "driver")
    with open(src, "w") as f:
        f.write(DRIVER)
    import pybind11
    ver = sysconfig.get_config_var("LDVERSION")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", STUBS, "-I", REF_SRC, "-I", pybind11.get_include(),
                    "-I", sysconfig.get_paths()["include"], src, "-o", exe, "-L", sysconfig.get_config_var("LIBDIR"),
                    f"-lpython{ver}"], check=True)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.ascontiguousarray(rows, dtype=np.float64).tofile(fin)
    subprocess.run([exe, fin, fout], check=True)
    out = np.fromfile(fout, dtype=np.float64).reshape(-1, len(OUT_COLS))
    assert out.shape[0] == len(rows)
    return out


def main():
    assert os.path.exists(os.path.join(REF_SRC, "BussiReservoirThermostat.h")), "needs the reference tree (build container only)"
    rng = np.random.default_rng(20261016)
    singles = random_cases(rng, 2000)
    edges = edge_cases()
    runs = sequences(rng)
    rows = singles + [r for _, r in edges] + [r for run in runs for r in run]
    out = run_driver(rows)
    n1, n2 = len(singles), len(singles) + len(edges)
    case_in = np.array(singles + [r for _, r in edges], dtype=np.float64)
    seq_in = np.array(runs, dtype=np.float64)
    res = dict(
        in_cols=np.array(IN_COLS), out_cols=np.array(OUT_COLS),
        case_in=case_in, case_out=out[:n2],
        case_name=np.array(["random"] * n1 + [name for name, _ in edges]),
        seq_in=seq_in, seq_out=out[n2:].reshape(seq_in.shape[0], seq_in.shape[1], len(OUT_COLS)),
    )
    np.savez_compressed(OUT, **res)
    print(f"wrote {OUT}: {n1} random calls, {len(edges)} edges, {seq_in.shape[0]} x {seq_in.shape[1]} sequence steps; "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
