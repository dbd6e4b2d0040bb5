// STAND-IN for hoomd/HOOMDMath.h, host only -- NOT HOOMD-blue.  Just enough declarations for the reference's thermostat
// headers (Thermostat.h, BussiReservoirThermostat.h) to compile with a plain C++ compiler, so that
// tests/golden/make_reference_bussi_golden.py can execute their arithmetic.  No arithmetic of its own.
//
// HOOMD-blue's own header pulls in the standard math functions and pybind11 (Thermostat.h names pybind11::tuple without
// including it), and declares Scalar inside namespace hoomd (Thermostat.h names hoomd::Scalar).
#ifndef STANDIN_THERMOSTAT_HOOMD_MATH_H_
#define STANDIN_THERMOSTAT_HOOMD_MATH_H_

#include <pybind11/pybind11.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <math.h>
#include <memory>
#include <stdexcept>

namespace hoomd
    {
typedef double Scalar; // HOOMD_LONGREAL_SIZE = 64, HOOMD-blue's default build
    } // namespace hoomd
#endif
