// STAND-IN for hoomd/RNGIdentifiers.h -- NOT HOOMD-blue.  The stream identifiers the thermostat headers name; the values
// are irrelevant here because the stand-in RandomGenerator (RandomNumbers.h) ignores its seed.
#ifndef STANDIN_THERMOSTAT_RNG_IDENTIFIERS_H_
#define STANDIN_THERMOSTAT_RNG_IDENTIFIERS_H_

#include <cstdint>

namespace hoomd
    {
struct RNGIdentifier
    {
    static const uint8_t MTTKThermostat = 0;
    static const uint8_t BussiThermostat = 1;
    };
    } // namespace hoomd
#endif
