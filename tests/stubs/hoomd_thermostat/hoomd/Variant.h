// STAND-IN for hoomd/Variant.h -- NOT HOOMD-blue.  A set point that returns the value the driver stored.
#ifndef STANDIN_THERMOSTAT_VARIANT_H_
#define STANDIN_THERMOSTAT_VARIANT_H_

#include "HOOMDMath.h"

namespace hoomd
    {
class Variant
    {
    public:
    explicit Variant(Scalar value = 0) : m_value(value) { }
    virtual ~Variant() { }
    virtual Scalar operator()(uint64_t timestep)
        {
        return m_value;
        }
    Scalar m_value;
    };
    } // namespace hoomd
#endif
