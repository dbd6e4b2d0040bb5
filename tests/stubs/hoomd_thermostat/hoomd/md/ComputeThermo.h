// STAND-IN for hoomd/md/ComputeThermo.h -- NOT HOOMD-blue.  compute() does nothing; the getters return the kinetic
// energies, degrees of freedom and temperatures the driver prescribed.
#ifndef STANDIN_THERMOSTAT_COMPUTE_THERMO_H_
#define STANDIN_THERMOSTAT_COMPUTE_THERMO_H_

#include "../HOOMDMath.h"

namespace hoomd::md
    {
class ComputeThermo
    {
    public:
    void compute(uint64_t timestep) { }
    Scalar getTranslationalDOF() const
        {
        return m_translational_dof;
        }
    Scalar getRotationalDOF() const
        {
        return m_rotational_dof;
        }
    Scalar getTranslationalKineticEnergy() const
        {
        return m_translational_kinetic_energy;
        }
    Scalar getRotationalKineticEnergy() const
        {
        return m_rotational_kinetic_energy;
        }
    Scalar getTranslationalTemperature() const
        {
        return m_translational_temperature;
        }
    Scalar getRotationalTemperature() const
        {
        return m_rotational_temperature;
        }
    Scalar m_translational_dof = 0;
    Scalar m_rotational_dof = 0;
    Scalar m_translational_kinetic_energy = 0;
    Scalar m_rotational_kinetic_energy = 0;
    Scalar m_translational_temperature = 0;
    Scalar m_rotational_temperature = 0;
    };
    } // namespace hoomd::md
#endif
