// STAND-IN for hoomd/ParticleGroup.h (and the SystemDefinition / ParticleData / ExecutionConfiguration it brings along)
// -- NOT HOOMD-blue.  Holders of the values the driver prescribes; the thermostat headers only read them.
#ifndef STANDIN_THERMOSTAT_PARTICLE_GROUP_H_
#define STANDIN_THERMOSTAT_PARTICLE_GROUP_H_

#include "HOOMDMath.h"

namespace hoomd
    {
struct Messenger
    {
    std::ostream& notice(unsigned int level)
        {
        return std::clog;
        }
    };

struct ExecutionConfiguration
    {
    std::shared_ptr<Messenger> msg = std::make_shared<Messenger>();
    int getRank() const
        {
        return 0;
        }
    };

class ParticleData
    {
    public:
    std::shared_ptr<ExecutionConfiguration> getExecConf() const
        {
        return m_exec_conf;
        }
    std::shared_ptr<ExecutionConfiguration> m_exec_conf = std::make_shared<ExecutionConfiguration>();
    };

class SystemDefinition
    {
    public:
    uint16_t getSeed() const
        {
        return m_seed;
        }
    std::shared_ptr<ParticleData> getParticleData() const
        {
        return m_pdata;
        }
    bool isDomainDecomposed() const
        {
        return false;
        }
    uint16_t m_seed = 0;
    std::shared_ptr<ParticleData> m_pdata = std::make_shared<ParticleData>();
    };

class ParticleGroup
    {
    public:
    unsigned int getNumMembersGlobal() const
        {
        return m_num_members;
        }
    unsigned int getMemberTag(unsigned int i) const
        {
        return m_first_tag;
        }
    Scalar getTranslationalDOF() const
        {
        return m_translational_dof;
        }
    Scalar getRotationalDOF() const
        {
        return m_rotational_dof;
        }
    unsigned int m_num_members = 1;
    unsigned int m_first_tag = 0;
    Scalar m_translational_dof = 0;
    Scalar m_rotational_dof = 0;
    };
    } // namespace hoomd
#endif
