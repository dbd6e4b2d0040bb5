// STAND-IN for hoomd/ForceCompute.h (and the GlobalArray / ArrayHandle / BoxDim / ParticleData / SystemDefinition /
// ExecutionConfiguration it brings along) -- NOT HOOMD-blue.  Host-side holders of the arrays the driver prescribes; the
// reference's CPU force class only reads them and writes m_force.  No arithmetic.  (tests/stubs/hoomd_cpp is a different
// stand-in, for the product's shim: it allocates on the device and is not used here.)
#ifndef STANDIN_FORCE_REFERENCE_FORCE_COMPUTE_H_
#define STANDIN_FORCE_REFERENCE_FORCE_COMPUTE_H_

#include "HOOMDMath.h"

namespace hoomd
    {
struct access_location
    {
    enum Enum
        {
        host,
        device
        };
    };

struct access_mode
    {
    enum Enum
        {
        read,
        readwrite,
        overwrite
        };
    };

template<class T> class GlobalArray
    {
    public:
    GlobalArray() { }
    explicit GlobalArray(size_t n) : m_data(n) { }
    std::vector<T> m_data;
    };

template<class T> class ArrayHandle
    {
    public:
    ArrayHandle(const GlobalArray<T>& array, access_location::Enum, access_mode::Enum)
        : data(const_cast<T*>(array.m_data.data()))
        {
        }
    T* const data;
    };

class BoxDim
    {
    public:
    BoxDim() : m_L {0, 0, 0} { }
    explicit BoxDim(Scalar3 L) : m_L(L) { }
    Scalar3 getL() const
        {
        return m_L;
        }

    private:
    Scalar3 m_L;
    };

//! notice() hands out a stream that discards what is written to it
struct Messenger
    {
    std::ostream& notice(unsigned int)
        {
        return m_null;
        }
    std::ostream m_null {nullptr};
    };

struct ExecutionConfiguration
    {
    std::shared_ptr<Messenger> msg = std::make_shared<Messenger>();
    };

class ParticleData
    {
    public:
    const GlobalArray<Scalar4>& getPositions() const
        {
        return m_pos;
        }
    const GlobalArray<Scalar>& getCharges() const
        {
        return m_charge;
        }
    const GlobalArray<int3>& getImages() const
        {
        return m_image;
        }
    unsigned int getN() const
        {
        return (unsigned int)m_pos.m_data.size();
        }
    const BoxDim& getGlobalBox() const
        {
        return m_box;
        }
    unsigned int getTypeByName(const std::string& name) const
        {
        for (unsigned int i = 0; i < m_type_names.size(); i++)
            if (m_type_names[i] == name)
                return i;
        throw std::runtime_error("Type " + name + " not found!");
        }
    std::shared_ptr<ExecutionConfiguration> getExecConf() const
        {
        return m_exec_conf;
        }

    GlobalArray<Scalar4> m_pos;
    GlobalArray<Scalar> m_charge;
    GlobalArray<int3> m_image;
    BoxDim m_box;
    std::vector<std::string> m_type_names;
    std::shared_ptr<ExecutionConfiguration> m_exec_conf = std::make_shared<ExecutionConfiguration>();
    };

class SystemDefinition
    {
    public:
    std::shared_ptr<ParticleData> getParticleData() const
        {
        return m_pdata;
        }
    std::shared_ptr<ParticleData> m_pdata = std::make_shared<ParticleData>();
    };

class ForceCompute
    {
    public:
    explicit ForceCompute(std::shared_ptr<SystemDefinition> sysdef)
        : m_sysdef(sysdef), m_pdata(sysdef->getParticleData()), m_exec_conf(m_pdata->getExecConf()),
          m_force(m_pdata->getN())
        {
        }
    virtual ~ForceCompute() { }

    protected:
    virtual void computeForces(uint64_t timestep) = 0;

    std::shared_ptr<SystemDefinition> m_sysdef;
    std::shared_ptr<ParticleData> m_pdata;
    std::shared_ptr<ExecutionConfiguration> m_exec_conf;
    GlobalArray<Scalar4> m_force;
    };
    } // namespace hoomd
#endif
