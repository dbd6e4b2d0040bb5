// STAND-IN for hoomd/RandomNumbers.h -- NOT HOOMD-blue.  No generator: every distribution object, when called, pops the
// next value of a stream the driver injected (standin_draws) and logs what was asked for (standin_log: the kind of
// distribution and its parameters), so that the driver can record which draws the reference consumed and in what order.
// The distributions return the injected value unchanged: no arithmetic happens here.
#ifndef STANDIN_THERMOSTAT_RANDOM_NUMBERS_H_
#define STANDIN_THERMOSTAT_RANDOM_NUMBERS_H_

#include <cstdint>
#include <deque>
#include <stdexcept>
#include <vector>

namespace hoomd
    {
struct StandinDraw
    {
    int kind;      // 0: NormalDistribution, 1: GammaDistribution
    double param0; // normal: sigma, gamma: alpha (shape)
    double param1; // normal: mu, gamma: b (scale)
    double value;  // the value handed out
    };

inline std::deque<double>& standin_draws()
    {
    static std::deque<double> q;
    return q;
    }
inline std::vector<StandinDraw>& standin_log()
    {
    static std::vector<StandinDraw> log;
    return log;
    }
inline double standin_pop(int kind, double param0, double param1)
    {
    if (standin_draws().empty())
        throw std::logic_error("stand-in RandomGenerator: injected draw stream exhausted");
    const double v = standin_draws().front();
    standin_draws().pop_front();
    standin_log().push_back(StandinDraw {kind, param0, param1, v});
    return v;
    }

struct Seed
    {
    Seed(uint8_t id, uint64_t timestep, uint16_t seed) { }
    };

struct Counter
    {
    Counter(uint32_t a = 0, uint32_t b = 0, uint32_t c = 0, uint16_t d = 0) { }
    };

class RandomGenerator
    {
    public:
    RandomGenerator(const Seed& seed, const Counter& counter) { }
    };

template<typename Real> class NormalDistribution
    {
    public:
    explicit NormalDistribution(Real sigma = Real(1.0), Real mu = Real(0.0)) : m_sigma(sigma), m_mu(mu) { }
    template<typename RNG> Real operator()(RNG& rng)
        {
        return Real(standin_pop(0, double(m_sigma), double(m_mu)));
        }

    private:
    Real m_sigma, m_mu;
    };

template<typename Real> class GammaDistribution
    {
    public:
    GammaDistribution(Real alpha, Real b) : m_alpha(alpha), m_b(b) { }
    template<typename RNG> Real operator()(RNG& rng)
        {
        return Real(standin_pop(1, double(m_alpha), double(m_b)));
        }

    private:
    Real m_alpha, m_b;
    };
    } // namespace hoomd
#endif
