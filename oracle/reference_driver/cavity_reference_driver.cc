// Runs the reference's own CPU force class, hoomd::cavitymd::CavityForceCompute, on prescribed inputs -- TEST
// INFRASTRUCTURE.  This file holds no line of the reference: it includes the class by name, oracle/Makefile compiles the
// reference's CavityForceCompute.cc next to it (on top of tests/stubs/hoomd_force_reference), and the result lives in
// oracle/_ref/, which is never committed.  tests/golden/make_reference_cavity_cpp_golden.py and
// tests/test_reference_cpp_live.py are the callers.
//
//   cavity_reference_cpu CASES RESULTS          (the reference's constructor prints to stdout: no data goes there)
//
// CASES, repeated until the end of the file (little endian, no padding):
//   uint32 N, uint32 n_types, n_types x char[16] (type names, NUL padded),
//   double Lx, Ly, Lz, omegac, couplstr, phmass,
//   double pos[N][4] (w: the type tag), double charge[N], int32 image[N][3]
// RESULTS, per case:
//   double force[N][4]   m_force after computeForces(); every entry held SENTINEL before the call
//   double energies[3]   harmonic, coupling, dipole-self (the public getters)
//   double dipole[3]     what computeDipoleMoment returns for findPhotonParticle's index (-1 included: it then skips nobody)
//   double K             cavity_force_params::K as the constructor computed it
//   int32 photon_idx, int32 N
#include "CavityForceCompute.h"

#include <cstdio>

using namespace hoomd;
using namespace hoomd::cavitymd;

static const double SENTINEL = -7.25;

class OpenedCavityForceCompute : public CavityForceCompute
    {
    public:
    using CavityForceCompute::CavityForceCompute;
    using CavityForceCompute::computeDipoleMoment;
    using CavityForceCompute::computeForces;
    using CavityForceCompute::computeUnwrappedPositions;
    using CavityForceCompute::findPhotonParticle;
    using CavityForceCompute::m_force;
    using CavityForceCompute::m_params;
    };

template<class T> static bool read_n(FILE* f, T* out, size_t n)
    {
    return n == 0 || fread(out, sizeof(T), n, f) == n;
    }

template<class T> static bool write_n(FILE* f, const T* in, size_t n)
    {
    return n == 0 || fwrite(in, sizeof(T), n, f) == n;
    }

int main(int argc, char** argv)
    {
    if (argc != 3)
        return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo)
        return 2;
    uint32_t head[2];
    while (fread(head, sizeof(uint32_t), 2, fi) == 2)
        {
        const unsigned int N = head[0];
        auto sysdef = std::make_shared<SystemDefinition>();
        ParticleData& pd = *sysdef->m_pdata;
        for (uint32_t t = 0; t < head[1]; t++)
            {
            char name[17] = {0};
            if (!read_n(fi, name, 16))
                return 3;
            pd.m_type_names.push_back(name);
            }
        double scal[6];
        if (!read_n(fi, scal, 6))
            return 3;
        pd.m_box = BoxDim(Scalar3 {scal[0], scal[1], scal[2]});
        pd.m_pos.m_data.resize(N);
        pd.m_charge.m_data.resize(N);
        pd.m_image.m_data.resize(N);
        if (!read_n(fi, pd.m_pos.m_data.data(), N) || !read_n(fi, pd.m_charge.m_data.data(), N)
            || !read_n(fi, pd.m_image.m_data.data(), N))
            return 3;

        OpenedCavityForceCompute fc(sysdef, scal[3], scal[4], scal[5]);
        for (Scalar4& f : fc.m_force.m_data)
            f = Scalar4 {SENTINEL, SENTINEL, SENTINEL, SENTINEL};
        fc.computeForces(0);

        const int photon_idx = fc.findPhotonParticle(pd.m_pos.m_data.data(), N);
        std::vector<vec3<Scalar>> unwrapped;
        fc.computeUnwrappedPositions(unwrapped, pd.m_pos.m_data.data(), pd.m_image.m_data.data(), pd.m_box, N);
        const vec3<Scalar> d = fc.computeDipoleMoment(unwrapped, pd.m_charge.m_data.data(), N, photon_idx);

        const double tail[7] = {fc.getHarmonicEnergy(), fc.getCouplingEnergy(), fc.getDipoleSelfEnergy(), d.x, d.y, d.z,
                                fc.m_params.K};
        const int32_t ints[2] = {photon_idx, (int32_t)N};
        if (!write_n(fo, fc.m_force.m_data.data(), N) || !write_n(fo, tail, 7) || !write_n(fo, ints, 2))
            return 4;
        }
    if (fclose(fo) != 0)
        return 4;
    fclose(fi);
    return 0;
    }
