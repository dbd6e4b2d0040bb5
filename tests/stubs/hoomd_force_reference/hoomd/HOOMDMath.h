// STAND-IN for hoomd/HOOMDMath.h, host only -- NOT HOOMD-blue.  Just enough names for the reference's CPU force class
// (CavityForceCompute.h / .cc) to compile with a plain C++ compiler, so that oracle/reference_driver can execute its
// arithmetic.  No arithmetic of its own: containers and one reinterpretation of bytes.
//
// UNVERIFIED against HOOMD-blue's own header (HOOMD-blue is not available where this was written): Scalar as double
// (HOOMD_LONGREAL_SIZE = 64, the default build), Scalar3 / Scalar4 / int3 as the plain x-y-z(-w) structs of the vector
// types, and __scalar_as_int as the int that shares storage with the low four bytes of the double (a union {int; Scalar}
// upstream, as we remember it; oracle/cavity_ref.c states the same).
#ifndef STANDIN_FORCE_REFERENCE_HOOMD_MATH_H_
#define STANDIN_FORCE_REFERENCE_HOOMD_MATH_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

struct int3
    {
    int x, y, z;
    };

namespace hoomd
    {
typedef double Scalar;

struct Scalar3
    {
    Scalar x, y, z;
    };

struct Scalar4
    {
    Scalar x, y, z, w;
    };

//! The int in the low four bytes of a Scalar (how pos.w carries the type id)
inline int __scalar_as_int(Scalar b)
    {
    int32_t a;
    std::memcpy(&a, &b, sizeof(a));
    return (int)a;
    }
    } // namespace hoomd
#endif
