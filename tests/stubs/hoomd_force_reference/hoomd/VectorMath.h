// STAND-IN for hoomd/VectorMath.h, host only -- NOT HOOMD-blue.  vec3<Real> with the operators the reference's CPU force
// class uses and no others: construction from three numbers and from a Scalar4 (x, y, z; w dropped), +, -, +=, scalar * vec3
// and dot.  This is the ONLY arithmetic the stand-in headers carry; every operator is component-wise, one IEEE operation per
// component, and dot is a.x*b.x + a.y*b.y + a.z*b.z evaluated left to right.
//
// UNVERIFIED: that association (and that scalar * vec3 is one multiplication per component) is HOOMD-blue upstream's as we
// remember it.  HOOMD-blue's own VectorMath.h was not available to compare with, so what a fixture made with this header
// pins is the reference's class on top of THIS vec3, not on top of HOOMD-blue's.
#ifndef STANDIN_FORCE_REFERENCE_VECTOR_MATH_H_
#define STANDIN_FORCE_REFERENCE_VECTOR_MATH_H_

#include "HOOMDMath.h"

namespace hoomd
    {
template<class Real> struct vec3
    {
    vec3() : x(0), y(0), z(0) { }
    vec3(const Real& _x, const Real& _y, const Real& _z) : x(_x), y(_y), z(_z) { }
    explicit vec3(const Scalar4& a) : x(a.x), y(a.y), z(a.z) { }
    Real x, y, z;
    };

template<class Real> inline vec3<Real> operator+(const vec3<Real>& a, const vec3<Real>& b)
    {
    return vec3<Real>(a.x + b.x, a.y + b.y, a.z + b.z);
    }

template<class Real> inline vec3<Real> operator-(const vec3<Real>& a, const vec3<Real>& b)
    {
    return vec3<Real>(a.x - b.x, a.y - b.y, a.z - b.z);
    }

template<class Real> inline vec3<Real>& operator+=(vec3<Real>& a, const vec3<Real>& b)
    {
    a.x += b.x;
    a.y += b.y;
    a.z += b.z;
    return a;
    }

template<class Real> inline vec3<Real> operator*(const Real& b, const vec3<Real>& a)
    {
    return vec3<Real>(a.x * b, a.y * b, a.z * b);
    }

template<class Real> inline Real dot(const vec3<Real>& a, const vec3<Real>& b)
    {
    return a.x * b.x + a.y * b.y + a.z * b.z;
    }
    } // namespace hoomd
#endif
