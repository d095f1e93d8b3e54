/* Host stand-in for include/metropolis_user_energy.h (test infrastructure only): lets the source that
 * metropolisengine_amd/pyenergy.py generates compile with a host C++ compiler, so that what the emitter writes can be
 * checked without a GPU.  The device qualifiers go away, me_fma is the C library's fused multiply-add. */
#ifndef METROPOLIS_USER_ENERGY_H
#define METROPOLIS_USER_ENERGY_H
#include <cmath>
#include <math.h>
#define __device__
#define __forceinline__ inline
inline float me_fma(float a, float b, float c) { return std::fma(a, b, c); }
inline double me_fma(double a, double b, double c) { return std::fma(a, b, c); }
#endif
